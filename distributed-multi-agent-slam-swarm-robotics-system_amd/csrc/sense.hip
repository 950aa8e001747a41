// sense.hip -- sensing a world: the sweeps and packets a bot would send from a pose in the context's map.
// The rules are this build's own (include/quasar_slam.h, "sensing a world", S1-S8): the inverse of the raycast.  A beam walks the
// reference's Bresenham line (raycast_common.h's recurrence) from the pose's cell to the far point's cell and returns the
// centre-to-centre distance to the first OCCUPIED cell; everything but the far point is integer.
//
//   sweeps  : one 64-lane workgroup (= one wave) per record, as gain.hip.  The wave loads the (2 C + 1)^2 patch around the start
//             cell, C = ceil(R / res) + 1, reading the stamp rows coalesced and nothing outside the grid, and packs it to a BIT a
//             cell with one ballot per 64 cells (only OCCUPIED matters): rows of 64-bit words in LDS.  Each lane then takes beams
//             lane, lane + 64, lane + 128 and walks its line over the patch; the line stays in the box its two ends span, so it
//             stays in the patch.
//   packets : four beams a record; four lanes per record read the stamps directly (a beam is 25 cells at the defaults, a patch
//             2601), 64 records a workgroup.
// A record's bytes (743, 751 or 42 at any byte address) are put together in LDS at the misalignment of their destination and
// leave as aligned dword stores, the partial dwords at either end bytewise: neighbouring records never share a store.
// No global atomics, no device-side waits, no graphs; the kernels write nothing but the caller's output.
#include <math.h>
#include <algorithm>

#include "raycast_common.h"

#define SN_MAGIC 0x4c525351u        // 'Q','S','R','L'
#define SN_REC_BYTES 768            // LDS bytes of a staged sweep record: >= 3 + 751, a multiple of 8
#define SN_QUAD_BLOCK 256           // packets: 64 records x 4 beams per workgroup
#define SN_QUAD_RECS (SN_QUAD_BLOCK / 4)
#define SN_QUAD_BYTES ((3 + SN_QUAD_RECS * QS_PACKET_SIZE + 7) & ~7)
#define SN_HOST_CHUNK ((size_t)4096)           // records a host call stages at a time (io_ws: about 6 MiB of sweeps)
#define SN_DEVICE_CHUNK ((size_t)1 << 24)      // records per launch of a device call

struct QsSenseArgs {
    const float *pose;                  // [n][3] x, y, yaw
    const unsigned char *agent;         // [n]; the three below: [n] or nullptr (= 0)
    const int *enc;
    const unsigned int *v2v;
    const unsigned char *lm;
    size_t n;                           // records of this launch
    double R, amp;
    float no_return;
    unsigned int dropout;
    unsigned long long seed, rec0;      // rec0: first_record + the index within the call of this launch's record 0
    int C;                              // patch radius, ceil(R / res) + 1
    bool noisy;                         // S7 is on
    float *ranges; int *hit_cell;       // the ranges form: [n][beams]; hit_cell may be nullptr
    unsigned char *pkts;                // the packet forms: record k at pkts + k * stride
    size_t stride;
};

struct SnPose { bool ok; double rx, ry, yaw; int x0, y0; };

// S2: the pose as a packet carries it; ok = finite and with a cell
__device__ inline SnPose sn_pose(const float *p, const QsGeom &geo)
{
    SnPose s;
    const float x = p[0], y = p[1], w = p[2];
    s.rx = (double)x; s.ry = (double)y; s.yaw = (double)w;
    s.x0 = s.y0 = 0;
    s.ok = isfinite(x) && isfinite(y) && isfinite(w);
    if (s.ok) {
        s.ok = qs_w2g_i32(s.rx, geo.ox, geo, s.x0);
        s.ok = qs_w2g_i32(s.ry, geo.oy, geo, s.y0) && s.ok;
    }
    return s;
}

// the OCCUPIED bit of a grid cell, from the wave's patch or from the stamps; a cell outside either reads as not OCCUPIED
struct SnOccPatch {
    const unsigned long long *bits; int pw, W, bx, by;     // rows of pw words; cell (bx, by) of the grid is bit 0 of row 0
    __device__ bool operator()(int x, int y) const
    {
        const unsigned int px = (unsigned int)(x - bx), py = (unsigned int)(y - by);
        if (px >= (unsigned int)W || py >= (unsigned int)W) return false;
        return (bits[py * pw + (px >> 6)] >> (px & 63u)) & 1ull;
    }
};
struct SnOccGrid {
    const unsigned int *stamps; int size;
    __device__ bool operator()(int x, int y) const
    {
        if ((unsigned int)x >= (unsigned int)size || (unsigned int)y >= (unsigned int)size) return false;
        return stamps[(size_t)y * size + x] & 1u;
    }
};

struct SnHit { float range; int cell; };

// S4-S7: beam `beam` of record `rec` (its index within the call plus first_record) at heading a
template <class Occ>
__device__ inline SnHit sn_beam(const SnPose &s, double a, const QsSenseArgs &q, const QsGeom &geo, const Occ &occ,
                                unsigned long long rec, int beam)
{
    SnHit h{q.no_return, -1};
    if (!s.ok) return h;
    double sa, ca;
    qs_sincos(a, &sa, &ca);
    const double ex = s.rx + q.R * ca, ey = s.ry + q.R * sa;                                   // S4
    int x1 = 0, y1 = 0;
    bool ok = qs_w2g_i32(ex, geo.ox, geo, x1);
    ok = qs_w2g_i32(ey, geo.oy, geo, y1) && ok;
    if (!ok) return h;
    // |cells| <= 2^30 and the far point lies R away: the differences are at most C (the test is never true)
    const long long ldx = llabs((long long)x1 - s.x0), ldy = llabs((long long)y1 - s.y0);
    if (ldx > q.C || ldy > q.C) return h;
    const int dx = (int)ldx, dy = (int)ldy, sx = s.x0 < x1 ? 1 : -1, sy = s.y0 < y1 ? 1 : -1;   // :161-164
    int x = s.x0, y = s.y0, err = dx - dy;
    bool hit = false;
    while (x != x1 || y != y1) {                                                               // cell 0 never blocks (S5)
        const int e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x += sx; }
        if (e2 < dx) { err += dx; y += sy; }
        if (occ(x, y)) { hit = true; break; }
    }
    if (!hit) return h;
    const long long hx = x - s.x0, hy = y - s.y0;
    double d = geo.res * sqrt((double)(hx * hx + hy * hy));                                    // S6
    bool drop = false;
    if (q.noisy) {                                                                             // S7
        unsigned long long z = q.seed + 0x9E3779B97F4A7C15ull * (1ull + rec * 256ull + (unsigned long long)beam);
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        z ^= z >> 31;
        const unsigned long long u = (z >> 40) + ((z >> 16) & 0xFFFFFFull);
        d = d + q.amp * ((double)u * 0x1p-24 - 1.0);
        drop = (z & 0xFFFFull) < (unsigned long long)q.dropout;
    }
    const float f = (float)d;
    if (!drop && (double)f <= q.R) { h.range = f; h.cell = y * geo.size + x; }
    return h;
}

// ---- a record's bytes through LDS --------------------------------------------------------------------------------------
// s[mis + j] is byte j of the output, mis = the destination's address & 3 (s itself is dword-aligned)
__device__ inline void sn_put8(unsigned char *s, unsigned int o, unsigned int v) { s[o] = (unsigned char)v; }
__device__ inline void sn_put16(unsigned char *s, unsigned int o, unsigned int v) { s[o] = (unsigned char)v; s[o + 1] = (unsigned char)(v >> 8); }
__device__ inline void sn_put32(unsigned char *s, unsigned int o, unsigned int v)
{
    s[o] = (unsigned char)v; s[o + 1] = (unsigned char)(v >> 8); s[o + 2] = (unsigned char)(v >> 16); s[o + 3] = (unsigned char)(v >> 24);
}
// magic, agent, x, y, yaw, encoder, v2v of both packet formats ('<4sBfffiI...'; the v0 sweep has no encoder and v2v); the pose's
// bits go through as they came
__device__ inline void sn_put_head(unsigned char *s, unsigned int o, const QsSenseArgs &q, size_t k, bool odometry)
{
    sn_put32(s, o, SN_MAGIC);
    sn_put8(s, o + 4, q.agent[k]);
    for (int j = 0; j < 3; j++) sn_put32(s, o + 5 + 4 * j, __float_as_uint(q.pose[3 * k + j]));
    if (odometry) {
        sn_put32(s, o + 17, q.enc ? (unsigned int)q.enc[k] : 0u);
        sn_put32(s, o + 21, q.v2v ? q.v2v[k] : 0u);
    }
}
// the nbytes at s + mis to dst: the dwords that lie wholly inside [dst, dst + nbytes) as dword stores, the rest bytewise
__device__ inline void sn_flush(const unsigned char *s, unsigned int mis, unsigned char *dst, unsigned int nbytes, int tid, int nthreads)
{
    unsigned char *w0 = dst - mis;
    const unsigned int total = mis + nbytes;
    for (unsigned int lo = 4u * tid; lo < total; lo += 4u * nthreads) {
        if (lo >= mis && lo + 4 <= total) *(unsigned int *)(w0 + lo) = *(const unsigned int *)(s + lo);
        else
            for (unsigned int b = lo < mis ? mis : lo; b < lo + 4 && b < total; b++) w0[b] = s[b];
    }
}

// ---- sweeps: one wave per record -----------------------------------------------------------------------------------------
// PKT: the record leaves as a 743 / 751-byte packet; otherwise its ranges (and hit cells) as arrays
template <bool PKT>
__global__ void __launch_bounds__(QS_WAVE)
qs_sense_sweep_kernel(QsSenseArgs q, QsGeom geo, const unsigned int *__restrict__ stamps)
{
    extern __shared__ unsigned long long s_bits[];      // [W][pw] the patch, W = 2 C + 1, the start cell in the middle; then the record
    const size_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const SnPose s = sn_pose(q.pose + 3 * k, geo);      // wave-uniform
    const int W = 2 * q.C + 1, pw = (W + 63) >> 6;
    const int bx = s.x0 - q.C, by = s.y0 - q.C;         // |x0| <= 2^30
    if (s.ok) {
        for (int py = 0; py < W; py++) {
            const int gy = by + py;
            const bool row_in = gy >= 0 && gy < geo.size;
            for (int w = 0; w < pw; w++) {
                const int px = 64 * w + lane, gx = bx + px;
                bool o = false;
                if (row_in && px < W && gx >= 0 && gx < geo.size) o = stamps[(size_t)gy * geo.size + gx] & 1u;
                const unsigned long long m = __ballot(o);
                if (lane == 0) s_bits[py * pw + w] = m;
            }
        }
    }
    unsigned char *s_rec = (unsigned char *)(s_bits + (size_t)W * pw);
    const bool odometry = q.stride == QS_SWEEP_SIZE_V0_ODO;
    const unsigned int mis = PKT ? (unsigned int)((unsigned long long)(q.pkts + k * q.stride) & 3ull) : 0u;
    const unsigned int r_off = mis + (odometry ? 27u : 19u);
    if (PKT && lane == 0) {
        sn_put_head(s_rec, mis, q, k, odometry);
        sn_put16(s_rec, mis + (odometry ? 25u : 17u), QS_SWEEP_BEAMS);
    }
    __syncthreads();
    const SnOccPatch occ{s_bits, pw, W, bx, by};
    const double kRad = 3.141592653589793 / 180.0;      // math.radians
    #pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = lane + QS_WAVE * t;
        if (i >= QS_SWEEP_BEAMS) break;
        const SnHit h = sn_beam(s, s.yaw + (double)(i - 90) * kRad, q, geo, occ, q.rec0 + k, i);
        if (PKT) sn_put32(s_rec, r_off + 4u * i, __float_as_uint(h.range));
        else {
            q.ranges[k * QS_SWEEP_BEAMS + i] = h.range;
            if (q.hit_cell) q.hit_cell[k * QS_SWEEP_BEAMS + i] = h.cell;
        }
    }
    if (PKT) {
        __syncthreads();
        sn_flush(s_rec, mis, q.pkts + k * q.stride, (unsigned int)q.stride, lane, QS_WAVE);
    }
}

// ---- packets: four lanes per record, the stamps read directly ----------------------------------------------------------------
template <bool PKT>
__global__ void __launch_bounds__(SN_QUAD_BLOCK)
qs_sense_quad_kernel(QsSenseArgs q, QsGeom geo, const unsigned int *__restrict__ stamps)
{
    __shared__ __attribute__((aligned(8))) unsigned char s_out[PKT ? SN_QUAD_BYTES : 8];
    const int tid = threadIdx.x, beam = tid & 3;
    const size_t k0 = (size_t)blockIdx.x * SN_QUAD_RECS, k = k0 + (tid >> 2);
    const unsigned int mis = PKT ? (unsigned int)((unsigned long long)(q.pkts + k0 * QS_PACKET_SIZE) & 3ull) : 0u;
    if (k < q.n) {
        const SnPose s = sn_pose(q.pose + 3 * k, geo);
        const double kPi = 3.141592653589793;           // math.pi
        const double ang = beam == 0 ? 0.0 : (beam == 1 ? kPi / 2 : (beam == 2 ? kPi : -kPi / 2));   // :61-66
        const SnHit h = sn_beam(s, s.yaw + ang, q, geo, SnOccGrid{stamps, geo.size}, q.rec0 + k, beam);
        if (PKT) {
            const unsigned int o = mis + (unsigned int)(k - k0) * QS_PACKET_SIZE;
            if (beam == 0) { sn_put_head(s_out, o, q, k, true); sn_put8(s_out, o + 41, q.lm ? q.lm[k] : 0u); }
            sn_put32(s_out, o + 25 + 4u * beam, __float_as_uint(h.range));
        } else {
            q.ranges[4 * k + beam] = h.range;
            if (q.hit_cell) q.hit_cell[4 * k + beam] = h.cell;
        }
    }
    if (PKT) {
        __syncthreads();
        const size_t m = q.n - k0 < (size_t)SN_QUAD_RECS ? q.n - k0 : (size_t)SN_QUAD_RECS;
        sn_flush(s_out, mis, q.pkts + k0 * QS_PACKET_SIZE, (unsigned int)(m * QS_PACKET_SIZE), tid, SN_QUAD_BLOCK);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
enum { SN_RANGES = 0, SN_SWEEPS = 1, SN_PACKETS = 2 };

// one call: what it reads and writes, host or device pointers alike
struct SnCall {
    int kind; bool host; const char *who;
    const float *pose; const uint8_t *agent; const int32_t *enc; const uint32_t *v2v; const uint8_t *lm;
    size_t n; int beams;
    float *ranges; int32_t *hit_cell; uint8_t *pkts; size_t stride;
};

// S8; C = the patch radius
static int sense_check(qs_ctx *c, const SnCall &s, const qs_sense_params *p, int &C)
{
    const std::string who(s.who);
    if (!p) return qs_fail(c, QS_E_INVAL, (who + ": params is NULL").c_str());
    if (s.kind == SN_SWEEPS && s.stride != QS_SWEEP_SIZE_V0 && s.stride != QS_SWEEP_SIZE_V0_ODO)
        return qs_fail(c, QS_E_INVAL, (who + ": stride must be 743 (v0) or 751 (v0 + odometry)").c_str());
    if (s.beams != QS_SWEEP_BEAMS && s.beams != 4) return qs_fail(c, QS_E_INVAL, (who + ": beams must be 181 or 4").c_str());
    if (!(isfinite(p->max_range) && p->max_range > 0)) return qs_fail(c, QS_E_INVAL, (who + ": max_range must be finite and > 0").c_str());
    const double cells = ceil(p->max_range / c->cfg.res);
    if (!(cells + 1 <= (double)QS_SENSE_MAX_CELLS))
        return qs_fail(c, QS_E_INVAL, (who + ": ceil(max_range / res) + 1 exceeds QS_SENSE_MAX_CELLS").c_str());
    if (!(isfinite(p->noise_amp) && p->noise_amp >= 0)) return qs_fail(c, QS_E_INVAL, (who + ": noise_amp must be finite and >= 0").c_str());
    if (p->dropout_q16 > 65536u) return qs_fail(c, QS_E_INVAL, (who + ": dropout_q16 above 65536").c_str());
    if (p->reserved[0] || p->reserved[1]) return qs_fail(c, QS_E_INVAL, (who + ": reserved fields must be 0").c_str());
    C = (int)cells + 1;
    return QS_OK;
}

// m records at device pointers
static hipError_t qs_launch_sense(qs_ctx *c, const SnCall &s, const QsSenseArgs &q)
{
    if (s.beams == 4) {
        const unsigned int blocks = (unsigned int)((q.n + SN_QUAD_RECS - 1) / SN_QUAD_RECS);
        hipLaunchKernelGGL(s.kind == SN_PACKETS ? qs_sense_quad_kernel<true> : qs_sense_quad_kernel<false>, dim3(blocks), dim3(SN_QUAD_BLOCK),
                           0, c->stream, q, c->geom, c->d_stamps.p);
        return hipGetLastError();
    }
    const size_t W = 2 * (size_t)q.C + 1, pw = (W + 63) >> 6;
    const bool pkt = s.kind == SN_SWEEPS;
    hipLaunchKernelGGL(pkt ? qs_sense_sweep_kernel<true> : qs_sense_sweep_kernel<false>, dim3((unsigned int)q.n), dim3(QS_WAVE),
                       W * pw * 8 + (pkt ? SN_REC_BYTES : 0), c->stream, q, c->geom, c->d_stamps.p);
    return hipGetLastError();
}

// the staging of one chunk of a host call, carved from io_ws (nullptr: only the bytes)
struct SnStage { float *pose; uint8_t *agent; int32_t *enc; uint32_t *v2v; uint8_t *lm; float *ranges; int32_t *hit_cell; uint8_t *pkts; size_t bytes; };
static SnStage sense_stage(void *ws, const SnCall &s, size_t m)
{
    SnStage t{};
    Carve k(ws);
    t.pose = k.take<float>(3 * m);
    if (s.kind != SN_RANGES) {
        t.agent = k.take<uint8_t>(m); t.enc = k.take<int32_t>(m); t.v2v = k.take<uint32_t>(m); t.lm = k.take<uint8_t>(m);
        t.pkts = k.take<uint8_t>(m * s.stride);
    } else {
        t.ranges = k.take<float>(m * s.beams); t.hit_cell = k.take<int32_t>(m * s.beams);
    }
    t.bytes = k.bytes;
    return t;
}

// The six entry points' one routine.  host: every pointer of the call is the caller's host memory, staged SN_HOST_CHUNK records at a
// time through io_ws (stream-ordered: the previous chunk's copies out have read it), and the call ends by waiting for the GPU.
static int sense_run(qs_ctx *c, const SnCall &s, const qs_sense_params *p)
{
    int C = 0;
    int rc = sense_check(c, s, p, C);
    if (rc != QS_OK) return rc;
    if (s.n == 0) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);                                            // S1: waiting edge rays go into the map first
    QsSenseArgs q{};
    q.R = p->max_range; q.amp = p->noise_amp; q.no_return = p->no_return; q.dropout = p->dropout_q16; q.seed = p->seed;
    q.C = C; q.noisy = p->noise_amp != 0.0 || p->dropout_q16 != 0;
    q.stride = s.stride;
    const size_t chunk = s.host ? SN_HOST_CHUNK : SN_DEVICE_CHUNK;
    for (size_t k0 = 0; k0 < s.n; k0 += chunk) {
        const size_t m = std::min(chunk, s.n - k0);
        q.n = m; q.rec0 = p->first_record + k0;
        if (!s.host) {
            q.pose = s.pose + 3 * k0;
            q.agent = s.agent ? s.agent + k0 : nullptr; q.enc = s.enc ? s.enc + k0 : nullptr;
            q.v2v = s.v2v ? s.v2v + k0 : nullptr; q.lm = s.lm ? s.lm + k0 : nullptr;
            q.ranges = s.ranges ? s.ranges + k0 * s.beams : nullptr; q.hit_cell = s.hit_cell ? s.hit_cell + k0 * s.beams : nullptr;
            q.pkts = s.pkts ? s.pkts + k0 * s.stride : nullptr;
            HIPCHK(c, qs_launch_sense(c, s, q));
            continue;
        }
        HIPCHK(c, c->io_ws.reserve(sense_stage(nullptr, s, m).bytes, c->stream, QS_IO_WS_FLOOR));
        const SnStage t = sense_stage(c->io_ws.p, s, m);
        HIPCHK(c, hipMemcpyAsync(t.pose, s.pose + 3 * k0, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
        q.pose = t.pose; q.agent = nullptr; q.enc = nullptr; q.v2v = nullptr; q.lm = nullptr;
        if (s.kind != SN_RANGES) {
            HIPCHK(c, hipMemcpyAsync(t.agent, s.agent + k0, m, hipMemcpyHostToDevice, c->stream));
            q.agent = t.agent;
            if (s.enc) { HIPCHK(c, hipMemcpyAsync(t.enc, s.enc + k0, 4 * m, hipMemcpyHostToDevice, c->stream)); q.enc = t.enc; }
            if (s.v2v) { HIPCHK(c, hipMemcpyAsync(t.v2v, s.v2v + k0, 4 * m, hipMemcpyHostToDevice, c->stream)); q.v2v = t.v2v; }
            if (s.lm) { HIPCHK(c, hipMemcpyAsync(t.lm, s.lm + k0, m, hipMemcpyHostToDevice, c->stream)); q.lm = t.lm; }
        }
        q.ranges = t.ranges; q.hit_cell = s.hit_cell ? t.hit_cell : nullptr; q.pkts = t.pkts;
        HIPCHK(c, qs_launch_sense(c, s, q));
        if (s.kind != SN_RANGES)
            HIPCHK(c, hipMemcpyAsync(s.pkts + k0 * s.stride, t.pkts, m * s.stride, hipMemcpyDeviceToHost, c->stream));
        else {
            HIPCHK(c, hipMemcpyAsync(s.ranges + k0 * s.beams, t.ranges, m * s.beams * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            if (s.hit_cell)
                HIPCHK(c, hipMemcpyAsync(s.hit_cell + k0 * s.beams, t.hit_cell, m * s.beams * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (s.host) HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

static int sense_ranges(qs_ctx *c, bool host, const char *who, const float *pose, size_t n, int32_t beams, const qs_sense_params *p,
                        float *ranges, int32_t *hit_cell)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pose != nullptr && ranges != nullptr));
    SnCall s{SN_RANGES, host, who, pose, nullptr, nullptr, nullptr, nullptr, n, beams, ranges, hit_cell, nullptr, 0};
    return sense_run(c, s, p);
}
static int sense_sweeps(qs_ctx *c, bool host, const char *who, const float *pose, const uint8_t *agent, const int32_t *enc,
                        const uint32_t *v2v, size_t n, const qs_sense_params *p, uint8_t *pkts, size_t stride)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pose != nullptr && agent != nullptr && pkts != nullptr));
    SnCall s{SN_SWEEPS, host, who, pose, agent, enc, v2v, nullptr, n, QS_SWEEP_BEAMS, nullptr, nullptr, pkts, stride};
    return sense_run(c, s, p);
}
static int sense_packets(qs_ctx *c, bool host, const char *who, const float *pose, const uint8_t *agent, const int32_t *enc,
                         const uint32_t *v2v, const uint8_t *lm, size_t n, const qs_sense_params *p, uint8_t *pkts)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pose != nullptr && agent != nullptr && pkts != nullptr));
    SnCall s{SN_PACKETS, host, who, pose, agent, enc, v2v, lm, n, 4, nullptr, nullptr, pkts, QS_PACKET_SIZE};
    return sense_run(c, s, p);
}

// ---- C ABI (semantics in include/quasar_slam.h, "sensing a world") ------------------------------------------------------------
extern "C" int qs_sense_ranges(qs_ctx *c, const float *pose_xyyaw, size_t n, int32_t beams, const qs_sense_params *params, float *ranges,
                               int32_t *hit_cell)
{
    return sense_ranges(c, true, "qs_sense_ranges", pose_xyyaw, n, beams, params, ranges, hit_cell);
}

extern "C" int qs_sense_ranges_device(qs_ctx *c, const float *d_pose_xyyaw, size_t n, int32_t beams, const qs_sense_params *params,
                                      float *d_ranges, int32_t *d_hit_cell)
{
    return sense_ranges(c, false, "qs_sense_ranges_device", d_pose_xyyaw, n, beams, params, d_ranges, d_hit_cell);
}

extern "C" int qs_sense_sweeps(qs_ctx *c, const float *pose_xyyaw, const uint8_t *agent, const int32_t *enc, const uint32_t *v2v, size_t n,
                               const qs_sense_params *params, uint8_t *pkts_out, size_t stride)
{
    return sense_sweeps(c, true, "qs_sense_sweeps", pose_xyyaw, agent, enc, v2v, n, params, pkts_out, stride);
}

extern "C" int qs_sense_sweeps_device(qs_ctx *c, const float *d_pose_xyyaw, const uint8_t *d_agent, const int32_t *d_enc,
                                      const uint32_t *d_v2v, size_t n, const qs_sense_params *params, uint8_t *d_pkts_out, size_t stride)
{
    return sense_sweeps(c, false, "qs_sense_sweeps_device", d_pose_xyyaw, d_agent, d_enc, d_v2v, n, params, d_pkts_out, stride);
}

extern "C" int qs_sense_packets(qs_ctx *c, const float *pose_xyyaw, const uint8_t *agent, const int32_t *enc, const uint32_t *v2v,
                                const uint8_t *landmark, size_t n, const qs_sense_params *params, uint8_t *pkts_out)
{
    return sense_packets(c, true, "qs_sense_packets", pose_xyyaw, agent, enc, v2v, landmark, n, params, pkts_out);
}

extern "C" int qs_sense_packets_device(qs_ctx *c, const float *d_pose_xyyaw, const uint8_t *d_agent, const int32_t *d_enc,
                                       const uint32_t *d_v2v, const uint8_t *d_landmark, size_t n, const qs_sense_params *params,
                                       uint8_t *d_pkts_out)
{
    return sense_packets(c, false, "qs_sense_packets_device", d_pose_xyyaw, d_agent, d_enc, d_v2v, d_landmark, n, params, d_pkts_out);
}
