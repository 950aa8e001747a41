// match.hip -- servo sweeps matched against the map before they are mapped (include/quasar_slam.h, "sweep matching"): a window
// of candidate poses (ix, iy cells, it angle steps) around the packet's pose, scored on a likelihood field of the occupied
// cells; the best candidate is the sweep's correction.
//
// One WORKGROUP (4 waves) per sweep, everything it touches in LDS:
//   1. wave 0 stages the record as the sweep mapper does (sweep_common.h);
//   2. the patch of the field the sweep can reach -- the robot's cell +- (ceil(smax / res) + 1 + W) cells, plus an apron of R
//      cells -- is read from the stamps as bytes (OCCUPIED = odd stamp -> R + 1, anything else and off-grid -> 0) and grown
//      by R rounds of a separable 3-wide max that loses 1 per round: L = max(0, R + 1 - Chebyshev distance).  The rounds work
//      on dwords (four cells a lane); a patch that hangs over the grid's edge is cut back to the grid afterwards.  No
//      whole-grid field exists: nothing persistent, nothing to invalidate.  The routine is field_patch.h's, shared with the
//      relocaliser (reloc.hip);
//   3. every wave holds all 181 beams (three a lane: d, hit flag, d * cos, d * sin of the beam angle, the trig from the
//      host's table) and takes rotations wave, wave + 4, ...: one sincos per rotation, the end-point cells of the hit beams,
//      compacted by ballot into the rotation's list of 16-bit patch offsets (the offset of candidate ix = iy = -W);
//   4. a lane takes (rotation, iy, FOUR adjacent ix): per beam two dword reads and a v_alignbyte give the four look-ups,
//      which are summed as bytes (255 / (R + 1) beams at a time cannot overflow one) and spilled into 16-bit sums; the
//      offsets are read four beams at a time (one 8-byte read).  Per four look-ups: 2.25 LDS reads and about six VALU
//      instructions;
//   5. the total order of the rule is one 64-bit key: max by shuffles within the wave, LDS across the four waves.
// qs_match_field_kernel is the plain whole-grid form of step 2 for tests and tools.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "sweep_common.h"
#include "field_patch.h"

#define MT_BLOCK 256
#define MT_NW (MT_BLOCK / QS_WAVE)
#define MT_OFFP 184               // 16-bit offsets per rotation: >= 181, a multiple of 4 (8-byte reads)
#define MT_NROT_MAX (2 * QS_MATCH_MAX_ANGLE_STEPS + 1)
#define MT_CHUNK ((size_t)1 << 16)   // records per launch of the host-side call (its results and rotations travel per chunk)

struct QsMatchArgs {
    int R, W, T, min_hits, min_percent;
    int half;                     // patch: the robot's cell +- half, half = reach + 1 + W
    int SA, pitch;                // side with the apron (2 (half + R) + 1) and bytes per row (a multiple of 4, an odd number of dwords)
    unsigned int off_b;           // byte offset of the second LDS region (dilation scratch, then the offset lists)
    double step;
    const double *tab;            // [2][181] cos, sin of (i - 90) * (pi / 180), the host's libm
    const unsigned int *stamps;
    qs_sweep_match *out;          // [n]
    double *rot;                  // [n][2 T + 1][2] or nullptr
};

__global__ void __launch_bounds__(MT_BLOCK)
qs_match_kernel(QsSweepArgs a, QsGeom geo, QsMatchArgs m)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ unsigned int s_rec[SW_DW];
    __shared__ int s_cnt[MT_NROT_MAX];
    __shared__ unsigned long long s_key[MT_NW];
    __shared__ int s_score0;
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const size_t k = blockIdx.x;
    const int nrot = 2 * m.T + 1;
    if (wave == 0) sw_stage(a, k, s_rec, lane);
    __syncthreads();
    const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
    const SwHead h = sw_head(a, k, s_rec, mis);
    if (!h.ok) {                                                   // (uniform over the workgroup)
        if (tid == 0) { qs_sweep_match z; memset(&z, 0, sizeof z); m.out[k] = z; }
        if (m.rot) for (int j = tid; j < 2 * nrot; j += MT_BLOCK) m.rot[k * 2 * (size_t)nrot + j] = 0.0;
        return;
    }

    // ---- the patch of the field ------------------------------------------------------------------------------------------
    unsigned int *A = (unsigned int *)s_dyn, *B = (unsigned int *)(s_dyn + m.off_b);
    int c0x = 0, c0y = 0;
    bool c0ok = qs_w2g_i32(h.rx, geo.ox, geo, c0x);
    c0ok = qs_w2g_i32(h.ry, geo.oy, geo, c0y) && c0ok;
    if (!c0ok) { c0x = 0; c0y = 0; }                               // (no beam of such a pose has a cell: nothing reads the patch)
    const int gx0 = c0x - m.half - m.R, gy0 = c0y - m.half - m.R;  // grid cell of patch byte (0, 0); |c0| <= 2^30
    mt_build_patch(A, B, m.stamps, geo.size, gx0, gy0, m.SA, m.pitch, m.R, tid, MT_BLOCK);

    // ---- beams, and per rotation the patch offsets of the hit beams' cells ---------------------------------------------------
    unsigned short *OFF = (unsigned short *)B;
    bool hit[3];
    double bx[3], by[3];
    int H = 0;
    #pragma unroll
    for (int q = 0; q < 3; q++) {
        const int i = lane + QS_WAVE * q;
        hit[q] = false; bx[q] = 0.0; by[q] = 0.0;
        if (i < QS_SWEEP_BEAMS) {
            const double d = (double)__uint_as_float(sw_u32(s_rec, mis, a.ranges_off + 4u * (unsigned int)i));
            hit[q] = qs_range_rule(d, a.smin, a.smax).valid;
            bx[q] = d * m.tab[i];
            by[q] = d * m.tab[QS_SWEEP_BEAMS + i];
        }
        H += __popcll(__ballot(hit[q]));
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int lo_ok = m.R + m.W, hi_ok = m.SA - 1 - m.R - m.W;     // a cell every shift of which stays inside the exact part
    for (int ti = wave; ti < nrot; ti += MT_NW) {
        const double th = h.yaw + (double)(ti - m.T) * m.step;
        double s, c;
        qs_sincos(th, &s, &c);
        if (m.rot && lane == 0) { double *o = m.rot + (k * (size_t)nrot + ti) * 2; o[0] = s; o[1] = c; }
        int cnt = 0;
        #pragma unroll
        for (int q = 0; q < 3; q++) {
            bool in = false;
            unsigned int off = 0;
            if (hit[q]) {
                const double ex = h.rx + (c * bx[q] - s * by[q]), ey = h.ry + (s * bx[q] + c * by[q]);
                int cx, cy;
                bool ok = qs_w2g_i32(ex, geo.ox, geo, cx);
                ok = qs_w2g_i32(ey, geo.oy, geo, cy) && ok;
                if (ok && c0ok) {
                    const long long ax = (long long)cx - gx0, ay = (long long)cy - gy0;
                    in = ax >= lo_ok && ax <= hi_ok && ay >= lo_ok && ay <= hi_ok;
                    off = (unsigned int)((ay - m.W) * m.pitch + (ax - m.W));
                }
            }
            const unsigned long long bal = __ballot(in);
            if (in) OFF[ti * MT_OFFP + cnt + __popcll(bal & lt)] = (unsigned short)off;
            cnt += __popcll(bal);
        }
        if (lane == 0) s_cnt[ti] = cnt;
    }
    __syncthreads();

    // ---- scores: a lane per (rotation, iy, four ix) --------------------------------------------------------------------------
    // (qs_trail_kernel, trail.hip, restates this loop over a trail's points: a change here belongs there too)
    const int ny = 2 * m.W + 1, G = (ny + 3) >> 2, per_rot = ny * G, NI = nrot * per_rot;
    const int span = (255 / (m.R + 1)) & ~3;                       // beams whose byte sums cannot overflow
    unsigned long long best = 0;
    for (int j = tid; j < NI; j += MT_BLOCK) {
        const int ti = j / per_rot, rem = j - ti * per_rot, yi = rem / G, g = rem - yi * G;
        const unsigned int lane_off = (unsigned int)(yi * m.pitch + 4 * g);
        const unsigned short *o = OFF + ti * MT_OFFP;
        const int cnt = s_cnt[ti];
        unsigned int lo = 0, hi = 0;
        for (int b0 = 0; b0 < cnt; b0 += span) {
            const int b1 = min(b0 + span, cnt);
            unsigned int acc = 0;
            int b = b0;
            for (; b + 4 <= b1; b += 4) {
                const uint2 q = *(const uint2 *)(o + b);
                acc += mt_look(A, lane_off + (q.x & 0xffffu));
                acc += mt_look(A, lane_off + (q.x >> 16));
                acc += mt_look(A, lane_off + (q.y & 0xffffu));
                acc += mt_look(A, lane_off + (q.y >> 16));
            }
            for (; b < b1; b++) acc += mt_look(A, lane_off + o[b]);
            lo += acc & 0x00ff00ffu;
            hi += (acc >> 8) & 0x00ff00ffu;
        }
        const unsigned int sc[4] = {lo & 0xffffu, hi & 0xffffu, lo >> 16, hi >> 16};
        const int it = ti - m.T, iy = yi - m.W;
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            const int ix = 4 * g + e - m.W;
            if (ix > m.W) break;
            // score, then small ix^2 + iy^2, small |it|, small it, small iy, small ix: every field "larger is better"
            const unsigned long long key = ((unsigned long long)sc[e] << 45) | ((unsigned long long)(32767 - (ix * ix + iy * iy)) << 30)
                                         | ((unsigned long long)(m.T - abs(it)) << 23) | ((unsigned long long)(m.T - it) << 16)
                                         | ((unsigned long long)(m.W - iy) << 8) | (unsigned long long)(m.W - ix);
            best = key > best ? key : best;
            if (it == 0 && iy == 0 && ix == 0) s_score0 = (int)sc[e];
        }
    }
    #pragma unroll
    for (int d = QS_WAVE / 2; d > 0; d >>= 1) {
        const unsigned long long other = __shfl_xor(best, d);
        best = other > best ? other : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < MT_NW; w++) best = s_key[w] > best ? s_key[w] : best;
        qs_sweep_match r;
        memset(&r, 0, sizeof r);
        r.ix = m.W - (int)(best & 255u);
        r.iy = m.W - (int)((best >> 8) & 255u);
        r.it = m.T - (int)((best >> 16) & 127u);
        r.score = (int)(best >> 45);
        r.score0 = s_score0;
        r.hits = H;
        r.accepted_record = 1;
        r.accepted_match = H >= m.min_hits && (long long)r.score * 100 >= (long long)m.min_percent * H * (m.R + 1);
        if (r.accepted_match) { r.dx = (double)r.ix * geo.res; r.dy = (double)r.iy * geo.res; r.dyaw = (double)r.it * m.step; }
        m.out[k] = r;
    }
}

// rule 1 over the whole grid, a cell per thread
__global__ void __launch_bounds__(256)
qs_match_field_kernel(const unsigned int *__restrict__ stamps, int size, int R, unsigned char *__restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= size || y >= size) return;
    int best = 0;
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++) {
            const int gx = x + dx, gy = y + dy;
            if (gx >= 0 && gx < size && gy >= 0 && gy < size && mt_occupied(stamps[(size_t)gy * size + gx]))
                best = max(best, R + 1 - max(abs(dx), abs(dy)));
        }
    out[(size_t)y * size + x] = (unsigned char)best;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
const char *qs_match_params_check(const qs_match_params *params, qs_match_params &p)
{
    p = qs_match_params{2, 6, 10, 20, 50, 0, 3.141592653589793 / 180.0};
    if (params) p = *params;
    if (p.radius < 0 || p.radius > QS_MATCH_MAX_RADIUS) return "radius must lie in [0, QS_MATCH_MAX_RADIUS]";
    if (p.window < 0) return "window must not be negative";
    if (p.angle_steps < 0 || p.angle_steps > QS_MATCH_MAX_ANGLE_STEPS) return "angle_steps must lie in [0, QS_MATCH_MAX_ANGLE_STEPS]";
    if (p.min_hits < 0) return "min_hits must not be negative";
    if (p.min_percent < 0 || p.min_percent > 100) return "min_percent must lie in [0, 100]";
    if (!(isfinite(p.angle_step) && p.angle_step >= 0)) return "angle_step must be finite and not negative";
    return nullptr;
}

int qs_match_setup(qs_ctx *c, const qs_match_params *params, const char *who, QsMatchSetup &ms)
{
    qs_match_params p;
    char msg[256];
    const char *bad = qs_match_params_check(params, p);
    const double reach = ceil(c->sweep_max / c->cfg.res);
    if (!bad && !(reach + p.radius + 2 <= QS_MATCH_MAX_REACH))
        bad = "the sweep filter's smax is too large for this resolution: ceil(smax / res) + radius + 2 exceeds QS_MATCH_MAX_REACH";
    else if (!bad && reach + p.window + p.radius + 2 > QS_MATCH_MAX_REACH)
        bad = "window is too large: ceil(smax / res) + window + radius + 2 exceeds QS_MATCH_MAX_REACH";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    ms.R = p.radius; ms.W = p.window; ms.T = p.angle_steps; ms.min_hits = p.min_hits; ms.min_percent = p.min_percent;
    ms.reach = (int)reach; ms.step = p.angle_step;
    return QS_OK;
}

int qs_sweep_call_ok(qs_ctx *c, size_t n, size_t stride, const char *who)
{
    char msg[256];
    const char *bad = nullptr;
    if (stride != QS_SWEEP_SIZE_V0 && stride != QS_SWEEP_SIZE_V0_ODO) bad = "stride must be 743 (v0) or 751 (v0 + odometry)";
    else if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0) bad = "sharded contexts (seq_stride > 1, shard_bots > 0) do not take sweeps";
    else if (n >= ((size_t)1 << 31)) bad = "at most 2^31 - 1 records per call";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    return QS_OK;
}

hipError_t qs_beam_table(qs_ctx *c)
{
    if (c->match_tab.p) return hipSuccess;                         // the beam angles' cos / sin: libm's, once per context
    static const double kRad = 3.141592653589793 / 180.0;
    double tab[2 * QS_SWEEP_BEAMS];
    for (int i = 0; i < QS_SWEEP_BEAMS; i++) {
        const double b = (double)(i - 90) * kRad;
        tab[i] = cos(b); tab[QS_SWEEP_BEAMS + i] = sin(b);
    }
    HIPRET(c->match_tab.alloc(2 * QS_SWEEP_BEAMS));
    return hipMemcpy(c->match_tab.p, tab, sizeof tab, hipMemcpyHostToDevice);
}

hipError_t qs_launch_match(qs_ctx *c, const QsMatchSetup &ms, const unsigned char *d_pkts, size_t n, size_t stride,
                           const unsigned short *d_lens, qs_sweep_match *out, double *rot, size_t graph_k0)
{
    if (n == 0) return hipSuccess;
    HIPRET(qs_beam_table(c));
    QsSweepArgs a;
    qs_sweep_args(c, d_pkts, n, stride, d_lens, graph_k0, a);
    QsMatchArgs m;
    m.R = ms.R; m.W = ms.W; m.T = ms.T; m.min_hits = ms.min_hits; m.min_percent = ms.min_percent;
    m.half = ms.reach + 1 + ms.W;
    m.SA = 2 * (m.half + ms.R) + 1;                               // <= 255 (qs_match_setup)
    m.pitch = (m.SA + 3) & ~3;
    if (!((m.pitch >> 2) & 1)) m.pitch += 4;                       // an odd number of dwords a row: rows start on different banks
    const size_t a_bytes = ((size_t)m.SA * m.pitch + 16 + 15) & ~(size_t)15;
    const size_t b_bytes = std::max((size_t)m.SA * m.pitch, (size_t)(2 * ms.T + 1) * MT_OFFP * sizeof(unsigned short));
    m.off_b = (unsigned int)a_bytes;
    m.step = ms.step;
    m.tab = c->match_tab.p; m.stamps = c->d_stamps.p; m.out = out; m.rot = rot;
    const size_t lds = a_bytes + ((b_bytes + 15) & ~(size_t)15);
    if (lds > 32 * 1024)                                           // the largest windows: up to 2 x 65 KiB of the CU's 160
        HIPRET(hipFuncSetAttribute((const void *)qs_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(qs_match_kernel, dim3((unsigned int)n), dim3(MT_BLOCK), lds, c->stream, a, c->geom, m);
    return hipGetLastError();
}

// ---- C ABI: sweep matching (semantics in include/quasar_slam.h; the matched ingest is sweep.hip's, next to pass A) --------------
extern "C" int qs_match_field(qs_ctx *c, int32_t radius, uint8_t *field_host)
{
    ARGCHK(c, c != nullptr && field_host != nullptr);
    if (radius < 0 || radius > QS_MATCH_MAX_RADIUS)
        return qs_fail(c, QS_E_INVAL, "qs_match_field: radius must lie in [0, QS_MATCH_MAX_RADIUS]");
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->io_ws.reserve(c->cells, c->stream, QS_IO_WS_FLOOR));
    const int size = c->cfg.size;
    hipLaunchKernelGGL(qs_match_field_kernel, dim3((size + 63) / 64, (size + 3) / 4), dim3(256), 0, c->stream, c->d_stamps.p, size,
                       (int)radius, (unsigned char *)c->io_ws.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(field_host, c->io_ws.p, c->cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_match_sweeps_device(qs_ctx *c, const qs_match_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                      const uint16_t *d_lens, qs_sweep_match *d_out, double *d_rot_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (d_pkts != nullptr && d_out != nullptr));
    QsMatchSetup ms;
    int rc = qs_match_setup(c, params, "qs_match_sweeps", ms);
    if (rc != QS_OK) return rc;
    rc = qs_sweep_call_ok(c, n, stride, "qs_match_sweeps");
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, qs_launch_match(c, ms, d_pkts, n, stride, d_lens, d_out, d_rot_out, QS_SWEEP_NO_GRAPH));
    return QS_OK;
}

extern "C" int qs_match_sweeps(qs_ctx *c, const qs_match_params *params, const uint8_t *pkts, size_t n, size_t stride,
                               const uint16_t *lens, qs_sweep_match *out, double *rot_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pkts != nullptr && out != nullptr));
    QsMatchSetup ms;
    int rc = qs_match_setup(c, params, "qs_match_sweeps", ms);
    if (rc != QS_OK) return rc;
    rc = qs_sweep_call_ok(c, n, stride, "qs_match_sweeps");
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    const size_t rot_per = (size_t)(2 * ms.T + 1) * 2;
    for (size_t k0 = 0; k0 < n; k0 += MT_CHUNK) {
        const size_t m = std::min(MT_CHUNK, n - k0);
        Staging s;
        rc = reserve_staging(c, m * stride, s);
        if (rc != QS_OK) return rc;
        Carve cv(nullptr);
        cv.take<qs_sweep_match>(m);
        if (rot_out) cv.take<double>(m * rot_per);
        HIPCHK(c, c->io_ws.reserve(cv.bytes, c->stream, QS_IO_WS_FLOOR));
        Carve io(c->io_ws.p);
        qs_sweep_match *d_out = io.take<qs_sweep_match>(m);
        double *d_rot = rot_out ? io.take<double>(m * rot_per) : nullptr;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, m * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, m * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_match(c, ms, s.pkts, m, stride, lens ? s.lens : nullptr, d_out, d_rot, QS_SWEEP_NO_GRAPH));
        HIPCHK(c, hipMemcpyAsync(out + k0, d_out, m * sizeof(qs_sweep_match), hipMemcpyDeviceToHost, c->stream));
        if (rot_out) HIPCHK(c, hipMemcpyAsync(rot_out + k0 * rot_per, d_rot, m * rot_per * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return QS_OK;
}

extern "C" int qs_last_sweep_matches(qs_ctx *c, qs_sweep_match *out, size_t n)
{
    ARGCHK(c, c != nullptr);
    if (!c->last_matches || n != c->last_matches_n)
        return qs_fail(c, QS_E_INVAL, "qs_last_sweep_matches: n does not match the last matched sweep ingest");
    if (n == 0) return QS_OK;
    ARGCHK(c, out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->match_out.p, n * sizeof(qs_sweep_match), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}
