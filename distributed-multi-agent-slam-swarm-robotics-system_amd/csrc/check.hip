// check.hip -- servo sweeps checked against the map they are about to be written into (include/quasar_slam.h, "sweep check",
// V1-V9): every beam is predicted from the map by sense.hip's walk and compared with the range the record carries.
//
// One 64-lane workgroup (= one wave) per record, as qs_sense_sweep_kernel.  The wave stages the record as the sweep mapper does
// (sweep_common.h), forms the ingest's pose and loads the (2 C + 1)^2 patch around the start cell, C = ceil(smax / res) + 1,
// reading the stamp rows coalesced and nothing outside the grid.  The patch is packed to TWO bits a cell, one ballot each per 64
// cells: plane 0 "not FREE" (UNKNOWN, OCCUPIED, off-grid), plane 1 "OCCUPIED"; rows of 64-bit words in LDS.  Each lane then takes
// beams lane, lane + 64, lane + 128 and walks its line over plane 0 -- the line stays in the box its two ends span, so it stays in
// the patch -- and reads plane 1 once, where the walk ends.  The class counts are ballots and popcounts; lane 0 writes the 56
// bytes of the result.  No global atomics, no device-side waits; the kernel writes nothing but the caller's outputs.
// The guarded ingest (qs_ingest_sweeps_checked*) is sweep.hip's, next to the matched ingest: it runs this kernel over the whole
// call and then the sweep kernels' VETO instantiations.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "sweep_common.h"

#define CK_HOST_CHUNK ((size_t)4096)           // records a host call stages at a time (about 3 MiB of sweeps, 1 MiB of results)
#define CK_DEVICE_CHUNK ((size_t)1 << 24)      // records per launch of a device call

struct QsCheckArgs {
    int C;                        // patch radius, ceil(smax / res) + 1
    double tol;
    int min_checked, max_bad_percent, count_missed;
    const double *tab;            // [2][181] cos, sin of (i - 90) * (pi / 180), the host's libm
    const unsigned int *stamps;
    qs_sweep_check *out;          // [n]
    unsigned char *cls;           // [n][181] or nullptr
};

// one bit of a plane of the wave's patch; the walk never leaves the patch (V4's bound on the far cell)
__device__ inline bool ck_bit(const unsigned long long *plane, int pw, int px, int py)
{
    return (plane[py * pw + (px >> 6)] >> (px & 63)) & 1ull;
}

// V6
__device__ inline int ck_class(bool hit, bool unknown, double p, bool ret, double d, double smin, double smax, double tol)
{
    if (hit) {
        if (ret) return d < p - tol ? QS_BEAM_NEARER : (d > p + tol ? QS_BEAM_FARTHER : QS_BEAM_AGREE);
        return (smin + tol < p && p <= smax - tol) ? QS_BEAM_MISSED : QS_BEAM_UNSEEN;
    }
    if (unknown) return (ret && d < p - tol) ? QS_BEAM_NEARER : QS_BEAM_UNSEEN;
    return ret ? QS_BEAM_NEARER : QS_BEAM_AGREE;                                                // clear
}

__global__ void __launch_bounds__(QS_WAVE)
qs_check_sweep_kernel(QsSweepArgs a, QsGeom geo, QsCheckArgs q)
{
    extern __shared__ unsigned long long s_planes[];     // [2][W][pw], W = 2 C + 1, the start cell in the middle; then the record
    const size_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const int W = 2 * q.C + 1, pw = (W + 63) >> 6;
    unsigned long long *s_nf = s_planes, *s_occ = s_planes + (size_t)W * pw;
    unsigned int *s_rec = (unsigned int *)(s_planes + 2 * (size_t)W * pw);
    sw_stage(a, k, s_rec, lane);
    __syncthreads();
    const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
    const SwHead h = sw_head(a, k, s_rec, mis);          // wave-uniform
    if (!h.ok) {
        if (lane == 0) { qs_sweep_check z; memset(&z, 0, sizeof z); z.status = QS_CHECK_NO_RECORD; q.out[k] = z; }
        if (q.cls)
            for (int i = lane; i < QS_SWEEP_BEAMS; i += QS_WAVE) q.cls[k * QS_SWEEP_BEAMS + i] = QS_BEAM_NO_RECORD;
        return;
    }
    // V2: the pose is usable when it is finite and has a start cell
    int x0 = 0, y0 = 0;
    bool usable = isfinite(h.rx) && isfinite(h.ry) && isfinite(h.yaw);
    if (usable) {
        usable = qs_w2g_i32(h.rx, geo.ox, geo, x0);
        usable = qs_w2g_i32(h.ry, geo.oy, geo, y0) && usable;
    }
    const int bx = x0 - q.C, by = y0 - q.C;              // |x0| <= 2^30
    double sn = 0.0, cs = 0.0;
    if (usable) {
        qs_sincos(h.yaw, &sn, &cs);                      // V3
        for (int py = 0; py < W; py++) {
            const int gy = by + py;
            const bool row_in = gy >= 0 && gy < geo.size;
            for (int w = 0; w < pw; w++) {
                const int px = 64 * w + lane, gx = bx + px;
                bool nf = true, occ = false;
                if (row_in && px < W && gx >= 0 && gx < geo.size) {
                    const unsigned int st = q.stamps[(size_t)gy * geo.size + gx];
                    occ = st & 1u;
                    nf = occ || st == 0u;                // V1
                }
                const unsigned long long m_nf = __ballot(nf), m_occ = __ballot(occ);
                if (lane == 0) { s_nf[py * pw + w] = m_nf; s_occ[py * pw + w] = m_occ; }
            }
        }
    }
    __syncthreads();
    int cnt[5] = {0, 0, 0, 0, 0};
    #pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = lane + QS_WAVE * t;
        int cls = -1;                                    // no beam: lanes 53..63 of the last round
        if (i < QS_SWEEP_BEAMS) {
            cls = QS_BEAM_UNSEEN;
            const double ci = cs * q.tab[i] - sn * q.tab[QS_SWEEP_BEAMS + i], si = sn * q.tab[i] + cs * q.tab[QS_SWEEP_BEAMS + i];
            const double ex = h.rx + a.smax * ci, ey = h.ry + a.smax * si;                          // V4
            int x1 = 0, y1 = 0;
            bool ok = usable && qs_w2g_i32(ex, geo.ox, geo, x1);
            ok = ok && qs_w2g_i32(ey, geo.oy, geo, y1);
            const long long ldx = llabs((long long)x1 - x0), ldy = llabs((long long)y1 - y0);
            if (ok && ldx <= q.C && ldy <= q.C) {
                const int dx = (int)ldx, dy = (int)ldy, sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;    // :161-164
                int x = x0, y = y0, err = dx - dy;
                bool stop = false;
                while (x != x1 || y != y1) {                                                       // cell 0 never ends the walk
                    const int e2 = 2 * err;
                    if (e2 > -dy) { err -= dy; x += sx; }
                    if (e2 < dx) { err += dx; y += sy; }
                    if (ck_bit(s_nf, pw, x - bx, y - by)) { stop = true; break; }
                }
                const bool hit = stop && ck_bit(s_occ, pw, x - bx, y - by);
                const long long hx = x - x0, hy = y - y0;
                const double p = geo.res * sqrt((double)(hx * hx + hy * hy));
                const double d = (double)__uint_as_float(sw_u32(s_rec, mis, a.ranges_off + 4u * (unsigned int)i));   // V5
                cls = ck_class(hit, stop && !hit, p, qs_range_rule(d, a.smin, a.smax).valid, d, a.smin, a.smax, q.tol);
            }
            if (q.cls) q.cls[k * QS_SWEEP_BEAMS + i] = (unsigned char)cls;
        }
        #pragma unroll
        for (int j = 0; j < 5; j++) cnt[j] += __popcll(__ballot(cls == j));
    }
    if (lane == 0) {                                     // V7
        qs_sweep_check r;
        memset(&r, 0, sizeof r);
        r.agree = cnt[QS_BEAM_AGREE]; r.nearer = cnt[QS_BEAM_NEARER]; r.farther = cnt[QS_BEAM_FARTHER];
        r.missed = cnt[QS_BEAM_MISSED]; r.unseen = cnt[QS_BEAM_UNSEEN];
        r.checked = r.agree + r.nearer + r.farther + r.missed;
        r.bad = r.nearer + r.farther + (q.count_missed ? r.missed : 0);
        r.status = r.checked < q.min_checked ? QS_CHECK_UNDECIDED
                 : (r.bad * 100 > q.max_bad_percent * r.checked ? QS_CHECK_CONTRADICTS : QS_CHECK_OK);
        r.accepted_record = 1;
        r.sin_yaw = sn; r.cos_yaw = cs;
        q.out[k] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// V8
int qs_check_setup(qs_ctx *c, const qs_check_params *params, const char *who, QsCheckSetup &cs)
{
    qs_check_params p = {2.0 * c->cfg.res, 20, 30, 0, 0};
    if (params) p = *params;
    char msg[256];
    const char *bad = nullptr;
    if (!(isfinite(p.tol) && p.tol >= 0)) bad = "tol must be finite and not negative";
    else if (p.min_checked < 0 || p.min_checked > QS_SWEEP_BEAMS) bad = "min_checked must lie in [0, 181]";
    else if (p.max_bad_percent < 0 || p.max_bad_percent > 100) bad = "max_bad_percent must lie in [0, 100]";
    else if (p.count_missed != 0 && p.count_missed != 1) bad = "count_missed must be 0 or 1";
    else if (p.reserved != 0) bad = "reserved must be 0";
    const double cells = ceil(c->sweep_max / c->cfg.res);
    if (!bad && !(cells + 1 <= (double)QS_SENSE_MAX_CELLS))
        bad = "the sweep filter's smax is too large for this resolution: ceil(smax / res) + 1 exceeds QS_SENSE_MAX_CELLS";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    cs.C = (int)cells + 1;
    cs.tol = p.tol; cs.min_checked = p.min_checked; cs.max_bad_percent = p.max_bad_percent; cs.count_missed = p.count_missed;
    return QS_OK;
}

hipError_t qs_launch_check(qs_ctx *c, const QsCheckSetup &cs, const unsigned char *d_pkts, size_t n, size_t stride,
                           const unsigned short *d_lens, qs_sweep_check *out, unsigned char *cls)
{
    if (n == 0) return hipSuccess;
    HIPRET(qs_beam_table(c));
    QsSweepArgs a;
    qs_sweep_args(c, d_pkts, n, stride, d_lens, QS_SWEEP_NO_GRAPH, a);
    QsCheckArgs q;
    q.C = cs.C; q.tol = cs.tol; q.min_checked = cs.min_checked; q.max_bad_percent = cs.max_bad_percent; q.count_missed = cs.count_missed;
    q.tab = c->match_tab.p; q.stamps = c->d_stamps.p;
    const size_t W = 2 * (size_t)cs.C + 1, pw = (W + 63) >> 6;
    const size_t lds = 2 * W * pw * 8 + SW_DW * sizeof(unsigned int);
    if (lds > 32 * 1024)                                           // the longest reaches: 66 176 bytes of the CU's 160 KiB at C = 255
        HIPRET(hipFuncSetAttribute((const void *)qs_check_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (size_t k0 = 0; k0 < n; k0 += CK_DEVICE_CHUNK) {
        const size_t m = std::min(CK_DEVICE_CHUNK, n - k0);
        a.pkts = d_pkts + k0 * stride; a.n = m; a.lens = d_lens ? d_lens + k0 : nullptr;
        q.out = out + k0; q.cls = cls ? cls + k0 * QS_SWEEP_BEAMS : nullptr;
        hipLaunchKernelGGL(qs_check_sweep_kernel, dim3((unsigned int)m), dim3(QS_WAVE), lds, c->stream, a, c->geom, q);
        HIPRET(hipGetLastError());
    }
    return hipSuccess;
}

// ---- C ABI: sweep check (semantics in include/quasar_slam.h; the guarded ingest is sweep.hip's) --------------------------------
extern "C" int qs_check_sweeps_device(qs_ctx *c, const qs_check_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                      const uint16_t *d_lens, qs_sweep_check *d_out, uint8_t *d_cls_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (d_pkts != nullptr && d_out != nullptr));
    QsCheckSetup cs;
    int rc = qs_check_setup(c, params, "qs_check_sweeps", cs);
    if (rc != QS_OK) return rc;
    rc = qs_sweep_call_ok(c, n, stride, "qs_check_sweeps");
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);                                            // V1: waiting edge rays go into the map first
    HIPCHK(c, qs_launch_check(c, cs, d_pkts, n, stride, d_lens, d_out, d_cls_out));
    return QS_OK;
}

extern "C" int qs_check_sweeps(qs_ctx *c, const qs_check_params *params, const uint8_t *pkts, size_t n, size_t stride,
                               const uint16_t *lens, qs_sweep_check *out, uint8_t *cls_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pkts != nullptr && out != nullptr));
    QsCheckSetup cs;
    int rc = qs_check_setup(c, params, "qs_check_sweeps", cs);
    if (rc != QS_OK) return rc;
    rc = qs_sweep_call_ok(c, n, stride, "qs_check_sweeps");
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    // staged CK_HOST_CHUNK records at a time (stream-ordered: the previous chunk's copies out have read the blocks)
    for (size_t k0 = 0; k0 < n; k0 += CK_HOST_CHUNK) {
        const size_t m = std::min(CK_HOST_CHUNK, n - k0);
        Staging s;
        rc = reserve_staging(c, m * stride, s);
        if (rc != QS_OK) return rc;
        Carve cv(nullptr);
        cv.take<qs_sweep_check>(m);
        if (cls_out) cv.take<uint8_t>(m * QS_SWEEP_BEAMS);
        HIPCHK(c, c->io_ws.reserve(cv.bytes, c->stream, QS_IO_WS_FLOOR));
        Carve io(c->io_ws.p);
        qs_sweep_check *d_out = io.take<qs_sweep_check>(m);
        uint8_t *d_cls = cls_out ? io.take<uint8_t>(m * QS_SWEEP_BEAMS) : nullptr;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, m * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, m * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_check(c, cs, s.pkts, m, stride, lens ? s.lens : nullptr, d_out, d_cls));
        HIPCHK(c, hipMemcpyAsync(out + k0, d_out, m * sizeof(qs_sweep_check), hipMemcpyDeviceToHost, c->stream));
        if (cls_out)
            HIPCHK(c, hipMemcpyAsync(cls_out + k0 * QS_SWEEP_BEAMS, d_cls, m * QS_SWEEP_BEAMS, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_last_sweep_checks(qs_ctx *c, qs_sweep_check *out, size_t n)
{
    ARGCHK(c, c != nullptr);
    if (!c->last_checks || n != c->last_checks_n)
        return qs_fail(c, QS_E_INVAL, "qs_last_sweep_checks: n does not match the last guarded sweep ingest");
    if (n == 0) return QS_OK;
    ARGCHK(c, out != nullptr);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->check_out.p, n * sizeof(qs_sweep_check), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}
