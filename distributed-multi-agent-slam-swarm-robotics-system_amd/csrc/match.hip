// match.hip -- servo sweeps matched against the map before they are mapped (include/quasar_slam.h, "sweep matching"): a window
// of candidate poses (ix, iy cells, it angle steps) around the packet's pose, scored on a likelihood field of the occupied
// cells; the best candidate is the sweep's correction.
//
// One WORKGROUP (4 waves) per sweep, everything it touches in LDS.  The window search is window_match.h's, shared with the trail
// matcher (trail.hip); what is the sweep's own:
//   1. wave 0 stages the record as the sweep mapper does (sweep_common.h);
//   2. the patch of the field the sweep can reach about the robot's cell, half = ceil(smax / res) + 1 + W (wm_build_patch).  No
//      whole-grid field exists: nothing persistent, nothing to invalidate;
//   3. every wave holds all 181 beams (sw_beams: the trig from the host's table) and takes rotations wave, wave + 4, ...: one
//      sincos per rotation, reported in `rot`, and the end points of the hit beams into the rotation's list (wm_list);
//   4. scores, the best key and the gate (wm_best, wm_result).
// qs_match_field_kernel is the plain whole-grid form of the field for tests and tools.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "sweep_common.h"
#include "window_match.h"

#define MT_OFFP 184               // 16-bit offsets per rotation: >= 181, a multiple of 4 (8-byte reads)
#define MT_CHUNK ((size_t)1 << 16)   // records per launch of the host-side call (its results and rotations travel per chunk)

struct QsMatchArgs {
    WmArgs w;
    const double *tab;            // [2][181] cos, sin of (i - 90) * (pi / 180), the host's libm
    qs_sweep_match *out;          // [n]
    double *rot;                  // [n][2 T + 1][2] or nullptr
};

__global__ void __launch_bounds__(WM_BLOCK)
qs_match_kernel(QsSweepArgs a, QsGeom geo, QsMatchArgs m)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ unsigned int s_rec[SW_DW];
    __shared__ int s_cnt[WM_NROT_MAX];
    __shared__ unsigned long long s_key[WM_NW];
    __shared__ int s_score0;
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const size_t k = blockIdx.x;
    const int nrot = 2 * m.w.T + 1;
    if (wave == 0) sw_stage(a, k, s_rec, lane);
    __syncthreads();
    const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
    const SwHead h = sw_head(a, k, s_rec, mis);
    if (!h.ok) {                                                   // (uniform over the workgroup)
        if (tid == 0) { qs_sweep_match z; memset(&z, 0, sizeof z); m.out[k] = z; }
        if (m.rot) for (int j = tid; j < 2 * nrot; j += WM_BLOCK) m.rot[k * 2 * (size_t)nrot + j] = 0.0;
        return;
    }
    unsigned int *A = (unsigned int *)s_dyn, *B = (unsigned int *)(s_dyn + m.w.off_b);
    const WmPatch p = wm_build_patch(m.w, geo, h.rx, h.ry, m.w.half, A, B, tid);

    // ---- beams, and per rotation the patch offsets of the hit beams' cells ---------------------------------------------------
    unsigned short *OFF = (unsigned short *)B;
    bool hit[3];
    double bx[3], by[3];
    const int H = sw_beams(a, s_rec, mis, m.tab, lane, hit, bx, by);
    for (int ti = wave; ti < nrot; ti += WM_NW) {
        const double th = h.yaw + (double)(ti - m.w.T) * m.w.step;
        double s, c;
        qs_sincos(th, &s, &c);
        if (m.rot && lane == 0) { double *o = m.rot + (k * (size_t)nrot + ti) * 2; o[0] = s; o[1] = c; }
        int cnt = 0;
        #pragma unroll
        for (int q = 0; q < 3; q++)
            wm_list(p, geo, hit[q], h.rx + (c * bx[q] - s * by[q]), h.ry + (s * bx[q] + c * by[q]), OFF + ti * MT_OFFP, cnt, lane);
        if (lane == 0) s_cnt[ti] = cnt;
    }
    __syncthreads();

    const unsigned long long best = wm_best(p, A, OFF, MT_OFFP, s_cnt, s_key, &s_score0, tid);
    if (tid == 0) {
        qs_sweep_match r;
        memset(&r, 0, sizeof r);
        wm_result(m.w, geo.res, best, s_score0, H, r);
        r.accepted_record = 1;
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

int qs_match_reach_setup(qs_ctx *c, const char *who, const qs_match_params &p, double reach, const char *what, const char *expr,
                         QsMatchSetup &ms)
{
    char msg[256];
    if (!(reach + p.radius + 2 <= QS_MATCH_MAX_REACH))
        snprintf(msg, sizeof msg, "%s: %s is too large for this resolution: ceil(%s / res) + radius + 2 exceeds QS_MATCH_MAX_REACH", who, what, expr);
    else if (reach + p.window + p.radius + 2 > QS_MATCH_MAX_REACH)
        snprintf(msg, sizeof msg, "%s: window is too large: ceil(%s / res) + window + radius + 2 exceeds QS_MATCH_MAX_REACH", who, expr);
    else {
        ms = QsMatchSetup{p.radius, p.window, p.angle_steps, p.min_hits, p.min_percent, (int)reach, p.angle_step};
        return QS_OK;
    }
    return qs_fail(c, QS_E_INVAL, msg);
}

int qs_match_setup(qs_ctx *c, const qs_match_params *params, const char *who, QsMatchSetup &ms)
{
    qs_match_params p;
    char msg[256];
    const char *bad = qs_match_params_check(params, p);
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    return qs_match_reach_setup(c, who, p, ceil(c->sweep_max / c->cfg.res), "the sweep filter's smax", "smax", ms);
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
    size_t lds;
    HIPRET(wm_args(c, ms, (const void *)qs_match_kernel, MT_OFFP, m.w, lds));
    m.tab = c->match_tab.p; m.out = out; m.rot = rot;
    hipLaunchKernelGGL(qs_match_kernel, dim3((unsigned int)n), dim3(WM_BLOCK), lds, c->stream, a, c->geom, m);
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
