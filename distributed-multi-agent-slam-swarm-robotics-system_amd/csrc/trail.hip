// trail.hip -- trails of 42-byte packets matched against the map (include/quasar_slam.h, "trail matching"): the last K packets of
// one bot, held together rigidly by the bot's own odometry, form one constellation of at most 4 K hit points; a window of
// candidate corrections (ix, iy cells, it angle steps about the trail's last pose) is scored on the likelihood field of sweep
// matching, and the best candidate is the trail's correction.
//
// One WORKGROUP (4 waves) per trail, nothing kept between calls:
//   1. the group's records (at most 64 x 64 bytes) are staged into LDS as the packet decoder stages a tile (decode.hip): dword
//      loads widened to alignment, the dwords that straddle the caller's buffer read bytewise; strides beyond 64 bytes are read
//      per lane;
//   2. wave 0, a lane per record: parse and accept (qs_ingest's rule), the anchor by a ballot, the bot's drift and offset from
//      the device, one sincos per record, four points; the hits are compacted by ballot into an LDS list of (qx, qy);
//   3. the patch of the field about the anchor's cell (wm_build_patch).  The launch sizes the LDS for +- (ceil((max_dist +
//      travel) / res) + 1 + W) cells plus an apron of R; a trail builds only what its own points can reach, +- (ceil(rmax / res)
//      + 1 + W), rmax the largest distance of a point from the anchor;
//   4. every wave takes rotations wave, wave + 4, ...: the points turned about the anchor by the host's (S, C), into the
//      rotation's list (wm_list);
//   5. scores, the best key and the gate (wm_best, wm_result).  No atomics.
// Steps 3 to 5 are the window search of window_match.h, shared with the sweep matcher (match.hip).
#include <math.h>
#include <string.h>
#include <algorithm>

#include "trail_common.h"
#include "window_match.h"

#define TR_PTS (4 * QS_TRAIL_MAX_RECORDS)    // points of one trail, and 16-bit offsets per rotation (a multiple of 4: 8-byte reads)
#define TR_CHUNK 512                         // trails per launch: their first records travel in the kernel's arguments

struct QsTrailArgs {
    TrRecords r;                  // the launch's records
    const double *offset, *drift; // [max_agent + 1], [max_agent + 1][2]
    int max_agent;
    WmArgs w;
    double travel2;
    qs_trail_match *out;          // [groups of the launch]
    double *rot;                  // [nrec][2] or nullptr
    unsigned short start[TR_CHUNK + 1];       // first record of each group of the launch (at most 512 x 64 = 2^15 records)
    double sc[WM_NROT_MAX][2];    // (S, C) of it * angle_step, it = -T .. T, the host's libm
};

__global__ void __launch_bounds__(WM_BLOCK)
qs_trail_kernel(QsTrailArgs m, QsGeom geo)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ unsigned int s_raw[TR_RAW_DW];
    __shared__ double2 s_q[TR_PTS];
    __shared__ int s_cnt[WM_NROT_MAX];
    __shared__ unsigned long long s_key[WM_NW];
    __shared__ double s_anchor[4];                                  // ax, ay, the largest |q|^2 of a point, unused
    __shared__ int s_head[4];                                      // H, records, anchor, agent
    __shared__ int s_score0;
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const unsigned int grp = blockIdx.x;
    const size_t rec0 = m.start[grp];
    const int K = (int)m.start[grp + 1] - (int)m.start[grp];       // 1 .. 64
    const int nrot = 2 * m.w.T + 1;
    const bool staged = m.r.stride <= TR_MAX_STRIDE;

    // ---- stage: the byte range of the group's records widened to dword boundaries -------------------------------------------------
    const unsigned int mis = staged ? tr_stage(m.r, rec0, K, s_raw, tid, WM_BLOCK) : 0u;
    __syncthreads();

    // ---- wave 0: a lane per record ---------------------------------------------------------------------------------------------
    if (wave == 0) {
        bool ok = false;
        int agent = 0;
        float x = 0.f, y = 0.f, yaw = 0.f, dist[4] = {0.f, 0.f, 0.f, 0.f};
        if (lane < K)
            ok = tr_parse(m.r, m.max_agent, rec0 + lane, staged, s_raw, mis + (unsigned int)lane * (unsigned int)m.r.stride, agent, x, y, yaw, dist);
        const unsigned long long acc = __ballot(ok);
        const int anchor = acc ? 63 - __clzll((long long)acc) : -1;
        const int bot = anchor >= 0 ? __shfl(agent, anchor) : 0;
        double rx = 0.0, ry = 0.0;
        if (anchor >= 0) {                                         // T3: ONE offset and ONE drift for the whole trail
            rx = ((double)x + m.offset[bot]) + m.drift[2 * bot];
            ry = (double)y + m.drift[2 * bot + 1];
        }
        const double ax = __shfl(rx, anchor >= 0 ? anchor : 0), ay = __shfl(ry, anchor >= 0 ? anchor : 0);
        const double ddx = rx - ax, ddy = ry - ay;
        const bool counts = ok && agent == bot && ddx * ddx + ddy * ddy <= m.travel2;
        const unsigned long long cb = __ballot(counts);
        double s = 0.0, c = 0.0;
        if (counts) qs_sincos((double)yaw, &s, &c);
        if (m.rot && lane < K) { double *o = m.rot + (rec0 + lane) * 2; o[0] = s; o[1] = c; }
        // T5: front (c, s), left (-s, c), back (-c, -s), right (s, -c)
        const double ux[4] = {c, -s, -c, s}, uy[4] = {s, c, -s, -c};
        const unsigned long long lt = (1ull << lane) - 1ull;
        int H = 0;
        double r2 = 0.0;
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            const double d = (double)dist[j];
            const bool hit = counts && geo.min_dist < d && d <= geo.max_dist;
            const unsigned long long bal = __ballot(hit);
            if (hit) {
                const double px = rx + d * ux[j], py = ry + d * uy[j];
                const double2 q = make_double2(px - ax, py - ay);
                s_q[H + __popcll(bal & lt)] = q;
                r2 = fmax(r2, q.x * q.x + q.y * q.y);
            }
            H += __popcll(bal);
        }
        #pragma unroll
        for (int d = QS_WAVE / 2; d > 0; d >>= 1) r2 = fmax(r2, __shfl_xor(r2, d));
        if (lane == 0) {
            s_anchor[0] = ax; s_anchor[1] = ay; s_anchor[2] = r2;
            s_head[0] = H; s_head[1] = __popcll(cb); s_head[2] = anchor; s_head[3] = bot;
        }
    }
    __syncthreads();
    const int H = s_head[0], records = s_head[1];
    if (records == 0) {                                            // (uniform over the workgroup)
        if (tid == 0) { qs_trail_match z; memset(&z, 0, sizeof z); z.anchor = -1; m.out[grp] = z; }
        return;
    }
    const double ax = s_anchor[0], ay = s_anchor[1];

    // ---- the patch of the field about the anchor's cell ---------------------------------------------------------------------------
    // The launch sizes the LDS for the reach travel allows; THIS trail's points lie within rmax of its anchor under every
    // rotation, so the patch it builds is +- (ceil(rmax / res) + 1 + W) cells plus the apron, never more than the launch's.
    int half = m.w.half;
    const double need = ceil(sqrt(s_anchor[2]) / geo.res) + 1.0 + (double)m.w.W;
    if (need < (double)half) half = (int)need;                     // (not a number: the launch's)
    unsigned int *A = (unsigned int *)s_dyn, *B = (unsigned int *)(s_dyn + m.w.off_b);
    const WmPatch p = wm_build_patch(m.w, geo, ax, ay, half, A, B, tid);

    // ---- per rotation the patch offsets of the points' cells ------------------------------------------------------------------------
    unsigned short *OFF = (unsigned short *)B;
    for (int ti = wave; ti < nrot; ti += WM_NW) {
        const double S = m.sc[ti][0], C = m.sc[ti][1];
        int cnt = 0;
        for (int p0 = 0; p0 < H; p0 += QS_WAVE) {
            const bool live = p0 + lane < H;
            const double2 q = live ? s_q[p0 + lane] : make_double2(0.0, 0.0);
            wm_list(p, geo, live, ax + (C * q.x - S * q.y), ay + (S * q.x + C * q.y), OFF + ti * TR_PTS, cnt, lane);
        }
        if (lane == 0) s_cnt[ti] = cnt;
    }
    __syncthreads();

    const unsigned long long best = wm_best(p, A, OFF, TR_PTS, s_cnt, s_key, &s_score0, tid);
    if (tid == 0) {
        qs_trail_match r;
        memset(&r, 0, sizeof r);
        wm_result(m.w, geo.res, best, s_score0, H, r);
        r.records = records;
        r.anchor = s_head[2];
        r.agent = (uint8_t)s_head[3];
        r.ax = ax; r.ay = ay;
        m.out[grp] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct QsTrailSetup : QsMatchSetup { double travel; };

// T8 and T1: the limits of qs_match_params, the travel, the reach of the patch, the context, the groups
static int trail_setup(qs_ctx *c, const qs_match_params *params, size_t n, size_t stride, const int32_t *gsize, size_t n_groups,
                       double travel, QsTrailSetup &ts)
{
    static const char *who = "qs_match_trails";
    qs_match_params p;
    char msg[256];
    const char *bad = qs_match_params_check(params, p);            // the limits of qs_match_params: match.hip's
    if (!bad && !(isfinite(travel) && travel >= 0)) bad = "travel must be finite and not negative";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    const int rc = qs_match_reach_setup(c, who, p, ceil((c->cfg.max_dist + travel) / c->cfg.res), "max_dist + travel", "(max_dist + travel)", ts);
    if (rc != QS_OK) return rc;
    ts.travel = travel;
    if (stride < QS_PACKET_SIZE_V1) bad = "stride must be at least 41";
    else if (c->cfg.seq_stride > 1 || c->cfg.shard_bots > 0) bad = "sharded contexts (seq_stride > 1, shard_bots > 0) do not match trails";
    else if (n >= ((size_t)1 << 31)) bad = "at most 2^31 - 1 records per call";
    if (bad) { snprintf(msg, sizeof msg, "%s: %s", who, bad); return qs_fail(c, QS_E_INVAL, msg); }
    size_t sum = 0;
    for (size_t g = 0; g < n_groups; g++) {
        if (gsize[g] < 1 || gsize[g] > QS_TRAIL_MAX_RECORDS) {
            snprintf(msg, sizeof msg, "%s: gsize[%zu] must lie in [1, QS_TRAIL_MAX_RECORDS]", who, g);
            return qs_fail(c, QS_E_INVAL, msg);
        }
        sum += (size_t)gsize[g];
    }
    if (sum != n) { snprintf(msg, sizeof msg, "%s: the group sizes must sum to n", who); return qs_fail(c, QS_E_INVAL, msg); }
    return QS_OK;
}

// n_groups groups (gsize: host, already checked) of device-resident records against the map as the stream finds it; rot
// (optional): [records][2].  Everything enqueued, nothing waited for
static hipError_t trail_launch(qs_ctx *c, const QsTrailSetup &ts, const unsigned char *d_pkts, size_t stride, const unsigned short *d_lens,
                               const int32_t *gsize, size_t n_groups, qs_trail_match *d_out, double *d_rot)
{
    if (n_groups == 0) return hipSuccess;
    QsTrailArgs m;
    memset(&m, 0, sizeof m);
    m.r.stride = stride;
    m.offset = c->d_offset.p; m.drift = c->d_drift.p; m.max_agent = c->cfg.max_agent;
    size_t lds;
    HIPRET(wm_args(c, ts, (const void *)qs_trail_kernel, TR_PTS, m.w, lds));
    m.travel2 = ts.travel * ts.travel;
    for (int it = -ts.T; it <= ts.T; it++) {                       // T6: the host's libm
        const double th = (double)it * ts.step;
        m.sc[it + ts.T][0] = sin(th); m.sc[it + ts.T][1] = cos(th);
    }
    size_t rec0 = 0;
    for (size_t g0 = 0; g0 < n_groups; g0 += TR_CHUNK) {
        const unsigned int ng = (unsigned int)std::min((size_t)TR_CHUNK, n_groups - g0);
        unsigned int nr = 0;
        for (unsigned int i = 0; i <= TR_CHUNK; i++) {
            m.start[i] = (unsigned short)nr;
            if (i < ng) nr += (unsigned int)gsize[g0 + i];
        }
        m.r.pkts = d_pkts + rec0 * stride; m.r.lens = d_lens ? d_lens + rec0 : nullptr; m.r.nrec = nr;
        m.out = d_out + g0; m.rot = d_rot ? d_rot + 2 * rec0 : nullptr;
        hipLaunchKernelGGL(qs_trail_kernel, dim3(ng), dim3(WM_BLOCK), lds, c->stream, m, c->geom);
        HIPRET(hipGetLastError());
        rec0 += nr;
    }
    return hipSuccess;
}

// ---- C ABI: trail matching (semantics in include/quasar_slam.h) -------------------------------------------------------------------
extern "C" int qs_match_trails_device(qs_ctx *c, const qs_match_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                      const uint16_t *d_lens, const int32_t *gsize, size_t n_groups, double travel,
                                      qs_trail_match *d_out, double *d_rot_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || d_pkts != nullptr);
    ARGCHK(c, n_groups == 0 || (gsize != nullptr && d_out != nullptr));
    QsTrailSetup ts;
    const int rc = trail_setup(c, params, n, stride, gsize, n_groups, travel, ts);
    if (rc != QS_OK || n_groups == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, trail_launch(c, ts, d_pkts, stride, d_lens, gsize, n_groups, d_out, d_rot_out));
    return QS_OK;
}

extern "C" int qs_match_trails(qs_ctx *c, const qs_match_params *params, const uint8_t *pkts, size_t n, size_t stride,
                               const uint16_t *lens, const int32_t *gsize, size_t n_groups, double travel, qs_trail_match *out,
                               double *rot_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || pkts != nullptr);
    ARGCHK(c, n_groups == 0 || (gsize != nullptr && out != nullptr));
    QsTrailSetup ts;
    int rc = trail_setup(c, params, n, stride, gsize, n_groups, travel, ts);
    if (rc != QS_OK || n_groups == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    size_t k0 = 0;
    for (size_t g0 = 0; g0 < n_groups; g0 += TR_CHUNK) {           // whole groups per round trip: one launch's worth
        const size_t ng = std::min((size_t)TR_CHUNK, n_groups - g0);
        size_t nk = 0;
        for (size_t g = g0; g < g0 + ng; g++) nk += (size_t)gsize[g];
        Staging s;
        rc = reserve_staging(c, nk * stride, s);
        if (rc != QS_OK) return rc;
        Carve cv(nullptr);
        cv.take<qs_trail_match>(ng);
        if (rot_out) cv.take<double>(2 * nk);
        HIPCHK(c, c->io_ws.reserve(cv.bytes, c->stream, QS_IO_WS_FLOOR));
        Carve io(c->io_ws.p);
        qs_trail_match *d_out = io.take<qs_trail_match>(ng);
        double *d_rot = rot_out ? io.take<double>(2 * nk) : nullptr;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, nk * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, nk * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, trail_launch(c, ts, s.pkts, stride, lens ? s.lens : nullptr, gsize + g0, ng, d_out, d_rot));
        HIPCHK(c, hipMemcpyAsync(out + g0, d_out, ng * sizeof(qs_trail_match), hipMemcpyDeviceToHost, c->stream));
        if (rot_out) HIPCHK(c, hipMemcpyAsync(rot_out + 2 * k0, d_rot, 2 * nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        k0 += nk;
    }
    return QS_OK;
}
