// sweep_graph.hip -- graph mode of the servo-sweep path (include/quasar_slam.h, "sweeps in the pose graph"): the signature pass.
// The firmware that sends sweeps computes no landmark byte, so the server derives one from the ranges: the median of 2w + 1
// beams to the right (beams 0 ..), front (.. 90 ..) and left (.. 180) through the firmware's detectLandmark table.  The pass
// also makes the record's ONE acceptance decision and fills the batch arrays exactly as qs_decode_kernel fills them for a
// 42-byte packet (accept, map_ok, agent, lm, px, py, yaw; the per-graph graph_batch and per-bot agent_ev counts), so that the
// SLAM stage -- node numbering, landmark events, the loop-closure chain, rx / ry -- runs over sweeps unchanged.  It does not
// touch QS_CNT_*: datagrams and accepted records are counted once, by the mapping kernels (sweep.hip).
//
// One WAVE per record, staged into the wave's LDS slot as pass A of the sweep mapper stages it.  Per sector lanes 0 .. 2w take
// one range each; an unusable range (NaN, +-inf, 0, negative) becomes +inf, so every value is a positive float or +inf and
// its BIT PATTERN orders as its value does: all compares are integer compares.  Each lane counts the values that order before
// its own by (value, beam); the lane that counts w holds the median, which a ballot finds and a readlane broadcasts.
#include <math.h>
#include <stdio.h>
#include <algorithm>

#include "sweep_common.h"

#define SG_BLOCK 256              // 4 waves: 4 records per round
#define SG_ROUNDS 4               // rounds per workgroup: the LDS counts reach HBM once per 16 records
#define SG_REJECTED 255

// the sector's value S as its bit pattern: beams first .. first + 2w
__device__ inline unsigned int sg_sector(const unsigned int *s, unsigned int mis, unsigned int ranges_off, int first, int w, int lane)
{
    const int m = 2 * w + 1;
    unsigned int v = 0x7f800000u;                                       // +inf
    if (lane < m) {
        const unsigned int u = sw_u32(s, mis, ranges_off + 4u * (unsigned int)(first + lane));
        // usable: finite and > 0 (sign clear, exponent not all ones, not zero)
        if ((u >> 31) == 0 && (u & 0x7f800000u) != 0x7f800000u && u != 0) v = u;
    }
    int before = 0;
    for (int j = 0; j < m; j++) {                                       // (j is uniform: a v_readlane each)
        const unsigned int vj = (unsigned int)__builtin_amdgcn_readlane((int)v, j);
        before += (vj < v || (vj == v && j < lane)) ? 1 : 0;
    }
    // (value, beam) is a total order: exactly one of the m lanes counts w
    const unsigned long long holder = __ballot(lane < m && before == w);
    const int src = __ffsll((long long)holder) - 1;
    return (unsigned int)__builtin_amdgcn_readlane((int)v, src);
}

// AgentFirmware_Bot1.ino:152-169 on the three sector values widened to fp64
__device__ inline int sg_decide(double f, double l, double r, double close, double open)
{
    const bool fc = f < close, lc = l < close, rc = r < close;
    const bool fo = f > open, lo = l > open, ro = r > open;
    if (fc && lc && rc) return 4;                                       // DEAD_END
    if (fc && lc) return 1;                                             // CORNER_L
    if (fc && rc) return 2;                                             // CORNER_R
    if (lc && rc && fo) return 3;                                       // CORRIDOR
    if (fo && lo && ro) return 5;                                       // OPEN
    return 0;
}

// lm_out == nullptr: record k of the chunk goes to slot k0 + k of the batch; otherwise only lm_out[k] is written
__global__ void __launch_bounds__(SG_BLOCK)
qs_sweep_signature_kernel(QsSweepArgs a, QsBatch b, size_t k0, int w, double close, double open, int bots_per_graph, int n_graphs,
                          unsigned long long *__restrict__ graph_batch, unsigned int *__restrict__ agent_ev,
                          unsigned char *__restrict__ lm_out)
{
    constexpr int NW = SG_BLOCK / QS_WAVE;
    __shared__ unsigned int s_rec[NW][SW_DW];
    __shared__ unsigned int s_agent_ev[QS_MAX_AGENT + 1];
    __shared__ unsigned int s_hist_small[64][2];
    const int tid = threadIdx.x, lane = tid & (QS_WAVE - 1), wave = tid >> 6;
    const bool small_g = n_graphs <= 64, fill = lm_out == nullptr;
    if (tid < 64) { s_hist_small[tid][0] = 0; s_hist_small[tid][1] = 0; }
    for (int t = tid; t <= QS_MAX_AGENT; t += SG_BLOCK) s_agent_ev[t] = 0;
    const size_t base = (size_t)blockIdx.x * NW * SG_ROUNDS;
    for (int r = 0; r < SG_ROUNDS; r++) {
        if (base + (size_t)r * NW >= a.n) break;                        // (uniform over the workgroup)
        const size_t k = base + (size_t)r * NW + wave;
        __syncthreads();                                                // the previous round's records are parsed
        sw_stage(a, k < a.n ? k : a.n, s_rec[wave], lane);
        __syncthreads();
        if (k >= a.n) continue;
        const unsigned int *s = s_rec[wave];
        const unsigned int mis = (unsigned int)(((unsigned long long)a.pkts + k * a.stride) & 3ull);
        int agent;
        bool ok = sw_accept(a, k, s, mis, agent);
        const float x = __uint_as_float(sw_u32(s, mis, 5)), y = __uint_as_float(sw_u32(s, mis, 9)),
                    yaw = __uint_as_float(sw_u32(s, mis, 13));
        ok = ok && isfinite(x) && isfinite(y) && isfinite(yaw);         // the packet path's test (decode.hip)
        int lm = 0;
        if (ok) {                                                       // (uniform over the wave)
            const unsigned int sr = sg_sector(s, mis, a.ranges_off, 0, w, lane);
            const unsigned int sf = sg_sector(s, mis, a.ranges_off, 90 - w, w, lane);
            const unsigned int sl = sg_sector(s, mis, a.ranges_off, 180 - 2 * w, w, lane);
            lm = sg_decide((double)__uint_as_float(sf), (double)__uint_as_float(sl), (double)__uint_as_float(sr), close, open);
        }
        if (lane != 0) continue;
        if (!fill) { lm_out[k] = (unsigned char)(ok ? lm : SG_REJECTED); continue; }
        const size_t i = k0 + k;
        if (ok) {
            b.agent[i] = (unsigned char)agent;
            b.lm[i] = (unsigned char)lm;
            b.px[i] = (double)x + a.offset[agent];                      // :851-852
            b.py[i] = (double)y;
            b.yaw[i] = (double)yaw;
            const int g = (agent - 1) / bots_per_graph;
            if (small_g) {
                atomicAdd(&s_hist_small[g][0], 1u);
                if (lm) atomicAdd(&s_hist_small[g][1], 1u);
            } else {
                atomicAdd(&graph_batch[2 * g], 1ull);
                if (lm) atomicAdd(&graph_batch[2 * g + 1], 1ull);
            }
            if (lm) atomicAdd(&s_agent_ev[agent], 1u);
        } else b.lm[i] = SG_REJECTED;                                   // (qs_last_sweep_nodes; nothing else reads a rejected record's)
        b.accept[i] = ok ? 1 : 0;
        if (b.map_ok != b.accept) b.map_ok[i] = (ok && agent >= b.own_lo && agent <= b.own_hi) ? 1 : 0;
    }
    if (!fill) return;
    __syncthreads();
    for (int t = tid; t <= a.max_agent; t += SG_BLOCK)
        if (s_agent_ev[t]) atomicAdd(&agent_ev[t], s_agent_ev[t]);
    if (small_g && tid < n_graphs) {
        if (s_hist_small[tid][0]) atomicAdd(&graph_batch[2 * tid], (unsigned long long)s_hist_small[tid][0]);
        if (s_hist_small[tid][1]) atomicAdd(&graph_batch[2 * tid + 1], (unsigned long long)s_hist_small[tid][1]);
    }
}

hipError_t qs_launch_sweep_signatures(qs_ctx *c, const qs_sweep_graph_params &p, const unsigned char *d_pkts, size_t n, size_t stride,
                                      const unsigned short *d_lens, size_t k0, unsigned char *lm_out)
{
    if (n == 0) return hipSuccess;
    QsSweepArgs a;
    qs_sweep_args(c, d_pkts, n, stride, d_lens, QS_SWEEP_NO_GRAPH, a);
    const size_t per = (size_t)(SG_BLOCK / QS_WAVE) * SG_ROUNDS;
    hipLaunchKernelGGL(qs_sweep_signature_kernel, dim3((unsigned int)((n + per - 1) / per)), dim3(SG_BLOCK), 0, c->stream, a, c->b, k0,
                       (int)p.half_width, p.close, p.open, c->bots_per_graph, c->n_graphs, c->d_graph_batch.p, c->sb.agent_ev, lm_out);
    return hipGetLastError();
}

// ---- graph mode's pass over ALL n records of a sweep call, before any chunk is mapped: the steps a packet ingest takes before
// its rays (qs_batch_prepare, its decoder, qs_batch_slam) with the signature kernel as the decoder.  host: pkts / lens are the
// caller's host buffers, staged one chunk at a time
int qs_sweep_graph_pass(qs_ctx *c, const uint8_t *pkts, bool host, size_t n, size_t stride, const uint16_t *lens, size_t chunk)
{
    int rc = qs_batch_prepare(c, n);
    if (rc != QS_OK) return rc;
    StageTimer t(c, QS_STAGE_DECODE);
    for (size_t k0 = 0; k0 < n; k0 += chunk) {
        const size_t m = std::min(chunk, n - k0);
        const uint8_t *d_pkts = pkts + k0 * stride;
        const uint16_t *d_lens = lens ? lens + k0 : nullptr;
        if (host) {
            Staging s;
            rc = reserve_staging(c, m * stride, s);                // (stream-ordered: the previous chunk's kernel has read its)
            if (rc != QS_OK) return rc;
            HIPCHK(c, hipMemcpyAsync(s.pkts, d_pkts, m * stride, hipMemcpyHostToDevice, c->stream));
            if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, d_lens, m * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
            d_pkts = s.pkts; d_lens = lens ? s.lens : nullptr;
        }
        HIPCHK(c, qs_launch_sweep_signatures(c, c->sg_params, d_pkts, m, stride, d_lens, k0, nullptr));
    }
    t.stop();
    return qs_batch_slam(c, n);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
static int sg_check(qs_ctx *c, const qs_sweep_graph_params &p, const char *who)
{
    char buf[160];
    const char *bad = nullptr;
    if (p.half_width < 0 || p.half_width > QS_SWEEP_GRAPH_MAX_HALF_WIDTH) bad = "half_width must be in 0..29";
    else if (!(isfinite(p.close) && p.close > 0)) bad = "close must be finite and > 0";
    else if (!(isfinite(p.open) && p.open >= p.close)) bad = "open must be finite and >= close";
    if (!bad) return QS_OK;
    snprintf(buf, sizeof buf, "%s: %s", who, bad);
    return qs_fail(c, QS_E_INVAL, buf);
}

extern "C" int qs_set_sweep_graph(qs_ctx *c, int32_t enable, const qs_sweep_graph_params *params)
{
    ARGCHK(c, c != nullptr);
    qs_sweep_graph_params p{5, 0, 0.40, 0.80};
    if (params) p = *params;
    int rc = sg_check(c, p, "qs_set_sweep_graph");
    if (rc != QS_OK) return rc;
    p.reserved = 0;
    c->sg_params = p;
    c->sweep_graph = enable != 0;
    return QS_OK;
}

extern "C" int qs_sweep_graph(qs_ctx *c, int32_t *enabled, qs_sweep_graph_params *out)
{
    ARGCHK(c, c != nullptr);
    if (enabled) *enabled = c->sweep_graph ? 1 : 0;
    if (out) *out = c->sg_params;
    return QS_OK;
}

static int sg_signatures_begin(qs_ctx *c, const qs_sweep_graph_params *params, size_t stride, qs_sweep_graph_params &p)
{
    p = params ? *params : c->sg_params;
    int rc = sg_check(c, p, "qs_sweep_signatures");
    if (rc != QS_OK) return rc;
    if (stride != QS_SWEEP_SIZE_V0 && stride != QS_SWEEP_SIZE_V0_ODO)
        return qs_fail(c, QS_E_INVAL, "qs_sweep_signatures: stride must be 743 (v0) or 751 (v0 + odometry)");
    HIPCHK(c, hipSetDevice(c->device));
    return QS_OK;
}

extern "C" int qs_sweep_signatures_device(qs_ctx *c, const qs_sweep_graph_params *params, const uint8_t *d_pkts, size_t n, size_t stride,
                                          const uint16_t *d_lens, uint8_t *d_lm_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (d_pkts != nullptr && d_lm_out != nullptr));
    qs_sweep_graph_params p;
    int rc = sg_signatures_begin(c, params, stride, p);
    if (rc != QS_OK || n == 0) return rc;
    HIPCHK(c, qs_launch_sweep_signatures(c, p, d_pkts, n, stride, d_lens, 0, d_lm_out));
    return QS_OK;
}

extern "C" int qs_sweep_signatures(qs_ctx *c, const qs_sweep_graph_params *params, const uint8_t *pkts, size_t n, size_t stride,
                                   const uint16_t *lens, uint8_t *lm_out)
{
    ARGCHK(c, c != nullptr);
    ARGCHK(c, n == 0 || (pkts != nullptr && lm_out != nullptr));
    qs_sweep_graph_params p;
    int rc = sg_signatures_begin(c, params, stride, p);
    if (rc != QS_OK || n == 0) return rc;
    const size_t chunk = (size_t)1 << 16;
    HIPCHK(c, c->io_ws.reserve(std::min(n, chunk), c->stream, QS_IO_WS_FLOOR));
    for (size_t k0 = 0; k0 < n; k0 += chunk) {
        const size_t m = std::min(chunk, n - k0);
        Staging s;
        rc = reserve_staging(c, m * stride, s);
        if (rc != QS_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(s.pkts, pkts + k0 * stride, m * stride, hipMemcpyHostToDevice, c->stream));
        if (lens) HIPCHK(c, hipMemcpyAsync(s.lens, lens + k0, m * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, qs_launch_sweep_signatures(c, p, s.pkts, m, stride, lens ? s.lens : nullptr, 0, (unsigned char *)c->io_ws.p));
        HIPCHK(c, hipMemcpyAsync(lm_out + k0, c->io_ws.p, m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return QS_OK;
}

extern "C" int qs_last_sweep_nodes(qs_ctx *c, int64_t *node, uint8_t *lm, size_t n)
{
    ARGCHK(c, c != nullptr);
    if (!c->last_sweeps || !c->last_sweep_graph || n != c->last_sweeps_n)
        return qs_fail(c, QS_E_INVAL, "qs_last_sweep_nodes: the last ingest was not a sweep ingest of n records in graph mode");
    if (n == 0) return QS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (node) HIPCHK(c, hipMemcpyAsync(node, c->sb.node, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (lm) HIPCHK(c, hipMemcpyAsync(lm, c->b.lm, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}
