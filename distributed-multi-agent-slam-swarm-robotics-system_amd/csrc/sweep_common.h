// sweep_common.h -- a servo-sweep record on the device: staging, header parse and beams shared by the sweep mapper (sweep.hip),
// the sweep matcher (match.hip) and the relocaliser (reloc.hip).
#pragma once
#include "raycast_common.h"

#define SW_DW 192                 // LDS dwords per staged record: >= (3 + 751 + 3) / 4 + 1 (the alignbyte reads one dword ahead)
#define SW_MAGIC 0x4c525351u      // 'Q','S','R','L'

struct QsSweepArgs {
    const unsigned char *pkts;    // record k at pkts + k * stride (this chunk)
    size_t n, stride;
    const unsigned short *lens;   // [n] or nullptr (every length == stride)
    unsigned int ranges_off;      // byte offset of r_0: 19 (v0) or 27 (v0 + odometry)
    int max_agent;
    const double *offset, *drift; // [max_agent + 1], [max_agent + 1][2]: read on the device, after every earlier launch
    double smin, smax;            // trust filter: smin < d <= smax
    unsigned char *accept;        // [n] out
    double *pose;                 // [n][3] out: rx, ry, yaw of accepted records
    unsigned long long ord_base;  // 4 * (seq0 - epoch_base) of record 0
    const qs_sweep_match *corr;   // [n] matched ingest only (the kernels' CORR instantiations): the correction of each record
    // graph mode (sweep_graph.hip): this chunk's slice of the batch the signature pass and the SLAM stage filled -- the ONE
    // acceptance decision, the agent and the chain's pose.  nullptr: acceptance and pose from the record, as without the mode
    const unsigned char *g_accept, *g_agent;
    const double *g_rx, *g_ry;
    unsigned long long *zone;     // the bots' zone boxes (the kernels' GRAPH instantiations)
    const qs_sweep_check *veto;   // [n] guarded ingest only (the kernels' VETO instantiations): the check of each record
};

// sweep.hip: everything of a that comes from the context (filter, offsets, drift); outputs and corr empty.  graph_k0: QS_SWEEP_NO_GRAPH,
// or the record of a graph-mode call these n records start at (their slice of the batch: acceptance, agent, rx, ry)
#define QS_SWEEP_NO_GRAPH ((size_t)-1)
void qs_sweep_args(const qs_ctx *c, const unsigned char *d_pkts, size_t n, size_t stride, const unsigned short *d_lens, size_t graph_k0,
                   QsSweepArgs &a);

// the record's dwords [addr & ~3, addr + stride) into s[0 .. 191]; dwords that reach outside the caller's buffer (its first and
// last bytes need not be dword-aligned) are read bytewise
__device__ inline void sw_stage(const QsSweepArgs &a, size_t k, unsigned int *s, int lane)
{
    const unsigned long long base = (unsigned long long)a.pkts, end = base + a.n * a.stride;
    const unsigned long long addr0 = base + k * a.stride, w0 = addr0 & ~3ull;
    unsigned int v[3];
    #pragma unroll
    for (int q = 0; q < 3; q++) {
        const unsigned long long p = w0 + 4ull * (unsigned long long)(lane + QS_WAVE * q);
        v[q] = 0;
        if (k < a.n && p < addr0 + a.stride) {
            if (p >= base && p + 4 <= end) v[q] = *(const unsigned int *)p;
            else
                for (int j = 0; j < 4; j++)
                    if (p + j >= base && p + j < end) v[q] |= (unsigned int)*(const unsigned char *)(p + j) << (8 * j);
        }
    }
    #pragma unroll
    for (int q = 0; q < 3; q++) s[lane + QS_WAVE * q] = v[q];
}

// little-endian u32 at byte o of the staged record (mis = the record's start within its first dword)
__device__ inline unsigned int sw_u32(const unsigned int *s, unsigned int mis, unsigned int o)
{
    const unsigned int b = mis + o;
    return __builtin_amdgcn_alignbyte(s[(b >> 2) + 1], s[b >> 2], b & 3u);
}

struct SwHead { bool ok; int agent; double rx, ry, yaw; };

// length, magic and agent of qs_ingest_sweeps' acceptance rule; the agent byte either way
__device__ inline bool sw_accept(const QsSweepArgs &a, size_t k, const unsigned int *s, unsigned int mis, int &agent)
{
    const int len = a.lens ? (int)a.lens[k] : (int)a.stride;
    agent = (int)(sw_u32(s, mis, 4) & 0xffu);
    return len == (int)a.stride && sw_u32(s, mis, 0) == SW_MAGIC && agent >= 1 && agent <= a.max_agent;
}

// GRAPH: acceptance, agent and (rx, ry) from the batch slice (decided and posed before this launch); otherwise from the record
template <bool GRAPH>
__device__ inline SwHead sw_head_t(const QsSweepArgs &a, size_t k, const unsigned int *s, unsigned int mis)
{
    SwHead h{false, 0, 0.0, 0.0, 0.0};
    if (GRAPH) {
        h.ok = a.g_accept[k] != 0;
        if (h.ok) {
            h.agent = a.g_agent[k];
            h.rx = a.g_rx[k]; h.ry = a.g_ry[k];
            h.yaw = (double)__uint_as_float(sw_u32(s, mis, 13));
        }
        return h;
    }
    h.ok = sw_accept(a, k, s, mis, h.agent);
    if (h.ok) {
        const int agent = h.agent;
        const float x = __uint_as_float(sw_u32(s, mis, 5)), y = __uint_as_float(sw_u32(s, mis, 9));
        h.rx = ((double)x + a.offset[agent]) + a.drift[2 * agent];      // offset first, then drift (:851-857)
        h.ry = (double)y + a.drift[2 * agent + 1];
        h.yaw = (double)__uint_as_float(sw_u32(s, mis, 13));
    }
    return h;
}

// the matcher's form: whichever the arguments say
__device__ inline SwHead sw_head(const QsSweepArgs &a, size_t k, const unsigned int *s, unsigned int mis)
{
    return a.g_accept ? sw_head_t<true>(a, k, s, mis) : sw_head_t<false>(a, k, s, mis);
}

// the 181 beams of a staged record, three a lane: hit flags, d * cos, d * sin of the beam angle (tab: [2][181], the host's
// table, qs_beam_table); returns H (every wave computes all of it)
__device__ inline int sw_beams(const QsSweepArgs &a, const unsigned int *s_rec, unsigned int mis, const double *tab, int lane,
                               bool hit[3], double bx[3], double by[3])
{
    int H = 0;
    #pragma unroll
    for (int q = 0; q < 3; q++) {
        const int i = lane + QS_WAVE * q;
        hit[q] = false; bx[q] = 0.0; by[q] = 0.0;
        if (i < QS_SWEEP_BEAMS) {
            const double d = (double)__uint_as_float(sw_u32(s_rec, mis, a.ranges_off + 4u * (unsigned int)i));
            hit[q] = qs_range_rule(d, a.smin, a.smax).valid;
            bx[q] = d * tab[i];
            by[q] = d * tab[QS_SWEEP_BEAMS + i];
        }
        H += __popcll(__ballot(hit[q]));
    }
    return H;
}

// matched ingest: the pose the sweep is cast from, rx' = rx + dx, ry' = ry + dy, yaw' = yaw + dyaw (one add each; a match
// that was not accepted carries zeros, which leave the pose bit for bit)
__device__ inline void sw_correct(const QsSweepArgs &a, size_t k, SwHead &h)
{
    if (!h.ok) return;
    const qs_sweep_match &m = a.corr[k];
    h.rx = h.rx + m.dx; h.ry = h.ry + m.dy; h.yaw = h.yaw + m.dyaw;
}

// guarded ingest: a record whose check says CONTRADICTS is withheld -- from here on it is a rejected record
__device__ inline void sw_veto(const QsSweepArgs &a, size_t k, SwHead &h)
{
    if (h.ok && a.veto[k].status == QS_CHECK_CONTRADICTS) h.ok = false;
}
