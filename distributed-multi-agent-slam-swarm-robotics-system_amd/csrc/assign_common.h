// assign_common.h -- what the greedy target assignments share (frontier_targets.hip: DESIGN.md §4.7, by distance;
// targets_by_path.hip: §4.12, by path cost, and §4.17, by gain over cost): the wave-resident top-K list, the blocked test, the greedy walk over the bots
// and the host loop that resumes it after a fallback scan.
//
// Each file supplies an entry type E, the (key, centroid) its lists order by:
//   bool before(E o) const               the strict order of the rule
//   E map(f) const                       f applied to every field (how an entry is shuffled across lanes)
// which is all the sorted list needs (as_insert, as_offer_if), and for the merge, the walk and the fallback also
//   static E none()                      the empty entry; it sorts last
//   bool valid() const                   not empty
//   typedef Part, CPart                  where chunk lists and per-block minima live, to write and to read;
//                                        static E load(CPart, o); void store(Part, o) const
//   typedef Item; Item item() const      what a bot's top-K list keeps of an entry; static int centroid(Item)
#pragma once
#include "qs_internal.h"

#define AS_K 32                   // candidates per bot (the top-K list of the greedy pass)
#define AS_CHUNK 1024             // centroids per (bot, chunk) work item of the top-K pass
#define AS_BOTS_PER_BLOCK 4       // one wave per bot, 4 waves per workgroup (they read the same centroids)
#define AS_FB_BLOCK 256

static_assert(AS_K <= QS_WAVE, "one list entry per lane");

static inline size_t as_chunks(size_t n_cent) { return (n_cent + AS_CHUNK - 1) / AS_CHUNK; }
static inline size_t as_fb_blocks(size_t n_cent) { return (n_cent + AS_FB_BLOCK - 1) / AS_FB_BLOCK; }

// the clusters every target call keeps as centroids: the roots of the frontier workspace with cnt >= min_cluster.  One
// predicate, so a compaction over it gives every call the same slots (frontier_targets.hip: centroids; gain.hip: viewpoints)
struct FtKeep {
    const unsigned int *cnt; int min_cluster;
    __device__ bool marked(size_t i) const
    {
        const unsigned int n = cnt[i];                      // non-zero only at a cluster's root
        return n != 0 && (long long)n >= (long long)min_cluster;
    }
};

struct QsAssignState { int next_bot, m, stop, pad; };   // greedy pass: first bot not yet decided, targets so far, 1 = needs a full scan

// ---- the wave-resident sorted list ------------------------------------------------------------------------------------
// Lanes 0..K-1 hold the list, sorted by E::before; empty entries are E::none() and sort last.
// Insert the wave-uniform candidate c unless K entries already come before it.  E::map is how an entry crosses lanes: every
// lane calls it with a shuffle, which it applies to each field.
template <typename E>
__device__ inline void as_insert(E &l, const E &c, int lane)
{
    const unsigned long long m = __ballot(lane < AS_K && l.before(c));
    const int p = __popcll(m);                          // entries before the candidate: lanes 0..p-1
    if (p >= AS_K) return;
    const E u = l.map([](auto v) { return __shfl_up(v, 1); });
    if (lane > p && lane < AS_K) l = u;
    if (lane == p) l = c;
}

// candidates (one per lane where cand is set) into the list, in lane order; from(src) is lane src's, in every lane
template <typename E, typename From>
__device__ inline void as_offer_if(E &l, bool cand, int lane, From from)
{
    unsigned long long m = __ballot(cand);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        as_insert(l, from(src), lane);
    }
}

// ... every lane's entry that comes before the K-th of the list
template <typename E>
__device__ inline void as_offer(E &l, const E &e, int lane)
{
    const E kth = l.map([](auto v) { return __shfl(v, AS_K - 1); });
    as_offer_if(l, e.valid() && e.before(kth), lane, [&](int src) { return e.map([src](auto v) { return __shfl(v, src); }); });
}

// one wave: the n entries at part[base0 ..) (a bot's chunk lists) merged into the exact top-K; len = entries in it
template <typename E>
__device__ inline E as_merge_lists(const typename E::CPart part, size_t base0, size_t n, int lane, int &len)
{
    E l = E::none();
    for (size_t base = 0; base < n; base += 64) {
        const size_t e = base + lane;
        as_offer(l, e < n ? E::load(part, base0 + e) : E::none(), lane);
    }
    len = __popcll(__ballot(lane < AS_K && l.valid()));
    return l;
}

// the smaller of the entries of a wave, in every lane
template <typename E>
__device__ inline E as_wave_min(E e)
{
    for (int off = 32; off > 0; off >>= 1) {
        const E o = e.map([off](auto v) { return __shfl_xor(v, off); });
        if (o.before(e)) e = o;
    }
    return e;
}

// ---- the blocked test ---------------------------------------------------------------------------------------------------
// centroid c at q against one target so far: taken (:975-976) / too close (:977-981).  fp64, no contraction (Makefile);
// r2_sep = the smallest double with sqrt(r2_sep) >= separation, so s < r2_sep <=> sqrt(s) < separation
__device__ inline bool as_blocked(int c, double2 q, int t_idx, double2 t, double r2_sep)
{
    const double dx = q.x - t.x, dy = q.y - t.y;
    return t_idx == c || dx * dx + dy * dy < r2_sep;
}

// targets t0 .. t0 + tn of the pass so far into LDS, by the nt threads of the workgroup (the caller places the barriers)
__device__ inline void as_stage(double2 *s_xy, int *s_idx, const double2 *__restrict__ asg_xy, const int *__restrict__ asg_idx,
                                int t0, int tn, int tid, int nt)
{
    for (int j = tid; j < tn; j += nt) { s_xy[j] = asg_xy[t0 + j]; s_idx[j] = asg_idx[t0 + j]; }
}

// ---- the fallback: every centroid for one bot, one thread per centroid, AS_FB_BLOCK threads ------------------------
// live: the thread has a centroid, j at q, that may be the bot's candidate.  One of the m targets so far blocks it, or key()
// makes its entry (none(): no finite key); the block's smallest entry goes to fb[blockIdx.x].
template <typename E, typename Key>
__device__ inline void as_fallback_block(bool live, int j, double2 q, int m, double r2_sep, const double2 *__restrict__ asg_xy,
                                         const int *__restrict__ asg_idx, const typename E::Part fb, Key key)
{
    __shared__ double2 s_xy[AS_FB_BLOCK];
    __shared__ int s_idx[AS_FB_BLOCK];
    __shared__ E s_e[AS_FB_BLOCK / QS_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool ok = live;
    for (int t0 = 0; t0 < m; t0 += AS_FB_BLOCK) {
        const int tn = min(AS_FB_BLOCK, m - t0);
        __syncthreads();
        as_stage(s_xy, s_idx, asg_xy, asg_idx, t0, tn, tid, AS_FB_BLOCK);
        __syncthreads();
        for (int t = 0; t < tn && ok; t++) if (as_blocked(j, q, s_idx[t], s_xy[t], r2_sep)) ok = false;
    }
    E e = as_wave_min(ok ? key() : E::none());
    if (lane == 0) s_e[wave] = e;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < AS_FB_BLOCK / QS_WAVE; w++) if (s_e[w].before(e)) e = s_e[w];
        e.store(fb, blockIdx.x);
    }
}

// ---- the greedy pass: one wave, the bots in order ----------------------------------------------------------------------
// A bot takes the first entry of its list that no target so far blocks.  The targets live in LDS (and in asg_* for a
// resumed pass).  fb_pending: the previous launch stopped at start_bot and a fallback scan has left its per-block minima
// in fb.  The policy P says what a decision leaves behind; lane 0 calls
//   assigned(b, m, item, t)   bot b takes the centroid the item names, at t, as target m
//   unassigned(b)             no centroid is left for bot b
// and every lane calls skip(b, lane): true when b is decided before its list is looked at.
template <typename E, typename P>
__device__ inline void as_greedy_walk(const P &pol, const double2 *__restrict__ cent, int n_bots, double r2_sep,
                                      const typename E::Item *__restrict__ list, const int *__restrict__ list_len, int start_bot,
                                      int start_m, int fb_pending, const typename E::CPart fb, int n_fb, double2 *__restrict__ asg_xy,
                                      int *__restrict__ asg_idx, QsAssignState *__restrict__ st)
{
    __shared__ double2 s_xy[QS_FT_MAX_BOTS];
    __shared__ int s_idx[QS_FT_MAX_BOTS];
    const int lane = threadIdx.x;
    int m = start_m, b = start_bot;
    as_stage(s_xy, s_idx, asg_xy, asg_idx, 0, m, lane, 64);
    __syncthreads();
    auto assign = [&](typename E::Item it) {
        const int c = E::centroid(it);
        const double2 t = cent[c];
        if (lane == 0) {
            s_xy[m] = t; s_idx[m] = c; asg_xy[m] = t; asg_idx[m] = c;
            pol.assigned(b, m, it, t);
        }
        m++;
        __syncthreads();
    };
    if (fb_pending) {
        E e = E::none();
        for (int q = lane; q < n_fb; q += 64) { const E o = E::load(fb, q); if (o.before(e)) e = o; }
        e = as_wave_min(e);
        if (e.valid()) assign(e.item());
        else if (lane == 0) pol.unassigned(b);
        b++;
    }
    for (; b < n_bots; b++) {
        if (pol.skip(b, lane)) continue;
        const int len = list_len[b];
        const typename E::Item *lst = list + (size_t)b * AS_K;
        int pick = -1;
        for (int k = 0; k < len; k++) {
            const int c = E::centroid(lst[k]);
            const double2 q = cent[c];
            bool blk = false;
            for (int j = lane; j < m; j += 64) blk |= as_blocked(c, q, s_idx[j], s_xy[j], r2_sep);
            if (__ballot(blk) == 0) { pick = k; break; }
        }
        if (pick >= 0) assign(lst[pick]);
        else if (len == AS_K) {                         // a full list, all of it ineligible: a whole-GPU scan decides
            if (lane == 0) { st->next_bot = b; st->m = m; st->stop = 1; }
            return;
        } else if (lane == 0) pol.unassigned(b);        // the list holds every centroid with a valid key
    }
    if (lane == 0) { st->next_bot = n_bots; st->m = m; st->stop = 0; }
}

// ---- the host loop --------------------------------------------------------------------------------------------------------
// greedy(start, m, pending) enqueues the file's greedy kernel, which ends in *d_st.  When the pass stopped at a bot whose
// full list is blocked, fallback(bot, m) enqueues the whole-GPU scan that decides it (QS_OK or the call's failure) and the
// pass resumes from that bot.  m: the targets assigned; fallbacks: the scans it took.
template <typename Greedy, typename Fallback>
static int as_run_greedy(qs_ctx *c, const char *no_progress, const QsAssignState *d_st, size_t n_bots, Greedy greedy,
                         Fallback fallback, int &m, uint64_t &fallbacks)
{
    int start = 0, pending = 0;
    m = 0;
    for (;;) {
        HIPCHK(c, greedy(start, m, pending));
        QsAssignState st;
        HIPCHK(c, hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        m = st.m;
        if (!st.stop) return QS_OK;
        if (st.next_bot < start || st.next_bot >= (int)n_bots || (pending && st.next_bot == start))
            return qs_fail(c, QS_E_HIP, no_progress);
        fallbacks++;
        start = st.next_bot; pending = 1;
        const int rc = fallback(start, m);
        if (rc != QS_OK) return rc;
    }
}
