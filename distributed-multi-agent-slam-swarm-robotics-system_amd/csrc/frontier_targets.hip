// frontier_targets.hip -- frontier target assignment on the device.
// Semantics: the greedy nearest-frontier assignment of server_nodes/dual_bot_mapper.py:958-992 (commented out in the
// reference as shipped), over the centroids of :951-956, whose TARG packets AgentFirmware_Bot1.ino:81-137 drives to.
//
//   centroids : the roots of the frontier workspace (frontier.hip) with cnt >= min_cluster, compacted in first-cell
//               order (compact.h), each divided on the device exactly as the host did it:
//               avg = sum / cnt (true division), w = o + (avg + 0.5) * res;
//   top-K     : for every bot the exact K best centroids by the key (sqrt(d2), index): one wave per (bot, chunk of
//               AS_CHUNK centroids) keeps a sorted list in lanes 0..K-1, then one wave per bot merges its chunk lists;
//   greedy    : ONE wave walks the bots in order; a bot takes the first entry of its list that is neither taken nor
//               within `separation` of a target assigned so far.  The list is the true top-K by the same key, so
//               its first eligible entry is the minimum over every eligible centroid.  When a full list (K entries)
//               is entirely ineligible the pass stops; a whole-GPU scan over all centroids finds that bot's pick and
//               the pass resumes (qs_frontier_targets drives the loop and counts these fallbacks).
// Arithmetic is the reference's: fp64, no contraction (Makefile), d2 = dx*dx + dy*dy, correctly rounded sqrt.  The
// separation test uses r2_sep = the smallest double with sqrt(r2_sep) >= separation, so s < r2_sep <=> sqrt(s) < sep.
// A key that is NaN or +inf (a NaN / inf / far-outlier bot) never enters a list: `NaN < inf` and `inf < inf` are false.
// The sorted list, the blocked test, the greedy walk and the host's stop / resume loop are assign_common.h's, shared with
// targets_by_path.hip; here are the entry they order by, the producer of the chunk lists and the fallback's key.
// qs_count_centroids is how every call over the centroids starts (here, targets_by_path.hip, territory.hip, gain.hip).
#include "assign_common.h"
#include "compact.h"

#define FT_NONE 0x7fffffff

// the workspace of one call, carved from ws (nullptr: only the bytes the block needs)
struct QsFtLayout {
    QsAssignState *st;
    double2 *cent, *bots, *tgt_xy, *asg_xy;
    long long *tgt_idx;
    int *asg_idx;
    double *part_key; int *part_idx;      // [n_bots][n_chunks][K]
    int *list_idx, *list_len;             // [n_bots][K], [n_bots]
    double *fb_key; int *fb_idx;          // [n_fb]: per-block minima of a fallback scan
    size_t bytes;
};

// ---- centroids ------------------------------------------------------------------------------------------------
struct FtEmitCentroid {
    const unsigned int *cnt; const unsigned long long *sumx, *sumy; double res, ox, oy; double2 *out;
    __device__ void put(size_t slot, size_t i) const
    {
        // cluster_centroid_world (:233-237, :127-131); the sums are < 2^53, so the conversions are exact
        const double n = (double)cnt[i];
        const double ax = (double)sumx[i] / n, ay = (double)sumy[i] / n;
        out[slot] = make_double2(ox + (ax + 0.5) * res, oy + (ay + 0.5) * res);
    }
};

hipError_t qs_launch_ft_centroids(qs_ctx *c, void *fr_ws, int32_t min_cluster, int phase, double2 *d_cent)
{
    const QsFrLayout F = qs_frontier_layout(c, fr_ws);
    // no cap on the writes: d_cent holds the total phase 0 counted
    return qs_compact(c->stream, FtKeep{F.cnt, min_cluster}, c->cells, phase != 0,
                      FtEmitCentroid{F.cnt, F.sumx, F.sumy, c->cfg.res, c->cfg.ox, c->cfg.oy, d_cent}, ~(size_t)0, F.chunk, F.total);
}

int qs_count_centroids(qs_ctx *c, int32_t min_cluster, void *&fws, size_t &n_cent)
{
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->frontier_ws.reserve(qs_frontier_layout(c, nullptr).bytes, c->stream));
    fws = c->frontier_ws.p;
    HIPCHK(c, qs_launch_frontier_label(c, fws, true));
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 0, nullptr));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, qs_frontier_layout(c, fws).total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    n_cent = (size_t)total;
    return QS_OK;
}

// ---- workspace ------------------------------------------------------------------------------------------------
static QsFtLayout qs_ft_layout(void *ws, size_t n_cent, size_t n_bots)
{
    QsFtLayout L;
    Carve k(ws);
    const size_t nk = n_bots * as_chunks(n_cent) * AS_K, nfb = as_fb_blocks(n_cent);
    L.st = k.take<QsAssignState>(1);
    L.cent = k.take<double2>(n_cent);
    L.bots = k.take<double2>(n_bots);
    L.tgt_idx = k.take<long long>(n_bots);
    L.tgt_xy = k.take<double2>(n_bots);
    L.asg_xy = k.take<double2>(n_bots);
    L.asg_idx = k.take<int>(n_bots);
    L.part_key = k.take<double>(nk);
    L.part_idx = k.take<int>(nk);
    L.list_idx = k.take<int>(n_bots * AS_K);
    L.list_len = k.take<int>(n_bots);
    L.fb_key = k.take<double>(nfb);
    L.fb_idx = k.take<int>(nfb);
    L.bytes = k.bytes;
    return L;
}

// ---- the entry of the lists: (sqrt(d2), index) ----------------------------------------------------------------------------
// (ka, ia) comes before (kb, ib): the reference's strict `<` from inf over centroids in index order, ka < kb || (ka == kb &&
// ia < ib).  Written without short-circuits: on entries that come out of shuffles the compiler otherwise branches per clause
__device__ inline bool ft_before(double ka, int ia, double kb, int ib) { return (ka < kb) | ((ka == kb) & (ia < ib)); }

struct FtEntry {
    double key; int idx;
    struct Part { double *key; int *idx; };
    struct CPart { const double *key; const int *idx; };
    typedef int Item;
    __device__ static FtEntry none() { return {__builtin_huge_val(), FT_NONE}; }
    __device__ bool valid() const { return key < __builtin_huge_val(); }
    __device__ bool before(FtEntry o) const { return ft_before(key, idx, o.key, o.idx); }
    template <typename F> __device__ FtEntry map(F f) const { return {f(key), f(idx)}; }
    __device__ static FtEntry load(const CPart p, size_t o) { return {p.key[o], p.idx[o]}; }
    __device__ void store(const Part p, size_t o) const { p.key[o] = key; p.idx[o] = idx; }
    __device__ Item item() const { return idx; }
    __device__ static int centroid(Item it) { return it; }
};
// the chunk kernel's entry carries d2 as well: its screen compares d2 with the K-th entry's and saves most sqrts
struct FtChunkEntry {
    double key; int idx; double d2;
    __device__ bool before(FtChunkEntry o) const { return ft_before(key, idx, o.key, o.idx); }
    template <typename F> __device__ FtChunkEntry map(F f) const { return {f(key), f(idx), f(d2)}; }
};

// one wave per (bot, chunk): the chunk's centroids in index order, 64 at a time.  Every entry of the list has a
// smaller index than the batch being read, so a centroid whose d2 is not below the K-th entry's d2 cannot come
// before it (its key is >= and its index larger): only the rest pay for a sqrt.
__global__ void __launch_bounds__(64 * AS_BOTS_PER_BLOCK)
qs_ft_topk_chunk_kernel(const double2 *__restrict__ cent, int n_cent, const double2 *__restrict__ bots, int n_bots,
                        int n_chunks, const FtEntry::Part part)
{
    const int lane = threadIdx.x & 63;
    const int bot = blockIdx.y * AS_BOTS_PER_BLOCK + (threadIdx.x >> 6), chunk = blockIdx.x;
    if (bot >= n_bots) return;                          // whole waves; no workgroup barrier below
    const double2 b = bots[bot];
    FtChunkEntry l{__builtin_huge_val(), FT_NONE, __builtin_huge_val()};
    const int lo = chunk * AS_CHUNK, hi = min(lo + AS_CHUNK, n_cent);
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        double d2 = __builtin_huge_val();
        if (j < hi) {
            const double2 q = cent[j];
            const double dx = b.x - q.x, dy = b.y - q.y;
            d2 = dx * dx + dy * dy;
        }
        const double kth_d2 = __shfl(l.d2, AS_K - 1);
        const bool cand = j < hi && d2 < kth_d2;        // false for NaN / inf
        const double key = cand ? sqrt(d2) : 0.0;
        as_offer_if(l, cand, lane, [&](int src) { return FtChunkEntry{__shfl(key, src), base + src, __shfl(d2, src)}; });
    }
    if (lane < AS_K) FtEntry{l.key, l.idx}.store(part, ((size_t)bot * n_chunks + chunk) * AS_K + lane);
}

// one wave per bot: merge its chunk lists into the exact top-K (list_idx, list_len = entries with a finite key)
__global__ void __launch_bounds__(64 * AS_BOTS_PER_BLOCK)
qs_ft_topk_merge_kernel(int n_bots, int n_chunks, const FtEntry::CPart part, int *__restrict__ list_idx, int *__restrict__ list_len)
{
    const int lane = threadIdx.x & 63;
    const int bot = blockIdx.x * AS_BOTS_PER_BLOCK + (threadIdx.x >> 6);
    if (bot >= n_bots) return;
    const size_t n = (size_t)n_chunks * AS_K;
    int len;
    const FtEntry l = as_merge_lists<FtEntry>(part, (size_t)bot * n, n, lane, len);
    if (lane < AS_K) list_idx[(size_t)bot * AS_K + lane] = l.item();
    if (lane == 0) list_len[bot] = len;
}

// ---- the greedy pass (assign_common.h): a decision leaves the bot's centroid and its position ---------------------------
struct FtPolicy {
    long long *tgt_idx; double2 *tgt_xy;
    __device__ void assigned(int b, int, int c, double2 t) const { tgt_idx[b] = c; tgt_xy[b] = t; }
    __device__ void unassigned(int b) const { tgt_idx[b] = -1; }
    __device__ bool skip(int, int) const { return false; }
};

__global__ void __launch_bounds__(64)
qs_ft_greedy_kernel(const double2 *__restrict__ cent, int n_bots, double r2_sep, const int *__restrict__ list_idx,
                    const int *__restrict__ list_len, int start_bot, int start_m, int fb_pending, const FtEntry::CPart fb, int n_fb,
                    double2 *__restrict__ asg_xy, int *__restrict__ asg_idx, long long *__restrict__ tgt_idx,
                    double2 *__restrict__ tgt_xy, QsAssignState *__restrict__ st)
{
    as_greedy_walk<FtEntry>(FtPolicy{tgt_idx, tgt_xy}, cent, n_bots, r2_sep, list_idx, list_len, start_bot, start_m, fb_pending,
                            fb, n_fb, asg_xy, asg_idx, st);
}

// ---- the fallback: every centroid for one bot ----------------------------------------------------------------
__global__ void __launch_bounds__(AS_FB_BLOCK)
qs_ft_fallback_kernel(const double2 *__restrict__ cent, int n_cent, const double2 *__restrict__ bots, int bot, int m,
                      double r2_sep, const double2 *__restrict__ asg_xy, const int *__restrict__ asg_idx, const FtEntry::Part fb)
{
    const int j = blockIdx.x * AS_FB_BLOCK + threadIdx.x;
    double2 q = make_double2(0.0, 0.0);
    if (j < n_cent) q = cent[j];
    as_fallback_block<FtEntry>(j < n_cent, j, q, m, r2_sep, asg_xy, asg_idx, fb, [&] {
        const double2 b = bots[bot];
        const double dx = b.x - q.x, dy = b.y - q.y;
        const double d = sqrt(dx * dx + dy * dy);
        return d < __builtin_huge_val() ? FtEntry{d, j} : FtEntry::none();
    });
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------
// centroids on the device, top-K lists, the greedy pass; the pass stops at a bot whose full list is ineligible, a whole-GPU
// scan decides that bot, and the pass resumes from it
extern "C" int qs_frontier_targets(qs_ctx *c, int32_t min_cluster, double separation, const double *bot_xy, size_t n_bots,
                                   int64_t *target_idx, double *target_xy, double *centroids_xy, size_t cap,
                                   size_t *n_centroids, uint64_t stats[4])
{
    ARGCHK(c, c != nullptr);
    if (n_bots > QS_FT_MAX_BOTS) return qs_fail(c, QS_E_INVAL, "qs_frontier_targets: n_bots above QS_FT_MAX_BOTS");
    ARGCHK(c, n_bots == 0 || (bot_xy && target_idx && target_xy));
    ARGCHK(c, cap == 0 || centroids_xy);
    void *fws;
    size_t n_cent;
    int rc = qs_count_centroids(c, min_cluster, fws, n_cent);
    if (rc != QS_OK) return rc;
    HIPCHK(c, c->ft_ws.reserve(qs_ft_layout(nullptr, n_cent, n_bots).bytes, c->stream));
    const QsFtLayout F = qs_ft_layout(c->ft_ws.p, n_cent, n_bots);
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 1, F.cent));
    uint64_t fallbacks = 0;
    std::vector<long long> tidx(n_bots, -1);
    std::vector<double> txy(2 * n_bots);
    if (n_bots && n_cent) {
        const double r2_sep = r2_threshold_for(separation);        // s < r2_sep <=> sqrt(s) < separation (0: nothing is too close)
        HIPCHK(c, hipMemcpyAsync(F.bots, bot_xy, n_bots * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        const int nch = (int)as_chunks(n_cent), nfb = (int)as_fb_blocks(n_cent);
        const unsigned int gy = (unsigned int)((n_bots + AS_BOTS_PER_BLOCK - 1) / AS_BOTS_PER_BLOCK);
        const FtEntry::Part part{F.part_key, F.part_idx}, fb{F.fb_key, F.fb_idx};
        const FtEntry::CPart cpart{F.part_key, F.part_idx}, cfb{F.fb_key, F.fb_idx};
        hipLaunchKernelGGL(qs_ft_topk_chunk_kernel, dim3((unsigned int)nch, gy), dim3(64 * AS_BOTS_PER_BLOCK), 0, c->stream,
                           F.cent, (int)n_cent, F.bots, (int)n_bots, nch, part);
        hipLaunchKernelGGL(qs_ft_topk_merge_kernel, dim3(gy), dim3(64 * AS_BOTS_PER_BLOCK), 0, c->stream,
                           (int)n_bots, nch, cpart, F.list_idx, F.list_len);
        int m;
        rc = as_run_greedy(c, "qs_frontier_targets: greedy pass made no progress", F.st, n_bots,
            [&](int start, int m, int pending) {
                hipLaunchKernelGGL(qs_ft_greedy_kernel, dim3(1), dim3(64), 0, c->stream, F.cent, (int)n_bots, r2_sep, F.list_idx,
                                   F.list_len, start, m, pending, cfb, nfb, F.asg_xy, F.asg_idx, F.tgt_idx, F.tgt_xy, F.st);
                return hipGetLastError();
            },
            [&](int bot, int m) {                                   // every centroid for the bot the pass stopped at
                hipLaunchKernelGGL(qs_ft_fallback_kernel, dim3((unsigned int)nfb), dim3(AS_FB_BLOCK), 0, c->stream,
                                   F.cent, (int)n_cent, F.bots, bot, m, r2_sep, F.asg_xy, F.asg_idx, fb);
                HIPCHK(c, hipGetLastError());
                return (int)QS_OK;
            }, m, fallbacks);
        if (rc != QS_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(tidx.data(), F.tgt_idx, n_bots * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(txy.data(), F.tgt_xy, n_bots * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    }
    const size_t nc = n_cent < cap ? n_cent : cap;
    if (nc) HIPCHK(c, hipMemcpyAsync(centroids_xy, F.cent, nc * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < n_bots; b++) {
        target_idx[b] = tidx[b];
        if (tidx[b] >= 0) { target_xy[2 * b] = txy[2 * b]; target_xy[2 * b + 1] = txy[2 * b + 1]; }
    }
    if (n_centroids) *n_centroids = n_cent;
    if (stats) { stats[0] = n_cent; stats[1] = AS_K; stats[2] = fallbacks; stats[3] = 0; }
    return QS_OK;
}
