// frontier_targets.hip -- frontier target assignment on the device.
// Semantics: the greedy nearest-frontier assignment of server_nodes/dual_bot_mapper.py:958-992 (commented out in the
// reference as shipped), over the centroids of :951-956, whose TARG packets AgentFirmware_Bot1.ino:81-137 drives to.
//
//   centroids : the roots of the frontier workspace (frontier.hip) with cnt >= min_cluster, compacted in first-cell
//               order (chunk count -> scan -> ranked write), each divided on the device exactly as the host did it:
//               avg = sum / cnt (true division), w = o + (avg + 0.5) * res;
//   top-K     : for every bot the exact K best centroids by the key (sqrt(d2), index): one wave per (bot, chunk of
//               FT_CHUNK centroids) keeps a sorted list in lanes 0..K-1, then one wave per bot merges its chunk lists;
//   greedy    : ONE wave walks the bots in order; a bot takes the first entry of its list that is neither taken nor
//               within `separation` of a target assigned so far.  The list is the true top-K by the same key, so
//               its first eligible entry is the minimum over every eligible centroid.  When a full list (K entries)
//               is entirely ineligible the pass stops; a whole-GPU scan over all centroids finds that bot's pick and
//               the pass resumes (qs_frontier_targets drives the loop and counts these fallbacks).
// Arithmetic is the reference's: fp64, no contraction (Makefile), d2 = dx*dx + dy*dy, correctly rounded sqrt.  The
// separation test uses r2_sep = the smallest double with sqrt(r2_sep) >= separation, so s < r2_sep <=> sqrt(s) < sep.
// A key that is NaN or +inf (a NaN / inf / far-outlier bot) never enters a list: `NaN < inf` and `inf < inf` are false.
#include "qs_internal.h"

#define FT_K 32                   // candidates per bot (the top-K list of the greedy pass)
#define FT_CHUNK 1024              // centroids per (bot, chunk) work item of the top-K pass
#define FT_BOTS_PER_BLOCK 4        // one wave per bot, 4 waves per workgroup (they read the same centroids)
#define FT_FB_BLOCK 256
#define FT_NONE 0x7fffffff

static_assert(FT_K <= QS_WAVE, "one list entry per lane");

struct QsFtState { int next_bot, m, stop, pad; };   // greedy pass: first bot not yet decided, targets so far, 1 = needs a full scan
// the workspace of one call, carved from ws (nullptr: only the bytes the block needs)
struct QsFtLayout {
    QsFtState *st;
    double2 *cent, *bots, *tgt_xy, *asg_xy;
    long long *tgt_idx;
    int *asg_idx;
    double *part_key; int *part_idx;      // [n_bots][n_chunks][K]
    int *list_idx, *list_len;             // [n_bots][K], [n_bots]
    double *fb_key; int *fb_idx;          // [n_fb]: per-block minima of a fallback scan
    size_t bytes;
};

// ---- centroids ------------------------------------------------------------------------------------------------
__device__ inline bool ft_keep(const unsigned int *cnt, size_t i, int min_cluster)
{
    const unsigned int n = cnt[i];                      // non-zero only at a cluster's root
    return n != 0 && (long long)n >= (long long)min_cluster;
}

__global__ void __launch_bounds__(256)
qs_ft_count_kernel(const unsigned int *__restrict__ cnt, size_t cells, int min_cluster, unsigned int *__restrict__ chunk_count)
{
    __shared__ unsigned int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * QS_FR_CHUNK;
    unsigned int m = 0;
    for (int q = 0; q < QS_FR_CHUNK / 256; q++) {
        const size_t i = base + q * 256 + threadIdx.x;
        if (i < cells && ft_keep(cnt, i, min_cluster)) m++;
    }
    if (m) atomicAdd(&s, m);
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
qs_ft_centroid_kernel(const unsigned int *__restrict__ cnt, const unsigned long long *__restrict__ sumx,
                      const unsigned long long *__restrict__ sumy, size_t cells, int min_cluster,
                      const unsigned int *__restrict__ chunk_off, double res, double ox, double oy, double2 *__restrict__ out)
{
    __shared__ unsigned int s_wave[256 / QS_WAVE];
    __shared__ unsigned int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = chunk_off[blockIdx.x];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * QS_FR_CHUNK;
    for (int q = 0; q < QS_FR_CHUNK / 256; q++) {
        const size_t i = base + q * 256 + tid;
        const bool on = i < cells && ft_keep(cnt, i, min_cluster);
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        unsigned int off = s_run;
        for (int v = 0; v < wave; v++) off += s_wave[v];
        if (on) {
            const size_t slot = off + __popcll(m & ((1ull << lane) - 1));
            // cluster_centroid_world (:233-237, :127-131); the sums are < 2^53, so the conversions are exact
            const double n = (double)cnt[i];
            const double ax = (double)sumx[i] / n, ay = (double)sumy[i] / n;
            out[slot] = make_double2(ox + (ax + 0.5) * res, oy + (ay + 0.5) * res);
        }
        __syncthreads();
        if (tid == 0) { unsigned int t = 0; for (int v = 0; v < 256 / QS_WAVE; v++) t += s_wave[v]; s_run += t; }
        __syncthreads();
    }
}

hipError_t qs_launch_ft_centroids(qs_ctx *c, void *fr_ws, int32_t min_cluster, int phase, double2 *d_cent)
{
    const QsFrLayout F = qs_frontier_layout(c, fr_ws);
    const size_t n_chunks = (c->cells + QS_FR_CHUNK - 1) / QS_FR_CHUNK;
    if (phase == 0) {
        hipLaunchKernelGGL(qs_ft_count_kernel, dim3((unsigned int)n_chunks), dim3(256), 0, c->stream, F.cnt, c->cells, min_cluster, F.chunk);
        hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : qs_launch_frontier_scan(c, fr_ws);
    }
    hipLaunchKernelGGL(qs_ft_centroid_kernel, dim3((unsigned int)n_chunks), dim3(256), 0, c->stream, F.cnt, F.sumx, F.sumy, c->cells,
                       min_cluster, F.chunk, c->cfg.res, c->cfg.ox, c->cfg.oy, d_cent);
    return hipGetLastError();
}

// ---- workspace ------------------------------------------------------------------------------------------------
static inline size_t ft_chunks(size_t n_cent) { return (n_cent + FT_CHUNK - 1) / FT_CHUNK; }
static inline size_t ft_fb_blocks(size_t n_cent) { return (n_cent + FT_FB_BLOCK - 1) / FT_FB_BLOCK; }

static QsFtLayout qs_ft_layout(void *ws, size_t n_cent, size_t n_bots)
{
    QsFtLayout L;
    Carve k(ws);
    const size_t nk = n_bots * ft_chunks(n_cent) * FT_K, nfb = ft_fb_blocks(n_cent);
    L.st = k.take<QsFtState>(1);
    L.cent = k.take<double2>(n_cent);
    L.bots = k.take<double2>(n_bots);
    L.tgt_idx = k.take<long long>(n_bots);
    L.tgt_xy = k.take<double2>(n_bots);
    L.asg_xy = k.take<double2>(n_bots);
    L.asg_idx = k.take<int>(n_bots);
    L.part_key = k.take<double>(nk);
    L.part_idx = k.take<int>(nk);
    L.list_idx = k.take<int>(n_bots * FT_K);
    L.list_len = k.take<int>(n_bots);
    L.fb_key = k.take<double>(nfb);
    L.fb_idx = k.take<int>(nfb);
    L.bytes = k.bytes;
    return L;
}

// ---- the key and the wave-resident sorted list --------------------------------------------------------------
// (ka, ia) comes before (kb, ib): the reference's strict `<` from inf over centroids in index order
__device__ inline bool ft_before(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// Lanes 0..K-1 hold the list, sorted by (key, index); empty entries are (inf, FT_NONE) and sort last.
// Insert the wave-uniform candidate (ck, ci) unless K entries already come before it.
__device__ inline void ft_insert(double &lk, int &li, double &ld2, double ck, int ci, double cd2, int lane)
{
    const unsigned long long m = __ballot(lane < FT_K && ft_before(lk, li, ck, ci));
    const int p = __popcll(m);                          // entries before the candidate: lanes 0..p-1
    if (p >= FT_K) return;
    const double uk = __shfl_up(lk, 1), ud2 = __shfl_up(ld2, 1);
    const int ui = __shfl_up(li, 1);
    if (lane > p && lane < FT_K) { lk = uk; li = ui; ld2 = ud2; }
    if (lane == p) { lk = ck; li = ci; ld2 = cd2; }
}

// one wave per (bot, chunk): the chunk's centroids in index order, 64 at a time.  Every entry of the list has a
// smaller index than the batch being read, so a centroid whose d2 is not below the K-th entry's d2 cannot come
// before it (its key is >= and its index larger): only the rest pay for a sqrt.
__global__ void __launch_bounds__(64 * FT_BOTS_PER_BLOCK)
qs_ft_topk_chunk_kernel(const double2 *__restrict__ cent, int n_cent, const double2 *__restrict__ bots, int n_bots,
                        int n_chunks, double *__restrict__ part_key, int *__restrict__ part_idx)
{
    const int lane = threadIdx.x & 63;
    const int bot = blockIdx.y * FT_BOTS_PER_BLOCK + (threadIdx.x >> 6), chunk = blockIdx.x;
    if (bot >= n_bots) return;                          // whole waves; no workgroup barrier below
    const double2 b = bots[bot];
    double lk = __builtin_huge_val(), ld2 = __builtin_huge_val();
    int li = FT_NONE;
    const int lo = chunk * FT_CHUNK, hi = min(lo + FT_CHUNK, n_cent);
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        double d2 = __builtin_huge_val();
        if (j < hi) {
            const double2 q = cent[j];
            const double dx = b.x - q.x, dy = b.y - q.y;
            d2 = dx * dx + dy * dy;
        }
        const double kth_d2 = __shfl(ld2, FT_K - 1);
        const bool cand = j < hi && d2 < kth_d2;        // false for NaN / inf
        const double key = cand ? sqrt(d2) : 0.0;
        unsigned long long m = __ballot(cand);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            ft_insert(lk, li, ld2, __shfl(key, src), base + src, __shfl(d2, src), lane);
        }
    }
    if (lane < FT_K) {
        const size_t o = ((size_t)bot * n_chunks + chunk) * FT_K + lane;
        part_key[o] = lk; part_idx[o] = li;
    }
}

// one wave per bot: merge its chunk lists into the exact top-K (list_idx, list_len = entries with a finite key)
__global__ void __launch_bounds__(64 * FT_BOTS_PER_BLOCK)
qs_ft_topk_merge_kernel(int n_bots, int n_chunks, const double *__restrict__ part_key, const int *__restrict__ part_idx,
                        int *__restrict__ list_idx, int *__restrict__ list_len)
{
    const int lane = threadIdx.x & 63;
    const int bot = blockIdx.x * FT_BOTS_PER_BLOCK + (threadIdx.x >> 6);
    if (bot >= n_bots) return;
    double lk = __builtin_huge_val(), ld2 = 0.0;
    int li = FT_NONE;
    const size_t n = (size_t)n_chunks * FT_K, base0 = (size_t)bot * n;
    for (size_t base = 0; base < n; base += 64) {
        const size_t e = base + lane;
        double k = __builtin_huge_val();
        int i = FT_NONE;
        if (e < n) { k = part_key[base0 + e]; i = part_idx[base0 + e]; }
        const double kth_k = __shfl(lk, FT_K - 1);
        const int kth_i = __shfl(li, FT_K - 1);
        unsigned long long m = __ballot(k < __builtin_huge_val() && ft_before(k, i, kth_k, kth_i));
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            ft_insert(lk, li, ld2, __shfl(k, src), __shfl(i, src), 0.0, lane);
        }
    }
    if (lane < FT_K) list_idx[(size_t)bot * FT_K + lane] = li;
    const int len = __popcll(__ballot(lane < FT_K && lk < __builtin_huge_val()));
    if (lane == 0) list_len[bot] = len;
}

// ---- the greedy pass: one wave, the bots in order ----------------------------------------------------------
// Targets assigned so far live in LDS (and in asg_* for a resumed pass).  fb_pending: the previous launch stopped at
// start_bot and a fallback scan has left its per-block minima in fb_key / fb_idx.
__global__ void __launch_bounds__(64)
qs_ft_greedy_kernel(const double2 *__restrict__ cent, int n_bots, double r2_sep, const int *__restrict__ list_idx,
                    const int *__restrict__ list_len, int start_bot, int start_m, int fb_pending,
                    const double *__restrict__ fb_key, const int *__restrict__ fb_idx, int n_fb,
                    double2 *__restrict__ asg_xy, int *__restrict__ asg_idx, long long *__restrict__ tgt_idx,
                    double2 *__restrict__ tgt_xy, QsFtState *__restrict__ st)
{
    __shared__ double2 s_xy[QS_FT_MAX_BOTS];
    __shared__ int s_idx[QS_FT_MAX_BOTS];
    const int lane = threadIdx.x;
    int m = start_m, b = start_bot;
    for (int j = lane; j < m; j += 64) { s_xy[j] = asg_xy[j]; s_idx[j] = asg_idx[j]; }
    __syncthreads();
    auto assign = [&](int c) {
        const double2 t = cent[c];
        if (lane == 0) {
            s_xy[m] = t; s_idx[m] = c; asg_xy[m] = t; asg_idx[m] = c;
            tgt_idx[b] = c; tgt_xy[b] = t;
        }
        m++;
        __syncthreads();
    };
    if (fb_pending) {
        double k = __builtin_huge_val();
        int i = FT_NONE;
        for (int q = lane; q < n_fb; q += 64) if (ft_before(fb_key[q], fb_idx[q], k, i)) { k = fb_key[q]; i = fb_idx[q]; }
        for (int off = 32; off > 0; off >>= 1) {
            const double ok = __shfl_xor(k, off);
            const int oi = __shfl_xor(i, off);
            if (ft_before(ok, oi, k, i)) { k = ok; i = oi; }
        }
        if (k < __builtin_huge_val()) assign(i);
        else if (lane == 0) tgt_idx[b] = -1;
        b++;
    }
    for (; b < n_bots; b++) {
        const int len = list_len[b];
        const int *lst = list_idx + (size_t)b * FT_K;
        int pick = -1;
        for (int k = 0; k < len; k++) {
            const int c = lst[k];
            const double2 q = cent[c];
            bool blk = false;
            for (int j = lane; j < m; j += 64) {
                const double2 t = s_xy[j];
                const double dx = q.x - t.x, dy = q.y - t.y;
                blk |= s_idx[j] == c || dx * dx + dy * dy < r2_sep;      // taken (:975-976) / too close (:977-981)
            }
            if (__ballot(blk) == 0) { pick = c; break; }
        }
        if (pick >= 0) assign(pick);
        else if (len == FT_K) {                          // a full list, all of it ineligible: a whole-GPU scan decides
            if (lane == 0) { st->next_bot = b; st->m = m; st->stop = 1; }
            return;
        } else if (lane == 0) tgt_idx[b] = -1;          // the list holds every centroid with a finite key
    }
    if (lane == 0) { st->next_bot = n_bots; st->m = m; st->stop = 0; }
}

// ---- the fallback: every centroid for one bot ----------------------------------------------------------------
__global__ void __launch_bounds__(FT_FB_BLOCK)
qs_ft_fallback_kernel(const double2 *__restrict__ cent, int n_cent, const double2 *__restrict__ bots, int bot, int m,
                      double r2_sep, const double2 *__restrict__ asg_xy, const int *__restrict__ asg_idx,
                      double *__restrict__ fb_key, int *__restrict__ fb_idx)
{
    __shared__ double2 s_xy[FT_FB_BLOCK];
    __shared__ int s_idx[FT_FB_BLOCK];
    __shared__ double s_k[FT_FB_BLOCK / QS_WAVE];
    __shared__ int s_i[FT_FB_BLOCK / QS_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * FT_FB_BLOCK + tid;
    double2 q = make_double2(0.0, 0.0);
    if (j < n_cent) q = cent[j];
    bool ok = j < n_cent;
    for (int t0 = 0; t0 < m; t0 += FT_FB_BLOCK) {
        __syncthreads();
        if (t0 + tid < m) { s_xy[tid] = asg_xy[t0 + tid]; s_idx[tid] = asg_idx[t0 + tid]; }
        __syncthreads();
        const int tn = min(FT_FB_BLOCK, m - t0);
        for (int t = 0; t < tn && ok; t++) {
            const double dx = q.x - s_xy[t].x, dy = q.y - s_xy[t].y;
            if (s_idx[t] == j || dx * dx + dy * dy < r2_sep) ok = false;
        }
    }
    double k = __builtin_huge_val();
    int i = FT_NONE;
    if (ok) {
        const double2 b = bots[bot];
        const double dx = b.x - q.x, dy = b.y - q.y;
        const double d = sqrt(dx * dx + dy * dy);
        if (d < __builtin_huge_val()) { k = d; i = j; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ok2 = __shfl_xor(k, off);
        const int oi = __shfl_xor(i, off);
        if (ft_before(ok2, oi, k, i)) { k = ok2; i = oi; }
    }
    if (lane == 0) { s_k[wave] = k; s_i[wave] = i; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < FT_FB_BLOCK / QS_WAVE; w++) if (ft_before(s_k[w], s_i[w], k, i)) { k = s_k[w]; i = s_i[w]; }
        fb_key[blockIdx.x] = k; fb_idx[blockIdx.x] = i;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------
// the lists, then the greedy pass from start_bot (fb_pending: a fallback scan has decided start_bot); it ends in QsFtState.
// start_bot == 0 && !fb_pending: the first launch of a call, which first builds the lists
static hipError_t qs_launch_ft_assign(qs_ctx *c, void *ws, size_t n_cent, size_t n_bots, double r2_sep,
                                      int start_bot, int start_m, int fb_pending)
{
    const QsFtLayout L = qs_ft_layout(ws, n_cent, n_bots);
    const int nch = (int)ft_chunks(n_cent);
    if (start_bot == 0 && !fb_pending) {
        const unsigned int gy = (unsigned int)((n_bots + FT_BOTS_PER_BLOCK - 1) / FT_BOTS_PER_BLOCK);
        hipLaunchKernelGGL(qs_ft_topk_chunk_kernel, dim3((unsigned int)nch, gy), dim3(64 * FT_BOTS_PER_BLOCK), 0, c->stream,
                           L.cent, (int)n_cent, L.bots, (int)n_bots, nch, L.part_key, L.part_idx);
        hipLaunchKernelGGL(qs_ft_topk_merge_kernel, dim3(gy), dim3(64 * FT_BOTS_PER_BLOCK), 0, c->stream,
                           (int)n_bots, nch, L.part_key, L.part_idx, L.list_idx, L.list_len);
    }
    hipLaunchKernelGGL(qs_ft_greedy_kernel, dim3(1), dim3(64), 0, c->stream, L.cent, (int)n_bots, r2_sep, L.list_idx,
                       L.list_len, start_bot, start_m, fb_pending, L.fb_key, L.fb_idx, (int)ft_fb_blocks(n_cent),
                       L.asg_xy, L.asg_idx, L.tgt_idx, L.tgt_xy, L.st);
    return hipGetLastError();
}

static hipError_t qs_launch_ft_fallback(qs_ctx *c, void *ws, size_t n_cent, size_t n_bots, double r2_sep,
                                        int bot, int m)
{
    const QsFtLayout L = qs_ft_layout(ws, n_cent, n_bots);
    hipLaunchKernelGGL(qs_ft_fallback_kernel, dim3((unsigned int)ft_fb_blocks(n_cent)), dim3(FT_FB_BLOCK), 0, c->stream,
                       L.cent, (int)n_cent, L.bots, bot, m, r2_sep, L.asg_xy, L.asg_idx, L.fb_key, L.fb_idx);
    return hipGetLastError();
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
    HIPCHK(c, hipSetDevice(c->device));
    SYNCCHK(c);
    HIPCHK(c, c->frontier_ws.reserve(qs_frontier_layout(c, nullptr).bytes, c->stream));
    void *fws = c->frontier_ws.p;
    HIPCHK(c, qs_launch_frontier_label(c, fws, true));
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 0, nullptr));
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, qs_frontier_layout(c, fws).total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n_cent = (size_t)total;
    HIPCHK(c, c->ft_ws.reserve(qs_ft_layout(nullptr, n_cent, n_bots).bytes, c->stream));
    const QsFtLayout F = qs_ft_layout(c->ft_ws.p, n_cent, n_bots);
    HIPCHK(c, qs_launch_ft_centroids(c, fws, min_cluster, 1, F.cent));
    uint64_t fallbacks = 0;
    std::vector<long long> tidx(n_bots, -1);
    std::vector<double> txy(2 * n_bots);
    if (n_bots && n_cent) {
        const double r2_sep = r2_threshold_for(separation);        // s < r2_sep <=> sqrt(s) < separation (0: nothing is too close)
        HIPCHK(c, hipMemcpyAsync(F.bots, bot_xy, n_bots * sizeof(double2), hipMemcpyHostToDevice, c->stream));
        int start = 0, m = 0, pending = 0;
        for (;;) {
            HIPCHK(c, qs_launch_ft_assign(c, c->ft_ws.p, n_cent, n_bots, r2_sep, start, m, pending));
            QsFtState st;
            HIPCHK(c, hipMemcpyAsync(&st, F.st, sizeof st, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (!st.stop) break;
            if (st.next_bot < start || st.next_bot >= (int)n_bots || (pending && st.next_bot == start))
                return qs_fail(c, QS_E_HIP, "qs_frontier_targets: greedy pass made no progress");
            fallbacks++;
            start = st.next_bot; m = st.m; pending = 1;
            HIPCHK(c, qs_launch_ft_fallback(c, c->ft_ws.p, n_cent, n_bots, r2_sep, start, m));
        }
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
    if (stats) { stats[0] = n_cent; stats[1] = FT_K; stats[2] = fallbacks; stats[3] = 0; }
    return QS_OK;
}
