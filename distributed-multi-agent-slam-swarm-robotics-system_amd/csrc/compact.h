// compact.h -- the order-preserving compaction every file uses.
// Items 0..n-1 in chunks of QS_COMPACT_CHUNK: a count per chunk, one exclusive scan of the counts (a single workgroup,
// grid_ops.hip), then every chunk writes its marked items at scan offset + rank, the rank from wave ballots, so the
// output keeps the items' order.  Written once over
//   a predicate: `bool marked(size_t i) const`              -- is item i kept, and
//   an emitter : `void put(size_t slot, size_t i) const`    -- what kept item i leaves at its slot;
// each caller instantiates it with its own pair (grid_ops.hip, frontier.hip, frontier_targets.hip).
#pragma once
#include "qs_internal.h"

#define QS_COMPACT_CHUNK 1024     // items per chunk = per workgroup of the count and write kernels
#define QS_COMPACT_BLOCK 256

// entries of the chunk array a compaction of n items needs
static inline size_t qs_compact_chunks(size_t n) { return (n + QS_COMPACT_CHUNK - 1) / QS_COMPACT_CHUNK; }

template <typename Pred>
__global__ void __launch_bounds__(QS_COMPACT_BLOCK)
qs_compact_count_kernel(const Pred pred, size_t n, unsigned int *__restrict__ chunk_count)
{
    __shared__ unsigned int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * QS_COMPACT_CHUNK;
    unsigned int m = 0;
    for (int q = 0; q < QS_COMPACT_CHUNK / QS_COMPACT_BLOCK; q++) {
        const size_t i = base + q * QS_COMPACT_BLOCK + threadIdx.x;
        if (i < n && pred.marked(i)) m++;
    }
    if (m) atomicAdd(&s, m);
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = s;
}

template <typename Pred, typename Emit>
__global__ void __launch_bounds__(QS_COMPACT_BLOCK)
qs_compact_write_kernel(const Pred pred, size_t n, const unsigned int *__restrict__ chunk_off, const Emit emit, size_t cap)
{
    __shared__ unsigned int s_wave[QS_COMPACT_BLOCK / QS_WAVE];
    __shared__ unsigned int s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = chunk_off[blockIdx.x];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * QS_COMPACT_CHUNK;
    for (int q = 0; q < QS_COMPACT_CHUNK / QS_COMPACT_BLOCK; q++) {
        const size_t i = base + q * QS_COMPACT_BLOCK + tid;
        const bool on = i < n && pred.marked(i);
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        unsigned int off = s_run;
        for (int v = 0; v < wave; v++) off += s_wave[v];
        if (on) {
            const size_t slot = off + __popcll(m & ((1ull << lane) - 1));
            if (slot < cap) emit.put(slot, i);
        }
        __syncthreads();
        if (tid == 0) { unsigned int t = 0; for (int v = 0; v < QS_COMPACT_BLOCK / QS_WAVE; v++) t += s_wave[v]; s_run += t; }
        __syncthreads();
    }
}

// the scan kernel's launcher (grid_ops.hip): chunk counts -> exclusive offsets in place, their sum -> *d_total
hipError_t qs_launch_compact_scan(hipStream_t stream, unsigned int *d_chunk, size_t n_chunks, unsigned long long *d_total);

// phase 0 (write == false): the chunk counts of the n items, scanned into offsets in d_chunk [qs_compact_chunks(n)], the
// total in *d_total; phase 1, after it: the ranked writes of the first `cap` marked items
template <typename Pred, typename Emit>
static hipError_t qs_compact(hipStream_t stream, const Pred pred, size_t n, bool write, const Emit emit, size_t cap,
                             unsigned int *d_chunk, unsigned long long *d_total)
{
    const size_t n_chunks = qs_compact_chunks(n);
    if (write) {
        hipLaunchKernelGGL((qs_compact_write_kernel<Pred, Emit>), dim3((unsigned int)n_chunks), dim3(QS_COMPACT_BLOCK), 0, stream,
                           pred, n, d_chunk, emit, cap);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(qs_compact_count_kernel<Pred>, dim3((unsigned int)n_chunks), dim3(QS_COMPACT_BLOCK), 0, stream, pred, n, d_chunk);
    return qs_launch_compact_scan(stream, d_chunk, n_chunks, d_total);
}
