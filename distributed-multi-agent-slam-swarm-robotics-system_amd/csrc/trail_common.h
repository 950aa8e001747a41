// trail_common.h -- what the kernels that read trails of 42-byte packets share (trail.hip: trail matching; reloc.hip: trail
// relocalisation): the staging of a trail's records into LDS, as the packet decoder stages a tile (decode.hip), and the parse
// and acceptance of one record (qs_ingest's rule, T2 of include/quasar_slam.h).
#pragma once
#include "raycast_common.h"

#define TR_MAX_STRIDE 64                     // records are staged through LDS when stride <= 64 bytes
#define TR_RAW_DW (QS_TRAIL_MAX_RECORDS * TR_MAX_STRIDE / 4 + 2)      // dwords of the staging area: 1026

// the records of one launch
struct TrRecords {
    const unsigned char *pkts;    // nrec records, `stride` bytes apart
    const unsigned short *lens;   // or nullptr
    size_t stride, nrec;
};

// the record's 42 bytes as eleven dwords from LDS (the record starts at any byte): twelve aligned reads shifted into place
__device__ inline void tr_record_lds(const unsigned int *s_raw, unsigned int off, unsigned int r[11])
{
    const unsigned int w0 = off >> 2, sh = off & 3u;
    unsigned int d[12];
    #pragma unroll
    for (int q = 0; q < 12; q++) d[q] = s_raw[w0 + q];
    #pragma unroll
    for (int q = 0; q < 11; q++) r[q] = __builtin_amdgcn_alignbyte(d[q + 1], d[q], sh);
}

// stage records [rec0, rec0 + K) (K <= QS_TRAIL_MAX_RECORDS, stride <= TR_MAX_STRIDE) into s_raw[TR_RAW_DW] with nthreads threads:
// the byte range widened to dword boundaries, the dwords that straddle the caller's buffer read bytewise, never a byte past it.
// Returns the misalignment of the first record: record i starts at byte mis + i * stride of s_raw.  The caller synchronises
__device__ __forceinline__ unsigned int tr_stage(const TrRecords &m, size_t rec0, int K, unsigned int *s_raw, int tid, int nthreads)
{
    const unsigned long long addr0 = (unsigned long long)m.pkts + rec0 * m.stride;
    const unsigned int mis = (unsigned int)(addr0 & 3ull);
    const unsigned int *src = (const unsigned int *)(addr0 - mis);
    const unsigned int ndw = (mis + (unsigned int)K * (unsigned int)m.stride + 3u) / 4u;       // <= 1025
    const unsigned long long buf0 = (unsigned long long)m.pkts, buf1 = buf0 + m.nrec * m.stride;
    for (unsigned int k = tid; k < ndw; k += nthreads) {
        const unsigned long long a = (unsigned long long)(src + k);
        unsigned int v;
        if (a >= buf0 && a + 4 <= buf1) v = src[k];
        else {                                                 // a dword that straddles the caller's buffer: bytewise
            v = 0;
            const unsigned char *p = (const unsigned char *)a;
            for (int q = 0; q < 4; q++)
                if (a + q >= buf0 && a + q < buf1) v |= (unsigned int)p[q] << (8 * q);
        }
        s_raw[k] = v;
    }
    // (a record's twelve-dword window may reach one dword past the staged range: its bytes are never looked at, but the
    // read stays inside s_raw, which holds 1026 dwords)
    for (unsigned int k = ndw + tid; k < ndw + 12u && k < TR_RAW_DW; k += nthreads) s_raw[k] = 0u;
    return mis;
}

// record i of the launch, parsed and accepted by qs_ingest's rule (T2): staged: from s_raw at byte `off`; otherwise read per
// lane from the caller's buffer, no byte past the record's length.  The outputs of a rejected record mean nothing
__device__ __forceinline__ bool tr_parse(const TrRecords &m, int max_agent, size_t i, bool staged, const unsigned int *s_raw, unsigned int off,
                                         int &agent, float &x, float &y, float &yaw, float dist[4])
{
    const int len = m.lens ? (int)m.lens[i] : (int)m.stride;
    if (!((len == QS_PACKET_SIZE || len == QS_PACKET_SIZE_V1) && (size_t)len <= m.stride)) return false;
    unsigned int r[11];
    if (staged) tr_record_lds(s_raw, off, r);
    else {
        const unsigned char *p = m.pkts + i * m.stride;
        #pragma unroll
        for (int q = 0; q < 11; q++) {
            unsigned int v = 0;
            #pragma unroll
            for (int e = 0; e < 4; e++)
                if (4 * q + e < len) v |= (unsigned int)p[4 * q + e] << (8 * e);
            r[q] = v;
        }
    }
    #define TR_U32(p) ((p) % 4 == 0 ? r[(p) / 4] : __builtin_amdgcn_alignbyte(r[(p) / 4 + 1], r[(p) / 4], (p) % 4))
    agent = (int)(r[1] & 0xffu);
    x = __uint_as_float(TR_U32(5)); y = __uint_as_float(TR_U32(9)); yaw = __uint_as_float(TR_U32(13));
    dist[0] = __uint_as_float(TR_U32(25)); dist[1] = __uint_as_float(TR_U32(29));
    dist[2] = __uint_as_float(TR_U32(33)); dist[3] = __uint_as_float(TR_U32(37));
    #undef TR_U32
    return r[0] == 0x4c525351u && agent >= 1 && agent <= max_agent && isfinite(x) && isfinite(y) && isfinite(yaw);
}
