// What hhx_groupstats.hip (output_statistics) and hhx_reassign.hip (the rounds of `haphic reassign`) share: the keys of full_link_dict turned into a
// symmetric adjacency by contig (count / scan / scatter), the order of a contig's cells and the bitonic network that establishes it.  The kernels
// live in an unnamed namespace: every translation unit that includes this header gets its own copy.
#pragma once
#include <algorithm>

#include "hhx_ingest.h"

namespace {
using namespace hhx;

constexpr int GS_THREADS = 256;
constexpr u64 GS_NONE = ~0ull;
constexpr i64 GS_PAD = INT64_MIN;                                                  // sum of a padding cell: sorts behind every real one

inline unsigned gs_grid(u64 n) {
    u64 b = (n + GS_THREADS - 1) / GS_THREADS;
    return (unsigned)std::max<u64>(1, std::min<u64>(b, 256 * 16));
}
inline i64 pow2_ceil(i64 v) {
    i64 p = 1;
    while (p < v) p <<= 1;
    return p;
}

// where the keys come from: the aggregated contig-pair table of an ingest handle (key != nullptr), or arrays in dict order
struct GsSource {
    i64 n;
    const u64 *key, *ord;
    const u32 *ht;
    const i32 *fi, *fj;
    const i64 *links;
};

__device__ __forceinline__ bool gs_entry(const GsSource &s, i64 e, i32 &a, i32 &b, i64 &links, u64 &pos) {
    if (s.key) {
        const u64 ord = s.ord[e];
        if (ord == NO_ORD) return false;                                           // not a key of full_link_dict (never was, or dropped)
        const u64 key = s.key[e] & KEY_MASK;
        a = (i32)(key >> ID_BITS);
        b = (i32)(key & ID_MASK);
        links = (i64)s.ht[4 * e] + (i64)s.ht[4 * e + 1] + (i64)s.ht[4 * e + 2] + (i64)s.ht[4 * e + 3];
        pos = 2 * ord;                                                             // only the relative order of the positions matters
        return true;
    }
    a = s.fi[e];
    b = s.fj[e];
    links = s.links[e];
    pos = 2 * (u64)e;
    return true;
}

__global__ __launch_bounds__(GS_THREADS) void k_gs_count(GsSource s, i32 n_ctg, unsigned long long *__restrict__ deg, int *__restrict__ bad) {
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < s.n; e += (i64)gridDim.x * blockDim.x) {
        i32 a, b;
        i64 links;
        u64 pos;
        if (!gs_entry(s, e, a, b, links, pos)) continue;
        if ((u32)a >= (u32)n_ctg || (u32)b >= (u32)n_ctg) { atomicExch(bad, 1); continue; }
        atomicAdd(&deg[a], 1ull);
        atomicAdd(&deg[b], 1ull);
    }
}

__global__ __launch_bounds__(GS_THREADS) void k_gs_scatter(GsSource s, i32 n_ctg, unsigned long long *__restrict__ cursor, i32 *__restrict__ partner,
                                                           i64 *__restrict__ lk, u64 *__restrict__ ps) {
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < s.n; e += (i64)gridDim.x * blockDim.x) {
        i32 a, b;
        i64 links;
        u64 pos;
        if (!gs_entry(s, e, a, b, links, pos)) continue;
        if ((u32)a >= (u32)n_ctg || (u32)b >= (u32)n_ctg) continue;
        const u64 x = atomicAdd(&cursor[a], 1ull);                                 // add_ctg_group(ctg_i, group_j) :2265
        partner[x] = b; lk[x] = links; ps[x] = pos;
        const u64 y = atomicAdd(&cursor[b], 1ull);                                 // add_ctg_group(ctg_j, group_i) :2266
        partner[y] = a; lk[y] = links; ps[y] = pos + 1;
    }
}

__device__ __forceinline__ bool gs_before(i64 sa, u64 fa, i64 sb, u64 fb) { return sa > sb || (sa == sb && fa < fb); }

// n2 = 2^k cells (cg, cs, cf) in any order -> ordered by (sum descending, first ascending).  The positions of the real cells are distinct, so
// this is a total order and the network needs no stability; padding cells (GS_PAD, GS_NONE) end up last.  All GS_THREADS threads call it.
__device__ __forceinline__ void gs_sort_cells(i32 *cg, i64 *cs, u64 *cf, i32 n2) {
    const int tid = threadIdx.x;
    for (i32 k = 2; k <= n2; k <<= 1)
        for (i32 j = k >> 1; j > 0; j >>= 1) {
            for (i32 t = tid; t < n2; t += GS_THREADS) {
                const i32 p = t ^ j;
                if (p > t) {
                    const i64 sa = cs[t], sb = cs[p];
                    const u64 fa = cf[t], fb = cf[p];
                    const bool swap = (t & k) == 0 ? gs_before(sb, fb, sa, fa) : gs_before(sa, fa, sb, fb);
                    if (swap) {
                        const i32 ga = cg[t], gb = cg[p];
                        cs[t] = sb; cs[p] = sa; cf[t] = fb; cf[p] = fa; cg[t] = gb; cg[p] = ga;
                    }
                }
            }
            __syncthreads();
        }
}

// sum() of q[from .. n) as the interpreter adds them, one by one from 0.0: plainly (sum_mode 0, CPython <= 3.11) or with Neumaier's compensation
// as CPython 3.12's sum() writes it (1).  One lane calls it.
__device__ __forceinline__ double gs_ordered_sum(const double *q, i32 from, i32 n, int sum_mode) {
    double total = 0.0;
    if (sum_mode == 0) {
        for (i32 r = from; r < n; ++r) total += q[r];
        return total;
    }
    double c = 0.0;
    for (i32 r = from; r < n; ++r) {
        const double x = q[r], t = total + x;
        if (fabs(total) >= fabs(x)) c += (total - t) + x;
        else c += (x - t) + total;
        total = t;
    }
    if (c != 0.0 && isfinite(c)) total += c;
    return total;
}

// the adjacency of `src` (on the device): row c holds, for every key that names contig c, the other contig, the links and the dict position
// 2 * key + side; the rows in no particular order inside.  Synchronises the stream.
struct GsAdjacency {
    DevBuf<i64> rowptr, lk;
    DevBuf<i32> partner;
    DevBuf<u64> ps;
    i64 n_adj = 0;
};
inline int gs_build_adjacency(const char *who, const GsSource &src, i32 n_ctg, GsAdjacency &A) {
    DevBuf<unsigned long long> d_deg, d_cursor;
    DevBuf<int> d_bad;
    if (d_deg.alloc((size_t)n_ctg + 2) || A.rowptr.alloc((size_t)n_ctg + 2) || d_cursor.alloc((size_t)n_ctg + 2) || d_bad.alloc(1)) return 1;
    HHX_HIP(hipMemsetAsync(d_deg.p, 0, sizeof(unsigned long long) * ((size_t)n_ctg + 2), g_stream));
    HHX_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), g_stream));
    KTimer kt("groupstats_adjacency", 2);
    if (src.n) {
        k_gs_count<<<gs_grid((u64)src.n), GS_THREADS, 0, g_stream>>>(src, n_ctg, d_deg.p, d_bad.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_TRY(exclusive_scan_i64(reinterpret_cast<const i64 *>(d_deg.p), A.rowptr.p, n_ctg, &A.n_adj));
    int bad = 0;
    HHX_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (bad) return fail("%s: a contig id outside [0, %d)", who, n_ctg);
    if (A.partner.alloc((size_t)A.n_adj + 1) || A.lk.alloc((size_t)A.n_adj + 1) || A.ps.alloc((size_t)A.n_adj + 1)) return 1;
    HHX_HIP(hipMemcpyAsync(d_cursor.p, A.rowptr.p, sizeof(i64) * ((size_t)n_ctg + 1), hipMemcpyDeviceToDevice, g_stream));
    if (src.n) {
        k_gs_scatter<<<gs_grid((u64)src.n), GS_THREADS, 0, g_stream>>>(src, n_ctg, d_cursor.p, A.partner.p, A.lk.p, A.ps.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipStreamSynchronize(g_stream));                                        // d_deg / d_cursor die here
    return 0;
}

}  // namespace
