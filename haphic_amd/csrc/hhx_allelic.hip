// --remove_allelic_links on the device tables (remove_allelic_HiC_links :474-692): the two halves of it that touch every key.
//   hhx_ingest_concordance  record_coord_pairs :454-465 + cal_concordance_ratio :419-428 as integers: per full_link_dict key, the modal
//                           counts of the diagonal / anti-diagonal windows of its first max_read_pairs read pairs (stream order)
//   hhx_ingest_drop_links   update_link_dicts :488-509 for a whole verdict at once + the isolated-fragment pass :678-692
// What lies between them — the cliques of the allele graph and the assignment problems — is host code (haphic_amd/allelic.py).
//
// The read pairs are grouped by contig pair with the stable key sort the coordinate lists and paired_links.clm already use
// (hhx::group_pairs, hhx_pairs.hip); the grouped records stay in HBM.  Both entries run on the calling thread's stream and pool arena and
// only READ the side records, so a queued paired_links.clm (hhx_ingest_write_clm_async) may be reading them at the same time.
// hhx_ingest_drop_links changes the tables and therefore first waits for the files queued on this handle.
#include <algorithm>

#include "hhx_ingest.h"
#include "hhx_sort.h"

using namespace hhx;

namespace {

constexpr int AL_SMALL = 256;          // up to here: all-pairs equality count out of LDS
constexpr int AL_CAP = 4096;           // largest max_read_pairs served (sorted in LDS: 32 KB per wavefront); documented in haphic_hip.h

inline unsigned grid_for(u64 n, unsigned per = 256) {
    u64 b = (n + per - 1) / per;
    if (b < 1) b = 1;
    if (b > 256 * 16) b = 256 * 16;
    return (unsigned)b;
}

// Python's // on int64 (floors; C truncates), w > 0
__device__ __forceinline__ i64 floor_div(i64 a, i64 w) {
    i64 q = a / w;
    if ((a % w) != 0 && a < 0) --q;
    return q;
}

// modal count of s_v[0..m) by all pairs: lane t counts the values equal to its own; every lane reads the same LDS word per step (a broadcast)
__device__ __forceinline__ i32 mode_all_pairs(const i64 *s_v, i32 m, int lane) {
    i32 best = 0;
    for (i32 t = lane; t < m; t += HHX_WAVE) {
        const i64 mine = s_v[t];
        i32 c = 0;
        for (i32 u = 0; u < m; ++u) c += s_v[u] == mine;
        best = max(best, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, HHX_WAVE));
    return best;
}

// modal count of s_v[0..m) by a bitonic sort of the n2 >= m slots (padding: INT64_MAX, above every window number) and the longest run
__device__ __forceinline__ i32 mode_sorted(i64 *s_v, i32 m, i32 n2, int lane) {
    for (i32 k = 2; k <= n2; k <<= 1)
        for (i32 j = k >> 1; j > 0; j >>= 1) {
            for (i32 t = lane; t < n2; t += HHX_WAVE) {
                const i32 p = t ^ j;
                if (p > t) {
                    const i64 a = s_v[t], b = s_v[p];
                    if ((a > b) == ((t & k) == 0)) { s_v[t] = b; s_v[p] = a; }
                }
            }
            __syncthreads();
        }
    i32 best = 0;
    for (i32 t = lane; t < m; t += HHX_WAVE) {
        const i64 mine = s_v[t];
        if (t && s_v[t - 1] == mine) continue;                 // not the start of a run
        i32 lo = t + 1, hi = m;                                // first position > t whose value differs
        while (lo < hi) { const i32 mid = (lo + hi) >> 1; if (s_v[mid] == mine) lo = mid + 1; else hi = mid; }
        best = max(best, lo - t);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, HHX_WAVE));
    return best;
}

// One wavefront (= one workgroup of 64) per contig pair.  CAP: slots of the LDS list; BIG: the pass for the keys with more than AL_SMALL
// evaluated pairs (it skips the others, the small pass skips these).  Outputs by dict position r = srank[g]; the small pass writes m of every key.
template <int CAP, bool BIG>
__global__ __launch_bounds__(HHX_WAVE) void k_concordance(i64 n_groups, const u64 *__restrict__ stk, const i64 *__restrict__ gstart, const u64 *__restrict__ srank,
                                                          const u64 *__restrict__ sxy, const UnitInfo *__restrict__ ctg, i64 max_pairs, i64 min_pairs,
                                                          i64 nwindows, i32 *__restrict__ m_out, i32 *__restrict__ diag, i32 *__restrict__ anti,
                                                          unsigned int *__restrict__ bad) {
    __shared__ i64 s_v[CAP];
    const int lane = threadIdx.x;
    for (i64 g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const i64 b = gstart[g], cnt = gstart[g + 1] - b, r = (i64)srank[g];
        const i32 m = (i32)(cnt < max_pairs ? cnt : max_pairs);
        const bool mine = BIG ? m > AL_SMALL : m <= AL_SMALL;
        const bool skip = m < min_pairs;                         // :589 — the host never evaluates them
        if (!BIG && lane == 0) { m_out[r] = m; if (skip) { diag[r] = 0; anti[r] = 0; } }
        if (!mine || skip || m == 0) continue;                   // (uniform over the workgroup: the barriers below are reached by all or none)
        const u64 key = stk[g];
        const i64 li = ctg[key >> ID_BITS].lenf & LEN_MASK, lj = ctg[key & ID_MASK].lenf & LEN_MASK;
        const i64 w = (li < lj ? li : lj) / nwindows;            // :421
        if (w <= 0) { if (lane == 0) atomicExch(bad, 1u); continue; }   // the reference raises ZeroDivisionError; refused by the caller
        i32 n2 = 1;
        if (BIG) while (n2 < m) n2 <<= 1;
        i32 res[2];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();                                     // the list of the previous pass / key has been read
            for (i32 t = lane; t < (BIG ? n2 : m); t += HHX_WAVE) {
                i64 v = INT64_MAX;
                if (t < m) {
                    const u64 xy = sxy[b + t];
                    const i64 x = (i64)(xy >> 32), y = (i64)(xy & 0xffffffffu);     // 64-bit: y + x reaches 2^33
                    v = pass == 0 ? floor_div(y - x, w) : (y + x) / w;              // :424 / :426
                }
                s_v[t] = v;
            }
            __syncthreads();
            res[pass] = BIG ? mode_sorted(s_v, m, n2, lane) : mode_all_pairs(s_v, m, lane);
        }
        if (lane == 0) { diag[r] = res[0]; anti[r] = res[1]; }
    }
}

}  // namespace

extern "C" int hhx_ingest_concordance(hhx_ingest *h, int64_t max_read_pairs, int64_t min_read_pairs, int64_t nwindows, int32_t *m, int32_t *diag,
                                      int32_t *anti) {
    if (!h || !h->finalized) return fail("ingest handle not finalized");
    if (!h->keep_pairs) return fail("hhx_ingest_concordance: the handle was not created with hhx_ingest_keep_pairs");
    if (max_read_pairs < 1 || nwindows < 1) return fail("hhx_ingest_concordance: max_read_pairs and nwindows must be positive");
    if (max_read_pairs > AL_CAP) { fail("hhx_ingest_concordance: max_read_pairs %lld is beyond the %d pairs a wavefront sorts in LDS", (long long)max_read_pairs, AL_CAP); return HHX_UNSUPPORTED; }
    if (min_read_pairs > max_read_pairs) min_read_pairs = max_read_pairs;       // a key that reached max_read_pairs is always evaluated (:461)
    PairGroups G;
    HHX_TRY(group_pairs(h, G, "hhx_ingest_concordance"));
    const i64 K = G.K;
    if (K == 0) return 0;
    if (!m || !diag || !anti) return fail("hhx_ingest_concordance: null output");
    KTimer kt("concordance");
    DevBuf<i32> out;
    DevBuf<unsigned int> bad;
    if (out.alloc((size_t)K * 3) || bad.alloc(1)) return 1;
    HHX_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned int), g_stream));
    HHX_HIP(hipMemsetAsync(out.p, 0, sizeof(i32) * (size_t)K * 3, g_stream));
    const unsigned grid = (unsigned)std::min<i64>(K, 256 * 64);
    k_concordance<AL_SMALL, false><<<grid, HHX_WAVE, 0, g_stream>>>(K, G.stk.p, G.gstart.p, G.srank.p, G.sxy.p, h->t.ctg, max_read_pairs, min_read_pairs, nwindows,
                                                                    out.p, out.p + K, out.p + 2 * K, bad.p);
    HHX_LAUNCH_CHECK();
    if (max_read_pairs > AL_SMALL) {
        k_concordance<AL_CAP, true><<<grid, HHX_WAVE, 0, g_stream>>>(K, G.stk.p, G.gstart.p, G.srank.p, G.sxy.p, h->t.ctg, max_read_pairs, min_read_pairs, nwindows,
                                                                     out.p, out.p + K, out.p + 2 * K, bad.p);
        HHX_LAUNCH_CHECK();
    }
    unsigned int hb = 0;
    HHX_HIP(hipMemcpyAsync(&hb, bad.p, sizeof hb, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(m, out.p, sizeof(i32) * (size_t)K, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(diag, out.p + K, sizeof(i32) * (size_t)K, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(anti, out.p + 2 * K, sizeof(i32) * (size_t)K, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (hb) { fail("hhx_ingest_concordance: a contig shorter than nwindows (window width 0)"); return HHX_UNSUPPORTED; }
    return 0;
}

// ================================================================================================ drop_links
namespace {

__global__ __launch_bounds__(256) void k_drop_keys(i64 n, const i32 *__restrict__ fi, const i32 *__restrict__ fj, const uint8_t *__restrict__ drop,
                                                   const i64 *__restrict__ pos, u64 *__restrict__ out) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x)
        if (drop[r]) out[pos[r]] = ((u64)(u32)fi[r] << ID_BITS) | (u64)(u32)fj[r];
}
__global__ __launch_bounds__(256) void k_flags_from_bytes(i64 n, const uint8_t *__restrict__ b, i64 *__restrict__ flag, int invert) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) flag[r] = ((b[r] != 0) != (invert != 0)) ? 1 : 0;
}

struct DropSet {             // the dropped contig pairs as ascending keys + what maps a flank row to its contig pair
    const u64 *keys;
    i64 n;
    const uint8_t *in_set;   // [n_frag]
    const i32 *frag_ctg;     // [n_frag], null: fragment == contig (the combined table)
    const UnitInfo *ctg;
};
__device__ __forceinline__ bool key_dropped(const DropSet &D, u64 key) {
    i64 lo = 0, hi = D.n;
    while (lo < hi) { const i64 mid = (lo + hi) >> 1; if (D.keys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < D.n && D.keys[lo] == key;
}
// :499-509 — the flank key (fi, fj) leaves when its contig pair was dropped and both fragments are in filtered_frags
__device__ __forceinline__ bool flank_leaves(const DropSet &D, i32 fi, i32 fj) {
    if (!(D.in_set[fi] && D.in_set[fj])) return false;
    u64 key = ((u64)(u32)fi << ID_BITS) | (u64)(u32)fj;
    if (D.frag_ctg) {
        i32 ci = D.frag_ctg[fi], cj = D.frag_ctg[fj];
        if (ci == cj) return false;                               // bins of one contig: never a full_link_dict key (:1736)
        if (D.ctg[ci].rank > D.ctg[cj].rank) { const i32 t = ci; ci = cj; cj = t; }      // ctg_pair_to_frag is keyed by the sorted contig names (:1731)
        key = ((u64)(u32)ci << ID_BITS) | (u64)(u32)cj;
    }
    return key_dropped(D, key);
}

// the rows of the aggregated tables: NO_ORD = "not in this dict" (hhx_ingest.h)
__global__ __launch_bounds__(256) void k_drop_rows(i64 n, const u64 *__restrict__ key, u64 *__restrict__ ord_full, u64 *__restrict__ ord_flank, DropSet D,
                                                   int do_full, int do_flank, unsigned long long *__restrict__ counts) {
    i64 cf = 0, ck = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const u64 k = key[i];
        if (do_flank && ord_flank[i] != NO_ORD && flank_leaves(D, (i32)(k >> ID_BITS), (i32)(k & ID_MASK))) { ord_flank[i] = NO_ORD; ++ck; }
        if (do_full && ord_full[i] != NO_ORD && key_dropped(D, k)) { ord_full[i] = NO_ORD; ++cf; }
    }
    cf = wave_sum_i64(cf); ck = wave_sum_i64(ck);
    if (lane_id() == 0) {
        if (cf) atomicAdd(&counts[0], (unsigned long long)cf);
        if (ck) atomicAdd(&counts[1], (unsigned long long)ck);
    }
}
// the flank table in dict order as it was before the drop: which rows leave, and :680-683 over those that stay
__global__ __launch_bounds__(256) void k_drop_flank_ordered(i64 n, const i32 *__restrict__ fi, const i32 *__restrict__ fj, DropSet D, uint8_t *__restrict__ dropped,
                                                            i64 *__restrict__ keep, uint8_t *__restrict__ remaining, unsigned long long *__restrict__ first_row,
                                                            unsigned long long *__restrict__ counts) {
    i64 ck = 0;
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
        const i32 a = fi[r], b = fj[r];
        const bool gone = flank_leaves(D, a, b);
        dropped[r] = gone ? 1 : 0;
        keep[r] = gone ? 0 : 1;
        ck += gone;
        if (!gone && D.in_set[a] && D.in_set[b]) {
            remaining[a] = 1; remaining[b] = 1;
            atomicMin(&first_row[a], (unsigned long long)(2 * r));
            atomicMin(&first_row[b], (unsigned long long)(2 * r + 1));
        }
    }
    ck = wave_sum_i64(ck);
    if (lane_id() == 0 && ck) atomicAdd(&counts[2], (unsigned long long)ck);
}
__global__ __launch_bounds__(256) void k_compact_f64(i64 n, const i64 *__restrict__ keep, const i64 *__restrict__ pos, const double *__restrict__ in, double *__restrict__ out) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x)
        if (keep[r]) out[pos[r]] = in[r];
}

}  // namespace

extern "C" int hhx_ingest_drop_links(hhx_ingest *h, const uint8_t *full_drop, const uint8_t *in_set, int64_t *n_full_left, int64_t *n_flank_left,
                                     uint8_t *flank_dropped, uint8_t *remaining, int64_t *first_row) {
    if (!h || !h->finalized) return fail("ingest handle not finalized");
    if (!full_drop || !in_set) return fail("hhx_ingest_drop_links: null pointer");
    if (!h->combined && h->frag_ctg.empty()) { fail("hhx_ingest_drop_links: the fragments of the contigs are not numbered in contig order"); return HHX_UNSUPPORTED; }
    files_wait_handle(h);                                        // queued files read the tables this call rewrites
    const i32 *ofi = nullptr, *ofj = nullptr;
    HHX_TRY(hhx_ingest_ordered_full_device(h, &ofi, &ofj));      // the dict-ordered tables as they are now
    const i64 K = h->n_full, F = h->n_flank;
    const i32 n_frag = h->t.n_frag;
    KTimer kt("drop_links");
    // ---- the dropped contig pairs as a sorted key array
    DevBuf<uint8_t> d_drop, d_in, d_gone, d_rem;
    DevBuf<i64> flag, pos, keep, kpos;
    DevBuf<unsigned long long> counts, d_first;
    if (d_drop.alloc((size_t)K + 1) || d_in.alloc((size_t)n_frag) || d_gone.alloc((size_t)F + 1) || d_rem.alloc((size_t)n_frag) || flag.alloc((size_t)K + 1) ||
        pos.alloc((size_t)K + 2) || keep.alloc((size_t)F + 1) || kpos.alloc((size_t)F + 2) || counts.alloc(3) || d_first.alloc((size_t)n_frag)) return 1;
    if (K) HHX_HIP(hipMemcpyAsync(d_drop.p, full_drop, (size_t)K, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_in.p, in_set, (size_t)n_frag, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemsetAsync(d_rem.p, 0, (size_t)n_frag, g_stream));
    HHX_HIP(hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned long long) * (size_t)n_frag, g_stream));
    HHX_HIP(hipMemsetAsync(counts.p, 0, sizeof(unsigned long long) * 3, g_stream));
    i64 n_drop = 0;
    DevBuf<u64> dk, dks;
    if (K) {
        k_flags_from_bytes<<<grid_for((u64)K), 256, 0, g_stream>>>(K, d_drop.p, flag.p, 0);
        HHX_LAUNCH_CHECK();
        HHX_TRY(exclusive_scan_i64(flag.p, pos.p, K, &n_drop));
    }
    if (dk.alloc((size_t)n_drop) || dks.alloc((size_t)n_drop)) return 1;
    if (n_drop) {
        k_drop_keys<<<grid_for((u64)K), 256, 0, g_stream>>>(K, ofi, ofj, d_drop.p, pos.p, dk.p);
        HHX_LAUNCH_CHECK();
        HHX_TRY(stable_sort_pairs_u64(dk.p, dks.p, nullptr, nullptr, n_drop, 2 * ID_BITS));
    }
    DevBuf<i32> d_fc;
    if (!h->combined) {
        if (d_fc.alloc((size_t)n_frag)) return 1;
        HHX_HIP(hipMemcpyAsync(d_fc.p, h->frag_ctg.data(), sizeof(i32) * (size_t)n_frag, hipMemcpyHostToDevice, g_stream));
    }
    const DropSet D{dks.p, n_drop, d_in.p, h->combined ? nullptr : d_fc.p, h->t.ctg};
    // ---- the flank table in dict order (before the drop): flank_dropped, remaining, and what survives of the float64 values
    if (F) {
        k_drop_flank_ordered<<<grid_for((u64)F), 256, 0, g_stream>>>(F, h->ordered.flank_i.p, h->ordered.flank_j.p, D, d_gone.p, keep.p, d_rem.p, d_first.p, counts.p);
        HHX_LAUNCH_CHECK();
    }
    // ---- the aggregated rows
    LinkRun *rf = h->runs[0].empty() ? nullptr : h->runs[0][0];
    LinkRun *rk = h->combined ? nullptr : (h->runs[1].empty() ? nullptr : h->runs[1][0]);
    if (rf && rf->n) {
        k_drop_rows<<<grid_for((u64)rf->n), 256, 0, g_stream>>>(rf->n, rf->key.p, rf->ord_full.p, rf->ord_flank.p, D, 1, h->combined ? 1 : 0, counts.p);
        HHX_LAUNCH_CHECK();
    }
    if (rk && rk->n) {
        k_drop_rows<<<grid_for((u64)rk->n), 256, 0, g_stream>>>(rk->n, rk->key.p, rk->ord_full.p, rk->ord_flank.p, D, 0, 1, counts.p);
        HHX_LAUNCH_CHECK();
    }
    i64 n_keep = 0;
    if (F) HHX_TRY(exclusive_scan_i64(keep.p, kpos.p, F, &n_keep));
    unsigned long long hc[3] = {0, 0, 0};
    HHX_HIP(hipMemcpyAsync(hc, counts.p, sizeof hc, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    h->links_dropped = h->links_dropped || hc[0] || hc[1];
    if ((i64)hc[0] != n_drop || hc[1] != hc[2] || n_keep != F - (i64)hc[2])
        return fail("hhx_ingest_drop_links: the rows and the dict-ordered tables disagree (%llu of %lld full keys, %llu / %llu flank keys)", hc[0], (long long)n_drop,
                    hc[1], hc[2]);
    // ---- the smaller dicts: counts, cached statistics, and the dict-ordered tables made again from the rows.  Two things are carried over:
    // the float64 flank values (weights of hhx_link_weights live only there) and frag_links (frag_link_dict does not change, :488-509)
    OrderedTables old = std::move(h->ordered);
    h->ordered = OrderedTables();
    h->n_full = K - (i64)hc[0];
    h->n_flank = F - (i64)hc[1];
    if (rf && rf->has_stats) { rf->stats[0] -= hc[0]; if (h->combined) rf->stats[1] -= hc[1]; }
    if (rk && rk->has_stats) rk->stats[1] -= hc[1];
    HHX_TRY(hhx_ingest_ordered_full_device(h, &ofi, &ofj));
    if (h->ordered.n_flank != n_keep) return fail("hhx_ingest_drop_links: %lld flank keys after the drop, %lld expected", (long long)h->ordered.n_flank, (long long)n_keep);
    if (F) {
        k_compact_f64<<<grid_for((u64)F), 256, 0, g_stream>>>(F, keep.p, kpos.p, old.flank_val.p, h->ordered.flank_val.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(h->ordered.frag_links.p, old.frag_links.p, sizeof(unsigned long long) * (size_t)n_frag, hipMemcpyDeviceToDevice, g_stream));
    if (flank_dropped && F) HHX_HIP(hipMemcpyAsync(flank_dropped, d_gone.p, (size_t)F, hipMemcpyDeviceToHost, g_stream));
    if (remaining) HHX_HIP(hipMemcpyAsync(remaining, d_rem.p, (size_t)n_frag, hipMemcpyDeviceToHost, g_stream));
    if (first_row) HHX_HIP(hipMemcpyAsync(first_row, d_first.p, sizeof(i64) * (size_t)n_frag, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (n_full_left) *n_full_left = h->n_full;
    if (n_flank_left) *n_flank_left = h->n_flank;
    return 0;
}
