// --remove_allelic_links on the device tables (remove_allelic_HiC_links :474-692): the two halves of it that touch every key.
//   hhx_ingest_concordance  record_coord_pairs :454-465 + cal_concordance_ratio :419-428 as integers: per full_link_dict key, the modal
//                           counts of the diagonal / anti-diagonal windows of its first max_read_pairs read pairs (stream order)
//   hhx_ingest_drop_links   update_link_dicts :488-509 for a whole verdict at once + the isolated-fragment pass :678-692
//   hhx_allelic_nonmax      the links between non-maximum matches :621-667 (stage 2) on plain host arrays: candidate keys x their allele groups,
//                           one sort by group pair, one worker per pair (matrix in LDS, linear_sum_assignment's own method and tie rule)
//   hhx_lsap_small          that solver alone, batched
// What lies between — the cliques of the allele graph (networkx) — is host code (haphic_amd/allelic.py).
//
// The read pairs are grouped by contig pair with the stable key sort the coordinate lists and paired_links.clm already use
// (hhx::group_pairs, hhx_pairs.hip); the grouped records stay in HBM.  The two hhx_ingest_ entries run on the calling thread's stream and pool arena and
// only READ the side records, so a queued paired_links.clm (hhx_ingest_write_clm_async) may be reading them at the same time.
// hhx_ingest_drop_links changes the tables and therefore first waits for the files queued on this handle.
#include <algorithm>
#include <cstdlib>

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

// ================================================================================================ stage 2: links between non-maximum matches
// remove_allelic_HiC_links :621-667.  A key both of whose contigs sit in allele groups yields one combination per (group of ctg_1) x (group of
// ctg_2); the combinations are sorted by their group pair (ga <= gb, ranks under the reference's tuple order), so the combinations of one pair
// are one run.  Every non-zero cell of the pair's degree x degree matrix (:552-568) is a key between the two groups, and every such key is
// a combination of this very run: the worker of a pair fills the matrix from its run, in both roles where a contig sits in both groups.
namespace {

constexpr int NM_MAXD = 8;             // largest allele group served (ploidy); documented in haphic_hip.h
constexpr u32 NM_NONE = 0xF;           // "not in the group" / "unassigned" in a 4-bit field
constexpr i64 NM_INF = INT64_MAX;      // +inf of shortestPathCosts: compared, never added to

__device__ __forceinline__ u32 nib(u32 w, int k) { return (w >> (4 * k)) & 0xFu; }
__device__ __forceinline__ u32 set_nib(u32 w, int k, u32 x) { return (w & ~(0xFu << (4 * k))) | (x << (4 * k)); }

// workgroups of the stage-2 passes at most (HHX_NONMAX_GRID, read at every launch: a test walks the grid-stride loops on two workgroups)
inline unsigned nonmax_grid(u64 n, unsigned per) {
    u64 b = (n + per - 1) / per;
    if (b < 1) b = 1;
    if (b > 256 * 16) b = 256 * 16;
    const char *e = getenv("HHX_NONMAX_GRID");
    if (e && atoi(e) > 0 && (u64)atoi(e) < b) b = (u64)atoi(e);
    return (unsigned)b;
}
inline size_t nonmax_lds_bytes(int d) { return (size_t)(d * d + 3 * d) * HHX_WAVE * sizeof(i64); }

// scipy.optimize.linear_sum_assignment (1.15: the shortest augmenting path method with dual variables, Crouse's variant of Jonker-Volgenant)
// on a d x d int64 cost matrix, minimising, with scipy's own scan order and tie rule, so that the assignment is scipy's among equal optima:
// `remaining` starts as [d-1 .. 0] and a visited column is replaced by the last one; a column as cheap as the cheapest so far takes its place
// only when it is unassigned.  All quantities are sums and differences of the integer costs (exact in scipy's doubles below 2^53).
// One problem per lane: cost cell (i, j) at cost[(i * d + j) * 64], u / v / sp element k at [k * 64] (the lane's own LDS column: no two lanes
// of a wave share a bank); path, row4col, col4row and remaining are 4-bit fields of a register.  Returns col4row.
__device__ __forceinline__ u32 lsap_solve(int d, const i64 *cost, i64 *u, i64 *v, i64 *sp) {
    u32 col4row = ~0u, row4col = ~0u;
    for (int k = 0; k < d; ++k) { u[k * HHX_WAVE] = 0; v[k * HHX_WAVE] = 0; }
    for (int cur = 0; cur < d; ++cur) {
        u32 remaining = 0, path = 0, SR = 0, SC = 0;
        for (int it = 0; it < d; ++it) { remaining |= (u32)(d - 1 - it) << (4 * it); sp[it * HHX_WAVE] = NM_INF; }
        int num_remaining = d, i = cur, sink = -1;
        i64 min_val = 0;
        while (sink < 0 && num_remaining > 0) {                  // (an unassigned column is left while cur < d: the second test never ends the loop)
            int index = 0;
            i64 lowest = NM_INF;
            SR |= 1u << i;
            const i64 ui = u[i * HHX_WAVE];
            for (int it = 0; it < num_remaining; ++it) {
                const int j = (int)nib(remaining, it);
                const i64 r = min_val + cost[(i * d + j) * HHX_WAVE] - ui - v[j * HHX_WAVE];
                i64 s = sp[j * HHX_WAVE];
                if (r < s) { path = set_nib(path, j, (u32)i); s = r; sp[j * HHX_WAVE] = r; }
                if (s < lowest || (s == lowest && nib(row4col, j) == NM_NONE)) { lowest = s; index = it; }
            }
            min_val = lowest;
            const int j = (int)nib(remaining, index);
            const u32 owner = nib(row4col, j);
            if (owner == NM_NONE) sink = j; else i = (int)owner;
            SC |= 1u << j;
            --num_remaining;
            remaining = set_nib(remaining, index, nib(remaining, num_remaining));
        }
        if (sink < 0) break;
        u[cur * HHX_WAVE] += min_val;
        for (int k = 0; k < d; ++k)
            if (((SR >> k) & 1u) && k != cur) u[k * HHX_WAVE] += min_val - sp[nib(col4row, k) * HHX_WAVE];     // a visited row other than cur is assigned, its column visited
        for (int j = 0; j < d; ++j)
            if ((SC >> j) & 1u) v[j * HHX_WAVE] -= min_val - sp[j * HHX_WAVE];
        int j = sink;
        for (int step = 0; step < d; ++step) {                   // flip the path back from the sink (at most d edges)
            const u32 r = nib(path, j);
            row4col = set_nib(row4col, j, r);
            const u32 before = nib(col4row, (int)r);
            col4row = set_nib(col4row, (int)r, (u32)j);
            if ((int)r == cur) break;
            j = (int)before;
        }
    }
    return col4row;
}

__global__ __launch_bounds__(HHX_WAVE) void k_lsap_small(i64 n, int d, const i64 *__restrict__ cost, i32 *__restrict__ col4row) {
    extern __shared__ __attribute__((aligned(16))) i64 s_nm[];
    const int lane = threadIdx.x;
    i64 *m = s_nm + lane, *u = m + (size_t)d * d * HHX_WAVE, *v = u + d * HHX_WAVE, *sp = v + d * HHX_WAVE;
    for (i64 p = (i64)blockIdx.x * HHX_WAVE + lane; p < n; p += (i64)gridDim.x * HHX_WAVE) {
        for (int c = 0; c < d * d; ++c) m[c * HHX_WAVE] = cost[p * d * d + c];
        const u32 sol = lsap_solve(d, m, u, v, sp);
        for (int k = 0; k < d; ++k) col4row[p * d + k] = (i32)nib(sol, k);
    }
}

// the groups of every contig (ctg_allele_group_dict :624-627): cg_ptr [n_ctg + 1], cg_grp ascending per contig
__global__ __launch_bounds__(256) void k_nonmax_count(i64 n, const i32 *__restrict__ ki, const i32 *__restrict__ kj, i32 n_ctg, const i32 *__restrict__ cg_ptr,
                                                      i64 *__restrict__ combos, unsigned long long *__restrict__ counters, unsigned int *__restrict__ flags) {
    i64 cand = 0;
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
        const i32 a = ki[r], b = kj[r];
        i64 c = 0;
        if (a < 0 || a >= n_ctg || b < 0 || b >= n_ctg) atomicExch(&flags[1], 1u);
        else c = (i64)(cg_ptr[a + 1] - cg_ptr[a]) * (i64)(cg_ptr[b + 1] - cg_ptr[b]);      // :639, :642-643
        combos[r] = c;
        cand += c > 0;
    }
    cand = wave_sum_i64(cand);
    if (lane_id() == 0 && cand) atomicAdd(&counters[0], (unsigned long long)cand);
}

// position of contig c in group g (tuple.index), NM_NONE when it is no member
__device__ __forceinline__ u32 pos_in(const i32 *__restrict__ gptr, const i32 *__restrict__ gmem, i32 g, i32 c) {
    const i32 b = gptr[g], e = gptr[g + 1];
    for (i32 t = b; t < e; ++t)
        if (gmem[t] == c) return (u32)(t - b);
    return NM_NONE;
}

// one (key, group_1, group_2) combination per slot: sort key ga * nG + gb, value = key index << 16 | the positions of ctg_1 and ctg_2 in ga and gb
__global__ __launch_bounds__(256) void k_nonmax_expand(i64 n, const i32 *__restrict__ ki, const i32 *__restrict__ kj, const i64 *__restrict__ off,
                                                       const i32 *__restrict__ cg_ptr, const i32 *__restrict__ cg_grp, const i32 *__restrict__ gptr,
                                                       const i32 *__restrict__ gmem, i64 nG, u64 *__restrict__ skey, u64 *__restrict__ sval,
                                                       unsigned int *__restrict__ flags) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
        i64 at = off[r];
        if (off[r + 1] == at) continue;
        const i32 c1 = ki[r], c2 = kj[r];
        const i32 b1 = cg_ptr[c1], e1 = cg_ptr[c1 + 1], b2 = cg_ptr[c2], e2 = cg_ptr[c2 + 1];
        for (i32 x = b1; x < e1; ++x)
            for (i32 y = b2; y < e2; ++y) {
                const i32 g1 = cg_grp[x], g2 = cg_grp[y];
                const i32 ga = g1 < g2 ? g1 : g2, gb = g1 < g2 ? g2 : g1;                  // group_pair :644
                const u32 a1 = pos_in(gptr, gmem, ga, c1), a2 = pos_in(gptr, gmem, ga, c2), p1 = pos_in(gptr, gmem, gb, c1), p2 = pos_in(gptr, gmem, gb, c2);
                // :652-659 — ctg_1 in group_pair[0] asks for ctg_2 in group_pair[1]; else ctg_2 in group_pair[0] and ctg_1 in group_pair[1]
                if (a1 != NM_NONE ? p2 == NM_NONE : (a2 == NM_NONE || p1 == NM_NONE)) atomicExch(&flags[0], 1u);
                skey[at] = (u64)ga * (u64)nG + (u64)gb;
                sval[at] = ((u64)r << 16) | a1 | (a2 << 4) | (p1 << 8) | (p2 << 12);
                ++at;
            }
    }
}

// One worker (lane) per group pair: the lane that holds the head of a run walks it.  The matrix holds -count (the reference solves
// linear_sum_assignment(-matrix) :568) in the lane's LDS column and never goes to global memory.  A run of one combination that fills one
// cell needs neither matrix nor solver: every optimal assignment contains the only non-zero cell, and its key is the only one that asks.
__global__ __launch_bounds__(HHX_WAVE) void k_nonmax_pairs(i64 n, const u64 *__restrict__ skey, const u64 *__restrict__ sval, const i64 *__restrict__ kcnt, i64 nG,
                                                          const i32 *__restrict__ gptr, int dmax, uint8_t *__restrict__ nonmax,
                                                          unsigned long long *__restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) i64 s_nm[];
    const int lane = threadIdx.x;
    i64 *m = s_nm + lane, *u = m + (size_t)dmax * dmax * HHX_WAVE, *v = u + dmax * HHX_WAVE, *sp = v + dmax * HHX_WAVE;
    i64 pairs = 0, solved = 0;
    for (i64 i = (i64)blockIdx.x * HHX_WAVE + lane; i < n; i += (i64)gridDim.x * HHX_WAVE) {
        const u64 k = skey[i];
        if (i > 0 && skey[i - 1] == k) continue;                // not the head of a run
        ++pairs;
        i64 e = i + 1;
        while (e < n && skey[e] == k) ++e;
        if (e == i + 1) {
            const u32 w = (u32)sval[i];
            const bool role_a = nib(w, 0) != NM_NONE && nib(w, 3) != NM_NONE, role_b = nib(w, 1) != NM_NONE && nib(w, 2) != NM_NONE;
            if (!(role_a && role_b)) continue;
        }
        const i32 ga = (i32)(k / (u64)nG), gb = (i32)(k % (u64)nG);
        const int la = gptr[ga + 1] - gptr[ga], lb = gptr[gb + 1] - gptr[gb];
        const int d = la > lb ? la : lb;                        // :553 (<= dmax: the host sized the LDS by the largest group)
        for (int c = 0; c < d * d; ++c) m[c * HHX_WAVE] = 0;
        for (i64 t = i; t < e; ++t) {
            const u64 val = sval[t];
            const u32 w = (u32)val;
            const i64 links = kcnt[val >> 16];
            const u32 a1 = nib(w, 0), a2 = nib(w, 1), p1 = nib(w, 2), p2 = nib(w, 3);
            if (a1 != NM_NONE && p2 != NM_NONE) m[(a1 * d + p2) * HHX_WAVE] = -links;       // ctg_1 a row of group_pair[0], ctg_2 a column of group_pair[1]
            if (a2 != NM_NONE && p1 != NM_NONE) m[(a2 * d + p1) * HHX_WAVE] = -links;       // ... and the other way round
        }
        int cells = 0;
        for (int c = 0; c < d * d; ++c) cells += m[c * HHX_WAVE] != 0;
        if (cells <= 1) continue;
        ++solved;
        const u32 sol = lsap_solve(d, m, u, v, sp);
        for (i64 t = i; t < e; ++t) {
            const u64 val = sval[t];
            const u32 w = (u32)val;
            const bool first = nib(w, 0) != NM_NONE;                                        // :652
            const u32 index_1 = first ? nib(w, 0) : nib(w, 1), index_2 = first ? nib(w, 3) : nib(w, 2);
            if (index_1 != NM_NONE && index_2 != NM_NONE && nib(sol, (int)index_1) != index_2) nonmax[val >> 16] = 1;      // :661 (idempotent byte store)
        }
    }
    pairs = wave_sum_i64(pairs); solved = wave_sum_i64(solved);
    if (lane == 0) {
        if (pairs) atomicAdd(&counters[1], (unsigned long long)pairs);
        if (solved) atomicAdd(&counters[2], (unsigned long long)solved);
    }
}

}  // namespace

extern "C" int hhx_lsap_small(int64_t n, int32_t d, const int64_t *cost, int32_t *col4row) {
    if (n < 0 || d < 1 || d > NM_MAXD) return fail("hhx_lsap_small: n >= 0 and 1 <= d <= %d", NM_MAXD);
    if (n == 0) return 0;
    if (!cost || !col4row) return fail("hhx_lsap_small: null pointer");
    const size_t cells = (size_t)n * d * d, outs = (size_t)n * d;
    DevBuf<i64> dc;
    DevBuf<i32> ds;
    if (dc.alloc(cells) || ds.alloc(outs)) return 1;
    HHX_HIP(hipMemcpyAsync(dc.p, cost, sizeof(i64) * cells, hipMemcpyHostToDevice, g_stream));
    {
        KTimer kt("lsap_small");
        k_lsap_small<<<nonmax_grid((u64)n, HHX_WAVE), HHX_WAVE, nonmax_lds_bytes(d), g_stream>>>(n, d, dc.p, ds.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(col4row, ds.p, sizeof(i32) * outs, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_allelic_nonmax(int64_t n_keys, const int32_t *ki, const int32_t *kj, const int64_t *kcnt, int32_t n_ctg, int32_t n_groups,
                                  const int64_t *gptr, const int32_t *gmem, uint8_t *nonmax, int64_t *counters, int32_t *assert_failed) {
    if (n_keys < 0 || n_ctg < 0 || n_groups < 0) return fail("hhx_allelic_nonmax: bad arguments");
    if (!counters || !assert_failed || (n_keys && (!ki || !kj || !kcnt || !nonmax)) || (n_groups && (!gptr || !gmem))) return fail("hhx_allelic_nonmax: null pointer");
    counters[0] = counters[1] = counters[2] = 0;
    *assert_failed = 0;
    // ---- the groups (few and small: host work): checked, then turned round into the groups of every contig
    int dmax = 0;
    const i64 n_mem = n_groups ? gptr[n_groups] : 0;
    if (n_groups && gptr[0] != 0) return fail("hhx_allelic_nonmax: gptr[0] must be 0");
    for (i32 g = 0; g < n_groups; ++g) {
        const i64 len = gptr[g + 1] - gptr[g];
        if (len < 0 || gptr[g + 1] > INT32_MAX) return fail("hhx_allelic_nonmax: gptr must ascend and fit 32 bits");
        if (len > NM_MAXD) { fail("hhx_allelic_nonmax: an allele group of %lld contigs is beyond the %d a lane solves in LDS", (long long)len, NM_MAXD); return HHX_UNSUPPORTED; }
        dmax = std::max(dmax, (int)len);
    }
    for (i64 t = 0; t < n_mem; ++t)
        if (gmem[t] < 0 || gmem[t] >= n_ctg) return fail("hhx_allelic_nonmax: group member %d is no contig id", (int)gmem[t]);
    if (n_keys) memset(nonmax, 0, (size_t)n_keys);
    if (n_keys == 0 || n_groups == 0 || n_mem == 0) return 0;
    std::vector<i32> h_gptr((size_t)n_groups + 1), cg_ptr((size_t)n_ctg + 1, 0), cg_grp((size_t)n_mem);
    for (i32 g = 0; g <= n_groups; ++g) h_gptr[g] = (i32)gptr[g];
    for (i64 t = 0; t < n_mem; ++t) ++cg_ptr[gmem[t] + 1];
    for (i32 c = 0; c < n_ctg; ++c) cg_ptr[c + 1] += cg_ptr[c];
    {
        std::vector<i32> fill(cg_ptr.begin(), cg_ptr.end() - 1);
        for (i32 g = 0; g < n_groups; ++g)
            for (i32 t = h_gptr[g]; t < h_gptr[g + 1]; ++t) cg_grp[fill[gmem[t]]++] = g;       // ascending group per contig
    }
    DevBuf<i32> d_ki, d_kj, d_gptr, d_gmem, d_cgp, d_cgg;
    DevBuf<i64> d_cnt, combos, off;
    DevBuf<unsigned long long> d_counters;
    DevBuf<unsigned int> flags;
    DevBuf<uint8_t> d_out;
    const size_t n = (size_t)n_keys;
    if (d_ki.alloc(n) || d_kj.alloc(n) || d_cnt.alloc(n) || combos.alloc(n + 1) || off.alloc(n + 2) || d_gptr.alloc(h_gptr.size()) || d_gmem.alloc((size_t)n_mem) ||
        d_cgp.alloc(cg_ptr.size()) || d_cgg.alloc(cg_grp.size()) || d_counters.alloc(3) || flags.alloc(2) || d_out.alloc(n)) return 1;
    HHX_HIP(hipMemcpyAsync(d_ki.p, ki, sizeof(i32) * n, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_kj.p, kj, sizeof(i32) * n, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_cnt.p, kcnt, sizeof(i64) * n, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_gptr.p, h_gptr.data(), sizeof(i32) * h_gptr.size(), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_gmem.p, gmem, sizeof(i32) * (size_t)n_mem, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_cgp.p, cg_ptr.data(), sizeof(i32) * cg_ptr.size(), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_cgg.p, cg_grp.data(), sizeof(i32) * cg_grp.size(), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemsetAsync(d_counters.p, 0, sizeof(unsigned long long) * 3, g_stream));
    HHX_HIP(hipMemsetAsync(flags.p, 0, sizeof(unsigned int) * 2, g_stream));
    HHX_HIP(hipMemsetAsync(d_out.p, 0, n, g_stream));
    KTimer kt("allelic_nonmax");
    // ---- 1) the combinations of every key: count, scan, expand
    k_nonmax_count<<<nonmax_grid((u64)n_keys, 256), 256, 0, g_stream>>>(n_keys, d_ki.p, d_kj.p, n_ctg, d_cgp.p, combos.p, d_counters.p, flags.p);
    HHX_LAUNCH_CHECK();
    i64 n_combos = 0;
    HHX_TRY(exclusive_scan_i64(combos.p, off.p, n_keys, &n_combos));
    unsigned int hf[2] = {0, 0};
    HHX_HIP(hipMemcpyAsync(hf, flags.p, sizeof hf, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (hf[1]) return fail("hhx_allelic_nonmax: a key names a contig outside [0, n_ctg)");
    unsigned long long hc[3] = {0, 0, 0};
    if (n_combos > 0) {
        DevBuf<u64> skey, sval, okey, oval;
        if (skey.alloc((size_t)n_combos) || sval.alloc((size_t)n_combos) || okey.alloc((size_t)n_combos) || oval.alloc((size_t)n_combos)) return 1;
        k_nonmax_expand<<<nonmax_grid((u64)n_keys, 256), 256, 0, g_stream>>>(n_keys, d_ki.p, d_kj.p, off.p, d_cgp.p, d_cgg.p, d_gptr.p, d_gmem.p, (i64)n_groups,
                                                                             skey.p, sval.p, flags.p);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(hf, flags.p, sizeof hf, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        if (hf[0]) {                                             // an assert of :652-659 would fail: the caller lets the reference raise it
            *assert_failed = 1;
            HHX_HIP(hipMemcpyAsync(hc, d_counters.p, sizeof hc, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipStreamSynchronize(g_stream));
            counters[0] = (i64)hc[0];
            return 0;
        }
        // ---- 2) by group pair: only the bits ga * nG + gb can have
        int bits = 1;
        while (bits < 64 && (((u64)n_groups * (u64)n_groups - 1) >> bits) != 0) ++bits;
        HHX_TRY(stable_sort_pairs_u64(skey.p, okey.p, sval.p, oval.p, n_combos, bits));
        // ---- 3) one worker per pair
        k_nonmax_pairs<<<nonmax_grid((u64)n_combos, HHX_WAVE), HHX_WAVE, nonmax_lds_bytes(dmax), g_stream>>>(n_combos, okey.p, oval.p, d_cnt.p, (i64)n_groups, d_gptr.p,
                                                                                                           dmax, d_out.p, d_counters.p);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(nonmax, d_out.p, n, hipMemcpyDeviceToHost, g_stream));
    }
    HHX_HIP(hipMemcpyAsync(hc, d_counters.p, sizeof hc, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    for (int k = 0; k < 3; ++k) counters[k] = (i64)hc[k];
    return 0;
}
