// Assembly correction (--correct_nrounds) on the device: HapHiC_cluster.py parse_pairs_for_correction :1300-1344 /
// parse_bam_for_correction :1362-1398 (pass one: per-contig coverage in bins of correct_resolution + the (lo, hi) position
// list of every intra-contig read pair), detect_break_points :943-1014, the per-pair half of break_and_update_ctgs
// :1063-1113 :1153 :1178 :1192-1197, and convert_ctg :1405-1411 (pass two: original contig / position -> corrected contig).
//
// Layout.  Contig c of the FASTA owns len_c // resolution + 1 bins of ONE flat int32 coverage array (segment = bin offset,
// bin count, length).  Break points are multiples of the resolution, so the children of a broken contig are VIEWS of their
// parent's bins (:1153 `cov[start//res : point//res]`, :1178 `cov[start//res:]` — numpy hands out views there too): a round
// of breaking rewrites the segment table and the pairs' labels, the coverage array stays where it is.
//
// Pass one per batch: k_cov_push keeps a record iff id1 == id2 >= 0, adds +1 / -1 to a difference array at the first bin
// and behind the last one (a slice that runs past the contig's bins is clipped as numpy clips it: the -1 is simply not
// written), flags it; the kept (contig, lo, hi) are compacted in file order (exclusive scan of the flags).  finalize: one
// stable radix sort by contig (hhx_sort.h: file order survives inside a contig, which is the order of `array('i').extend`
// :1342), a wave-per-segment scan of the difference array into the coverage.
//
// Everything is int32, as the reference's `array('i')` / ndarray(int32): contigs of 2^31 bp and more are refused.
#include "hhx_sort.h"

using namespace hhx;

struct hhx_correct {
    i32 res = 0;
    i64 total_bins = 0;
    bool finalized = false;
    // segment table (host copies + device)
    std::vector<i64> seg_off, pair_off;      // pair_off[n_seg + 1]
    std::vector<i32> seg_nb, seg_len;
    DevBuf<i64> d_seg_off;
    DevBuf<i32> d_seg_nb, d_seg_len;
    DevBuf<i32> cov, diff, cand;             // [total_bins]: coverage, pending +-1, break-point candidates of the last detect
    DevBuf<unsigned long long> cnt;          // kept pairs per segment
    DevBuf<i32> bad;                         // 1: a negative position was pushed
    // kept pairs: per push (key = contig, val = hi << 32 | lo) until finalize, afterwards `pairs` in segment order
    std::vector<DevBuf<u64>> chunk_key, chunk_val;
    std::vector<i64> chunk_n;
    DevBuf<u64> pairs;
    i64 n_pairs = 0;
    std::vector<i32> bp_bin;                 // break-point bins of the last detect, segment order
};

struct hhx_remap {
    i32 n_src = 0;
    DevBuf<i32> off, pos, id;
};

namespace {

constexpr int CR_T = 256;

template <class T>
int upload(DevBuf<T> &d, const T *h, size_t n) {
    if (d.alloc(n)) return 1;
    if (n) HHX_HIP(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, g_stream));
    return 0;
}

__device__ __forceinline__ i32 wave_max_i32(i32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, HHX_WAVE));
    return v;
}
__device__ __forceinline__ i32 wave_total_i32(i32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, HHX_WAVE);
    return v;
}

// one atomic add per distinct word among the active lanes of the wave (leader election by ballot); every lane of the wave must call it
template <class T>
__device__ __forceinline__ void wave_merged_add(T *base, i64 word, i32 value, bool active) {
    u64 todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const i64 w = __shfl(word, leader, HHX_WAVE);
        const u64 same = __ballot(active && word == w);
        i32 sum = active && word == w ? value : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, HHX_WAVE);
        if (lane_id() == leader) atomicAdd(&base[w], (T)sum);
        todo &= ~same;
    }
}

// :1327-1342.  flag[k] = 1 iff record k is kept; its coverage goes to the difference array at once.  AGG ("correct_agg"): the three adds of
// a record are merged across the wave first — worth it only when neighbouring records hit the same words (a file grouped by contig).
template <bool AGG>
__global__ __launch_bounds__(CR_T) void k_cov_push(i64 n, const i32 *__restrict__ id1, const i32 *__restrict__ pos1, const i32 *__restrict__ id2,
                                                   const i32 *__restrict__ pos2, i32 n_ctg, const i64 *__restrict__ seg_off,
                                                   const i32 *__restrict__ seg_nb, i32 res, i32 *__restrict__ diff,
                                                   unsigned long long *__restrict__ cnt, i32 *__restrict__ flag, i32 *__restrict__ bad) {
    if (AGG) {
        for (i64 k0 = (i64)blockIdx.x * CR_T; k0 < n; k0 += (i64)gridDim.x * CR_T) {          // whole waves walk together
            const i64 k = k0 + threadIdx.x;
            const bool in = k < n;
            const i32 a = in ? id1[k] : -1, b = in ? id2[k] : -1;
            bool keep = in && a == b && a >= 0 && a < n_ctg;
            i32 lo = 0, hi = 0;
            if (keep) {
                const i32 p = pos1[k], q = pos2[k];
                lo = min(p, q); hi = max(p, q);
                if (lo < 0) { *bad = 1; keep = false; }
            }
            const i64 off = keep ? seg_off[a] : 0;
            const i32 nb = keep ? seg_nb[a] : 0, sb = lo / res, eb = hi / res;
            wave_merged_add(diff, off + sb, 1, keep && sb < nb);
            wave_merged_add(diff, off + eb + 1, -1, keep && eb + 1 < nb);
            wave_merged_add(cnt, (i64)(keep ? a : 0), 1, keep);
            if (in) flag[k] = keep;
        }
        return;
    }
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T) {
        const i32 a = id1[k], b = id2[k];
        i32 keep = a == b && a >= 0 && a < n_ctg;                 // ref == mref, ref in fa_dict (-1: unknown name, -2: filtered BAM record)
        if (keep) {
            const i32 p = pos1[k], q = pos2[k];
            const i32 lo = min(p, q), hi = max(p, q);             // sorted([pos, mpos]) :1337
            if (lo < 0) { *bad = 1; keep = 0; }                   // same value from every writer
            else {
                const i64 off = seg_off[a];
                const i32 nb = seg_nb[a], sb = lo / res, eb = hi / res;
                if (sb < nb) atomicAdd(&diff[off + sb], 1);       // cov[sb : eb + 1] += 1 :1341, clipped at the contig's last bin
                if (eb + 1 < nb) atomicAdd(&diff[off + eb + 1], -1);
                atomicAdd(&cnt[a], 1ull);
            }
        }
        flag[k] = keep;
    }
}

__global__ __launch_bounds__(CR_T) void k_cov_compact(i64 n, const i32 *__restrict__ id1, const i32 *__restrict__ pos1, const i32 *__restrict__ pos2,
                                                      const i32 *__restrict__ flag, const i32 *__restrict__ at, u64 *__restrict__ key,
                                                      u64 *__restrict__ val) {
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T)
        if (flag[k]) {
            const i32 p = pos1[k], q = pos2[k];
            key[at[k]] = (u64)(u32)id1[k];
            val[at[k]] = ((u64)(u32)max(p, q) << 32) | (u64)(u32)min(p, q);     // in memory: lo, hi — two items of array('i')
        }
}

// A table that is not finalized yet, handed to another one (the ranks of a --gpus N job each fill a table from their byte range of the file):
// k_export_pairs narrows the kept records of one push to (contig, lo, hi) int32 columns; k_absorb_diff adds a partial difference array
// (difference arrays of disjoint record sets add); k_absorb_pairs appends records behind those already kept, counted per contig as k_cov_push
// counts them.  A record no push could have kept (contig outside the table, lo < 0, lo > hi) raises `bad` and is not counted; the caller then
// drops the whole chunk.
__global__ __launch_bounds__(CR_T) void k_export_pairs(i64 n, const u64 *__restrict__ key, const u64 *__restrict__ val, i32 *__restrict__ ctg,
                                                       i32 *__restrict__ lo_hi) {
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T) {
        const u64 v = val[k];
        ctg[k] = (i32)(u32)key[k];
        lo_hi[2 * k] = (i32)(u32)v;
        lo_hi[2 * k + 1] = (i32)(u32)(v >> 32);
    }
}

__global__ __launch_bounds__(CR_T) void k_absorb_diff(i64 n, const i32 *__restrict__ part, i32 *__restrict__ diff) {
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T) diff[k] += part[k];
}

__global__ __launch_bounds__(CR_T) void k_absorb_pairs(i64 n, const i32 *__restrict__ ctg, const i32 *__restrict__ lo_hi, i32 n_ctg,
                                                       u64 *__restrict__ key, u64 *__restrict__ val, unsigned long long *__restrict__ cnt,
                                                       i32 *__restrict__ bad) {
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T) {
        const i32 a = ctg[k], lo = lo_hi[2 * k], hi = lo_hi[2 * k + 1];
        const bool ok = a >= 0 && a < n_ctg && lo >= 0 && lo <= hi;
        key[k] = (u64)(u32)(ok ? a : 0);
        val[k] = ((u64)(u32)hi << 32) | (u64)(u32)lo;
        if (ok) atomicAdd(&cnt[a], 1ull);
        else *bad = 1;                                            // same value from every writer
    }
}

// cov[seg] += inclusive scan of diff[seg]; diff[seg] = 0.  One wave per segment (the typical contig has a few dozen bins).
__global__ __launch_bounds__(HHX_WAVE) void k_apply_diff(i32 n, const i64 *__restrict__ off_of, const i32 *__restrict__ nb_of, i32 *__restrict__ diff,
                                                         i32 *__restrict__ cov) {
    const int lane = threadIdx.x;
    for (i32 s = blockIdx.x; s < n; s += gridDim.x) {
        const i64 off = off_of[s];
        const i32 nb = nb_of[s];
        i32 carry = 0;
        for (i32 base = 0; base < nb; base += HHX_WAVE) {
            const i32 i = base + lane;
            i32 v = i < nb ? diff[off + i] : 0;
#pragma unroll
            for (int o = 1; o < HHX_WAVE; o <<= 1) {
                const i32 u = __shfl_up(v, o, HHX_WAVE);
                if (lane >= o) v += u;
            }
            if (i < nb) { cov[off + i] += carry + v; diff[off + i] = 0; }
            carry += __shfl(v, HHX_WAVE - 1, HHX_WAVE);
        }
    }
}

// s[k] of the segment's sorted coverage, all values in [0, 2^(top + 1)): the largest r with #{c < r} <= k, built bit by bit
__device__ __forceinline__ i32 kth_smallest(const i32 *__restrict__ c, i32 nb, i32 k, int top, int lane) {
    u32 r = 0;
    for (int bit = top; bit >= 0; --bit) {
        const u32 t = r | (1u << bit);
        i32 below = 0;
        for (i32 i = lane; i < nb; i += HHX_WAVE) below += (u32)c[i] < t;
        if (wave_total_i32(below) <= k) r = t;
    }
    return (i32)r;
}

// detect_break_points :943-1014 for every segment of the table, one wave per segment.  The reference's arithmetic, kept as it is:
//   median_cov  = numpy.median(cov_list): the middle value, or for an even bin count the float64 mean (a + b) / 2 of the two
//                 middle values; median 0 -> no break point (:954)
//   cov_cutoff  = median_cov * median_cov_ratio (float64); a bin is high iff float64(cov) >= cov_cutoff (:964)
//   adjacent high bins merge (closed intervals [n res, (n + 1) res] share an end point :965); a run of k bins is k * res long and
//   counts iff float64(k * res) >= max(min_region_cutoff, len * region_len_ratio) (:960 :973, float64)
//   fewer than two counting runs -> no break point (:977).  A valley = the bins strictly between two consecutive counting runs,
//   high bins of short runs included (:981 :989-990).  Its candidate: the leftmost 0-coverage bin if it has one (:993-996), else its
//   first minimum (argmin :999).  If any valley has a zero, every zero candidate is a break point (bin * res, 0), in order (:1005);
//   else the one candidate of smallest coverage, the earliest on ties (sorted is stable :1008).
// The sequential walk over the bins is done by the whole wave in step (64 bins loaded at once, handed round with __shfl; the
// state is wave-uniform); lane 0 writes.  cand[off + t] = bin of break point t; n_bp / bp_cov per segment.
__global__ __launch_bounds__(HHX_WAVE) void k_detect(i32 n_seg, const i64 *__restrict__ seg_off, const i32 *__restrict__ seg_nb,
                                                     const i32 *__restrict__ seg_len, i32 res, const i32 *__restrict__ cov, double median_cov_ratio,
                                                     double region_len_ratio, double min_region_cutoff, i32 *__restrict__ cand,
                                                     i32 *__restrict__ n_bp, i32 *__restrict__ bp_cov) {
    const int lane = threadIdx.x;
    for (i32 s = blockIdx.x; s < n_seg; s += gridDim.x) {
        const i64 off = seg_off[s];
        const i32 nb = seg_nb[s];
        const i32 *c = cov + off;
        i32 out_n = 0, out_cov = 0;
        i32 mx = 0;
        for (i32 i = lane; i < nb; i += HHX_WAVE) mx = max(mx, c[i]);
        mx = wave_max_i32(mx);
        double median = 0.0;
        if (nb > 0 && mx > 0) {
            const int top = 31 - __clz(mx);
            if (nb & 1) median = (double)kth_smallest(c, nb, nb / 2, top, lane);
            else median = ((double)kth_smallest(c, nb, nb / 2 - 1, top, lane) + (double)kth_smallest(c, nb, nb / 2, top, lane)) / 2.0;
        }
        if (median != 0.0) {
            const double cov_cutoff = median * median_cov_ratio;
            const double region_cutoff = fmax(min_region_cutoff, (double)seg_len[s] * region_len_ratio);
            i64 run = 0;                                          // high bins of the run being walked
            i32 n_counting = 0;                                   // counting runs closed so far
            i32 vz = -1, vminb = -1, vminv = INT32_MAX;           // bins since the last counting run: leftmost zero, first minimum
            i32 rz = -1, rminb = -1, rminv = INT32_MAX;           // the same over the bins of the current run (a valley's, if the run stays short)
            i32 nz = 0, bestb = -1, bestv = INT32_MAX;
            for (i32 base = 0; base <= nb; base += HHX_WAVE) {
                const i32 mine = base + lane < nb ? c[base + lane] : 0;
                const i32 lim = min((i32)HHX_WAVE, nb + 1 - base);      // one step past the last bin closes an open run
                for (i32 j = 0; j < lim; ++j) {
                    const i32 i = base + j;
                    const bool end = i == nb;
                    const i32 v = __shfl(mine, j, HHX_WAVE);
                    const bool high = !end && (double)v >= cov_cutoff;
                    if (high) {
                        ++run;
                        if (v == 0 && rz < 0) rz = i;
                        if (v < rminv) { rminv = v; rminb = i; }
                        continue;
                    }
                    if (run > 0) {
                        if ((double)(run * (i64)res) >= region_cutoff) {
                            if (n_counting > 0) {                 // a valley is closed
                                if (vz >= 0) { if (lane == 0) cand[off + nz] = vz; ++nz; }
                                else if (vminb >= 0 && vminv < bestv) { bestv = vminv; bestb = vminb; }
                            }
                            ++n_counting;
                            vz = -1; vminb = -1; vminv = INT32_MAX;
                        } else {                                  // a short run belongs to the valley around it
                            if (vz < 0) vz = rz;
                            if (rminb >= 0 && rminv < vminv) { vminv = rminv; vminb = rminb; }
                        }
                        run = 0; rz = -1; rminb = -1; rminv = INT32_MAX;
                    }
                    if (!end) {
                        if (v == 0 && vz < 0) vz = i;
                        if (v < vminv) { vminv = v; vminb = i; }
                    }
                }
            }
            if (nz > 0) { out_n = nz; out_cov = 0; }
            else if (bestb >= 0) { if (lane == 0) cand[off] = bestb; out_n = 1; out_cov = bestv; }
        }
        if (lane == 0) { n_bp[s] = out_n; bp_cov[s] = out_cov; }
    }
}

__global__ __launch_bounds__(CR_T) void k_gather_i32(i64 n, const i64 *__restrict__ idx, const i32 *__restrict__ src, i32 *__restrict__ dst) {
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T) dst[k] = src[idx[k]];
}

struct BreakTables {
    const i64 *pair_begin, *out_base, *bin_off;     // per broken contig: its pairs [pair_begin, pair_begin + n), where they go, its bins
    const i32 *n_pairs, *nb, *bp_off, *bp_pos, *child_base;
    const unsigned char *zero;
};

// :1081-1113 for the pairs of the broken contigs, one workgroup per broken contig.  Non-zero coverage at the (single) break
// point bp: a pair whose closed [lo, hi] meets the closed [bp, bp + res] (:1076 :1089) is dropped and its coverage taken back
// (:1091-1092, through the difference array); every other pair — and every pair in the zero-coverage case — moves both ends to
// the child that holds them (pos_shift :1036-1052: the child of x starts at the largest break point <= x, child 0 at 0;
// new = x - start) and survives iff both ends name the same child (:1099).  key = the child's segment id, n_child = dropped.
// lose_inner (bit 1 of the flag): the parent is itself a piece that does not start at position 1 of its original contig.  pos_shift
// :1050 then names every child but the last `raw:{p + start}-{next break point}` with an end that is NOT shifted by the parent's start,
// a key no later round looks up (the children are called raw:{s + shift}-{point + shift} :1138): those pairs are lost to the
// reference, so they are dropped here too — the position lists of such children are empty, as ctg_link_pos_dict[child] is.
__global__ __launch_bounds__(CR_T) void k_break_pairs(i32 n_broken, BreakTables t, i32 res, i32 n_child, const u64 *__restrict__ pairs,
                                                      u64 *__restrict__ okey, u64 *__restrict__ oval, i32 *__restrict__ diff,
                                                      unsigned long long *__restrict__ cnt) {
    for (i32 b = blockIdx.x; b < n_broken; b += gridDim.x) {
        const i64 src = t.pair_begin[b], dst = t.out_base[b], off = t.bin_off[b];
        const i32 n = t.n_pairs[b], nb = t.nb[b], b0 = t.bp_off[b], b1 = t.bp_off[b + 1], child0 = t.child_base[b];
        const bool zero = (t.zero[b] & 1) != 0, lose_inner = (t.zero[b] & 2) != 0;
        const i32 bp = t.bp_pos[b0];
        for (i32 k = threadIdx.x; k < n; k += CR_T) {
            const u64 v = pairs[src + k];
            const i32 lo = (i32)(u32)v, hi = (i32)(u32)(v >> 32);
            u64 key = (u64)(u32)n_child, val = v;
            if (!zero && (i64)lo <= (i64)bp + res && hi >= bp) {
                const i32 sb = lo / res, eb = hi / res;
                if (sb < nb) atomicAdd(&diff[off + sb], -1);
                if (eb + 1 < nb) atomicAdd(&diff[off + eb + 1], 1);
            } else {
                i32 ci = 0, cj = 0, si = 0, sj = 0;
                for (i32 q = b0; q < b1; ++q) {
                    const i32 p = t.bp_pos[q];
                    if (p <= lo) { ++ci; si = p; }
                    if (p <= hi) { ++cj; sj = p; }
                }
                if (ci == cj && !(lose_inner && ci < b1 - b0)) {
                    key = (u64)(u32)(child0 + ci);
                    val = ((u64)(u32)(hi - sj) << 32) | (u64)(u32)(lo - si);
                    atomicAdd(&cnt[child0 + ci], 1ull);
                }
            }
            okey[dst + k] = key;
            oval[dst + k] = val;
        }
    }
}

// convert_ctg :1405-1411 (and its copies :1447 :1477 :1516): source contig s owns entries [off[s], off[s + 1]) of (break position
// ascending, corrected contig id); the entry of x is the one with the largest position <= x.  No entry: -1 (not in the corrected FASTA).
__global__ __launch_bounds__(CR_T) void k_remap(i64 n, i32 *__restrict__ id, i32 *__restrict__ pos, i32 n_src, const i32 *__restrict__ off,
                                                const i32 *__restrict__ mpos, const i32 *__restrict__ mid) {
    for (i64 k = (i64)blockIdx.x * CR_T + threadIdx.x; k < n; k += (i64)gridDim.x * CR_T) {
        const i32 s = id[k];
        if (s < 0) continue;                                      // unknown name / filtered record / unmapped end: as it came
        i32 nid = -1, shift = 0;
        if (s < n_src) {
            const i32 x = pos[k];
            for (i32 q = off[s], e = off[s + 1]; q < e && mpos[q] <= x; ++q) { nid = mid[q]; shift = mpos[q]; }
        }
        id[k] = nid;
        if (nid >= 0) pos[k] -= shift;
    }
}

unsigned grid_for(i64 n, int per_block) { return (unsigned)std::max<i64>(1, std::min<i64>((n + per_block - 1) / per_block, 256 * 8)); }

int bits_for(u64 max_value) {
    int b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

int sync_segments(hhx_correct *c) {
    const size_t n = c->seg_off.size();
    HHX_TRY(upload(c->d_seg_off, c->seg_off.data(), n));
    HHX_TRY(upload(c->d_seg_nb, c->seg_nb.data(), n));
    HHX_TRY(upload(c->d_seg_len, c->seg_len.data(), n));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

}  // namespace

extern "C" int hhx_correct_create(i32 n_ctg, const i64 *ctg_len, i32 resolution, hhx_correct **out) {
    if (!out) return fail("null pointer");
    if (n_ctg < 0 || resolution <= 0 || (n_ctg && !ctg_len)) return fail("hhx_correct_create: bad arguments");
    hhx_correct *c = new hhx_correct();
    c->res = resolution;
    i64 total = 0;
    for (i32 k = 0; k < n_ctg; ++k) {
        if (ctg_len[k] < 0 || ctg_len[k] >= (i64)INT32_MAX) {
            delete c;
            return fail("hhx_correct_create: contig %d is %lld bp long; assembly correction keeps int32 positions (array('i') in the reference) "
                        "and refuses contigs of 2^31 bp and more", k, (long long)ctg_len[k]);
        }
        c->seg_off.push_back(total);
        c->seg_nb.push_back((i32)(ctg_len[k] / resolution + 1));            // :1311
        c->seg_len.push_back((i32)ctg_len[k]);
        total += ctg_len[k] / resolution + 1;
    }
    c->total_bins = total;
    int rc = sync_segments(c) || c->cov.alloc((size_t)total) || c->diff.alloc((size_t)total) || c->cand.alloc((size_t)total) ||
             c->cnt.alloc((size_t)n_ctg) || c->bad.alloc(1);
    const size_t nb = sizeof(i32) * (size_t)(total ? total : 1);
    if (!rc && (hipMemsetAsync(c->cov.p, 0, nb, g_stream) != hipSuccess || hipMemsetAsync(c->diff.p, 0, nb, g_stream) != hipSuccess ||
                hipMemsetAsync(c->cnt.p, 0, sizeof(unsigned long long) * (size_t)(n_ctg ? n_ctg : 1), g_stream) != hipSuccess ||
                hipMemsetAsync(c->bad.p, 0, sizeof(i32), g_stream) != hipSuccess || hipStreamSynchronize(g_stream) != hipSuccess))
        rc = fail("hhx_correct_create: clearing the tables failed");
    if (rc) { delete c; return 1; }
    *out = c;
    return 0;
}

extern "C" int hhx_correct_push(hhx_correct *c, i64 n, const i32 *id1, const i32 *pos1, const i32 *id2, const i32 *pos2, int on_device) {
    if (!c) return fail("null handle");
    if (c->finalized) return fail("hhx_correct_push: the table is finalized");
    if (n < 0 || n > (i64)INT32_MAX) return fail("hhx_correct_push: batch of %lld records", (long long)n);
    if (n == 0) return 0;
    if (!id1 || !pos1 || !id2 || !pos2) return fail("null pointer");
    DevBuf<i32> d[4];
    const i32 *src[4] = {id1, pos1, id2, pos2};
    if (!on_device)
        for (int k = 0; k < 4; ++k) {
            if (d[k].alloc((size_t)n)) return 1;
            HHX_HIP(hipMemcpyAsync(d[k].p, src[k], sizeof(i32) * (size_t)n, hipMemcpyHostToDevice, g_stream));
            src[k] = d[k].p;
        }
    DevBuf<i32> flag, at;
    if (flag.alloc((size_t)n) || at.alloc((size_t)n + 1)) return 1;
    {
        KTimer kt("correct_push");
        auto kernel = tune_get("correct_agg", 0) ? k_cov_push<true> : k_cov_push<false>;
        kernel<<<grid_for(n, CR_T), CR_T, 0, g_stream>>>(n, src[0], src[1], src[2], src[3], (i32)c->seg_off.size(), c->d_seg_off.p, c->d_seg_nb.p,
                                                        c->res, c->diff.p, c->cnt.p, flag.p, c->bad.p);
    }
    HHX_LAUNCH_CHECK();
    i64 kept = 0;
    HHX_TRY(exclusive_scan_i32(flag.p, at.p, n, &kept));
    i32 bad = 0;
    HHX_HIP(hipMemcpyAsync(&bad, c->bad.p, sizeof bad, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (bad) return fail("hhx_correct_push: a negative position (the reference's slice arithmetic :1338-1341 has no meaning for it)");
    if (kept) {
        DevBuf<u64> key, val;
        if (key.alloc((size_t)kept) || val.alloc((size_t)kept)) return 1;
        k_cov_compact<<<grid_for(n, CR_T), CR_T, 0, g_stream>>>(n, src[0], src[1], src[3], flag.p, at.p, key.p, val.p);
        HHX_LAUNCH_CHECK();
        c->chunk_key.push_back(std::move(key));
        c->chunk_val.push_back(std::move(val));
        c->chunk_n.push_back(kept);
    }
    HHX_HIP(hipStreamSynchronize(g_stream));                       // the staging buffers of a host push go back to the pool here
    prof_count("correct_records", n);
    return 0;
}

extern "C" int hhx_correct_export(hhx_correct *c, i32 *resolution, i64 *n_bins, i64 *n_pairs, i32 *cov_diff, i64 pair_first, i64 pair_count,
                                  i32 *pair_ctg, i32 *pair_lo_hi, int on_device) {
    if (!c) return fail("null handle");
    if (c->finalized) return fail("hhx_correct_export: the table is finalized (its difference array is spent)");
    i64 total = 0;
    for (i64 k : c->chunk_n) total += k;
    if (resolution) *resolution = c->res;
    if (n_bins) *n_bins = c->total_bins;
    if (n_pairs) *n_pairs = total;
    if ((pair_ctg == nullptr) != (pair_lo_hi == nullptr)) return fail("hhx_correct_export: the pair columns come together");
    if (pair_ctg && (pair_first < 0 || pair_count < 0 || pair_first > total || pair_count > total - pair_first))
        return fail("hhx_correct_export: records [%lld, %lld + %lld) of %lld", (long long)pair_first, (long long)pair_first, (long long)pair_count,
                    (long long)total);
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (cov_diff && c->total_bins) HHX_HIP(hipMemcpyAsync(cov_diff, c->diff.p, sizeof(i32) * (size_t)c->total_bins, kind, g_stream));
    DevBuf<i32> d_ctg, d_lh;                                       // staging of a host call: back to the pool behind the copies
    if (pair_ctg && pair_count) {
        i32 *ctg = pair_ctg, *lh = pair_lo_hi;
        if (!on_device) {
            if (d_ctg.alloc((size_t)pair_count) || d_lh.alloc(2 * (size_t)pair_count)) return 1;
            ctg = d_ctg.p; lh = d_lh.p;
        }
        const i64 end = pair_first + pair_count;
        i64 begin = 0, at = 0;                                     // begin: first record of chunk k in push order; at: records written
        for (size_t k = 0; k < c->chunk_n.size() && begin < end; begin += c->chunk_n[k], ++k) {
            const i64 lo = std::max(begin, pair_first), hi = std::min(begin + c->chunk_n[k], end);
            if (hi <= lo) continue;
            k_export_pairs<<<grid_for(hi - lo, CR_T), CR_T, 0, g_stream>>>(hi - lo, c->chunk_key[k].p + (lo - begin), c->chunk_val[k].p + (lo - begin),
                                                                          ctg + at, lh + 2 * at);
            HHX_LAUNCH_CHECK();
            at += hi - lo;
        }
        if (!on_device) {
            HHX_HIP(hipMemcpyAsync(pair_ctg, ctg, sizeof(i32) * (size_t)pair_count, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipMemcpyAsync(pair_lo_hi, lh, sizeof(i32) * 2 * (size_t)pair_count, hipMemcpyDeviceToHost, g_stream));
        }
    }
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_correct_absorb(hhx_correct *c, i32 resolution, i64 n_bins, const i32 *cov_diff, i64 n_pairs, const i32 *pair_ctg,
                                  const i32 *pair_lo_hi, int on_device) {
    if (!c) return fail("null handle");
    if (c->finalized) return fail("hhx_correct_absorb: the table is finalized");
    if (resolution != c->res) return fail("hhx_correct_absorb: a table of resolution %d into one of resolution %d", resolution, c->res);
    if (n_bins != c->total_bins) return fail("hhx_correct_absorb: a table of %lld bins into one of %lld", (long long)n_bins, (long long)c->total_bins);
    if (n_pairs < 0 || n_pairs > (i64)INT32_MAX) return fail("hhx_correct_absorb: %lld pair records", (long long)n_pairs);
    if (n_pairs && (!pair_ctg || !pair_lo_hi)) return fail("null pointer");
    const bool with_diff = cov_diff != nullptr && n_bins > 0;      // null: a further piece of a table whose difference array came with an earlier one
    DevBuf<i32> d_diff, d_ctg, d_lh;
    if (!on_device) {
        if (with_diff) {
            HHX_TRY(upload(d_diff, cov_diff, (size_t)n_bins));
            cov_diff = d_diff.p;
        }
        if (n_pairs) {
            HHX_TRY(upload(d_ctg, pair_ctg, (size_t)n_pairs));
            HHX_TRY(upload(d_lh, pair_lo_hi, 2 * (size_t)n_pairs));
            pair_ctg = d_ctg.p; pair_lo_hi = d_lh.p;
        }
    }
    if (n_pairs) {                                                 // the same growth as a push: one more chunk behind those kept so far
        DevBuf<u64> key, val;
        if (key.alloc((size_t)n_pairs) || val.alloc((size_t)n_pairs)) return 1;
        {
            KTimer kt("correct_absorb");
            k_absorb_pairs<<<grid_for(n_pairs, CR_T), CR_T, 0, g_stream>>>(n_pairs, pair_ctg, pair_lo_hi, (i32)c->seg_off.size(), key.p, val.p,
                                                                          c->cnt.p, c->bad.p);
        }
        HHX_LAUNCH_CHECK();
        i32 bad = 0;
        HHX_HIP(hipMemcpyAsync(&bad, c->bad.p, sizeof bad, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        if (bad) return fail("hhx_correct_absorb: a record no push keeps (contig outside the table, or not 0 <= lo <= hi); the table cannot be finalized any more");
        c->chunk_key.push_back(std::move(key));
        c->chunk_val.push_back(std::move(val));
        c->chunk_n.push_back(n_pairs);
    }
    if (with_diff) {
        KTimer kt("correct_absorb");
        k_absorb_diff<<<grid_for(n_bins, CR_T), CR_T, 0, g_stream>>>(n_bins, cov_diff, c->diff.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipStreamSynchronize(g_stream));                       // the caller's arrays (and the staging buffers of a host call) are free again
    prof_count("correct_absorbed_pairs", n_pairs);
    return 0;
}

extern "C" int hhx_correct_finalize(hhx_correct *c, i64 *n_kept) {
    if (!c) return fail("null handle");
    if (c->finalized) return fail("hhx_correct_finalize: called twice");
    const i32 n_seg = (i32)c->seg_off.size();
    i64 total = 0;
    for (i64 k : c->chunk_n) total += k;
    if (total) {
        DevBuf<u64> key, val, skey;
        if (key.alloc((size_t)total) || val.alloc((size_t)total) || skey.alloc((size_t)total) || c->pairs.alloc((size_t)total)) return 1;
        i64 at = 0;
        for (size_t k = 0; k < c->chunk_n.size(); ++k) {
            HHX_HIP(hipMemcpyAsync(key.p + at, c->chunk_key[k].p, sizeof(u64) * (size_t)c->chunk_n[k], hipMemcpyDeviceToDevice, g_stream));
            HHX_HIP(hipMemcpyAsync(val.p + at, c->chunk_val[k].p, sizeof(u64) * (size_t)c->chunk_n[k], hipMemcpyDeviceToDevice, g_stream));
            at += c->chunk_n[k];
            c->chunk_key[k].release();                             // stream-ordered pool: the block is reused only behind the copy above
            c->chunk_val[k].release();
        }
        HHX_HIP(hipStreamSynchronize(g_stream));
        c->chunk_key.clear(); c->chunk_val.clear(); c->chunk_n.clear();
        KTimer kt("correct_sort");
        HHX_TRY(stable_sort_pairs_u64(key.p, skey.p, val.p, c->pairs.p, total, bits_for((u64)std::max(1, n_seg - 1))));
    }
    c->n_pairs = total;
    std::vector<unsigned long long> cnt((size_t)n_seg);
    if (n_seg) HHX_HIP(hipMemcpyAsync(cnt.data(), c->cnt.p, sizeof(unsigned long long) * (size_t)n_seg, hipMemcpyDeviceToHost, g_stream));
    if (n_seg) {
        KTimer kt("correct_scan");
        k_apply_diff<<<grid_for(n_seg, 1), HHX_WAVE, 0, g_stream>>>(n_seg, c->d_seg_off.p, c->d_seg_nb.p, c->diff.p, c->cov.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipStreamSynchronize(g_stream));
    c->pair_off.assign((size_t)n_seg + 1, 0);
    for (i32 s = 0; s < n_seg; ++s) c->pair_off[s + 1] = c->pair_off[s] + (i64)cnt[s];
    if (c->pair_off[n_seg] != total) return fail("hhx_correct_finalize: %lld pairs counted, %lld kept", (long long)c->pair_off[n_seg], (long long)total);
    c->finalized = true;
    if (n_kept) *n_kept = total;
    return 0;
}

extern "C" int hhx_correct_shape(hhx_correct *c, i32 *n_seg, i64 *n_bins, i64 *n_pairs) {
    if (!c) return fail("null handle");
    if (n_seg) *n_seg = (i32)c->seg_off.size();
    if (n_bins) *n_bins = c->total_bins;
    if (n_pairs) *n_pairs = c->n_pairs;
    return 0;
}

extern "C" int hhx_correct_fetch_segments(hhx_correct *c, i64 *bin_off, i32 *n_bins, i32 *len, i64 *pair_off) {
    if (!c) return fail("null handle");
    if (!c->finalized) return fail("hhx_correct_fetch_segments: finalize first");
    const size_t n = c->seg_off.size();
    if (bin_off) memcpy(bin_off, c->seg_off.data(), n * sizeof(i64));
    if (n_bins) memcpy(n_bins, c->seg_nb.data(), n * sizeof(i32));
    if (len) memcpy(len, c->seg_len.data(), n * sizeof(i32));
    if (pair_off) memcpy(pair_off, c->pair_off.data(), (n + 1) * sizeof(i64));
    return 0;
}

extern "C" int hhx_correct_fetch_coverage(hhx_correct *c, i32 *cov) {
    if (!c || !cov) return fail("null pointer");
    if (!c->finalized) return fail("hhx_correct_fetch_coverage: finalize first");
    if (c->total_bins) HHX_HIP(hipMemcpyAsync(cov, c->cov.p, sizeof(i32) * (size_t)c->total_bins, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_correct_fetch_pairs(hhx_correct *c, i32 *lo_hi) {
    if (!c || !lo_hi) return fail("null pointer");
    if (!c->finalized) return fail("hhx_correct_fetch_pairs: finalize first");
    if (c->n_pairs) HHX_HIP(hipMemcpyAsync(lo_hi, c->pairs.p, sizeof(u64) * (size_t)c->n_pairs, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_correct_detect(hhx_correct *c, double median_cov_ratio, double region_len_ratio, i64 min_region_cutoff, i32 *n_bp, i32 *bp_cov,
                                  i64 *n_total) {
    if (!c) return fail("null handle");
    if (!c->finalized) return fail("hhx_correct_detect: finalize first");
    const i32 n_seg = (i32)c->seg_off.size();
    c->bp_bin.clear();
    if (n_total) *n_total = 0;
    if (n_seg == 0) return 0;
    if (!n_bp || !bp_cov) return fail("null pointer");
    DevBuf<i32> d_n, d_cov;
    if (d_n.alloc((size_t)n_seg) || d_cov.alloc((size_t)n_seg)) return 1;
    {
        KTimer kt("correct_detect");
        k_detect<<<grid_for(n_seg, 1), HHX_WAVE, 0, g_stream>>>(n_seg, c->d_seg_off.p, c->d_seg_nb.p, c->d_seg_len.p, c->res, c->cov.p, median_cov_ratio,
                                                               region_len_ratio, (double)min_region_cutoff, c->cand.p, d_n.p, d_cov.p);
    }
    HHX_LAUNCH_CHECK();
    HHX_HIP(hipMemcpyAsync(n_bp, d_n.p, sizeof(i32) * (size_t)n_seg, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(bp_cov, d_cov.p, sizeof(i32) * (size_t)n_seg, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    std::vector<i64> idx;
    for (i32 s = 0; s < n_seg; ++s) {
        if (n_bp[s] < 0 || n_bp[s] > c->seg_nb[s]) return fail("hhx_correct_detect: segment %d reports %d break points", s, n_bp[s]);
        for (i32 t = 0; t < n_bp[s]; ++t) idx.push_back(c->seg_off[s] + t);
    }
    if (!idx.empty()) {
        DevBuf<i64> d_idx;
        DevBuf<i32> d_out;
        HHX_TRY(upload(d_idx, idx.data(), idx.size()));
        if (d_out.alloc(idx.size())) return 1;
        k_gather_i32<<<grid_for((i64)idx.size(), CR_T), CR_T, 0, g_stream>>>((i64)idx.size(), d_idx.p, c->cand.p, d_out.p);
        HHX_LAUNCH_CHECK();
        c->bp_bin.resize(idx.size());
        HHX_HIP(hipMemcpyAsync(c->bp_bin.data(), d_out.p, sizeof(i32) * idx.size(), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
    }
    if (n_total) *n_total = (i64)idx.size();
    return 0;
}

extern "C" int hhx_correct_fetch_break_points(hhx_correct *c, i32 *bp_bin) {
    if (!c) return fail("null handle");
    if (!c->bp_bin.empty()) {
        if (!bp_bin) return fail("null pointer");
        memcpy(bp_bin, c->bp_bin.data(), c->bp_bin.size() * sizeof(i32));
    }
    return 0;
}

extern "C" int hhx_correct_break(hhx_correct *c, i32 n_broken, const i32 *seg, const i64 *bp_off, const i32 *bp_pos, const uint8_t *zero) {
    if (!c) return fail("null handle");
    if (!c->finalized) return fail("hhx_correct_break: finalize first");
    if (n_broken < 0 || (n_broken && (!seg || !bp_off || !bp_pos || !zero))) return fail("hhx_correct_break: bad arguments");
    const i32 n_seg = (i32)c->seg_off.size();
    std::vector<i64> pair_begin, out_base, bin_off, n_off, n_poff;
    std::vector<i32> n_pairs, nb, h_bp_off, child_base, n_nb, n_len;
    i64 m = 0;
    i32 n_child = 0;
    for (i32 b = 0; b < n_broken; ++b) {
        const i32 s = seg[b];
        if (s < 0 || s >= n_seg || (b && s <= seg[b - 1])) return fail("hhx_correct_break: segment ids must ascend inside the table");
        const i64 b0 = bp_off[b], b1 = bp_off[b + 1];
        if ((b == 0 && b0 != 0) || b1 <= b0 || b1 > (i64)INT32_MAX) return fail("hhx_correct_break: contig %d has no break point", s);
        if (!(zero[b] & 1) && b1 - b0 != 1) return fail("hhx_correct_break: a break at non-zero coverage is a single point (:1074)");
        const i64 np = c->pair_off[s + 1] - c->pair_off[s];
        if (np > (i64)INT32_MAX) return fail("hhx_correct_break: contig %d holds %lld pairs", s, (long long)np);
        pair_begin.push_back(c->pair_off[s]); out_base.push_back(m); bin_off.push_back(c->seg_off[s]);
        n_pairs.push_back((i32)np); nb.push_back(c->seg_nb[s]); h_bp_off.push_back((i32)b0); child_base.push_back(n_child);
        m += np;
        i32 start = 0;
        for (i64 q = b0; q <= b1; ++q) {                           // the children :1122-1182: [start, point) ..., [start, len)
            const bool last = q == b1;
            const i32 point = last ? c->seg_len[s] : bp_pos[q];
            if (!last && (point <= start || point >= c->seg_len[s] || point % c->res))
                return fail("hhx_correct_break: break point %d of contig %d (length %d) is not an ascending multiple of the resolution", point, s, c->seg_len[s]);
            n_off.push_back(c->seg_off[s] + start / c->res);
            n_nb.push_back(last ? c->seg_nb[s] - start / c->res : point / c->res - start / c->res);      // :1178 / :1153
            n_len.push_back(point - start);
            start = point;
            ++n_child;
        }
    }
    h_bp_off.push_back(n_broken ? (i32)bp_off[n_broken] : 0);
    std::vector<unsigned long long> cnt((size_t)n_child, 0);
    DevBuf<u64> npairs_buf;
    if (n_broken) {
        DevBuf<i64> d_pb, d_ob, d_bo;
        DevBuf<i32> d_np, d_nb, d_bpo, d_bpp, d_cb;
        DevBuf<unsigned char> d_z;
        HHX_TRY(upload(d_pb, pair_begin.data(), pair_begin.size()));
        HHX_TRY(upload(d_ob, out_base.data(), out_base.size()));
        HHX_TRY(upload(d_bo, bin_off.data(), bin_off.size()));
        HHX_TRY(upload(d_np, n_pairs.data(), n_pairs.size()));
        HHX_TRY(upload(d_nb, nb.data(), nb.size()));
        HHX_TRY(upload(d_bpo, h_bp_off.data(), h_bp_off.size()));
        HHX_TRY(upload(d_bpp, bp_pos, (size_t)bp_off[n_broken]));
        HHX_TRY(upload(d_cb, child_base.data(), child_base.size()));
        HHX_TRY(upload(d_z, (const unsigned char *)zero, (size_t)n_broken));
        DevBuf<unsigned long long> d_cnt;                           // the handle is touched only once nothing can fail any more
        if (d_cnt.alloc((size_t)n_child)) return 1;
        HHX_HIP(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long) * (size_t)n_child, g_stream));
        if (m) {
            DevBuf<u64> okey, oval, skey;
            if (okey.alloc((size_t)m) || oval.alloc((size_t)m) || skey.alloc((size_t)m) || npairs_buf.alloc((size_t)m)) return 1;
            const BreakTables t{d_pb.p, d_ob.p, d_bo.p, d_np.p, d_nb.p, d_bpo.p, d_bpp.p, d_cb.p, d_z.p};
            {
                KTimer kt("correct_break");
                k_break_pairs<<<grid_for(n_broken, 1), CR_T, 0, g_stream>>>(n_broken, t, c->res, n_child, c->pairs.p, okey.p, oval.p, c->diff.p, d_cnt.p);
            }
            HHX_LAUNCH_CHECK();
            HHX_TRY(stable_sort_pairs_u64(okey.p, skey.p, oval.p, npairs_buf.p, m, bits_for((u64)n_child)));
            k_apply_diff<<<grid_for(n_broken, 1), HHX_WAVE, 0, g_stream>>>(n_broken, d_bo.p, d_nb.p, c->diff.p, c->cov.p);      // :1092
            HHX_LAUNCH_CHECK();
        }
        HHX_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(unsigned long long) * (size_t)n_child, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        c->cnt = std::move(d_cnt);
    }
    // the children are the table now: every contig that was not broken this round has left it (:1192-1197)
    c->seg_off = n_off; c->seg_nb = n_nb; c->seg_len = n_len;
    c->pair_off.assign((size_t)n_child + 1, 0);
    for (i32 s = 0; s < n_child; ++s) c->pair_off[s + 1] = c->pair_off[s] + (i64)cnt[s];
    c->n_pairs = c->pair_off[n_child];
    c->pairs = std::move(npairs_buf);                              // survivors first, in child order; the dropped tail is never read
    c->bp_bin.clear();
    return sync_segments(c);
}

extern "C" int hhx_correct_destroy(hhx_correct *c) {
    delete c;
    return 0;
}

extern "C" int hhx_remap_create(i32 n_src, const i32 *off, const i32 *break_pos, const i32 *new_id, hhx_remap **out) {
    if (!out) return fail("null pointer");
    if (n_src < 0 || (n_src && !off)) return fail("hhx_remap_create: bad arguments");
    const i32 n = n_src ? off[n_src] : 0;
    if (n_src && (off[0] != 0 || n < 0)) return fail("hhx_remap_create: inconsistent offsets");
    for (i32 s = 0; s < n_src; ++s) {
        if (off[s + 1] < off[s]) return fail("hhx_remap_create: inconsistent offsets");
        for (i32 q = off[s]; q < off[s + 1]; ++q)
            if (!break_pos || !new_id || (q > off[s] && break_pos[q] <= break_pos[q - 1]))
                return fail("hhx_remap_create: the break positions of source contig %d do not ascend", s);
    }
    hhx_remap *r = new hhx_remap();
    r->n_src = n_src;
    static const i32 zero = 0;
    int rc = upload(r->off, n_src ? off : &zero, (size_t)n_src + 1) || upload(r->pos, break_pos, (size_t)n) || upload(r->id, new_id, (size_t)n);
    if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) rc = fail("hhx_remap_create: upload failed");
    if (rc) { delete r; return 1; }
    *out = r;
    return 0;
}

extern "C" int hhx_remap_apply(hhx_remap *r, i64 n, i32 *dev_id, i32 *dev_pos) {
    if (!r) return fail("null handle");
    if (n < 0) return fail("hhx_remap_apply: negative count");
    if (n == 0) return 0;
    if (!dev_id || !dev_pos) return fail("null pointer");
    KTimer kt("correct_remap");
    k_remap<<<grid_for(n, CR_T), CR_T, 0, g_stream>>>(n, dev_id, dev_pos, r->n_src, r->off.p, r->pos.p, r->id.p);
    HHX_LAUNCH_CHECK();
    return 0;
}

extern "C" int hhx_remap_destroy(hhx_remap *r) {
    delete r;
    return 0;
}
