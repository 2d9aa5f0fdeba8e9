// Per-contig group statistics of output_statistics (HapHiC_cluster.py:2279-2478), the last step of `haphic cluster`.
//   parse_link_dict :2252-2268     ctg_group_link_dict[ctg][group] = summed links between the contig and the group's contigs: for every key
//                                  (ctg_i, ctg_j) of full_link_dict, in dict order, (ctg_i, group[ctg_j]) and (ctg_j, group[ctg_i]); a partner
//                                  that is 'ungrouped' contributes nothing
//   sorted(...) :2365              the cells of a contig by links, largest first; the sort is stable, so equal cells stay in the order in which
//                                  they first received a contribution
//   cal_link_density :2271-2276    links / group_RE[g] for the contig's own group, links / (group_RE[g] + ctg_RE - 1) for every other
//   sum([...]) :2376               the densities of all cells but the first, added one by one in that order
// What the statistics keep of a contig is three numbers, so the cells are never written out: the table becomes a symmetric adjacency by contig
// (count / scan / scatter, built once per call), and one workgroup per (contig, set) accumulates `sum` (64-bit integer add) and `first` (64-bit
// min of the dict position 2 * key + side) per group in an LDS table, compacts the occupied slots, sorts them by (sum descending, first
// ascending) with a bitonic network, forms the quotients in parallel and lets one lane add them in order — plainly (CPython <= 3.11) or with
// Neumaier's compensation (CPython >= 3.12), as sum() of the running interpreter does.  A set whose n_groups fits the table indexes it by group id,
// any other hashes the id; a contig with more distinct groups than the table holds (hhx_tune "groupstats_lds_slots") is listed and redone by a
// second kernel on a per-workgroup table in HBM, indexed by group id.  All sets of a call share the adjacency; the workgroups of one contig are
// neighbours in the grid, so its row is read from HBM once.  Integer sums are exact; the quotients are IEEE divisions of the sums converted to
// float64, which equals Python's int / int below 2^53.  No fused multiply-add, no reassociation (the library is built with -ffp-contract=off).
#include "hhx_groupstats.h"

namespace {

constexpr i64 GS_SLOTS_DEFAULT = 2048, GS_SLOTS_MIN = 16, GS_SLOTS_MAX = 2048;     // 40 bytes of LDS per slot: 80 KB by default, two workgroups per CU (1024 slots measured slower at C3: DESIGN.md)
constexpr int GS_SPILL_GRID = 1024;                                                // workgroups of the spill kernel at most
constexpr size_t GS_SPILL_BYTES = (size_t)2 << 30;                                 // ... and HBM for their tables at most

struct GsSets {
    const i32 *group;        // [n_sets][n_ctg], -1 = ungrouped
    const i32 *n_groups;     // [n_sets]
    const i64 *re_off;       // [n_sets]: where the set's group_RE starts
    const i64 *group_re, *ctg_re;
    i32 n_ctg, n_sets;
    int sum_mode;
};
struct GsOut {
    i32 *n_cells;
    i64 *max_links;
    i32 *max_group;
    double *other_sum;
};

// The n cells (cg, cs, cf) of one contig, padded to n2 = 2^k slots, in any order -> the outputs of (row, set).  cf is reused for the quotients.
__device__ __forceinline__ void gs_finish(i32 *cg, i64 *cs, u64 *cf, i32 n, i32 n2, i32 row, i32 set, const GsSets &S, const GsOut &O) {
    const int tid = threadIdx.x;
    gs_sort_cells(cg, cs, cf, n2);
    const i32 own = S.group[(size_t)set * S.n_ctg + row];
    const i64 *gre = S.group_re + S.re_off[set];
    const i64 cre = S.ctg_re[row];
    double *q = reinterpret_cast<double *>(cf);
    for (i32 r = 1 + tid; r < n; r += GS_THREADS) {                                // cal_link_density :2271-2276 of every cell but the first
        const i32 g = cg[r];
        const i64 den = g == own ? gre[g] : gre[g] + cre - 1;
        q[r] = (double)cs[r] / (double)den;
    }
    __syncthreads();
    if (tid == 0) {
        const double total = gs_ordered_sum(q, 1, n, S.sum_mode);
        const size_t o = (size_t)set * S.n_ctg + row;
        O.n_cells[o] = n;
        O.max_links[o] = cs[0];
        O.max_group[o] = cg[0];
        O.other_sum[o] = total;
    }
}

__device__ __forceinline__ void gs_write_empty(i32 row, i32 set, const GsSets &S, const GsOut &O) {
    const size_t o = (size_t)set * S.n_ctg + row;
    O.n_cells[o] = 0;
    O.max_links[o] = 0;
    O.max_group[o] = -1;
    O.other_sum[o] = 0.0;
}

// one workgroup per (contig, set); item = row * n_sets + set.  Dynamic LDS: 40 bytes per slot.
__global__ __launch_bounds__(GS_THREADS) void k_gs_rows(const i64 *__restrict__ rowptr, const i32 *__restrict__ partner, const i64 *__restrict__ lk,
                                                        const u64 *__restrict__ ps, GsSets S, GsOut O, i32 cap, unsigned long long *__restrict__ n_spill,
                                                        i32 *__restrict__ spill_items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_lds[];
    __shared__ int s_n, s_over;
    unsigned long long *hsum = reinterpret_cast<unsigned long long *>(gs_lds);
    unsigned long long *hfirst = hsum + cap;
    i64 *cs = reinterpret_cast<i64 *>(hfirst + cap);
    u64 *cf = reinterpret_cast<u64 *>(cs + cap);
    i32 *hkey = reinterpret_cast<i32 *>(cf + cap);
    i32 *cg = hkey + cap;
    const int tid = threadIdx.x;
    const i32 item = (i32)blockIdx.x, row = item / S.n_sets, set = item - row * S.n_sets;
    const i64 beg = rowptr[row], end = rowptr[row + 1], len = end - beg;
    if (len == 0) {
        if (tid == 0) gs_write_empty(row, set, S, O);
        return;
    }
    // a short row clears, scans and sorts a table of its own size
    i32 cap_e = cap, bits = 0;
    while (cap_e > 2 && (i64)(cap_e >> 1) >= 2 * len) cap_e >>= 1;
    while ((1 << bits) < cap_e) ++bits;
    const i32 ng = S.n_groups[set];
    const bool direct = ng <= cap_e;                                               // the group id is the slot: no probe ever moves on
    for (i32 t = tid; t < cap_e; t += GS_THREADS) { hkey[t] = -1; hsum[t] = 0; hfirst[t] = GS_NONE; }
    if (tid == 0) { s_n = 0; s_over = 0; }
    __syncthreads();
    const i32 *grp = S.group + (size_t)set * S.n_ctg;
    for (i64 e = beg + tid; e < end; e += GS_THREADS) {
        const i32 g = grp[partner[e]];
        if (g < 0) continue;                                                       // 'ungrouped' :2255
        u32 h = direct ? (u32)g : ((u32)g * 0x9E3779B1u) >> (32 - bits);
        bool placed = false;
        for (i32 probe = 0; probe < cap_e; ++probe) {
            const i32 prev = atomicCAS(&hkey[h], -1, g);
            if (prev == -1 || prev == g) {
                atomicAdd(&hsum[h], (unsigned long long)lk[e]);
                atomicMin(&hfirst[h], (unsigned long long)ps[e]);
                placed = true;
                break;
            }
            h = (h + 1) & (u32)(cap_e - 1);
        }
        if (!placed) s_over = 1;                                                   // more distinct groups than slots
    }
    __syncthreads();
    if (s_over) {
        if (tid == 0) spill_items[atomicAdd(n_spill, 1ull)] = item;
        return;
    }
    for (i32 t = tid; t < cap_e; t += GS_THREADS)
        if (hkey[t] != -1) {
            const int i = atomicAdd(&s_n, 1);
            cg[i] = hkey[t]; cs[i] = (i64)hsum[t]; cf[i] = hfirst[t];
        }
    __syncthreads();
    const i32 n = s_n;
    if (n == 0) {                                                                  // every partner ungrouped: the contig is not in the dict
        if (tid == 0) gs_write_empty(row, set, S, O);
        return;
    }
    i32 n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (i32 t = n + tid; t < n2; t += GS_THREADS) { cg[t] = -1; cs[t] = GS_PAD; cf[t] = GS_NONE; }
    __syncthreads();
    gs_finish(cg, cs, cf, n, n2, row, set, S, O);
}

// the listed (contig, set) items again, on a table in HBM that is indexed by group id: tsum / tfirst [g_cap] and the cell list [p_cap] of this
// workgroup.  tsum is all zero and tfirst all ones between two items (set by the host before the launch, restored by the scan).
__global__ __launch_bounds__(GS_THREADS) void k_gs_spill(const i64 *__restrict__ rowptr, const i32 *__restrict__ partner, const i64 *__restrict__ lk,
                                                         const u64 *__restrict__ ps, GsSets S, GsOut O, i64 n_items, const i32 *__restrict__ items,
                                                         i64 g_cap, i64 p_cap, unsigned long long *tsum_all, unsigned long long *tfirst_all, i32 *cg_all,
                                                         i64 *cs_all, u64 *cf_all) {
    __shared__ int s_n;
    unsigned long long *tsum = tsum_all + (size_t)blockIdx.x * g_cap, *tfirst = tfirst_all + (size_t)blockIdx.x * g_cap;
    i32 *cg = cg_all + (size_t)blockIdx.x * p_cap;
    i64 *cs = cs_all + (size_t)blockIdx.x * p_cap;
    u64 *cf = cf_all + (size_t)blockIdx.x * p_cap;
    const int tid = threadIdx.x;
    for (i64 it = blockIdx.x; it < n_items; it += gridDim.x) {
        const i32 item = items[it], row = item / S.n_sets, set = item - row * S.n_sets;
        const i64 beg = rowptr[row], end = rowptr[row + 1];
        const i32 ng = S.n_groups[set];
        const i32 *grp = S.group + (size_t)set * S.n_ctg;
        if (tid == 0) s_n = 0;
        for (i64 e = beg + tid; e < end; e += GS_THREADS) {
            const i32 g = grp[partner[e]];
            if (g < 0) continue;
            atomicAdd(&tsum[g], (unsigned long long)lk[e]);
            atomicMin(&tfirst[g], (unsigned long long)ps[e]);
        }
        __threadfence();
        __syncthreads();
        for (i32 g = tid; g < ng; g += GS_THREADS) {
            // read where the atomics wrote (past the CU's vector cache), and leave the slot as the next item expects it
            const unsigned long long f = __hip_atomic_load(&tfirst[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (f != GS_NONE) {
                const unsigned long long v = __hip_atomic_load(&tsum[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int i = atomicAdd(&s_n, 1);
                cg[i] = g; cs[i] = (i64)v; cf[i] = f;
                __hip_atomic_store(&tsum[g], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&tfirst[g], GS_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __threadfence();
        __syncthreads();
        const i32 n = s_n;
        if (n == 0) {
            if (tid == 0) gs_write_empty(row, set, S, O);
        } else {
            i32 n2 = 1;
            while (n2 < n) n2 <<= 1;
            for (i32 t = n + tid; t < n2; t += GS_THREADS) { cg[t] = -1; cs[t] = GS_PAD; cf[t] = GS_NONE; }
            __syncthreads();
            gs_finish(cg, cs, cf, n, n2, row, set, S, O);
        }
        __syncthreads();                                                           // s_n and the cell list are the next item's
    }
}

int gs_unsupported(const char *why) {
    fail("%s", why);
    return HHX_UNSUPPORTED;
}

// the shared implementation: `src` is on the device
int gs_run(const char *who, GsSource src, i32 n_ctg, i32 n_sets, const i32 *group_host, const i32 *n_groups, const i64 *group_re_host,
           const i64 *ctg_re_host, int sum_mode, i32 *n_cells, i64 *max_links, i32 *max_group, double *other_sum) {
    if (sum_mode != 0 && sum_mode != 1) return gs_unsupported("group_stats: sum_mode is 0 (plain sum) or 1 (Neumaier's, CPython >= 3.12)");
    const size_t cells = (size_t)n_ctg * (size_t)n_sets;
    if (cells == 0) return 0;
    if (cells >= ((size_t)1 << 31)) return gs_unsupported("group_stats: contigs x sets beyond 2^31 - 1 workgroups");
    if (!group_host || !n_groups || !ctg_re_host || !n_cells || !max_links || !max_group || !other_sum) return fail("%s: null pointer", who);
    // ---- the sets: every group id is checked here, so that no kernel indexes a table out of bounds
    std::vector<i64> re_off((size_t)n_sets);
    i64 n_re = 0, g_max = 0;
    for (i32 s = 0; s < n_sets; ++s) {
        if (n_groups[s] < 0) return fail("%s: n_groups[%d] is negative", who, s);
        re_off[(size_t)s] = n_re;
        n_re += n_groups[s];
        g_max = std::max<i64>(g_max, n_groups[s]);
        const i32 *g = group_host + (size_t)s * n_ctg;
        for (i32 c = 0; c < n_ctg; ++c)
            if (g[c] < -1 || g[c] >= n_groups[s]) return fail("%s: group id %d of contig %d in set %d (n_groups %d)", who, g[c], c, s, n_groups[s]);
    }
    if (n_re && !group_re_host) return fail("%s: null pointer", who);
    DevBuf<i32> d_group, d_ng, d_ncells, d_maxg, d_items;
    DevBuf<i64> d_reoff, d_gre, d_cre, d_maxl;
    DevBuf<double> d_other;
    DevBuf<unsigned long long> d_nspill;
    if (d_group.alloc(cells) || d_ng.alloc((size_t)n_sets) || d_reoff.alloc((size_t)n_sets) || d_gre.alloc((size_t)n_re + 1) || d_cre.alloc((size_t)n_ctg) ||
        d_ncells.alloc(cells) || d_maxg.alloc(cells) || d_maxl.alloc(cells) || d_other.alloc(cells) || d_items.alloc(cells) ||
        d_nspill.alloc(1))
        return 1;
    HHX_HIP(hipMemcpyAsync(d_group.p, group_host, sizeof(i32) * cells, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_ng.p, n_groups, sizeof(i32) * (size_t)n_sets, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_reoff.p, re_off.data(), sizeof(i64) * (size_t)n_sets, hipMemcpyHostToDevice, g_stream));
    if (n_re) HHX_HIP(hipMemcpyAsync(d_gre.p, group_re_host, sizeof(i64) * (size_t)n_re, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_cre.p, ctg_re_host, sizeof(i64) * (size_t)n_ctg, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemsetAsync(d_nspill.p, 0, sizeof(unsigned long long), g_stream));
    // ---- (a) the symmetric adjacency by contig: count, scan, scatter
    GsAdjacency A;
    HHX_TRY(gs_build_adjacency(who, src, n_ctg, A));
    const i64 *rowptr = A.rowptr.p, *lk = A.lk.p;
    const i32 *partner = A.partner.p;
    const u64 *ps = A.ps.p;
    // ---- (b) one workgroup per (contig, set)
    i64 slots = std::max<i64>(GS_SLOTS_MIN, std::min<i64>(GS_SLOTS_MAX, tune_get("groupstats_lds_slots", GS_SLOTS_DEFAULT)));
    while (slots & (slots - 1)) slots &= slots - 1;                                 // a power of two, rounded down
    const GsSets S{d_group.p, d_ng.p, d_reoff.p, d_gre.p, d_cre.p, n_ctg, n_sets, sum_mode};
    const GsOut O{d_ncells.p, d_maxl.p, d_maxg.p, d_other.p};
    HHX_TRY((raise_dynamic_lds<k_gs_rows>((int)GS_SLOTS_MAX * 40)));                  // beside the kernel's two static words
    {
        KTimer kt("groupstats_rows");
        k_gs_rows<<<(unsigned)cells, GS_THREADS, (size_t)slots * 40, g_stream>>>(rowptr, partner, lk, ps, S, O, (i32)slots, d_nspill.p,
                                                                                 d_items.p);
        HHX_LAUNCH_CHECK();
    }
    unsigned long long n_spill = 0;
    HHX_HIP(hipMemcpyAsync(&n_spill, d_nspill.p, sizeof n_spill, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    prof_count("groupstats_spilled", (i64)n_spill);
    // ---- (c) the rows with more distinct groups than slots
    if (n_spill) {
        const i64 g_cap = std::max<i64>(1, g_max), p_cap = pow2_ceil(g_cap);
        const size_t per = (size_t)g_cap * 16 + (size_t)p_cap * 20;
        const i64 wgs = std::max<i64>(1, std::min<i64>(std::min<i64>(GS_SPILL_GRID, (i64)n_spill), (i64)(GS_SPILL_BYTES / per)));
        DevBuf<unsigned long long> tsum, tfirst;
        DevBuf<i32> cg;
        DevBuf<i64> cs;
        DevBuf<u64> cf;
        if (tsum.alloc((size_t)wgs * g_cap) || tfirst.alloc((size_t)wgs * g_cap) || cg.alloc((size_t)wgs * p_cap) || cs.alloc((size_t)wgs * p_cap) ||
            cf.alloc((size_t)wgs * p_cap)) return 1;
        HHX_HIP(hipMemsetAsync(tsum.p, 0, sizeof(unsigned long long) * (size_t)wgs * g_cap, g_stream));
        HHX_HIP(hipMemsetAsync(tfirst.p, 0xff, sizeof(unsigned long long) * (size_t)wgs * g_cap, g_stream));
        {
            KTimer kt("groupstats_spill");
            k_gs_spill<<<(unsigned)wgs, GS_THREADS, 0, g_stream>>>(rowptr, partner, lk, ps, S, O, (i64)n_spill, d_items.p, g_cap, p_cap, tsum.p,
                                                                   tfirst.p, cg.p, cs.p, cf.p);
            HHX_LAUNCH_CHECK();
        }
        HHX_HIP(hipStreamSynchronize(g_stream));                                    // the tables are released when this scope ends
    }
    HHX_HIP(hipMemcpyAsync(n_cells, d_ncells.p, sizeof(i32) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(max_links, d_maxl.p, sizeof(i64) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(max_group, d_maxg.p, sizeof(i32) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(other_sum, d_other.p, sizeof(double) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

}  // namespace

extern "C" int hhx_ingest_group_stats(hhx_ingest *h, int32_t n_sets, const int32_t *group_host, const int32_t *n_groups, const int64_t *group_re_host,
                                      const int64_t *ctg_re_host, int sum_mode, int32_t *n_cells, int64_t *max_links, int32_t *max_group,
                                      double *other_sum) {
    if (!h || !h->finalized) return fail("ingest handle not finalized");
    if (n_sets < 0) return fail("hhx_ingest_group_stats: bad arguments");
    const LinkRun *r = h->table(0);
    GsSource src{};
    if (r && r->n) {
        src.n = r->n;
        src.key = r->key.p;
        src.ord = r->ord_full.p;
        src.ht = r->ht.p;
    }
    return gs_run("hhx_ingest_group_stats", src, h->t.n_ctg, n_sets, group_host, n_groups, group_re_host, ctg_re_host, sum_mode, n_cells, max_links,
                  max_group, other_sum);
}

extern "C" int hhx_group_stats(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const int64_t *links, int on_device, int32_t n_ctg,
                               int32_t n_sets, const int32_t *group_host, const int32_t *n_groups, const int64_t *group_re_host,
                               const int64_t *ctg_re_host, int sum_mode, int32_t *n_cells, int64_t *max_links, int32_t *max_group, double *other_sum) {
    if (n_keys < 0 || n_ctg < 0 || n_sets < 0) return fail("hhx_group_stats: bad arguments");
    if (n_keys && (!frag_i || !frag_j || !links)) return fail("hhx_group_stats: null pointer");
    DevBuf<i32> di, dj;
    DevBuf<i64> dl;
    GsSource src{};
    src.n = n_keys;
    src.fi = frag_i; src.fj = frag_j; src.links = links;
    if (n_keys && !on_device) {
        if (di.alloc((size_t)n_keys) || dj.alloc((size_t)n_keys) || dl.alloc((size_t)n_keys)) return 1;
        HHX_HIP(hipMemcpyAsync(di.p, frag_i, sizeof(i32) * (size_t)n_keys, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(dj.p, frag_j, sizeof(i32) * (size_t)n_keys, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(dl.p, links, sizeof(i64) * (size_t)n_keys, hipMemcpyHostToDevice, g_stream));
        src.fi = di.p; src.fj = dj.p; src.links = dl.p;
    }
    return gs_run("hhx_group_stats", src, n_ctg, n_sets, group_host, n_groups, group_re_host, ctg_re_host, sum_mode, n_cells, max_links, max_group,
                  other_sum);
}
