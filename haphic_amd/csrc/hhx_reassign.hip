// The rescue and reassignment rounds of `haphic reassign` (HapHiC_reassign.py run_reassignment :266-427) and the group-pair sums of its
// agglomerative step (:494-508).
//   A round walks the contigs in one fixed order; each contig is judged against the state left by all earlier contigs of the round: its cells
//   (links to every group) ordered by (sum descending, position in the inner dict ascending), the four filters :335-368, the densities of the other
//   cells added one by one as the interpreter's sum() adds them, the verdict :392-424.  A contig that is rescued or reassigned changes group_RE of
//   two groups — which every later density reads — and, for each of its neighbours, the cells of its former and its new group (update :270-285).
// So the walk is sequential in its movers only.  The handle keeps the dense [contigs x groups] tables `sum` and `stamp` (the cell's position in its
// inner dict: 2 * key + side of its first contribution, or 2 * n_keys + number of the move that created it) and the symmetric adjacency by contig.
// One round is a chain of launch pairs on one stream:
//   k_ra_evaluate   one workgroup per contig of a window of the visiting order that starts at the cursor (device memory): compacts the non-zero
//                   cells of the row (zero cells weigh nothing in any verdict while min_links >= 1), orders them with the bitonic network of
//                   hhx_groupstats.h, forms the quotients in parallel, lets one lane add them in order and writes a verdict and a target group
//   k_ra_commit     one workgroup: finds the first mover of the window, tallies the verdicts up to and including it (final: nothing they read has
//                   changed), applies that one move across its lanes, advances the cursor past the mover and sets the next window (twice the
//                   distance just covered, at most the knob "reassign_window"): nothing judged after a mover is kept
// The host reads the cursor back once per RA_BATCH pairs; pairs launched past the end return at once.  No kernel waits for another workgroup.
// A row of up to "groupstats_lds_slots" groups is ordered in LDS, a wider one on a per-workgroup table in HBM.  Everything that reaches a comparison
// is an integer or a correctly rounded float64 operation (-ffp-contract=off), so the result equals the reference's below 2^53.
#include <memory>

#include "hhx_groupstats.h"
#include "hhx_internal.h"

namespace {

constexpr i64 RA_WINDOW_DEFAULT = 512, RA_WINDOW_MAX = 4096;
constexpr int RA_BATCH = 16;                       // launch pairs between two reads of the cursor
constexpr i64 RA_SLOTS_MAX = 2048;                 // 20 bytes of LDS per slot
enum { ST_CURSOR = 0, ST_WINDOW, ST_MOVES, ST_COUNT0, ST_PAIRS = ST_COUNT0 + 4, ST_WORDS };
enum { V_CONSISTENT = 0, V_RESCUED, V_REASSIGNED, V_NOT_RESCUED };

struct RaParams {
    double min_links, min_link_density, min_density_ratio, ambiguous_cutoff;
    int is_rescue_round, gfa, sum_mode;
    i32 n_groups, n_order, window_max;
    u64 stamp_base;
};

struct RaTables {
    unsigned long long *sum, *stamp;               // [n_ctg][n_groups]
    i32 *group;
    i64 *group_re;
    const i64 *ctg_re;
    const i32 *order;
    const uint8_t *flags;                          // bit 0: RE filter passed, bit 1: short enough to be reassigned
    i64 *state;
    i32 *verdict, *target;                         // of the window
};

// slots != 0: the cells in dynamic LDS (slots of them); else on this workgroup's p_cap cells of the tables in HBM
__global__ __launch_bounds__(GS_THREADS) void k_ra_evaluate(RaTables T, RaParams P, i32 slots, i64 p_cap, i32 *__restrict__ g_all, i64 *__restrict__ s_all,
                                                            u64 *__restrict__ f_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ra_lds[];
    __shared__ int s_n;
    const i64 cursor = T.state[ST_CURSOR], window = T.state[ST_WINDOW];
    if ((i64)blockIdx.x >= window || cursor + (i64)blockIdx.x >= P.n_order) return;
    const int tid = threadIdx.x;
    const i32 c = T.order[cursor + blockIdx.x], G = P.n_groups;
    i64 *cs;
    u64 *cf;
    i32 *cg;
    if (slots) {
        cs = reinterpret_cast<i64 *>(ra_lds);
        cf = reinterpret_cast<u64 *>(cs + slots);
        cg = reinterpret_cast<i32 *>(cf + slots);
    } else {
        cs = s_all + (size_t)blockIdx.x * p_cap;
        cf = f_all + (size_t)blockIdx.x * p_cap;
        cg = g_all + (size_t)blockIdx.x * p_cap;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const unsigned long long *row = T.sum + (size_t)c * G, *row_stamp = T.stamp + (size_t)c * G;
    for (i32 g = tid; g < G; g += GS_THREADS) {
        const i64 v = (i64)row[g];
        if (v != 0) {
            const int i = atomicAdd(&s_n, 1);
            cg[i] = g; cs[i] = v; cf[i] = row_stamp[g];
        }
    }
    __syncthreads();
    const i32 n = s_n;
    int verdict = V_NOT_RESCUED;
    i32 target = -1;
    if ((T.flags[c] & 1) && n > 0) {               // :335 (an inner dict of zeros alone fails min_links next: the same count)
        i32 n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (i32 t = n + tid; t < n2; t += GS_THREADS) { cg[t] = -1; cs[t] = GS_PAD; cf[t] = GS_NONE; }
        __syncthreads();
        gs_sort_cells(cg, cs, cf, n2);
        const i32 own = T.group[c];
        const i64 cre = T.ctg_re[c];
        double *q = reinterpret_cast<double *>(cf);
        for (i32 r = tid; r < n; r += GS_THREADS) {                                // cal_link_density :288-294
            const i32 g = cg[r];
            const i64 den = g == own ? T.group_re[g] : T.group_re[g] + cre - 1;
            q[r] = (double)cs[r] / (double)den;
        }
        __syncthreads();
        if (tid == 0) {
            const i64 max_links = cs[0], second = n > 1 ? cs[1] : 0;
            if ((double)max_links < P.min_links) {
            } else if (!P.is_rescue_round && (double)second / (double)max_links >= P.ambiguous_cutoff) {
            } else if (q[0] < P.min_link_density) {
            } else {
                const double other = gs_ordered_sum(q, 1, n, P.sum_mode);
                const double avg = other != 0.0 ? (P.gfa ? other / (double)(n - 1) : other / (double)(G - 1)) : 1000000000.0;
                const bool ratio_ok = q[0] / avg >= P.min_density_ratio;
                if (own < 0) {
                    if (ratio_ok) { verdict = V_RESCUED; target = cg[0]; }
                } else if ((i64)row[own] == max_links) {
                    verdict = V_CONSISTENT;
                } else if (!P.is_rescue_round && (T.flags[c] & 2) && ratio_ok) {
                    verdict = V_REASSIGNED; target = cg[0];
                } else {
                    verdict = V_CONSISTENT;
                }
            }
        }
    }
    if (tid == 0) { T.verdict[blockIdx.x] = verdict; T.target[blockIdx.x] = target; }
}

__global__ __launch_bounds__(GS_THREADS) void k_ra_commit(RaTables T, RaParams P, const i64 *__restrict__ rowptr, const i32 *__restrict__ partner,
                                                          const i64 *__restrict__ lk) {
    __shared__ int s_first, s_cnt[4];
    const int tid = threadIdx.x;
    const i64 cursor = T.state[ST_CURSOR], window = T.state[ST_WINDOW], moves = T.state[ST_MOVES];
    if (cursor >= P.n_order) return;
    const i64 left = (i64)P.n_order - cursor;
    const i32 m = (i32)(window < left ? window : left), G = P.n_groups;
    if (tid == 0) s_first = m;
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    for (i32 i = tid; i < m; i += GS_THREADS)
        if (T.target[i] >= 0) atomicMin(&s_first, i);
    __syncthreads();
    const i32 first = s_first, upto = first < m ? first + 1 : m;
    for (i32 i = tid; i < upto; i += GS_THREADS) atomicAdd(&s_cnt[T.verdict[i]], 1);
    if (first < m) {                                                               // update :270-285 for the one mover
        const i32 c = T.order[cursor + first], former = T.group[c], to = T.target[first];
        const unsigned long long stamp = P.stamp_base + (u64)moves;
        for (i64 e = rowptr[c] + tid; e < rowptr[c + 1]; e += GS_THREADS) {
            const size_t cell = (size_t)partner[e] * G;
            const unsigned long long v = (unsigned long long)lk[e];
            if (former >= 0) atomicAdd(&T.sum[cell + former], 0ull - v);
            atomicAdd(&T.sum[cell + to], v);
            atomicMin(&T.stamp[cell + to], stamp);                                 // a cell that exists keeps its position, also through zero
        }
    }
    __syncthreads();                                                               // every lane has read the state and group[c]
    if (tid < 4) T.state[ST_COUNT0 + tid] += s_cnt[tid];
    if (tid == 0) {
        i64 next = 2 * window;
        if (first < m) {
            const i32 c = T.order[cursor + first], former = T.group[c], to = T.target[first];
            const i64 d = T.ctg_re[c] - 1;
            if (former >= 0) T.group_re[former] -= d;                              // :417
            T.group_re[to] += d;                                                   // :403 :418
            T.group[c] = to;
            T.state[ST_MOVES] = moves + 1;
            next = 2 * ((i64)first + 1);
        }
        T.state[ST_CURSOR] = cursor + upto;
        T.state[ST_WINDOW] = next < P.window_max ? next : P.window_max;
        T.state[ST_PAIRS] += 1;
    }
}

// :318-324: the contigs of the dismissed groups become 'ungrouped', every contig's links to those groups 0
__global__ __launch_bounds__(GS_THREADS) void k_ra_dismiss(i32 n_ctg, i32 n_groups, const uint8_t *__restrict__ dismissed, i32 *__restrict__ group,
                                                           unsigned long long *__restrict__ sum) {
    const i64 cells = (i64)n_ctg * n_groups;
    for (i64 x = (i64)blockIdx.x * blockDim.x + threadIdx.x; x < cells; x += (i64)gridDim.x * blockDim.x)
        if (dismissed[x % n_groups]) sum[x] = 0;
    for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctg; c += (i64)gridDim.x * blockDim.x) {
        const i32 g = group[c];
        if (g >= 0 && dismissed[g]) group[c] = -1;
    }
}

// :496-508 on ids: key k counts when both contigs are members, both have a group and the groups differ
__global__ __launch_bounds__(GS_THREADS) void k_ra_pair_sums(i64 n, const i32 *__restrict__ fi, const i32 *__restrict__ fj, const i64 *__restrict__ links,
                                                             const uint8_t *__restrict__ member, const i32 *__restrict__ group, i32 n_groups,
                                                             unsigned long long *__restrict__ sums, unsigned long long *__restrict__ first) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) {
        const i32 a = fi[k], b = fj[k];
        if (!member[a] || !member[b]) continue;
        const i32 ga = group[a], gb = group[b];
        if (ga < 0 || gb < 0 || ga == gb) continue;
        const size_t cell = (size_t)(ga < gb ? ga : gb) * n_groups + (ga < gb ? gb : ga);
        atomicAdd(&sums[cell], (unsigned long long)links[k]);
        atomicMin(&first[cell], (unsigned long long)k);
    }
}

int ra_unsupported(const char *why) {
    fail("%s", why);
    return HHX_UNSUPPORTED;
}

}  // namespace

struct hhx_reassign {
    i32 n_ctg = 0, n_groups = 0;
    i64 n_keys = 0, moves = 0;                      // moves: of all rounds so far (the stamps of the cells they create)
    DevBuf<i32> fi, fj, group, order, verdict, target;
    DevBuf<i64> links, group_re, ctg_re, state;
    DevBuf<uint8_t> flags, dismissed;
    DevBuf<unsigned long long> sum, stamp;
    GsAdjacency adj;
};

namespace {

// keys: where frag_i / frag_j / links lie (hipMemcpyHostToDevice or hipMemcpyDeviceToDevice)
int ra_create(const char *who, hipMemcpyKind keys, int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const int64_t *links, int32_t n_ctg,
              const int32_t *group_host, int32_t n_groups, hhx_reassign **out) {
    if (!out) return fail("%s: null pointer", who);
    *out = nullptr;
    if (n_keys < 0 || n_ctg < 0 || n_groups < 0) return fail("%s: bad arguments", who);
    if ((n_ctg && !group_host) || (n_keys && (!frag_i || !frag_j || !links))) return fail("%s: null pointer", who);
    for (i32 c = 0; c < n_ctg; ++c)
        if (group_host[c] < -1 || group_host[c] >= n_groups) return fail("%s: group id %d of contig %d (n_groups %d)", who, group_host[c], c, n_groups);
    const size_t cells = (size_t)n_ctg * (size_t)n_groups;
    size_t free_b = 0, total_b = 0;
    HHX_HIP(hipMemGetInfo(&free_b, &total_b));
    if (cells * 16 > total_b / 2) return ra_unsupported("reassign: two tables of n_ctg * n_groups 8-byte cells are more than half of the device's memory");
    std::unique_ptr<hhx_reassign> h(new hhx_reassign);
    h->n_ctg = n_ctg; h->n_groups = n_groups; h->n_keys = n_keys;
    if (h->fi.alloc((size_t)n_keys + 1) || h->fj.alloc((size_t)n_keys + 1) || h->links.alloc((size_t)n_keys + 1) || h->group.alloc((size_t)n_ctg + 1) ||
        h->group_re.alloc((size_t)n_groups + 1) || h->ctg_re.alloc((size_t)n_ctg + 1) || h->flags.alloc((size_t)n_ctg + 1) ||
        h->dismissed.alloc((size_t)n_groups + 1) || h->state.alloc(ST_WORDS) || h->sum.alloc(cells + 1) || h->stamp.alloc(cells + 1) ||
        h->verdict.alloc(RA_WINDOW_MAX) || h->target.alloc(RA_WINDOW_MAX)) return 1;
    if (n_keys) {
        HHX_HIP(hipMemcpyAsync(h->fi.p, frag_i, sizeof(i32) * (size_t)n_keys, keys, g_stream));
        HHX_HIP(hipMemcpyAsync(h->fj.p, frag_j, sizeof(i32) * (size_t)n_keys, keys, g_stream));
        HHX_HIP(hipMemcpyAsync(h->links.p, links, sizeof(i64) * (size_t)n_keys, keys, g_stream));
    }
    if (n_ctg) HHX_HIP(hipMemcpyAsync(h->group.p, group_host, sizeof(i32) * (size_t)n_ctg, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemsetAsync(h->state.p, 0, sizeof(i64) * ST_WORDS, g_stream));
    HHX_HIP(hipMemsetAsync(h->sum.p, 0, sizeof(unsigned long long) * (cells + 1), g_stream));
    HHX_HIP(hipMemsetAsync(h->stamp.p, 0xff, sizeof(unsigned long long) * (cells + 1), g_stream));
    GsSource src{};
    src.n = n_keys;
    src.fi = h->fi.p; src.fj = h->fj.p; src.links = h->links.p;
    HHX_TRY(gs_build_adjacency(who, src, n_ctg, h->adj));                           // checks every contig id, so that no kernel below indexes out of bounds
    h->adj.ps.release();                                                            // the positions live on as stamps
    if (cells) HHX_TRY(launch_group_link_sums(n_keys, h->fi.p, h->fj.p, h->links.p, h->group.p, n_groups, h->sum.p, h->stamp.p));
    HHX_HIP(hipStreamSynchronize(g_stream));
    *out = h.release();
    return 0;
}

}  // namespace

extern "C" int hhx_reassign_create(int64_t n_keys, const int32_t *frag_i, const int32_t *frag_j, const int64_t *links, int32_t n_ctg,
                                   const int32_t *group_host, int32_t n_groups, hhx_reassign **out) {
    return ra_create("hhx_reassign_create", hipMemcpyHostToDevice, n_keys, frag_i, frag_j, links, n_ctg, group_host, n_groups, out);
}

int hhx_reassign_create_device(const char *who, i64 n_keys, const i32 *frag_i, const i32 *frag_j, const i64 *links, i32 n_ctg, const i32 *group_host,
                               i32 n_groups, hhx_reassign **out) {
    return ra_create(who, hipMemcpyDeviceToDevice, n_keys, frag_i, frag_j, links, n_ctg, group_host, n_groups, out);
}

extern "C" int hhx_reassign_cells(hhx_reassign *h, int64_t *sums_host, int64_t *first_host) {
    if (!h || !sums_host || !first_host) return fail("hhx_reassign_cells: null pointer");
    const size_t cells = (size_t)h->n_ctg * (size_t)h->n_groups;
    if (!cells) return 0;
    HHX_HIP(hipMemcpyAsync(sums_host, h->sum.p, sizeof(i64) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(first_host, h->stamp.p, sizeof(i64) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_reassign_round(hhx_reassign *h, int32_t *group_host, int64_t *group_re_host, const int64_t *ctg_re_host, int32_t n_order,
                                  const int32_t *order_host, const uint8_t *flags_host, const uint8_t *dismissed_host, double min_links,
                                  double min_link_density, double min_density_ratio, double ambiguous_cutoff, int is_rescue_round, int gfa,
                                  int sum_mode, int64_t *counts, int64_t *launches) {
    if (!h) return fail("hhx_reassign_round: null handle");
    if (sum_mode != 0 && sum_mode != 1) return ra_unsupported("reassign: sum_mode is 0 (plain sum) or 1 (Neumaier's, CPython >= 3.12)");
    if (n_order < 0 || !counts || (n_order && !order_host)) return fail("hhx_reassign_round: bad arguments");
    const i32 n_ctg = h->n_ctg, G = h->n_groups;
    if ((n_ctg && (!group_host || !ctg_re_host || !flags_host)) || (G && !group_re_host)) return fail("hhx_reassign_round: null pointer");
    if (!(min_links >= 1.0)) return fail("hhx_reassign_round: min_links below 1 (zero cells would weigh)");
    for (i32 c = 0; c < n_ctg; ++c)
        if (group_host[c] < -1 || group_host[c] >= G) return fail("hhx_reassign_round: group id %d of contig %d (n_groups %d)", group_host[c], c, G);
    for (i32 k = 0; k < n_order; ++k)
        if ((u32)order_host[k] >= (u32)n_ctg) return fail("hhx_reassign_round: contig id %d in the visiting order (n_ctg %d)", order_host[k], n_ctg);
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (launches) *launches = 0;
    if (h->order.n < (size_t)n_order + 1 && h->order.alloc((size_t)n_order + 1)) return 1;
    if (n_ctg) {
        HHX_HIP(hipMemcpyAsync(h->group.p, group_host, sizeof(i32) * (size_t)n_ctg, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(h->ctg_re.p, ctg_re_host, sizeof(i64) * (size_t)n_ctg, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(h->flags.p, flags_host, (size_t)n_ctg, hipMemcpyHostToDevice, g_stream));
    }
    if (G) HHX_HIP(hipMemcpyAsync(h->group_re.p, group_re_host, sizeof(i64) * (size_t)G, hipMemcpyHostToDevice, g_stream));
    if (n_order) HHX_HIP(hipMemcpyAsync(h->order.p, order_host, sizeof(i32) * (size_t)n_order, hipMemcpyHostToDevice, g_stream));
    const i64 window = std::max<i64>(1, std::min<i64>(RA_WINDOW_MAX, tune_get("reassign_window", RA_WINDOW_DEFAULT)));
    i64 slots = std::max<i64>(16, std::min<i64>(RA_SLOTS_MAX, tune_get("groupstats_lds_slots", RA_SLOTS_MAX)));
    while (slots & (slots - 1)) slots &= slots - 1;
    const i64 p_cap = pow2_ceil(std::max<i32>(1, G));
    const bool lds = p_cap <= slots;
    i64 st[ST_WORDS] = {};
    const i64 moves0 = h->moves;
    st[ST_WINDOW] = window;
    st[ST_MOVES] = moves0;
    HHX_HIP(hipMemcpyAsync(h->state.p, st, sizeof st, hipMemcpyHostToDevice, g_stream));
    if (dismissed_host && n_ctg && G) {
        HHX_HIP(hipMemcpyAsync(h->dismissed.p, dismissed_host, (size_t)G, hipMemcpyHostToDevice, g_stream));
        k_ra_dismiss<<<gs_grid((u64)n_ctg * (u64)G), GS_THREADS, 0, g_stream>>>(n_ctg, G, h->dismissed.p, h->group.p, h->sum.p);
        HHX_LAUNCH_CHECK();
    }
    DevBuf<i32> g_all;
    DevBuf<i64> s_all;
    DevBuf<u64> f_all;
    if (!lds && (g_all.alloc((size_t)window * p_cap) || s_all.alloc((size_t)window * p_cap) || f_all.alloc((size_t)window * p_cap))) return 1;
    const RaTables T{h->sum.p, h->stamp.p, h->group.p, h->group_re.p, h->ctg_re.p, h->order.p, h->flags.p, h->state.p, h->verdict.p, h->target.p};
    const RaParams P{min_links, min_link_density, min_density_ratio, ambiguous_cutoff, is_rescue_round != 0, gfa != 0, sum_mode, G, n_order, (i32)window,
                     2 * (u64)h->n_keys};
    {
        KTimer kt("reassign_round");
        while (n_order && G && st[ST_CURSOR] < n_order) {
            for (int b = 0; b < RA_BATCH; ++b) {
                k_ra_evaluate<<<(unsigned)window, GS_THREADS, lds ? (size_t)p_cap * 20 : 0, g_stream>>>(T, P, lds ? (i32)p_cap : 0, p_cap, g_all.p, s_all.p,
                                                                                                      f_all.p);
                HHX_LAUNCH_CHECK();
                k_ra_commit<<<1, GS_THREADS, 0, g_stream>>>(T, P, h->adj.rowptr.p, h->adj.partner.p, h->adj.lk.p);
                HHX_LAUNCH_CHECK();
            }
            HHX_HIP(hipMemcpyAsync(st, h->state.p, sizeof st, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipStreamSynchronize(g_stream));
        }
    }
    h->moves = st[ST_MOVES];
    if (n_order && !G) st[ST_COUNT0 + V_NOT_RESCUED] = n_order;                     // no group at all: every inner dict is empty :335
    for (int k = 0; k < 4; ++k) counts[k] = st[ST_COUNT0 + k];
    if (launches) *launches = st[ST_PAIRS];
    prof_count("reassign_launch_pairs", st[ST_PAIRS]);
    prof_count("reassign_movers", st[ST_MOVES] - moves0);
    if (n_ctg) HHX_HIP(hipMemcpyAsync(group_host, h->group.p, sizeof(i32) * (size_t)n_ctg, hipMemcpyDeviceToHost, g_stream));
    if (G) HHX_HIP(hipMemcpyAsync(group_re_host, h->group_re.p, sizeof(i64) * (size_t)G, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_reassign_pair_sums(hhx_reassign *h, const uint8_t *member_host, const int32_t *group_of_ctg_host, int32_t n_groups, int64_t *sums_host,
                                      int64_t *first_host) {
    if (!h) return fail("hhx_reassign_pair_sums: null handle");
    if (n_groups < 0) return fail("hhx_reassign_pair_sums: bad arguments");
    const size_t cells = (size_t)n_groups * (size_t)n_groups;
    if (!cells) return 0;
    if (!sums_host || !first_host || (h->n_ctg && (!member_host || !group_of_ctg_host))) return fail("hhx_reassign_pair_sums: null pointer");
    for (i32 c = 0; c < h->n_ctg; ++c)
        if (group_of_ctg_host[c] < -1 || group_of_ctg_host[c] >= n_groups)
            return fail("hhx_reassign_pair_sums: group id %d of contig %d (n_groups %d)", group_of_ctg_host[c], c, n_groups);
    DevBuf<uint8_t> member;
    DevBuf<i32> group;
    DevBuf<unsigned long long> sums, first;
    if (member.alloc((size_t)h->n_ctg + 1) || group.alloc((size_t)h->n_ctg + 1) || sums.alloc(cells) || first.alloc(cells)) return 1;
    if (h->n_ctg) {
        HHX_HIP(hipMemcpyAsync(member.p, member_host, (size_t)h->n_ctg, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(group.p, group_of_ctg_host, sizeof(i32) * (size_t)h->n_ctg, hipMemcpyHostToDevice, g_stream));
    }
    HHX_HIP(hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * cells, g_stream));
    HHX_HIP(hipMemsetAsync(first.p, 0xff, sizeof(unsigned long long) * cells, g_stream));
    if (h->n_keys) {
        KTimer kt("reassign_pair_sums");
        k_ra_pair_sums<<<gs_grid((u64)h->n_keys), GS_THREADS, 0, g_stream>>>(h->n_keys, h->fi.p, h->fj.p, h->links.p, member.p, group.p, n_groups, sums.p,
                                                                            first.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(sums_host, sums.p, sizeof(i64) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(first_host, first.p, sizeof(i64) * cells, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_reassign_destroy(hhx_reassign *h) {
    if (h) {
        (void)hipStreamSynchronize(g_stream);
        delete h;
    }
    return 0;
}
