// `haphic sort`, fast sorting (HapHiC_sort.py fast_sort :470-615): the dense work of one group, per round, on the device.
//
//   link matrix      dict_to_matrix :60-88        k_sg_scatter (round 1), k_sg_emit_dense (later rounds)
//   density graph    get_density_graph :158-192   k_sg_density: L[i][j] in float64 from the two lengths -> float32, D = S / L in float32
//   confidence       :195-244                     k_sg_top3 (the three largest of every row, with multiplicity) + k_sg_conf (one thread per edge)
//   re-aggregation   update :406-435              k_sg_agg_lds | k_sg_agg_global (scatter-add of the round-1 edges through map[old] -> new),
//                                                 k_sg_rowcount + scan + k_sg_emit_edges (the lower-triangle edge list in row-major order)
//
// Nothing here depends on the order in which entries are visited: the accumulators are integers, the float32 divide is the correctly rounded one
// (no fast-math flag, -ffp-contract=off), and the two places where float32 / libm order would show are REPORTED to the host instead of guessed:
// cells whose integer sum exceeds 2^24 (the reference adds numpy.float32 one at a time) and geometric-mean products whose float64 root lies within
// 2 ulp of a float32 rounding boundary (Python's ** and a correctly rounded sqrt differ by an ulp now and then).
//
// The seam between the two re-aggregation paths: the new shape x new shape accumulator of u32 cells lives in the LDS of every workgroup (merged once
// with 64-bit global atomics) while  shape <= SG_LDS_SHAPE (192: 144 KiB of the 160 KiB of a CU)  and the weights of the group sum to less than 2^32
// (so no workgroup's partial sum can wrap); everything else adds straight to the 64-bit accumulator in HBM.  hhx_tune "sort_lds_shape" lowers the seam.
//
//   spanning forest  fast_sort :567-595           hhx_sort_graph_forest: filter_confidence_graph :247-255 on the cells, then the forest networkx's Kruskal
//                                                 builds from Graph(confidence_graph), its edges in Kruskal's order, a tree label and a path position per node
//
// Kruskal over the upper triangle in row-major order with a stable descending sort is the unique maximum spanning forest under the strict total order
// (weight descending, u ascending, v ascending), u < v.  Every cell is a float32 widened to float64 (a confidence) or twice one (the sister weight),
// so the float32 bits of a cell order like the cell (a sister weight past FLT_MAX becomes +inf, still above every confidence it was above): one u64 key
// per edge,  ~float32 bits << 32 | u * shape + v,  ascending = Kruskal's order; the two keys of a pair that is both a list edge and a sister pair are
// equal and the second is skipped.  Boruvka on the ranks: every component takes its lowest-rank outgoing edge with an atomic min, hooks onto the other
// side (the smaller index stays root where two components chose each other), a chase to the roots relabels the nodes.  When every node has degree 1 or
// 2 the trees are paths: pointer doubling over the 2 * shape (node, side) slots gives every node both ends of its path and the distance to each.
//
// Two forms, the same phase functions in both.  ONE workgroup of 1024 threads keeps keys (bitonic sort), chosen flags, labels, hooks and the jump
// pointers in LDS and finishes in one launch while  shape <= SF_LDS_SHAPE (2048)  and the edges that survive the filter number at most `cap`, the
// largest power of two with  12 * cap + 48 * shape + SF_LDS_STATIC <= 160 KiB  (shape 2048: cap 4096, a path-and-cycle graph has at most 1.5 * shape
// edges); a group with more edges reports so and is redone by the other form: one launch per phase on arrays in HBM, the radix sort of hhx_sort.h,
// one host round trip per Boruvka round.  hhx_tune "sort_forest_lds" lowers the seam (0: always HBM).  shape <= 65535 (the key holds u * shape + v).
#include <algorithm>

#include "hhx_common.h"
#include "hhx_sort.h"

using namespace hhx;

namespace {
constexpr int SG_T = 256;
constexpr int SG_WAVES = SG_T / HHX_WAVE;
constexpr int SG_LDS_SHAPE = 192;
constexpr i64 SG_LIST_CAP = 1 << 20;            // flagged geometric-mean pairs / cells above 2^24 a call can report
constexpr u64 SG_EXACT = 1ull << 24;            // float32 sums of non-negative integers are exact up to here
constexpr int SF_T = 1024;                      // the one workgroup of the LDS form of the forest
constexpr int SF_LDS_SHAPE = 2048;
constexpr int SF_LDS_BYTES = 160 * 1024;
constexpr int SF_LDS_STATIC = 4608;             // the static LDS of k_sf_lds (scan partials, counters), rounded up
constexpr i32 SF_MAX_SHAPE = 65535;
constexpr int SF_MAX_ROUNDS = 40;               // Boruvka at least halves the components with an outgoing edge per round: 16 rounds at shape 65535
constexpr u32 SF_NONE = 0xFFFFFFFFu;
constexpr int SF_N_STATS = HHX_SORT_FOREST_N_STATS;
}  // namespace

struct hhx_sort_graph {
    i32 shape0 = 0, shape = 0;                  // round-1 shape; the current one (the leading block of S / D)
    i64 ld = 0;                                 // row pitch of S and D: the shape they were built at (remove_shortest_path keeps it)
    i64 n0 = 0, nc = 0;                         // round-1 edges; edges of the current list (dropped ones included: `dead` hides them)
    u64 total_w = 0;
    bool own_list = false;                      // the current list is c_i / c_j (after a re-aggregation), else the round-1 edges
    i64 n_flag = 0, n_over = 0;
    i64 stats[HHX_SORT_GRAPH_N_STATS] = {0, 0, 0, 0};
    i64 fstats[SF_N_STATS] = {0, 0, 0, 0, 0};   // forests through LDS, through HBM, Boruvka rounds and jump rounds of the last one, confidence copies
    bool have_conf = false, have_forest = false;
    i32 n_pairs = 0;                            // sister pairs of the last confidence call (in `pairs`)
    i32 f_shape = 0, f_not_paths = 0;           // the last forest
    i64 f_chosen = 0;
    DevBuf<i32> f_eu, f_ev, f_label, f_pos;
    DevBuf<i64> f_res;
    DevBuf<i32> e_a, e_b, c_i, c_j, map, rowcnt, rowptr, pairs, flag;
    DevBuf<i64> e_w, counter, over;
    DevBuf<float> c_w, S, D, top;
    DevBuf<double> C, len;
    DevBuf<u64> acc;
    DevBuf<u32> maxbits;
    DevBuf<unsigned char> dead;
};

// ------------------------------------------------------------------ link matrix of round 1
static __global__ __launch_bounds__(SG_T) void k_sg_scatter(const i32 *__restrict__ a, const i32 *__restrict__ b, const i64 *__restrict__ w, i64 n,
                                                            float *__restrict__ S, i64 ld) {
    for (i64 e = (i64)blockIdx.x * SG_T + threadIdx.x; e < n; e += (i64)gridDim.x * SG_T) {
        const float v = (float)w[e];            // coo_matrix(..., dtype=float32): the integer rounded to nearest even
        S[(i64)a[e] * ld + b[e]] = v;
        S[(i64)b[e] * ld + a[e]] = v;
    }
}

// ------------------------------------------------------------------ density
// METHOD 0 sum, 1 multiplication, 2 geometric_mean (:177-182); the diagonal of L is 1 (add_self_loops :187)
template <int METHOD>
static __global__ __launch_bounds__(SG_T) void k_sg_density(const float *__restrict__ S, float *__restrict__ D, i64 ld, i32 n, const double *__restrict__ len,
                                                            i32 *__restrict__ flag, i64 *__restrict__ n_flag, i64 cap) {
    const i32 c = blockIdx.x * SG_T + threadIdx.x;
    if (c >= n) return;
    const double b = len[c];
    for (i32 r = blockIdx.y; r < n; r += gridDim.y) {
        float L = 1.0f;
        if (r != c) {
            const double a = len[r];
            double v;
            if (METHOD == 0) v = a + b;
            else if (METHOD == 1) v = a * b;
            else {
                v = sqrt(a * b);
                // a float32 rounding boundary is a float64 whose low 29 mantissa bits are 1 0000...: within 2 ulp of one, Python's (a * b) ** 0.5
                // may fall on the other side -> the host recomputes the pair with ** (hhx_sort_graph_patch_len)
                const i64 low = (i64)((u64)__double_as_longlong(v) & 0x1FFFFFFFull) - 0x10000000ll;
                if (r < c && low >= -2 && low <= 2) {
                    const i64 k = (i64)atomicAdd((unsigned long long *)n_flag, 1ull);
                    if (k < cap) { flag[2 * k] = r; flag[2 * k + 1] = c; }
                }
            }
            L = (float)v;
        }
        D[(i64)r * ld + c] = S[(i64)r * ld + c] / L;
    }
}

static __global__ void k_sg_patch_len(i64 n, const i32 *__restrict__ pi, const i32 *__restrict__ pj, const float *__restrict__ L, const float *__restrict__ S,
                                      float *__restrict__ D, i64 ld) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const i64 x = (i64)pi[k] * ld + pj[k], y = (i64)pj[k] * ld + pi[k];
    D[x] = S[x] / L[k];
    D[y] = S[y] / L[k];
}

// ------------------------------------------------------------------ confidence
__device__ __forceinline__ void sg_push(float &t0, float &t1, float &t2, float v) {
    if (v > t0) { t2 = t1; t1 = t0; t0 = v; }
    else if (v > t1) { t2 = t1; t1 = v; }
    else if (v > t2) t2 = v;
}

// one wave per row of the leading n x n block of D: its three largest values, equal values counted as often as they occur
static __global__ __launch_bounds__(SG_T) void k_sg_top3(const float *__restrict__ D, i64 ld, i32 n, float *__restrict__ top) {
    const int lane = lane_id();
    for (i32 r = blockIdx.x * SG_WAVES + threadIdx.x / HHX_WAVE; r < n; r += gridDim.x * SG_WAVES) {
        float t0 = -1.0f, t1 = -1.0f, t2 = -1.0f;           // densities are >= 0
        const float *row = D + (i64)r * ld;
        for (i32 c = lane; c < n; c += HHX_WAVE) sg_push(t0, t1, t2, row[c]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float u0 = __shfl_xor(t0, o, HHX_WAVE), u1 = __shfl_xor(t1, o, HHX_WAVE), u2 = __shfl_xor(t2, o, HHX_WAVE);
            sg_push(t0, t1, t2, u0);
            sg_push(t0, t1, t2, u1);
            sg_push(t0, t1, t2, u2);
        }
        if (lane == 0) { top[3 * (i64)r] = t0; top[3 * (i64)r + 1] = t1; top[3 * (i64)r + 2] = t2; }
    }
}

// one thread per edge (i, j): the second largest of {row i minus one instance of d} + {row j} (:211-217) is the second of the merged
// candidates (top-3 of row i minus one d, else its top-2) and (top-2 of row j).  C: n x n float64, zeroed; maxbits: the float32 bits of MAXS.
static __global__ __launch_bounds__(SG_T) void k_sg_conf(const i32 *__restrict__ ei, const i32 *__restrict__ ej, i64 ne, const unsigned char *__restrict__ dead,
                                                         const float *__restrict__ D, i64 ld, i32 n, const float *__restrict__ top, double *__restrict__ C,
                                                         u32 *__restrict__ maxbits) {
    float best = 0.0f;
    for (i64 e = (i64)blockIdx.x * SG_T + threadIdx.x; e < ne; e += (i64)gridDim.x * SG_T) {
        const i32 i = ei[e], j = ej[e];
        if (dead[i] || dead[j]) continue;
        const float d = D[(i64)i * ld + j];
        const float a0 = top[3 * (i64)i], a1 = top[3 * (i64)i + 1], a2 = top[3 * (i64)i + 2];
        float x0, x1;
        if (d == a0) { x0 = a1; x1 = a2; }
        else if (d == a1) { x0 = a0; x1 = a2; }
        else { x0 = a0; x1 = a1; }
        const float b0 = top[3 * (i64)j], b1 = top[3 * (i64)j + 1];
        const float second = x0 >= b0 ? fmaxf(x1, b0) : fmaxf(x0, b1);
        float conf;
        if (d == 0.0f) conf = 0.0f;
        else if (second == 0.0f) conf = 2.0f;
        else conf = d / second;
        C[(i64)i * n + j] = (double)conf;
        C[(i64)j * n + i] = (double)conf;
        best = fmaxf(best, conf);
    }
    best = wave_max_f32(best);
    if (lane_id() == 0 && best > 0.0f) atomicMax(maxbits, __float_as_uint(best));       // non-negative floats order like their bits
}

// sister edges :238-242 and MAXS itself behind the matrix (one copy takes both to the host)
static __global__ void k_sg_sister(const i32 *__restrict__ pa, const i32 *__restrict__ pb, i32 n_pairs, const u32 *__restrict__ maxbits, double *__restrict__ C,
                                   i32 n) {
    const double maxs = (double)__uint_as_float(*maxbits);
    const double w = maxs > 1.0 ? 2.0 * maxs : 2.0;
    const i32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) C[(i64)n * n] = maxs;
    if (k >= n_pairs) return;
    C[(i64)pa[k] * n + pb[k]] = w;
    C[(i64)pb[k] * n + pa[k]] = w;
}

// ------------------------------------------------------------------ re-aggregation
__device__ __forceinline__ i64 sg_cell(const i32 *__restrict__ map, i32 a, i32 b, i32 ns) {
    const i32 i = map[a], j = map[b];
    if (i < 0 || j < 0 || i == j || (i ^ 1) == j) return -1;        // trimmed / removed ends, the same new end, sisters (:412)
    return (i64)max(i, j) * ns + min(i, j);
}

static __global__ __launch_bounds__(SG_T) void k_sg_agg_global(const i32 *__restrict__ a, const i32 *__restrict__ b, const i64 *__restrict__ w, i64 n,
                                                               const i32 *__restrict__ map, i32 ns, u64 *__restrict__ acc) {
    for (i64 e = (i64)blockIdx.x * SG_T + threadIdx.x; e < n; e += (i64)gridDim.x * SG_T) {
        const i64 cell = sg_cell(map, a[e], b[e], ns);
        if (cell >= 0) atomicAdd((unsigned long long *)&acc[cell], (unsigned long long)w[e]);
    }
}

static __global__ __launch_bounds__(SG_T) void k_sg_agg_lds(const i32 *__restrict__ a, const i32 *__restrict__ b, const i64 *__restrict__ w, i64 n,
                                                            const i32 *__restrict__ map, i32 ns, u64 *__restrict__ acc) {
    extern __shared__ u32 sg_cells[];                       // ns * ns cells; the group's weights sum to < 2^32
    const i32 n_cells = ns * ns;
    for (i32 k = threadIdx.x; k < n_cells; k += SG_T) sg_cells[k] = 0;
    __syncthreads();
    for (i64 e = (i64)blockIdx.x * SG_T + threadIdx.x; e < n; e += (i64)gridDim.x * SG_T) {
        const i64 cell = sg_cell(map, a[e], b[e], ns);
        if (cell >= 0) atomicAdd(&sg_cells[cell], (u32)w[e]);
    }
    __syncthreads();
    for (i32 k = threadIdx.x; k < n_cells; k += SG_T) {
        const u32 v = sg_cells[k];
        if (v) atomicAdd((unsigned long long *)&acc[k], (unsigned long long)v);
    }
}

// one wave per row r: the non-zero cells left of the diagonal, and the cells the float32 sum of the reference may round (> 2^24)
static __global__ __launch_bounds__(SG_T) void k_sg_rowcount(const u64 *__restrict__ acc, i32 ns, i32 *__restrict__ rowcnt, i64 *__restrict__ over,
                                                             i64 *__restrict__ n_over, i64 cap) {
    const int lane = lane_id();
    for (i32 r = blockIdx.x * SG_WAVES + threadIdx.x / HHX_WAVE; r < ns; r += gridDim.x * SG_WAVES) {
        i32 cnt = 0;
        for (i32 c = lane; c < r; c += HHX_WAVE) {
            const u64 v = acc[(i64)r * ns + c];
            cnt += v != 0;
            if (v > SG_EXACT) {
                const i64 k = (i64)atomicAdd((unsigned long long *)n_over, 1ull);
                if (k < cap) over[k] = (i64)r * ns + c;
            }
        }
        cnt = wave_sum_i32(cnt);
        if (lane == 0) rowcnt[r] = cnt;
    }
}

// the new sub_HT_dict as arrays: keys (i_1, i_2), i_1 > i_2, in row-major order (:409-435), placed by the row offsets and a ballot rank
static __global__ __launch_bounds__(SG_T) void k_sg_emit_edges(const u64 *__restrict__ acc, i32 ns, const i32 *__restrict__ rowptr, i32 *__restrict__ oi,
                                                               i32 *__restrict__ oj, float *__restrict__ ow) {
    const int lane = lane_id();
    const u64 lt = (1ull << lane) - 1ull;
    for (i32 r = blockIdx.x * SG_WAVES + threadIdx.x / HHX_WAVE; r < ns; r += gridDim.x * SG_WAVES) {
        i32 at = rowptr[r];
        for (i32 c0 = 0; c0 < r; c0 += HHX_WAVE) {
            const i32 c = c0 + lane;
            const u64 v = c < r ? acc[(i64)r * ns + c] : 0;
            const u64 m = __ballot(v != 0);
            if (v != 0) {
                const i32 p = at + __popcll(m & lt);
                oi[p] = r;
                oj[p] = c;
                ow[p] = (float)v;
            }
            at += __popcll(m);
        }
    }
}

static __global__ __launch_bounds__(SG_T) void k_sg_emit_dense(const u64 *__restrict__ acc, i32 ns, float *__restrict__ S) {
    const i32 c = blockIdx.x * SG_T + threadIdx.x;
    if (c >= ns) return;
    for (i32 r = blockIdx.y; r < ns; r += gridDim.y)
        S[(i64)r * ns + c] = r == c ? 0.0f : (float)acc[(i64)max(r, c) * ns + min(r, c)];
}

static __global__ void k_sg_patch_cells(i64 n, const i64 *__restrict__ pos, const i64 *__restrict__ ordinal, const float *__restrict__ val, i32 ns,
                                        float *__restrict__ S, float *__restrict__ ow) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const i64 r = pos[k] / ns, c = pos[k] % ns;
    S[r * ns + c] = val[k];
    S[c * ns + r] = val[k];
    ow[ordinal[k]] = val[k];
}

// ------------------------------------------------------------------ spanning forest (head of this file)
// The phases below take (tid, nt): thread tid of nt walks items tid, tid + nt, ...  k_sf_lds runs them in one workgroup on LDS arrays with a barrier
// between two phases, the k_sf_* wrappers run one phase each over arrays in HBM.  Node arrays hold `n` entries, slot arrays 2 * n.
struct SfEdges {                                           // the candidates: the current edge list (dead ends hidden) and the sister pairs
    const i32 *ci, *cj;
    i64 nc;
    const unsigned char *dead;
    const i32 *pa, *pb;
    i32 np;
};

__device__ __forceinline__ void sf_filter(i64 tid, i64 nt, const SfEdges &E, double *__restrict__ C, i32 n, double cutoff) {
    for (i64 e = tid; e < E.nc; e += nt) {
        const i32 i = E.ci[e], j = E.cj[e];
        if (i >= n || j >= n || E.dead[i] || E.dead[j]) continue;
        if (C[(i64)i * n + j] <= cutoff) { C[(i64)i * n + j] = 0.0; C[(i64)j * n + i] = 0.0; }
    }
}

// appends the key of every candidate whose cell is not 0 (any order: the sort follows); *count goes past cap when they do not fit
__device__ __forceinline__ void sf_collect(i64 tid, i64 nt, const SfEdges &E, const double *__restrict__ C, i32 n, u64 *keys, u32 cap, u32 *count) {
    for (i64 e = tid; e < E.nc + E.np; e += nt) {
        i32 a, b;
        if (e < E.nc) {
            a = E.ci[e]; b = E.cj[e];
            if (a >= n || b >= n || E.dead[a] || E.dead[b]) continue;
        } else {
            a = E.pa[e - E.nc]; b = E.pb[e - E.nc];
        }
        const double c = C[(i64)a * n + b];
        if (c == 0.0) continue;
        const u32 k = atomicAdd(count, 1u);
        if (k < cap) keys[k] = ((u64)(~__float_as_uint((float)c)) << 32) | ((u32)min(a, b) * (u32)n + (u32)max(a, b));
    }
}

__device__ __forceinline__ bool sf_twin(const u64 *keys, u32 r) { return r > 0 && keys[r] == keys[r - 1]; }      // a list edge that is a sister pair too

__device__ __forceinline__ void sf_init(i64 tid, i64 nt, i32 n, i32 *comp, u32 *best, i32 *deg, i32 *minv, i32 *nb) {
    for (i64 v = tid; v < n; v += nt) {
        comp[v] = (i32)v; best[v] = SF_NONE; deg[v] = 0; minv[v] = INT32_MAX; nb[2 * v] = -1; nb[2 * v + 1] = -1;
    }
}

__device__ __forceinline__ void sf_best(i64 tid, i64 nt, const u64 *keys, u32 ne, i32 n, const i32 *comp, u32 *best, i32 *any) {
    for (i64 r = tid; r < ne; r += nt) {
        if (sf_twin(keys, (u32)r)) continue;
        const u32 uv = (u32)keys[r];
        const i32 cu = comp[uv / (u32)n], cv = comp[uv % (u32)n];
        if (cu == cv) continue;
        atomicMin(&best[cu], (u32)r);
        atomicMin(&best[cv], (u32)r);
        *any = 1;
    }
}

// every component (its root c has comp[c] == c) hooks onto the other side of its best edge; two that chose each other keep the smaller as root
__device__ __forceinline__ void sf_hook(i64 tid, i64 nt, i32 n, const u64 *keys, const i32 *comp, const u32 *best, i32 *parent, i32 *chosen) {
    for (i64 c = tid; c < n; c += nt) {
        i32 p = (i32)c;
        const u32 r = best[c];
        if (comp[c] == c && r != SF_NONE) {
            chosen[r] = 1;
            const u32 uv = (u32)keys[r];
            const i32 cu = comp[uv / (u32)n], cv = comp[uv % (u32)n];
            const i32 other = cu == c ? cv : cu;
            p = (best[other] == r && c < other) ? (i32)c : other;
        }
        parent[c] = p;
    }
}

// the hooks form trees (ranks are distinct): walk to the root, at most n steps
__device__ __forceinline__ void sf_root(i64 tid, i64 nt, i32 n, const i32 *comp, const i32 *parent, i32 *root) {
    for (i64 c = tid; c < n; c += nt) {
        i32 r = (i32)c;
        if (comp[c] == c)
            for (i32 step = 0; step < n && parent[r] != r; ++step) r = parent[r];
        root[c] = r;
    }
}

__device__ __forceinline__ void sf_relabel(i64 tid, i64 nt, i32 n, i32 *comp, const i32 *root, u32 *best) {
    for (i64 v = tid; v < n; v += nt) { comp[v] = root[comp[v]]; best[v] = SF_NONE; }
}

__device__ __forceinline__ void sf_degree(i64 tid, i64 nt, const u64 *keys, u32 ne, i32 n, const i32 *chosen, i32 *deg, i32 *nb) {
    for (i64 r = tid; r < ne; r += nt) {
        if (!chosen[r]) continue;
        const u32 uv = (u32)keys[r];
        const i32 u = (i32)(uv / (u32)n), v = (i32)(uv % (u32)n);
        const i32 su = atomicAdd(&deg[u], 1), sv = atomicAdd(&deg[v], 1);
        if (su < 2) nb[2 * u + su] = v;
        if (sv < 2) nb[2 * v + sv] = u;
    }
}

__device__ __forceinline__ void sf_label_min(i64 tid, i64 nt, i32 n, const i32 *comp, i32 *minv) {
    for (i64 v = tid; v < n; v += nt) atomicMin(&minv[comp[v]], (i32)v);
}

__device__ __forceinline__ void sf_label_out(i64 tid, i64 nt, i32 n, const i32 *comp, const i32 *minv, const i32 *deg, i32 *__restrict__ label,
                                             i32 *not_paths) {
    for (i64 v = tid; v < n; v += nt) {
        label[v] = minv[comp[v]];
        if (deg[v] < 1 || deg[v] > 2) *not_paths = 1;
    }
}

__device__ __forceinline__ void sf_emit(const u64 *keys, i32 n, u32 r, i32 at, i32 *__restrict__ eu, i32 *__restrict__ ev) {
    const u32 uv = (u32)keys[r];
    eu[at] = (i32)(uv / (u32)n);
    ev[at] = (i32)(uv % (u32)n);
}

// slot x = 2 * v + s: leaving node v through its neighbour s.  T[x]: the slot reached (2 * node + the side that leads on), D[x]: the steps taken;
// a slot with no neighbour is its own target.  One doubling: T[x] <- T[T[x]], D[x] <- D[x] + D[T[x]].
__device__ __forceinline__ void sf_jump_init(i64 tid, i64 nt, i32 n, const i32 *nb, i32 *T, i32 *D) {
    for (i64 x = tid; x < 2 * (i64)n; x += nt) {
        const i32 w = nb[x];
        if (w < 0) { T[x] = (i32)x; D[x] = 0; }
        else { T[x] = 2 * w + (nb[2 * w] == (i32)(x >> 1) ? 1 : 0); D[x] = 1; }
    }
}

__device__ __forceinline__ void sf_jump(i64 tid, i64 nt, i32 n, const i32 *Ti, const i32 *Di, i32 *To, i32 *Do) {
    for (i64 x = tid; x < 2 * (i64)n; x += nt) {
        const i32 t = Ti[x];
        To[x] = Ti[t];
        Do[x] = Di[x] + Di[t];
    }
}

// position along the path, counted from the end with the smaller index; -1 everywhere when some tree is no path
__device__ __forceinline__ void sf_pos(i64 tid, i64 nt, i32 n, const i32 *T, const i32 *D, bool paths, i32 *__restrict__ pos) {
    for (i64 v = tid; v < n; v += nt) pos[v] = !paths ? -1 : ((T[2 * v] >> 1) < (T[2 * v + 1] >> 1) ? D[2 * v] : D[2 * v + 1]);
}

// res[0] = 1: more edges than `cap` (nothing else is written then), res[1] = chosen edges, res[2] = not_paths, res[3] = Boruvka rounds
static __global__ __launch_bounds__(SF_T) void k_sf_lds(SfEdges E, double *__restrict__ C, i32 n, double cutoff, u32 cap, int jump_rounds,
                                                        i32 *__restrict__ eu, i32 *__restrict__ ev, i32 *__restrict__ label, i32 *__restrict__ pos,
                                                        i64 *__restrict__ res) {
    extern __shared__ u64 sf_mem[];
    __shared__ i32 part[SF_T];
    __shared__ u32 s_count;
    __shared__ i32 s_any, s_not_paths;
    u64 *keys = sf_mem;                                    // cap
    i32 *chosen = (i32 *)(keys + cap);                     // cap
    i32 *node = chosen + cap;                              // 12 * n: comp best parent root | deg minv | nb nb | T0 T0 D0 D0; T1 D1 later take the first four
    i32 *comp = node, *parent = node + 2 * (i64)n, *root = node + 3 * (i64)n, *deg = node + 4 * (i64)n, *minv = node + 5 * (i64)n;
    u32 *best = (u32 *)(node + n);
    i32 *nb = node + 6 * (i64)n, *T0 = node + 8 * (i64)n, *D0 = node + 10 * (i64)n, *T1 = node, *D1 = node + 2 * (i64)n;
    const int tid = threadIdx.x;
    if (tid == 0) { s_count = 0; s_not_paths = 0; }
    sf_filter(tid, SF_T, E, C, n, cutoff);
    sf_init(tid, SF_T, n, comp, best, deg, minv, nb);
    __syncthreads();                                       // the filtered cells are read back by other threads of this workgroup
    sf_collect(tid, SF_T, E, C, n, keys, cap, &s_count);
    __syncthreads();
    const u32 ne = s_count;
    if (ne > cap) {
        if (tid == 0) res[0] = 1;
        return;
    }
    u32 P = 1;
    while (P < ne) P <<= 1;
    for (u32 k = ne + tid; k < P; k += SF_T) keys[k] = ~0ull;
    for (u32 k = tid; k < ne; k += SF_T) chosen[k] = 0;
    __syncthreads();
    for (u32 k = 2; k <= P; k <<= 1)
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 i = tid; i < P; i += SF_T) {
                const u32 l = i ^ j;
                if (l > i) {
                    const u64 a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    int rounds = 0;
    for (; rounds < SF_MAX_ROUNDS; ++rounds) {
        if (tid == 0) s_any = 0;
        __syncthreads();
        sf_best(tid, SF_T, keys, ne, n, comp, best, &s_any);
        __syncthreads();
        if (!s_any) break;
        sf_hook(tid, SF_T, n, keys, comp, best, parent, chosen);
        __syncthreads();
        sf_root(tid, SF_T, n, comp, parent, root);
        __syncthreads();
        sf_relabel(tid, SF_T, n, comp, root, best);
        __syncthreads();
    }
    sf_degree(tid, SF_T, keys, ne, n, chosen, deg, nb);
    sf_label_min(tid, SF_T, n, comp, minv);
    __syncthreads();
    sf_label_out(tid, SF_T, n, comp, minv, deg, label, &s_not_paths);
    // the chosen edges in rank order: every thread takes a run of ranks, the runs' counts are scanned
    const u32 per = (ne + SF_T - 1) / SF_T, lo = min(ne, (u32)tid * per), hi = min(ne, lo + per);
    i32 cnt = 0;
    for (u32 r = lo; r < hi; ++r) cnt += chosen[r];
    part[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < SF_T; off <<= 1) {
        const i32 add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    i32 at = part[tid] - cnt;
    for (u32 r = lo; r < hi; ++r)
        if (chosen[r]) sf_emit(keys, n, r, at++, eu, ev);
    const bool paths = !s_not_paths;
    if (tid == 0) { res[0] = 0; res[1] = part[SF_T - 1]; res[2] = s_not_paths; res[3] = rounds; }
    __syncthreads();                                       // comp .. root are free from here: T1 / D1
    if (paths) {
        sf_jump_init(tid, SF_T, n, nb, T0, D0);
        __syncthreads();
        for (int k = 0; k < jump_rounds; ++k) {
            if (k & 1) sf_jump(tid, SF_T, n, T1, D1, T0, D0);
            else sf_jump(tid, SF_T, n, T0, D0, T1, D1);
            __syncthreads();
        }
    }
    sf_pos(tid, SF_T, n, (jump_rounds & 1) ? T1 : T0, (jump_rounds & 1) ? D1 : D0, paths, pos);
}

// the HBM form: one phase per launch
#define SF_TID const i64 tid = (i64)blockIdx.x * blockDim.x + threadIdx.x, nt = (i64)gridDim.x * blockDim.x
static __global__ __launch_bounds__(SG_T) void k_sf_filter(SfEdges E, double *__restrict__ C, i32 n, double cutoff) { SF_TID; sf_filter(tid, nt, E, C, n, cutoff); }
static __global__ __launch_bounds__(SG_T) void k_sf_collect(SfEdges E, const double *__restrict__ C, i32 n, u64 *keys, u32 cap, u32 *count) {
    SF_TID;
    sf_collect(tid, nt, E, C, n, keys, cap, count);
}
static __global__ __launch_bounds__(SG_T) void k_sf_init(i32 n, i32 *comp, u32 *best, i32 *deg, i32 *minv, i32 *nb) { SF_TID; sf_init(tid, nt, n, comp, best, deg, minv, nb); }
static __global__ __launch_bounds__(SG_T) void k_sf_best(const u64 *keys, u32 ne, i32 n, const i32 *comp, u32 *best, i32 *any) {
    SF_TID;
    sf_best(tid, nt, keys, ne, n, comp, best, any);
}
static __global__ __launch_bounds__(SG_T) void k_sf_hook(i32 n, const u64 *keys, const i32 *comp, const u32 *best, i32 *parent, i32 *chosen) {
    SF_TID;
    sf_hook(tid, nt, n, keys, comp, best, parent, chosen);
}
static __global__ __launch_bounds__(SG_T) void k_sf_root(i32 n, const i32 *comp, const i32 *parent, i32 *root) { SF_TID; sf_root(tid, nt, n, comp, parent, root); }
static __global__ __launch_bounds__(SG_T) void k_sf_relabel(i32 n, i32 *comp, const i32 *root, u32 *best) { SF_TID; sf_relabel(tid, nt, n, comp, root, best); }
static __global__ __launch_bounds__(SG_T) void k_sf_degree(const u64 *keys, u32 ne, i32 n, const i32 *chosen, i32 *deg, i32 *nb, const i32 *comp, i32 *minv) {
    SF_TID;
    sf_degree(tid, nt, keys, ne, n, chosen, deg, nb);
    sf_label_min(tid, nt, n, comp, minv);
}
static __global__ __launch_bounds__(SG_T) void k_sf_label_out(i32 n, const i32 *comp, const i32 *minv, const i32 *deg, i32 *label, i32 *not_paths) {
    SF_TID;
    sf_label_out(tid, nt, n, comp, minv, deg, label, not_paths);
}
static __global__ __launch_bounds__(SG_T) void k_sf_emit(const u64 *keys, u32 ne, i32 n, const i32 *chosen, const i32 *at, i32 *eu, i32 *ev) {
    SF_TID;
    for (i64 r = tid; r < ne; r += nt)
        if (chosen[r]) sf_emit(keys, n, (u32)r, at[r], eu, ev);
}
static __global__ __launch_bounds__(SG_T) void k_sf_jump_init(i32 n, const i32 *nb, i32 *T, i32 *D) { SF_TID; sf_jump_init(tid, nt, n, nb, T, D); }
static __global__ __launch_bounds__(SG_T) void k_sf_jump(i32 n, const i32 *Ti, const i32 *Di, i32 *To, i32 *Do) { SF_TID; sf_jump(tid, nt, n, Ti, Di, To, Do); }
static __global__ __launch_bounds__(SG_T) void k_sf_pos(i32 n, const i32 *T, const i32 *D, int paths, i32 *pos) { SF_TID; sf_pos(tid, nt, n, T, D, paths != 0, pos); }
#undef SF_TID

// ------------------------------------------------------------------ host side
static inline unsigned sg_grid(i64 n, i64 per_block) { return (unsigned)std::max<i64>(1, std::min<i64>((n + per_block - 1) / per_block, 2048)); }

template <class T>
static int sg_upload(DevBuf<T> &buf, const T *host, size_t n) {
    if (buf.alloc(n)) return 1;
    if (n) HHX_HIP(hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_create(int32_t shape, int64_t n_edges, const int32_t *ei, const int32_t *ej, const int64_t *w, hhx_sort_graph **out) {
    if (!out) return fail("hhx_sort_graph_create: null out");
    *out = nullptr;
    if (shape < 4 || (shape & 1)) return fail("hhx_sort_graph_create: shape %d (an even shape of at least 4 is needed: two contigs)", shape);
    if (n_edges <= 0 || !ei || !ej || !w) return fail("hhx_sort_graph_create: null or empty edge list");
    u64 total = 0;
    for (i64 e = 0; e < n_edges; ++e) {
        if (ei[e] < 0 || ei[e] >= shape || ej[e] < 0 || ej[e] >= shape || ei[e] == ej[e])
            return fail("hhx_sort_graph_create: edge %lld (%d, %d) outside shape %d", (long long)e, ei[e], ej[e], shape);
        if (w[e] < 0 || w[e] > (i64)1 << 53) return fail("hhx_sort_graph_create: weight %lld of edge %lld is not a count", (long long)w[e], (long long)e);
        total += (u64)w[e];
        if (total > 1ull << 62) return fail("hhx_sort_graph_create: the weights sum past 2^62");
    }
    hhx_sort_graph *g = new hhx_sort_graph;
    auto build = [&]() -> int {
        g->shape0 = g->shape = shape;
        g->ld = shape;
        g->n0 = g->nc = n_edges;
        g->total_w = total;
        const size_t cells = (size_t)shape * shape;
        HHX_TRY(sg_upload(g->e_a, ei, (size_t)n_edges));
        HHX_TRY(sg_upload(g->e_b, ej, (size_t)n_edges));
        HHX_TRY(sg_upload(g->e_w, w, (size_t)n_edges));
        if (g->S.alloc(cells) || g->D.alloc(cells) || g->C.alloc(cells + 1) || g->acc.alloc(cells) || g->top.alloc(3 * (size_t)shape) ||
            g->map.alloc(shape) || g->rowcnt.alloc(shape) || g->rowptr.alloc((size_t)shape + 1) || g->pairs.alloc(shape) || g->len.alloc(shape) ||
            g->dead.alloc(shape) || g->counter.alloc(1) || g->maxbits.alloc(1))
            return 1;
        HHX_HIP(hipMemsetAsync(g->S.p, 0, cells * sizeof(float), g_stream));
        HHX_HIP(hipMemsetAsync(g->dead.p, 0, shape, g_stream));
        {
            KTimer kt("sort_matrix");
            k_sg_scatter<<<sg_grid(n_edges, SG_T * 4), SG_T, 0, g_stream>>>(g->e_a.p, g->e_b.p, g->e_w.p, n_edges, g->S.p, g->ld);
            HHX_LAUNCH_CHECK();
        }
        HHX_HIP(hipStreamSynchronize(g_stream));          // the host arrays are the caller's
        return 0;
    };
    if (build()) { delete g; return 1; }
    *out = g;
    return 0;
}

extern "C" int hhx_sort_graph_shape(const hhx_sort_graph *g, int32_t *shape, int64_t *ld, int64_t *n_edges) {
    if (!g) return fail("hhx_sort_graph_shape: null handle");
    if (shape) *shape = g->shape;
    if (ld) *ld = g->ld;
    if (n_edges) *n_edges = g->nc;
    return 0;
}

extern "C" int hhx_sort_graph_density(hhx_sort_graph *g, const double *len, int method, int64_t *n_flagged) {
    if (!g || !len) return fail("hhx_sort_graph_density: null handle or lengths");
    if (method < 0 || method > 2) return fail("hhx_sort_graph_density: method %d (0 sum, 1 multiplication, 2 geometric_mean)", method);
    const i32 n = g->shape;
    for (i32 k = 0; k < n; ++k)
        if (!(len[k] > 0.0) || len[k] > 1e300) return fail("hhx_sort_graph_density: length %g of index %d", len[k], k);
    HHX_HIP(hipMemcpyAsync(g->len.p, len, (size_t)n * sizeof(double), hipMemcpyHostToDevice, g_stream));
    const i64 cap = std::min<i64>((i64)n * (n - 1) / 2, SG_LIST_CAP);
    g->n_flag = 0;
    if (method == 2) {
        if (g->flag.n < (size_t)(2 * cap) && g->flag.alloc((size_t)(2 * cap))) return 1;
        HHX_HIP(hipMemsetAsync(g->counter.p, 0, sizeof(i64), g_stream));
    }
    const dim3 grid((unsigned)((n + SG_T - 1) / SG_T), (unsigned)std::min<i32>(n, 1024));
    {
        KTimer kt("sort_density");
        if (method == 0) k_sg_density<0><<<grid, SG_T, 0, g_stream>>>(g->S.p, g->D.p, g->ld, n, g->len.p, nullptr, nullptr, 0);
        else if (method == 1) k_sg_density<1><<<grid, SG_T, 0, g_stream>>>(g->S.p, g->D.p, g->ld, n, g->len.p, nullptr, nullptr, 0);
        else k_sg_density<2><<<grid, SG_T, 0, g_stream>>>(g->S.p, g->D.p, g->ld, n, g->len.p, g->flag.p, g->counter.p, cap);
        HHX_LAUNCH_CHECK();
    }
    if (method == 2) HHX_HIP(hipMemcpyAsync(&g->n_flag, g->counter.p, sizeof(i64), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));              // `len` is the caller's
    if (g->n_flag > cap) return fail("hhx_sort_graph_density: %lld geometric-mean pairs sit on a float32 rounding boundary (at most %lld are reported)",
                                     (long long)g->n_flag, (long long)cap);
    g->stats[3] = g->n_flag;
    if (n_flagged) *n_flagged = g->n_flag;
    return 0;
}

extern "C" int hhx_sort_graph_fetch_flagged(hhx_sort_graph *g, int32_t *pairs) {
    if (!g || !pairs) return fail("hhx_sort_graph_fetch_flagged: null handle or output");
    if (g->n_flag) HHX_HIP(hipMemcpyAsync(pairs, g->flag.p, (size_t)g->n_flag * 2 * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_patch_len(hhx_sort_graph *g, int64_t n, const int32_t *pi, const int32_t *pj, const float *L) {
    if (!g) return fail("hhx_sort_graph_patch_len: null handle");
    if (n <= 0) return 0;
    if (!pi || !pj || !L) return fail("hhx_sort_graph_patch_len: null arrays");
    for (i64 k = 0; k < n; ++k)
        if (pi[k] < 0 || pi[k] >= g->shape || pj[k] < 0 || pj[k] >= g->shape || pi[k] == pj[k] || !(L[k] > 0.0f))
            return fail("hhx_sort_graph_patch_len: pair %lld (%d, %d) outside shape %d, or a length that is not positive", (long long)k, pi[k], pj[k], g->shape);
    DevBuf<i32> di, dj;
    DevBuf<float> dl;
    HHX_TRY(sg_upload(di, pi, (size_t)n));
    HHX_TRY(sg_upload(dj, pj, (size_t)n));
    HHX_TRY(sg_upload(dl, L, (size_t)n));
    k_sg_patch_len<<<(unsigned)((n + SG_T - 1) / SG_T), SG_T, 0, g_stream>>>(n, di.p, dj.p, dl.p, g->S.p, g->D.p, g->ld);
    HHX_LAUNCH_CHECK();
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

// the launches of both confidence entries: C and, behind it, MAXS are on the device when this returns (nothing waited for)
static int sg_confidence_launch(hhx_sort_graph *g, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, const char *who) {
    const i32 n = g->shape;
    if (n_pairs < 0 || 2 * (i64)n_pairs > n || (n_pairs && (!pair_a || !pair_b))) return fail("%s: %d sister pairs for shape %d", who, n_pairs, n);
    for (i32 k = 0; k < n_pairs; ++k)
        if (pair_a[k] < 0 || pair_a[k] >= n || pair_b[k] < 0 || pair_b[k] >= n || pair_a[k] == pair_b[k])
            return fail("%s: sister pair %d (%d, %d) outside shape %d", who, k, pair_a[k], pair_b[k], n);
    const size_t cells = (size_t)n * n;
    g->have_conf = false;
    g->have_forest = false;
    if (n_pairs) {
        HHX_HIP(hipMemcpyAsync(g->pairs.p, pair_a, (size_t)n_pairs * sizeof(i32), hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(g->pairs.p + n_pairs, pair_b, (size_t)n_pairs * sizeof(i32), hipMemcpyHostToDevice, g_stream));
    }
    HHX_HIP(hipMemsetAsync(g->C.p, 0, (cells + 1) * sizeof(double), g_stream));
    HHX_HIP(hipMemsetAsync(g->maxbits.p, 0, sizeof(u32), g_stream));
    {
        KTimer kt("sort_confidence", 3);
        k_sg_top3<<<sg_grid(n, SG_WAVES), SG_T, 0, g_stream>>>(g->D.p, g->ld, n, g->top.p);
        HHX_LAUNCH_CHECK();
        const i32 *ci = g->own_list ? g->c_i.p : g->e_a.p, *cj = g->own_list ? g->c_j.p : g->e_b.p;
        if (g->nc) {
            k_sg_conf<<<sg_grid(g->nc, SG_T), SG_T, 0, g_stream>>>(ci, cj, g->nc, g->dead.p, g->D.p, g->ld, n, g->top.p, g->C.p, g->maxbits.p);
            HHX_LAUNCH_CHECK();
        }
        k_sg_sister<<<(unsigned)(std::max(n_pairs, 1) + SG_T - 1) / SG_T, SG_T, 0, g_stream>>>(g->pairs.p, g->pairs.p + n_pairs, n_pairs, g->maxbits.p, g->C.p, n);
        HHX_LAUNCH_CHECK();
    }
    g->n_pairs = n_pairs;
    g->have_conf = true;
    return 0;
}

static int sg_copy_confidence(hhx_sort_graph *g, double *out, size_t count) {
    {
        KTimer kt("sort_confidence_copy");
        HHX_HIP(hipMemcpyAsync(out, g->C.p, count * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    }
    HHX_HIP(hipStreamSynchronize(g_stream));
    g->fstats[4] += 1;
    return 0;
}

extern "C" int hhx_sort_graph_confidence(hhx_sort_graph *g, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double *out) {
    if (!g || !out) return fail("hhx_sort_graph_confidence: null handle or output");
    HHX_TRY(sg_confidence_launch(g, n_pairs, pair_a, pair_b, "hhx_sort_graph_confidence"));
    return sg_copy_confidence(g, out, (size_t)g->shape * g->shape + 1);
}

extern "C" int hhx_sort_graph_confidence_device(hhx_sort_graph *g, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double *maxs) {
    if (!g || !maxs) return fail("hhx_sort_graph_confidence_device: null handle or output");
    HHX_TRY(sg_confidence_launch(g, n_pairs, pair_a, pair_b, "hhx_sort_graph_confidence_device"));
    HHX_HIP(hipMemcpyAsync(maxs, g->C.p + (size_t)g->shape * g->shape, sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));              // the pair arrays are the caller's
    return 0;
}

extern "C" int hhx_sort_graph_fetch_confidence(hhx_sort_graph *g, double *out) {
    if (!g || !out) return fail("hhx_sort_graph_fetch_confidence: null handle or output");
    if (!g->have_conf) return fail("hhx_sort_graph_fetch_confidence: no confidence graph computed at the current shape");
    return sg_copy_confidence(g, out, (size_t)g->shape * g->shape);
}

extern "C" int hhx_sort_graph_drop(hhx_sort_graph *g, int32_t a, int32_t b) {
    if (!g) return fail("hhx_sort_graph_drop: null handle");
    const i32 n = g->shape;
    if (n < 6) return fail("hhx_sort_graph_drop: shape %d has no path to spare", n);
    if (!((a == n - 1 && b == n - 2) || (a == n - 2 && b == n - 1)))
        return fail("hhx_sort_graph_drop: (%d, %d) are not the last two indices of shape %d", a, b, n);
    HHX_HIP(hipMemsetAsync(g->dead.p + (n - 2), 1, 2, g_stream));
    g->shape = n - 2;
    g->have_conf = g->have_forest = false;                // C was laid out for the old shape
    return 0;
}

// ------------------------------------------------------------------ spanning forest
static int sf_forest_hbm(hhx_sort_graph *g, const SfEdges &E, double cutoff, int jump_rounds, i64 *res_host) {
    const i32 n = g->shape;
    const i64 n_cand = E.nc + E.np;
    DevBuf<u64> raw, keys;
    DevBuf<i32> node, flags;
    DevBuf<u32> count;
    if (raw.alloc((size_t)n_cand) || node.alloc(16 * (size_t)n) || flags.alloc(SF_MAX_ROUNDS + 1) || count.alloc(1)) return 1;
    i32 *comp = node.p, *parent = node.p + 2 * (i64)n, *root = node.p + 3 * (i64)n, *deg = node.p + 4 * (i64)n, *minv = node.p + 5 * (i64)n;
    u32 *best = (u32 *)(node.p + n);
    i32 *nb = node.p + 6 * (i64)n, *T0 = node.p + 8 * (i64)n, *D0 = node.p + 10 * (i64)n, *T1 = node.p + 12 * (i64)n, *D1 = node.p + 14 * (i64)n;
    HHX_HIP(hipMemsetAsync(count.p, 0, sizeof(u32), g_stream));
    HHX_HIP(hipMemsetAsync(flags.p, 0, (SF_MAX_ROUNDS + 1) * sizeof(i32), g_stream));
    const unsigned gn = sg_grid(n, SG_T), gc = sg_grid(n_cand, SG_T);
    u32 ne = 0;
    {
        KTimer kt("sort_forest_edges", 3);
        k_sf_filter<<<gc, SG_T, 0, g_stream>>>(E, g->C.p, n, cutoff);
        HHX_LAUNCH_CHECK();
        k_sf_collect<<<gc, SG_T, 0, g_stream>>>(E, g->C.p, n, raw.p, (u32)n_cand, count.p);
        HHX_LAUNCH_CHECK();
        k_sf_init<<<gn, SG_T, 0, g_stream>>>(n, comp, best, deg, minv, nb);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(&ne, count.p, sizeof(u32), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if ((i64)ne > n_cand) return fail("hhx_sort_graph_forest: %u edges out of %lld candidates", ne, (long long)n_cand);
    DevBuf<i32> chosen, at;
    if (keys.alloc(ne) || chosen.alloc(ne) || at.alloc((size_t)ne + 1)) return 1;
    HHX_TRY(stable_sort_pairs_u64(raw.p, keys.p, nullptr, nullptr, ne, 64));
    if (ne) HHX_HIP(hipMemsetAsync(chosen.p, 0, (size_t)ne * sizeof(i32), g_stream));
    const unsigned ge = sg_grid(ne, SG_T);
    int rounds = 0;
    for (; ne && rounds < SF_MAX_ROUNDS; ++rounds) {
        i32 any = 0;
        KTimer kt("sort_forest_round", 4);
        k_sf_best<<<ge, SG_T, 0, g_stream>>>(keys.p, ne, n, comp, best, flags.p + rounds);
        HHX_LAUNCH_CHECK();
        k_sf_hook<<<gn, SG_T, 0, g_stream>>>(n, keys.p, comp, best, parent, chosen.p);      // a round without an outgoing edge changes nothing
        HHX_LAUNCH_CHECK();
        k_sf_root<<<gn, SG_T, 0, g_stream>>>(n, comp, parent, root);
        HHX_LAUNCH_CHECK();
        k_sf_relabel<<<gn, SG_T, 0, g_stream>>>(n, comp, root, best);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(&any, flags.p + rounds, sizeof(i32), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        if (!any) break;
    }
    i32 *not_paths = flags.p + SF_MAX_ROUNDS;
    i64 total = 0;
    {
        KTimer kt("sort_forest_emit", 3);
        k_sf_degree<<<std::max(ge, gn), SG_T, 0, g_stream>>>(keys.p, ne, n, chosen.p, deg, nb, comp, minv);
        HHX_LAUNCH_CHECK();
        k_sf_label_out<<<gn, SG_T, 0, g_stream>>>(n, comp, minv, deg, g->f_label.p, not_paths);
        HHX_LAUNCH_CHECK();
        if (ne) {
            HHX_TRY(exclusive_scan_i32(chosen.p, at.p, ne, &total));               // synchronises
            k_sf_emit<<<ge, SG_T, 0, g_stream>>>(keys.p, ne, n, chosen.p, at.p, g->f_eu.p, g->f_ev.p);
            HHX_LAUNCH_CHECK();
        }
    }
    i32 np_host = 0;
    HHX_HIP(hipMemcpyAsync(&np_host, not_paths, sizeof(i32), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (total >= n) return fail("hhx_sort_graph_forest: %lld edges chosen among %d nodes", (long long)total, n);
    {
        KTimer kt("sort_forest_jump", jump_rounds + 2);
        const unsigned g2 = sg_grid(2 * (i64)n, SG_T);
        if (!np_host) {
            k_sf_jump_init<<<g2, SG_T, 0, g_stream>>>(n, nb, T0, D0);
            HHX_LAUNCH_CHECK();
            for (int k = 0; k < jump_rounds; ++k) {
                if (k & 1) k_sf_jump<<<g2, SG_T, 0, g_stream>>>(n, T1, D1, T0, D0);
                else k_sf_jump<<<g2, SG_T, 0, g_stream>>>(n, T0, D0, T1, D1);
                HHX_LAUNCH_CHECK();
            }
        }
        k_sf_pos<<<gn, SG_T, 0, g_stream>>>(n, (jump_rounds & 1) ? T1 : T0, (jump_rounds & 1) ? D1 : D0, !np_host, g->f_pos.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipStreamSynchronize(g_stream));              // the scratch arrays go back to the pool
    res_host[0] = 0; res_host[1] = total; res_host[2] = np_host; res_host[3] = rounds;
    return 0;
}

extern "C" int hhx_sort_graph_forest(hhx_sort_graph *g, double cutoff, int64_t *n_chosen, int32_t *not_paths) {
    if (!g) return fail("hhx_sort_graph_forest: null handle");
    if (!(cutoff == cutoff)) return fail("hhx_sort_graph_forest: the cutoff is not a number");
    if (!g->have_conf) return fail("hhx_sort_graph_forest: no confidence graph computed at the current shape");
    const i32 n = g->shape;
    if (n > SF_MAX_SHAPE) return fail("hhx_sort_graph_forest: shape %d (at most %d)", n, SF_MAX_SHAPE);
    if (g->nc + g->n_pairs >= (i64)1 << 31) return fail("hhx_sort_graph_forest: %lld candidate edges", (long long)(g->nc + g->n_pairs));
    g->have_forest = false;
    if (g->f_res.n < 4 && (g->f_eu.alloc(g->shape0) || g->f_ev.alloc(g->shape0) || g->f_label.alloc(g->shape0) || g->f_pos.alloc(g->shape0) || g->f_res.alloc(4)))
        return 1;
    const SfEdges E = {g->own_list ? g->c_i.p : g->e_a.p, g->own_list ? g->c_j.p : g->e_b.p, g->nc, g->dead.p, g->pairs.p, g->pairs.p + g->n_pairs, g->n_pairs};
    int jump_rounds = 0;                                   // doubling covers a path of n nodes after ceil(log2(n)) rounds
    while ((1 << jump_rounds) < n) ++jump_rounds;
    const i64 lds_shape = std::max<i64>(0, std::min<i64>(tune_get("sort_forest_lds", SF_LDS_SHAPE), SF_LDS_SHAPE));
    i64 res[4] = {1, 0, 0, 0};
    if (n <= lds_shape) {                                  // the seam (head of this file)
        u32 cap = 1;
        while (12 * (i64)(2 * cap) + 48 * (i64)n + SF_LDS_STATIC <= SF_LDS_BYTES) cap *= 2;
        HHX_TRY((raise_dynamic_lds<k_sf_lds>(SF_LDS_BYTES - SF_LDS_STATIC)));
        HHX_HIP(hipMemsetAsync(g->f_res.p, 0, 4 * sizeof(i64), g_stream));
        {
            KTimer kt("sort_forest_lds");
            k_sf_lds<<<1, SF_T, 12 * (size_t)cap + 48 * (size_t)n, g_stream>>>(E, g->C.p, n, cutoff, cap, jump_rounds, g->f_eu.p, g->f_ev.p, g->f_label.p,
                                                                            g->f_pos.p, g->f_res.p);
            HHX_LAUNCH_CHECK();
        }
        HHX_HIP(hipMemcpyAsync(res, g->f_res.p, 4 * sizeof(i64), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
    }
    const bool lds = res[0] == 0;
    if (!lds) HHX_TRY(sf_forest_hbm(g, E, cutoff, jump_rounds, res));
    g->fstats[lds ? 0 : 1] += 1;
    g->fstats[2] = res[3];
    g->fstats[3] = res[2] ? 0 : jump_rounds;
    g->f_shape = n;
    g->f_chosen = res[1];
    g->f_not_paths = (i32)res[2];
    g->have_forest = true;
    if (n_chosen) *n_chosen = g->f_chosen;
    if (not_paths) *not_paths = g->f_not_paths;
    return 0;
}

extern "C" int hhx_sort_graph_fetch_forest(hhx_sort_graph *g, int32_t *eu, int32_t *ev, int32_t *label, int32_t *pos) {
    if (!g || !label || !pos) return fail("hhx_sort_graph_fetch_forest: null handle or output");
    if (!g->have_forest) return fail("hhx_sort_graph_fetch_forest: no forest computed at the current shape");
    if (g->f_chosen && (!eu || !ev)) return fail("hhx_sort_graph_fetch_forest: null output");
    if (g->f_chosen) {
        HHX_HIP(hipMemcpyAsync(eu, g->f_eu.p, (size_t)g->f_chosen * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(ev, g->f_ev.p, (size_t)g->f_chosen * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
    }
    HHX_HIP(hipMemcpyAsync(label, g->f_label.p, (size_t)g->f_shape * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(pos, g->f_pos.p, (size_t)g->f_shape * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_forest_stats(const hhx_sort_graph *g, int64_t *values) {
    if (!g || !values) return fail("hhx_sort_graph_forest_stats: null handle or output");
    for (int k = 0; k < SF_N_STATS; ++k) values[k] = g->fstats[k];
    return 0;
}

extern "C" int hhx_sort_graph_aggregate(hhx_sort_graph *g, int32_t new_shape, const int32_t *map, int64_t *n_edges, int64_t *n_over) {
    if (!g || !map) return fail("hhx_sort_graph_aggregate: null handle or map");
    const i32 ns = new_shape;
    if (ns < 2 || (ns & 1) || ns > g->shape0) return fail("hhx_sort_graph_aggregate: new shape %d (even, 2 .. %d)", ns, g->shape0);
    for (i32 k = 0; k < g->shape0; ++k)
        if (map[k] < -1 || map[k] >= ns) return fail("hhx_sort_graph_aggregate: map[%d] = %d outside [-1, %d)", k, map[k], ns);
    const size_t cells = (size_t)ns * ns;
    HHX_HIP(hipMemcpyAsync(g->map.p, map, (size_t)g->shape0 * sizeof(i32), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemsetAsync(g->acc.p, 0, cells * sizeof(u64), g_stream));
    HHX_HIP(hipMemsetAsync(g->counter.p, 0, sizeof(i64), g_stream));
    const i64 lds_shape = std::max<i64>(0, std::min<i64>(tune_get("sort_lds_shape", SG_LDS_SHAPE), SG_LDS_SHAPE));
    const bool lds = ns <= lds_shape && g->total_w < (1ull << 32);        // the seam (head of this file)
    {
        KTimer kt("sort_aggregate");
        if (lds) {
            HHX_TRY((raise_dynamic_lds<k_sg_agg_lds>(SG_LDS_SHAPE * SG_LDS_SHAPE * (int)sizeof(u32))));
            const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>((g->n0 + SG_T * 16 - 1) / (SG_T * 16), 256));
            k_sg_agg_lds<<<grid, SG_T, cells * sizeof(u32), g_stream>>>(g->e_a.p, g->e_b.p, g->e_w.p, g->n0, g->map.p, ns, g->acc.p);
        } else {
            k_sg_agg_global<<<sg_grid(g->n0, SG_T * 4), SG_T, 0, g_stream>>>(g->e_a.p, g->e_b.p, g->e_w.p, g->n0, g->map.p, ns, g->acc.p);
        }
        HHX_LAUNCH_CHECK();
    }
    g->stats[lds ? 0 : 1] += 1;
    const i64 cap = std::min<i64>((i64)ns * (ns - 1) / 2, SG_LIST_CAP);
    if (g->over.n < (size_t)cap && g->over.alloc((size_t)cap)) return 1;
    i64 total = 0;
    {
        KTimer kt("sort_emit", 3);
        k_sg_rowcount<<<sg_grid(ns, SG_WAVES), SG_T, 0, g_stream>>>(g->acc.p, ns, g->rowcnt.p, g->over.p, g->counter.p, cap);
        HHX_LAUNCH_CHECK();
        HHX_TRY(exclusive_scan_i32(g->rowcnt.p, g->rowptr.p, ns, &total));       // synchronises
        if (g->c_i.alloc((size_t)total) || g->c_j.alloc((size_t)total) || g->c_w.alloc((size_t)total)) return 1;
        k_sg_emit_edges<<<sg_grid(ns, SG_WAVES), SG_T, 0, g_stream>>>(g->acc.p, ns, g->rowptr.p, g->c_i.p, g->c_j.p, g->c_w.p);
        HHX_LAUNCH_CHECK();
        const dim3 grid((unsigned)((ns + SG_T - 1) / SG_T), (unsigned)std::min<i32>(ns, 1024));
        k_sg_emit_dense<<<grid, SG_T, 0, g_stream>>>(g->acc.p, ns, g->S.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemsetAsync(g->dead.p, 0, g->shape0, g_stream));
    HHX_HIP(hipMemcpyAsync(&g->n_over, g->counter.p, sizeof(i64), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    g->shape = ns;
    g->ld = ns;
    g->nc = total;
    g->own_list = true;
    g->have_conf = g->have_forest = false;
    g->stats[2] = g->n_over;
    if (g->n_over > cap) return fail("hhx_sort_graph_aggregate: %lld cells sum past 2^24 (at most %lld are reported)", (long long)g->n_over, (long long)cap);
    if (n_edges) *n_edges = total;
    if (n_over) *n_over = g->n_over;
    return 0;
}

extern "C" int hhx_sort_graph_fetch_edges(hhx_sort_graph *g, int32_t *ei, int32_t *ej, float *w) {
    if (!g) return fail("hhx_sort_graph_fetch_edges: null handle");
    if (!g->own_list) return fail("hhx_sort_graph_fetch_edges: no re-aggregation yet (the round-1 edges are the caller's)");
    if (g->nc && (!ei || !ej || !w)) return fail("hhx_sort_graph_fetch_edges: null output");
    if (g->nc) {
        HHX_HIP(hipMemcpyAsync(ei, g->c_i.p, (size_t)g->nc * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(ej, g->c_j.p, (size_t)g->nc * sizeof(i32), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(w, g->c_w.p, (size_t)g->nc * sizeof(float), hipMemcpyDeviceToHost, g_stream));
    }
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_fetch_over(hhx_sort_graph *g, int64_t *cells) {
    if (!g || !cells) return fail("hhx_sort_graph_fetch_over: null handle or output");
    if (g->n_over) HHX_HIP(hipMemcpyAsync(cells, g->over.p, (size_t)g->n_over * sizeof(i64), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_patch_cells(hhx_sort_graph *g, int64_t n, const int64_t *cells, const int64_t *ordinal, const float *val) {
    if (!g) return fail("hhx_sort_graph_patch_cells: null handle");
    if (n <= 0) return 0;
    if (!cells || !ordinal || !val || !g->own_list) return fail("hhx_sort_graph_patch_cells: null arrays, or no re-aggregation yet");
    const i64 ns = g->shape;
    if (g->ld != ns) return fail("hhx_sort_graph_patch_cells: the matrix has been cut since its re-aggregation");
    for (i64 k = 0; k < n; ++k)
        if (cells[k] < 0 || cells[k] >= ns * ns || cells[k] / ns <= cells[k] % ns || ordinal[k] < 0 || ordinal[k] >= g->nc)
            return fail("hhx_sort_graph_patch_cells: cell %lld / edge %lld outside the lower triangle of shape %lld / the %lld edges", (long long)cells[k],
                        (long long)ordinal[k], (long long)ns, (long long)g->nc);
    DevBuf<i64> dc, dord;
    DevBuf<float> dv;
    HHX_TRY(sg_upload(dc, cells, (size_t)n));
    HHX_TRY(sg_upload(dord, ordinal, (size_t)n));
    HHX_TRY(sg_upload(dv, val, (size_t)n));
    k_sg_patch_cells<<<(unsigned)((n + SG_T - 1) / SG_T), SG_T, 0, g_stream>>>(n, dc.p, dord.p, dv.p, (i32)ns, g->S.p, g->c_w.p);
    HHX_LAUNCH_CHECK();
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

// the leading shape x shape block of the link matrix (which 0) or the density graph (which 1), for the tests and the bench
extern "C" int hhx_sort_graph_fetch_dense(hhx_sort_graph *g, int which, float *out) {
    if (!g || !out) return fail("hhx_sort_graph_fetch_dense: null handle or output");
    if (which != 0 && which != 1) return fail("hhx_sort_graph_fetch_dense: which = %d (0 link matrix, 1 density graph)", which);
    const size_t row = (size_t)g->shape * sizeof(float);
    HHX_HIP(hipMemcpy2DAsync(out, row, which ? g->D.p : g->S.p, (size_t)g->ld * sizeof(float), row, (size_t)g->shape, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_stats(const hhx_sort_graph *g, int64_t *values) {
    if (!g || !values) return fail("hhx_sort_graph_stats: null handle or output");
    for (int k = 0; k < HHX_SORT_GRAPH_N_STATS; ++k) values[k] = g->stats[k];
    return 0;
}

extern "C" int hhx_sort_graph_destroy(hhx_sort_graph *g) {
    delete g;
    return 0;
}
