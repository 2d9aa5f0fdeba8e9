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
#include <algorithm>

#include "hhx_common.h"

using namespace hhx;

namespace {
constexpr int SG_T = 256;
constexpr int SG_WAVES = SG_T / HHX_WAVE;
constexpr int SG_LDS_SHAPE = 192;
constexpr i64 SG_LIST_CAP = 1 << 20;            // flagged geometric-mean pairs / cells above 2^24 a call can report
constexpr u64 SG_EXACT = 1ull << 24;            // float32 sums of non-negative integers are exact up to here
}  // namespace

struct hhx_sort_graph {
    i32 shape0 = 0, shape = 0;                  // round-1 shape; the current one (the leading block of S / D)
    i64 ld = 0;                                 // row pitch of S and D: the shape they were built at (remove_shortest_path keeps it)
    i64 n0 = 0, nc = 0;                         // round-1 edges; edges of the current list (dropped ones included: `dead` hides them)
    u64 total_w = 0;
    bool own_list = false;                      // the current list is c_i / c_j (after a re-aggregation), else the round-1 edges
    i64 n_flag = 0, n_over = 0;
    i64 stats[HHX_SORT_GRAPH_N_STATS] = {0, 0, 0, 0};
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

extern "C" int hhx_sort_graph_confidence(hhx_sort_graph *g, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double *out) {
    if (!g || !out) return fail("hhx_sort_graph_confidence: null handle or output");
    const i32 n = g->shape;
    if (n_pairs < 0 || 2 * (i64)n_pairs > n || (n_pairs && (!pair_a || !pair_b))) return fail("hhx_sort_graph_confidence: %d sister pairs for shape %d", n_pairs, n);
    for (i32 k = 0; k < n_pairs; ++k)
        if (pair_a[k] < 0 || pair_a[k] >= n || pair_b[k] < 0 || pair_b[k] >= n || pair_a[k] == pair_b[k])
            return fail("hhx_sort_graph_confidence: sister pair %d (%d, %d) outside shape %d", k, pair_a[k], pair_b[k], n);
    const size_t cells = (size_t)n * n;
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
    {
        KTimer kt("sort_confidence_copy");
        HHX_HIP(hipMemcpyAsync(out, g->C.p, (cells + 1) * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    }
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_sort_graph_drop(hhx_sort_graph *g, int32_t a, int32_t b) {
    if (!g) return fail("hhx_sort_graph_drop: null handle");
    const i32 n = g->shape;
    if (n < 6) return fail("hhx_sort_graph_drop: shape %d has no path to spare", n);
    if (!((a == n - 1 && b == n - 2) || (a == n - 2 && b == n - 1)))
        return fail("hhx_sort_graph_drop: (%d, %d) are not the last two indices of shape %d", a, b, n);
    HHX_HIP(hipMemsetAsync(g->dead.p + (n - 2), 1, 2, g_stream));
    g->shape = n - 2;
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
