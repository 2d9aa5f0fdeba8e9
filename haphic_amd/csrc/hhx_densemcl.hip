// --dense_matrix Markov clustering on the device: the reference's numpy code path of scripts/HapHiC_cluster.py
//   run_mcl_clustering :2144-2149   normalize(link_matrix, 'l1', axis=0), numpy.linalg.matrix_power(matrix, expansion)
//   mcl                :2026-2062   matrix_power (:2035), power + normalize (:2040), prune (:2042), allclose (:2051)
//   prune              :1999-2014   dense branch: copy, zero the entries < pruning, restore the first column maximum, normalize
//   interpret_result   :2065-2095   dense branch (:2080): served by hhx_dmat_to_csr + hhx_interpret
//
// State.  M (n x n float32, column-stochastic) is kept as T = M^T, row-major: (X @ Y)^T = Y^T X^T, so every product of the reference is
// one product of the same kind on T, and the column sums / column maxima of the reference are row operations here.  The handle
// (hhx_dmat) holds an ld x ld block with ld = n rounded up to 128.
//
// PADDING INVARIANT: every entry of the block outside [0, n) x [0, n) is ZERO, always.  The GEMM reads and writes whole 128 x 128
// tiles without a bounds check or a store mask: a padded row of A or a padded column of B is zero, so the padded part of the
// product is zero again and the invariant carries over.  The row kernels (epilogue, allclose, from_csr / to_csr) touch the entries
// [0, n) x [0, n) alone; the copies move the whole block; the uploads clear the block before they fill it.
//
// Arithmetic.  One accumulator per output element, k ascending over the whole K loop, no split-K: v_mfma_f32_32x32x2_f32 is an f32
// fmaf chain in k order, so the product has the same bits on every launch.  Sums of a row are float32 in one fixed order (per
// thread a strided chain, then a shuffle tree, then the four waves in order).
#include "hhx_common.h"
#include "hhx_internal.h"

#include <algorithm>
#include <climits>

using namespace hhx;

struct hhx_dmat {
    i32 n = 0;
    i64 ld = 0;                 // row pitch AND number of allocated rows: n rounded up to GEMM_T
    hhx::DevBuf<float> x;       // ld * ld floats, T = M^T row-major, zero outside n x n
};

namespace {

// ---------------------------------------------------------------------------------------------------------------- GEMM
// C = A * B on ld x ld blocks.  Workgroup: 256 threads = 2 x 2 waves on a 128 x 128 tile of C, K in steps of 32; wave: 2 x 2
// tiles of 32 x 32 (4 x 16 accumulator registers).  Two LDS buffers: the global loads of K-step t+1 are issued before the MFMAs of
// step t and written to the other buffer after them, one barrier per step.
// LDS images.  A 4-byte LDS access is served in two groups of 32 lanes (0-31, 32-63) on 32 banks, bank = dword address mod 32:
//   A tile [row i][k], row pitch 33: lane l reads A[i = l & 31][k = 2s + (l >> 5)] — the 32 lanes of a group read 32 rows of one k: banks
//   33 i + k = i + k mod 32, all different.  The staging writes it with 4-byte stores: a group of 32 lanes holds 4 rows x 8 float4, element j at
//   bank row + 4 q + j (row = 0..3, q = 0..7), all different too
//   B tile [k][column j], row pitch 128: lane l reads B[k = 2s + (l >> 5)][j = l & 31] — 32 consecutive dwords of one k row; staged with 16-byte stores
constexpr int GEMM_T = 128, GEMM_K = 32, A_PITCH = 33, B_PITCH = 128;
constexpr int A_TILE = GEMM_T * A_PITCH, B_TILE = GEMM_K * B_PITCH;          // floats
constexpr int GEMM_LDS_BYTES = 2 * (A_TILE + B_TILE) * (int)sizeof(float);   // 66560: two workgroups per CU
static_assert(A_TILE % 4 == 0, "the B tile behind the A tile stays 16-byte aligned");
constexpr int N_XCD = 8;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// two workgroups per CU (LDS) = two waves per SIMD: up to 256 registers each, so that the staged tile never spills into the K loop
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_dmcl_gemm(const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ C, i64 ld,
                                                   int tiles, int nwg) {
    extern __shared__ __align__(16) float lds[];
    // consecutive workgroup ids go round the 8 XCDs: give every XCD one contiguous run of tiles (neighbours share A rows in its L2);
    // bijective for any nwg
    const int bid = blockIdx.x, q = nwg / N_XCD, rem = nwg % N_XCD, xcd = bid % N_XCD, idx = bid / N_XCD;
    const int swz = xcd < rem ? xcd * (q + 1) + idx : rem * (q + 1) + (xcd - rem) * q + idx;
    const i64 m0 = (i64)(swz / tiles) * GEMM_T, n0 = (i64)(swz % tiles) * GEMM_T;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
    // staging: 4 float4 of A (row = idx >> 3, k = 4 (idx & 7)) and 4 float4 of B (k = idx >> 5, column = 4 (idx & 31)) per thread
    const float *ga = A + (size_t)(m0 + (t >> 3)) * (size_t)ld + 4 * (t & 7);
    const float *gb = B + (size_t)(t >> 5) * (size_t)ld + n0 + 4 * (t & 31);
    const size_t a_step = (size_t)32 * (size_t)ld, b_step = (size_t)8 * (size_t)ld;       // 256 threads further: 32 rows of A, 8 k rows of B
    const int sa = (t >> 3) * A_PITCH + 4 * (t & 7), sb = (t >> 5) * B_PITCH + 4 * (t & 31);
    float4 ra[4], rb[4];
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int nk = (int)(ld / GEMM_K);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        ra[p] = *reinterpret_cast<const float4 *>(ga + p * a_step);
        rb[p] = *reinterpret_cast<const float4 *>(gb + p * b_step);
    }
    {
        float *as = lds, *bs = lds + A_TILE;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float *wa = as + sa + p * 32 * A_PITCH;
            wa[0] = ra[p].x; wa[1] = ra[p].y; wa[2] = ra[p].z; wa[3] = ra[p].w;
            *reinterpret_cast<float4 *>(bs + sb + p * 8 * B_PITCH) = rb[p];
        }
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const float *as = lds + (kt & 1) * (A_TILE + B_TILE), *bs = as + A_TILE;
        // the last step stages its own tile once more (into the buffer nobody reads again): no branch around the loads, so the staged
        // registers stay registers
        const int kn = kt + 1 < nk ? kt + 1 : kt;
        const float *na = ga + (size_t)kn * GEMM_K, *nb = gb + (size_t)kn * GEMM_K * (size_t)ld;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            ra[p] = *reinterpret_cast<const float4 *>(na + p * a_step);
            rb[p] = *reinterpret_cast<const float4 *>(nb + p * b_step);
        }
        const float *fa = as + (wm * 64 + r) * A_PITCH + h, *fb = bs + h * B_PITCH + wn * 64 + r;
#pragma unroll
        for (int s = 0; s < GEMM_K / 2; ++s) {                       // k = 2 s + h, ascending
            const float a0 = fa[2 * s], a1 = fa[32 * A_PITCH + 2 * s];
            const float b0 = fb[2 * s * B_PITCH], b1 = fb[2 * s * B_PITCH + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        float *was = lds + ((kt + 1) & 1) * (A_TILE + B_TILE), *wbs = was + A_TILE;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float *wa = was + sa + p * 32 * A_PITCH;
            wa[0] = ra[p].x; wa[1] = ra[p].y; wa[2] = ra[p].z; wa[3] = ra[p].w;
            *reinterpret_cast<float4 *>(wbs + sb + p * 8 * B_PITCH) = rb[p];
        }
        __syncthreads();
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  No mask: the padding invariant
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float *c = C + (size_t)(m0 + wm * 64 + i * 32 + 4 * h) * (size_t)ld + n0 + wn * 64 + j * 32 + r;
#pragma unroll
            for (int e = 0; e < 16; ++e) c[(size_t)((e & 3) + 8 * (e >> 2)) * (size_t)ld] = acc[i][j][e];
        }
}

// ---------------------------------------------------------------------------------------------------------------- row epilogue
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, HHX_WAVE);
    return __shfl(v, 0, HHX_WAVE);
}
constexpr int ROW_T = 256;
constexpr i32 ROW_LDS_MAX = 30720;          // floats of a row kept in LDS (120 KB); longer rows go through HBM (L2) between the passes

__device__ __forceinline__ float block_sum_f32(float v, float *red) {
    v = wave_sum_f32(v);
    if (lane_id() == 0) red[threadIdx.x / HHX_WAVE] = v;
    __syncthreads();
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// "inflate, normalise, prune, normalise" (:2040-2042 with :2003-2014) for one column of M = one row of T per workgroup, in place.
//   pass 1  v = power(x, inflation) (INFLATE), s1 = sum |v|
//   pass 2  q = v / s1 (NORM; s1 == 0: q = v), the maximum of q and its FIRST position (argmax(axis=0): lowest row index of M)
//   pass 3  p = q if q >= pruning or at the argmax, else 0; s2 = sum |p|
//   pass 4  x = p / s2 (s2 == 0: p)
// flags: 1 INFLATE, 2 NORM, 4 PRUNE.  mcl(): 7; the public prune(): 4; the pre-normalisation of the link matrix (:2144): 2.
// Every thread visits the same entries j = t, t + 256, ... in every pass, so the row needs no barrier of its own.
template <bool LDSROW>
__global__ __launch_bounds__(ROW_T) void k_dmcl_inflate_normalize_prune(i32 n, i64 ld, float *__restrict__ x, int flags, double r, int square, float thr) {
    extern __shared__ __align__(16) float rowbuf[];
    __shared__ float red[4];
    __shared__ float red_v[4];
    __shared__ i32 red_j[4];
    float *g = x + (size_t)blockIdx.x * (size_t)ld;
    const int t = threadIdx.x;
    const bool inflate = flags & 1, norm = flags & 2, prune = flags & 4;
    float s = 0.0f;
    if (norm || LDSROW || inflate)
        for (i32 j = t; j < n; j += ROW_T) {
            float v = g[j];
            if (inflate) v = square ? v * v : hhx_powr(v, r);
            if (LDSROW) rowbuf[j] = v;
            else if (inflate) g[j] = v;
            s += fabsf(v);
        }
    const float *row = LDSROW ? rowbuf : g;
    float s1 = 0.0f;
    if (norm) s1 = block_sum_f32(s, red);
    const bool scale1 = norm && s1 != 0.0f;
    if (!prune) {
        for (i32 j = t; j < n; j += ROW_T) g[j] = scale1 ? row[j] / s1 : row[j];
        return;
    }
    float best = -INFINITY;
    i32 best_j = INT_MAX;
    for (i32 j = t; j < n; j += ROW_T) {
        const float q = scale1 ? row[j] / s1 : row[j];
        if (q > best) { best = q; best_j = j; }                       // strict >: the lowest index of this thread
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_down(best, o, HHX_WAVE);
        const i32 oj = __shfl_down(best_j, o, HHX_WAVE);
        if (ob > best || (ob == best && oj < best_j)) { best = ob; best_j = oj; }
    }
    if (lane_id() == 0) { red_v[t / HHX_WAVE] = best; red_j[t / HHX_WAVE] = best_j; }
    __syncthreads();
    best = red_v[0];
    best_j = red_j[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (red_v[w] > best || (red_v[w] == best && red_j[w] < best_j)) { best = red_v[w]; best_j = red_j[w]; }
    float s2p = 0.0f;
    for (i32 j = t; j < n; j += ROW_T) {
        const float q = scale1 ? row[j] / s1 : row[j];
        if (q >= thr || j == best_j) s2p += fabsf(q);
    }
    const float s2 = block_sum_f32(s2p, red);
    for (i32 j = t; j < n; j += ROW_T) {
        const float q = scale1 ? row[j] / s1 : row[j];
        const float p = (q >= thr || j == best_j) ? q : 0.0f;
        g[j] = s2 != 0.0f ? p / s2 : p;
    }
}

// allclose(matrix, last_matrix) :2051 — |a - b| <= 1e-8 + 1e-5 |b| on every entry, evaluated in float32 as numpy does for float32
// arrays.  flag[0] is raised by the first entry that fails; a workgroup looks at the flag before every row and leaves when it is up.
__global__ __launch_bounds__(ROW_T) void k_dmcl_allclose(i32 n, i64 ld, const float *__restrict__ a, const float *__restrict__ b, unsigned int *flag) {
    const float rtol = (float)1e-5, atol = (float)1e-8;
    for (i32 row = blockIdx.x; row < n; row += gridDim.x) {
        if (*(volatile unsigned int *)flag) return;
        const float *pa = a + (size_t)row * (size_t)ld, *pb = b + (size_t)row * (size_t)ld;
        bool bad = false;
        for (i32 j = threadIdx.x; j < n; j += ROW_T) {
            const float u = pa[j], v = pb[j];
            const float tol = atol + rtol * fabsf(v);
            if (!(fabsf(u - v) <= tol)) bad = true;
        }
        if (__any(bad)) {
            if (lane_id() == 0) atomicExch(flag, 1u);
            return;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- CSR(T) <-> block
constexpr int CSR_WAVES = ROW_T / HHX_WAVE;
inline unsigned csr_grid(i32 n) { return (unsigned)std::max<i64>(1, std::min<i64>(((i64)n + CSR_WAVES - 1) / CSR_WAVES, 256 * 32)); }

// scatter: one wave per row of CSR(T) into the zeroed block
__global__ __launch_bounds__(ROW_T) void k_dmcl_from_csr(i32 n, const i32 *__restrict__ indptr, const i32 *__restrict__ indices, const float *__restrict__ data,
                                                         float *__restrict__ x, i64 ld) {
    const int lane = lane_id();
    for (i32 row = blockIdx.x * CSR_WAVES + threadIdx.x / HHX_WAVE; row < n; row += gridDim.x * CSR_WAVES) {
        float *g = x + (size_t)row * (size_t)ld;
        for (i32 p = indptr[row] + lane; p < indptr[row + 1]; p += HHX_WAVE) {
            const i32 c = indices[p];
            if (c >= 0 && c < n) g[c] = data[p];
        }
    }
}
// compaction: FILL = false counts the non-zero entries of every row, FILL = true writes them in column order behind the scanned counts
template <bool FILL>
__global__ __launch_bounds__(ROW_T) void k_dmcl_to_csr(i32 n, const float *__restrict__ x, i64 ld, i32 *__restrict__ cnt, const i32 *__restrict__ indptr,
                                                       i32 *__restrict__ indices, float *__restrict__ data) {
    const int lane = lane_id();
    for (i32 row = blockIdx.x * CSR_WAVES + threadIdx.x / HHX_WAVE; row < n; row += gridDim.x * CSR_WAVES) {
        const float *g = x + (size_t)row * (size_t)ld;
        i32 o = FILL ? indptr[row] : 0;
        for (i32 j0 = 0; j0 < n; j0 += HHX_WAVE) {
            const i32 j = j0 + lane;
            const float v = j < n ? g[j] : 0.0f;
            const bool k = v != 0.0f;
            const u64 mask = __ballot(k);
            if (FILL && k) {
                const i32 pos = o + __popcll(mask & ((1ull << lane) - 1ull));
                indices[pos] = j;
                data[pos] = v;
            }
            o += __popcll(mask);
        }
        if (!FILL && lane == 0) cnt[row] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
int dmat_alloc(i32 n, hhx_dmat **out) {
    if (n < 1) return fail("hhx_dmat: the matrix must have at least one row (got %d)", n);
    hhx_dmat *d = new hhx_dmat;
    d->n = n;
    d->ld = ((i64)n + GEMM_T - 1) / GEMM_T * GEMM_T;
    if (d->x.alloc((size_t)d->ld * (size_t)d->ld)) {
        const std::string why = g_err;
        const i64 ld = d->ld;
        delete d;
        return fail("hhx_dmat: a %lld x %lld float32 block (%lld bytes, n = %d) does not fit the device: %s", (long long)ld, (long long)ld,
                    (long long)(ld * ld * 4), n, why.c_str());
    }
    *out = d;
    return 0;
}
size_t dmat_bytes(const hhx_dmat *d) { return sizeof(float) * (size_t)d->ld * (size_t)d->ld; }

int dmat_gemm_into(const hhx_dmat *a, const hhx_dmat *b, hhx_dmat *c) {
    HHX_TRY((raise_dynamic_lds<k_dmcl_gemm>(GEMM_LDS_BYTES)));
    const i64 tiles = a->ld / GEMM_T;
    if (tiles * tiles > INT_MAX) return fail("hhx_dmat_gemm: n = %d is beyond the grid", a->n);
    KTimer kt("dmcl_gemm");
    k_dmcl_gemm<<<(unsigned)(tiles * tiles), 256, GEMM_LDS_BYTES, g_stream>>>(a->x.p, b->x.p, c->x.p, a->ld, (int)tiles, (int)(tiles * tiles));
    HHX_LAUNCH_CHECK();
    return 0;
}
int dmat_gemm(const hhx_dmat *a, const hhx_dmat *b, hhx_dmat **out) {
    hhx_dmat *c = nullptr;
    HHX_TRY(dmat_alloc(a->n, &c));
    const int rc = dmat_gemm_into(a, b, c);
    if (rc) { delete c; return rc; }
    *out = c;
    return 0;
}
int dmat_copy(const hhx_dmat *m, hhx_dmat **out) {
    hhx_dmat *c = nullptr;
    HHX_TRY(dmat_alloc(m->n, &c));
    const hipError_t e = hipMemcpyAsync(c->x.p, m->x.p, dmat_bytes(m), hipMemcpyDeviceToDevice, g_stream);
    if (e != hipSuccess) { delete c; return fail("hipMemcpyAsync failed: %s", hipGetErrorString(e)); }
    *out = c;
    return 0;
}
int dmat_epilogue(hhx_dmat *m, int flags, double inflation, double pruning) {
    const double r = (double)(float)inflation;
    const int square = inflation == 2.0;
    KTimer kt("dmcl_epilogue");
    if (m->n <= ROW_LDS_MAX) {
        const int bytes = (int)sizeof(float) * ROW_LDS_MAX;
        HHX_TRY((raise_dynamic_lds<k_dmcl_inflate_normalize_prune<true>>(bytes)));
        k_dmcl_inflate_normalize_prune<true><<<(unsigned)m->n, ROW_T, sizeof(float) * (size_t)m->n, g_stream>>>(m->n, m->ld, m->x.p, flags, r, square, (float)pruning);
    } else
        k_dmcl_inflate_normalize_prune<false><<<(unsigned)m->n, ROW_T, 0, g_stream>>>(m->n, m->ld, m->x.p, flags, r, square, (float)pruning);
    HHX_LAUNCH_CHECK();
    return 0;
}
// numpy.linalg.matrix_power(M, e) in its own association order, on T: fmatmul(X, Y) = X @ Y is gemm(Y^T, X^T)
int dmat_power(const hhx_dmat *t, int e, hhx_dmat **out) {
    if (e == 1) return dmat_copy(t, out);
    if (e == 2) return dmat_gemm(t, t, out);                         // M @ M
    if (e == 3) {                                                    // (M @ M) @ M
        hhx_dmat *sq = nullptr;
        HHX_TRY(dmat_gemm(t, t, &sq));
        const int rc = dmat_gemm(t, sq, out);
        delete sq;
        return rc;
    }
    // binary decomposition: z = M, M^2, M^4, ...; result = result @ z for every set bit, lowest first
    const hhx_dmat *z = nullptr, *result = nullptr;
    int rc = 0;
    auto drop = [&](const hhx_dmat *p) { if (p && p != t) delete const_cast<hhx_dmat *>(p); };
    while (e > 0 && !rc) {
        if (!z) z = t;
        else {
            hhx_dmat *z2 = nullptr;
            rc = dmat_gemm(z, z, &z2);                               // z @ z
            if (rc) break;
            if (z != result) drop(z);
            z = z2;
        }
        const int bit = e & 1;
        e >>= 1;
        if (bit) {
            if (!result) result = z;
            else {
                hhx_dmat *r2 = nullptr;
                rc = dmat_gemm(z, result, &r2);                      // result @ z
                if (rc) break;
                if (result != z) drop(result);
                result = r2;
            }
        }
    }
    if (rc) { if (z != result) drop(z); drop(result); return rc; }
    if (z != result) drop(z);
    if (result == t) return dmat_copy(t, out);
    *out = const_cast<hhx_dmat *>(result);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- C ABI
extern "C" int hhx_dmat_from_host(i32 n, const float *m, hhx_dmat **out) {
    if (!m || !out) return fail("null pointer");
    hhx_dmat *d = nullptr;
    HHX_TRY(dmat_alloc(n, &d));
    DevBuf<float> packed;                                            // M as the caller has it; the block takes its transpose
    int rc = packed.alloc((size_t)n * (size_t)n);
    if (rc) fail("hhx_dmat_from_host: the %d x %d staging copy does not fit the device: %s", n, n, std::string(g_err).c_str());
    auto hip = [&](hipError_t e, const char *what) { if (e != hipSuccess && !rc) rc = fail("%s failed: %s", what, hipGetErrorString(e)); };
    if (!rc) hip(hipMemsetAsync(d->x.p, 0, dmat_bytes(d), g_stream), "hipMemsetAsync");
    if (!rc) hip(hipMemcpyAsync(packed.p, m, sizeof(float) * (size_t)n * (size_t)n, hipMemcpyHostToDevice, g_stream), "hipMemcpyAsync");
    if (!rc) rc = hhx_transpose_f32(packed.p, n, d->x.p, d->ld, n, n);
    if (!rc) hip(hipStreamSynchronize(g_stream), "hipStreamSynchronize");
    if (rc) { delete d; return rc; }
    *out = d;
    return 0;
}

extern "C" int hhx_dmat_from_csr(const hhx_csr *t, hhx_dmat **out) {
    if (!t || !out) return fail("null pointer");
    if (t->n_rows != t->n_cols) return fail("hhx_dmat_from_csr needs a square matrix");
    hhx_dmat *d = nullptr;
    HHX_TRY(dmat_alloc(t->n_rows, &d));
    hipError_t e = hipMemsetAsync(d->x.p, 0, dmat_bytes(d), g_stream);
    if (e == hipSuccess) {
        k_dmcl_from_csr<<<csr_grid(d->n), ROW_T, 0, g_stream>>>(d->n, t->indptr.p, t->indices.p, t->data.p, d->x.p, d->ld);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { delete d; return fail("hhx_dmat_from_csr failed: %s", hipGetErrorString(e)); }
    *out = d;
    return 0;
}

extern "C" int hhx_dmat_to_host(const hhx_dmat *m, float *out) {
    if (!m || !out) return fail("null pointer");
    DevBuf<float> packed;
    if (packed.alloc((size_t)m->n * (size_t)m->n)) return 1;
    HHX_TRY(hhx_transpose_f32(m->x.p, m->ld, packed.p, m->n, m->n, m->n));
    HHX_HIP(hipMemcpyAsync(out, packed.p, sizeof(float) * (size_t)m->n * (size_t)m->n, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_dmat_to_csr(const hhx_dmat *m, hhx_csr **out) {
    if (!m || !out) return fail("null pointer");
    const i32 n = m->n;
    DevBuf<i32> cnt, optr;
    if (cnt.alloc((size_t)n + 1) || optr.alloc((size_t)n + 1)) return 1;
    k_dmcl_to_csr<false><<<csr_grid(n), ROW_T, 0, g_stream>>>(n, m->x.p, m->ld, cnt.p, nullptr, nullptr, nullptr);
    HHX_LAUNCH_CHECK();
    i64 total = 0;
    HHX_TRY(exclusive_scan_i32(cnt.p, optr.p, n, &total));
    if (total > INT_MAX) return fail("hhx_dmat_to_csr: %lld non-zero entries exceed the int32 index range of hhx_csr", (long long)total);
    hhx_csr *p = nullptr;
    HHX_TRY(hhx_csr_alloc_internal(n, n, total, &p));
    hipError_t e = hipMemcpyAsync(p->indptr.p, optr.p, sizeof(i32) * ((size_t)n + 1), hipMemcpyDeviceToDevice, g_stream);
    if (e == hipSuccess) {
        k_dmcl_to_csr<true><<<csr_grid(n), ROW_T, 0, g_stream>>>(n, m->x.p, m->ld, nullptr, p->indptr.p, p->indices.p, p->data.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g_stream);         // cnt / optr die with this frame
    if (e != hipSuccess) { hhx_csr_free(p); return fail("hhx_dmat_to_csr failed: %s", hipGetErrorString(e)); }
    *out = p;
    return 0;
}

extern "C" int hhx_dmat_copy(const hhx_dmat *m, hhx_dmat **out) {
    if (!m || !out) return fail("null pointer");
    return dmat_copy(m, out);
}

extern "C" int hhx_dmat_shape(const hhx_dmat *m, i32 *n, i64 *ld, i64 *bytes) {
    if (!m) return fail("null matrix");
    if (n) *n = m->n;
    if (ld) *ld = m->ld;
    if (bytes) *bytes = (i64)dmat_bytes(m);
    return 0;
}

extern "C" int hhx_dmat_free(hhx_dmat *m) {
    delete m;
    return 0;
}

extern "C" int hhx_dmat_gemm(const hhx_dmat *a, const hhx_dmat *b, hhx_dmat **out) {
    if (!a || !b || !out) return fail("null pointer");
    if (a->n != b->n) return fail("hhx_dmat_gemm: shape mismatch (%d, %d)", a->n, b->n);
    return dmat_gemm(b, a, out);                                     // (a @ b)^T = T_b * T_a
}

extern "C" int hhx_dmat_normalize_l1(hhx_dmat *m) {
    if (!m) return fail("null matrix");
    return dmat_epilogue(m, 2, 2.0, 0.0);
}

extern "C" int hhx_dmat_prune(const hhx_dmat *m, double pruning, hhx_dmat **out) {
    if (!m || !out) return fail("null pointer");
    hhx_dmat *c = nullptr;
    HHX_TRY(dmat_copy(m, &c));
    const int rc = dmat_epilogue(c, 4, 2.0, pruning);
    if (rc) { delete c; return rc; }
    *out = c;
    return 0;
}

extern "C" int hhx_dmat_power(const hhx_dmat *m, int expansion, hhx_dmat **out) {
    if (!m || !out) return fail("null pointer");
    if (expansion < 1) return fail("expansion must be >= 1");
    return dmat_power(m, expansion, out);
}

extern "C" int hhx_dmat_mcl(const hhx_dmat *pre_expanded, int done, int expansion, double inflation, int max_iter, double pruning, hhx_dmat **result,
                            int *n_iter, int *converged) {
    if (!pre_expanded || !result || !n_iter || !converged) return fail("null pointer");
    if (done < 0) return fail("hhx_dmat_mcl: done must be >= 0");
    if (expansion < 1) return fail("expansion must be >= 1");
    if (!(inflation > 0)) return fail("inflation must be positive");
    *n_iter = done;
    *converged = 0;
    hhx_dmat *cur = nullptr;                         // the matrix the previous iteration left (== last_matrix, :2057)
    DevBuf<unsigned int> flag;
    if (flag.alloc(1)) return 1;
    int rc = 0;
    for (int it = done; it < max_iter && !rc; ++it) {
        const hhx_dmat *src = cur ? cur : pre_expanded;
        hhx_dmat *p = nullptr;
        rc = it != 0 ? dmat_power(src, expansion, &p) : dmat_copy(src, &p);      // :2030-2035
        if (rc) break;
        rc = dmat_epilogue(p, 7, inflation, pruning);                             // :2040-2042
        if (rc) { delete p; break; }
        *n_iter = it + 1;
        bool stop = false;
        if (it > 1 && cur) {                                                       // :2051; the first iteration of a resumed call has no last_matrix
            unsigned int h = 1;
            hipError_t e = hipMemsetAsync(flag.p, 0, sizeof h, g_stream);
            if (e == hipSuccess) {
                KTimer kt("dmcl_allclose");
                k_dmcl_allclose<<<(unsigned)std::min<i32>(p->n, 2048), ROW_T, 0, g_stream>>>(p->n, p->ld, p->x.p, cur->x.p, flag.p);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&h, flag.p, sizeof h, hipMemcpyDeviceToHost, g_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
            if (e != hipSuccess) { delete p; rc = fail("hhx_dmat_mcl: the convergence test failed: %s", hipGetErrorString(e)); break; }
            stop = h == 0;
        }
        delete cur;
        cur = p;
        if (stop) { *converged = 1; break; }
    }
    if (rc) { delete cur; return rc; }
    if (!cur) rc = dmat_copy(pre_expanded, &cur);     // max_iter <= done: nothing to do
    if (rc) return rc;
    *result = cur;
    return 0;
}
