// Matrix normalisation and vmax of `haphic plot`: HapHiC_plot.py bnewt :291-404 (Knight-Ruiz balancing) and
// normalize_matrix :407-504.  The reference balances every intra-scaffold block and the whole matrix A = counts + 0.00001 with
// dense float64 numpy (A @ v per inner step, diag(x) @ A @ diag(x) as two GEMMs), walks every block cell in Python to collect the
// off-diagonal values, and takes their np.median.  Here the counts live in HBM as int32 and A[i][j] = (double)c + 0.00001 is formed
// in registers, so a mat-vec streams 4 n^2 bytes (the reference's float64 copy: 8 n^2):
//   * k_matvec: one wave per row, 16-byte loads of four counts (a row of a sub-block starts at any 4-byte offset: scalar head up to
//     the next 16-byte boundary, int4 body, scalar tail), the vector operand x * p formed at the load, the epilogue writing v / rk / Z
//     (residual form) or w (inner form) and the workgroup's share of rk@rk, rk@Z or p@w;
//   * k_update: ynew = y + alpha p, rk -= alpha w, Z = rk / v and the shares of min(ynew), max(ynew), rk@Z in one vector pass
//     (rk and Z may be advanced before the step is accepted: both early exits recompute them from x);
//   * every reduction is a tree of fixed shape (lane tree, then workgroup partials folded by one workgroup in index order): no
//     floating-point atomics, two runs give the same bits;
//   * the host loop of a large block reads back five scalars per inner step; blocks of at most PN_SMALL bins run the whole of bnewt
//     inside one workgroup each, all of them in ONE launch (a genome has tens to thousands of scaffolds of a few hundred bins);
//   * k_apply writes (x[i] * A[i][j]) * x[j] — the product order of d @ A @ d for diagonal d — with the block's x inside a scaffold
//     block, the whole matrix's x elsewhere, and exactly 0.0 where the count is 0 (zero_indices :418 :454);
//   * the median is a radix select (8 bits a pass) over the bit patterns of the gathered off-diagonal block cells: non-negative
//     doubles order like their bits; the two middle values go back to the host.
#include "hhx_common.h"

#include <algorithm>
#include <cmath>

using namespace hhx;

namespace {

constexpr int PN_T = 256, PN_ROWS = PN_T / HHX_WAVE;       // k_matvec: one wave per row, 4 rows per workgroup
constexpr int PN_SMALL = 512, PN_ST = 1024, PN_SW = PN_ST / HHX_WAVE;      // one-workgroup bnewt: largest block, threads, waves
constexpr double PN_EPS = 0.00001;                          // contact_matrix + 0.00001 :420
constexpr double PN_TOL = 1e-6, PN_DELTA = 0.1, PN_DELTA_UP = 3.0, PN_G = 0.9, PN_ETAMAX = 0.1;
constexpr int PN_MAX_OUTER = 1000, PN_MAX_INNER = 10000;
constexpr i64 PN_CHUNK_CELLS = (i64)1 << 24;                // cells per upload / apply chunk (128 MiB of int64 / float64)

}  // namespace

struct hhx_plotnorm {
    i32 n = 0, n_blocks = 0;
    bool valid = false, balanced = false;
    std::vector<i32> lo, hi;
    std::vector<i64> off;                                   // off-diagonal cells of the blocks before block g; off[n_blocks] = all
    DevBuf<i32> counts, blk_of, d_lo, d_hi;
    DevBuf<i64> d_off;
    DevBuf<double> x_all, x_blk, vec;                       // vec: 7 work vectors of n
    DevBuf<double> part, scal;
};

namespace {

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, HHX_WAVE));
    return __shfl(v, 0, HHX_WAVE);
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, HHX_WAVE));
    return __shfl(v, 0, HHX_WAVE);
}

// sum_j ((double)row[j] + 0.00001) * (a[j] * b[j]) over j < m by one wave (b == nullptr: a[j] alone).  Every lane returns the sum.
__device__ __forceinline__ double row_dot(const i32 *__restrict__ row, int m, const double *__restrict__ a, const double *__restrict__ b, int lane) {
    const int mis = (int)(((uintptr_t)row >> 2) & 3);
    const int head = min(m, (4 - mis) & 3);
    const int body = (m - head) >> 2;
    double acc = 0.0;
    if (lane < head) acc += ((double)row[lane] + PN_EPS) * (b ? a[lane] * b[lane] : a[lane]);
    const int4 *q = (const int4 *)(row + head);
#pragma unroll 2
    for (int k = lane; k < body; k += HHX_WAVE) {
        const int4 c = q[k];
        const int j = head + 4 * k;
        const double u0 = b ? a[j] * b[j] : a[j], u1 = b ? a[j + 1] * b[j + 1] : a[j + 1];
        const double u2 = b ? a[j + 2] * b[j + 2] : a[j + 2], u3 = b ? a[j + 3] * b[j + 3] : a[j + 3];
        acc += ((double)c.x + PN_EPS) * u0;
        acc += ((double)c.y + PN_EPS) * u1;
        acc += ((double)c.z + PN_EPS) * u2;
        acc += ((double)c.w + PN_EPS) * u3;
    }
    const int j = head + 4 * body + lane;
    if (j < m) acc += ((double)row[j] + PN_EPS) * (b ? a[j] * b[j] : a[j]);
    return wave_sum_f64(acc);
}

// the work vectors of one bnewt (slices of length-n arrays, indexed by the global bin)
struct PnVec { double *x, *v, *rk, *Z, *p, *w, *y, *y2; };

// mode 0: v = x * (A @ x), rk = 1 - v, Z = rk / v, p = Z; shares of rk@rk and rk@Z.   mode 1: w = x * (A @ (x * p)) + v * p; share of p@w.
// mode 2: out = A @ a (the plain product).  `base`: cell (lo, lo) of the block, `n`: the row pitch.
__global__ __launch_bounds__(PN_T) void k_matvec(const i32 *__restrict__ base, i64 n, int m, int mode, PnVec s, const double *__restrict__ a,
                                                 double *__restrict__ out, double *__restrict__ part, int pcap) {
    __shared__ double s0[PN_ROWS], s1[PN_ROWS];
    const int wv = threadIdx.x / HHX_WAVE, lane = lane_id();
    const int i = blockIdx.x * PN_ROWS + wv;
    double c0 = 0.0, c1 = 0.0;
    if (i < m) {
        const i32 *row = base + (i64)i * n;
        if (mode == 0) {
            const double d = row_dot(row, m, s.x, nullptr, lane);
            const double v = s.x[i] * d, rk = 1.0 - v, Z = rk / v;
            if (lane == 0) { s.v[i] = v; s.rk[i] = rk; s.Z[i] = Z; s.p[i] = Z; }
            c0 = rk * rk; c1 = rk * Z;
        } else if (mode == 1) {
            const double d = row_dot(row, m, s.x, s.p, lane);
            const double p = s.p[i], w = s.x[i] * d + s.v[i] * p;
            if (lane == 0) s.w[i] = w;
            c0 = p * w;
        } else {
            const double d = row_dot(row, m, a, nullptr, lane);
            if (lane == 0) out[i] = d;
        }
    }
    if (mode == 2) return;
    if (lane == 0) { s0[wv] = c0; s1[wv] = c1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int k = 0; k < PN_ROWS; ++k) { t0 += s0[k]; t1 += s1[k]; }
        part[blockIdx.x] = t0; part[pcap + blockIdx.x] = t1;
    }
}

// ynew = y + alpha p (into y2), rk -= alpha w, Z = rk / v; shares of min(ynew), max(ynew), rk@Z in part[0 / pcap / 2 pcap + block]
__global__ __launch_bounds__(PN_T) void k_update(int m, PnVec s, const double *__restrict__ scal, double *__restrict__ part, int pcap) {
    __shared__ double s0[PN_ROWS], s1[PN_ROWS], s2[PN_ROWS];
    const double alpha = scal[3];
    const int i = blockIdx.x * PN_T + threadIdx.x, wv = threadIdx.x / HHX_WAVE;
    double mn = INFINITY, mx = -INFINITY, rz = 0.0;
    if (i < m) {
        const double ap = alpha * s.p[i];
        const double yn = s.y[i] + ap;
        const double rk = s.rk[i] - alpha * s.w[i], Z = rk / s.v[i];
        s.y2[i] = yn; s.rk[i] = rk; s.Z[i] = Z;
        mn = yn; mx = yn; rz = rk * Z;
    }
    mn = wave_min_f64(mn); mx = wave_max_f64(mx); rz = wave_sum_f64(rz);
    if (lane_id() == 0) { s0[wv] = mn; s1[wv] = mx; s2[wv] = rz; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < PN_ROWS; ++k) { mn = fmin(mn, s0[k]); mx = fmax(mx, s1[k]); t += s2[k]; }
        part[blockIdx.x] = mn; part[pcap + blockIdx.x] = mx; part[2 * pcap + blockIdx.x] = t;
    }
}

// the step to the bound (:368-370 / :373-375): share of min((bound - y) / ap) over ap < 0 (up == 0) or ynew > bound (up == 1)
__global__ __launch_bounds__(PN_T) void k_gamma(int m, PnVec s, const double *__restrict__ scal, double bound, int up, double *__restrict__ part) {
    __shared__ double s0[PN_ROWS];
    const double alpha = scal[3];
    const int i = blockIdx.x * PN_T + threadIdx.x, wv = threadIdx.x / HHX_WAVE;
    double g = INFINITY;
    if (i < m) {
        const double ap = alpha * s.p[i];
        if (up ? s.y2[i] > bound : ap < 0.0) g = (bound - s.y[i]) / ap;
    }
    g = wave_min_f64(g);
    if (lane_id() == 0) s0[wv] = g;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < PN_ROWS; ++k) g = fmin(g, s0[k]);
        part[blockIdx.x] = g;
    }
}

// folds `count` workgroup shares of up to three arrays (op: 0 sum, 1 min, 2 max) in index order: thread t takes t, t + 256, ..., then a fixed LDS
// tree.  scal[k] = result of array k; rho_on: scal[3] = rho / scal[0] (alpha = rho_km1 / (p @ w) :361)
__global__ __launch_bounds__(PN_T) void k_fold(const double *__restrict__ part, int pcap, int count, int n_arr, int op0, int op1, int op2, int rho_on,
                                               double rho, double *__restrict__ scal) {
    __shared__ double sh[PN_T];
    for (int a = 0; a < n_arr; ++a) {
        const int op = a == 0 ? op0 : a == 1 ? op1 : op2;
        double t = op == 0 ? 0.0 : op == 1 ? INFINITY : -INFINITY;
        for (int k = threadIdx.x; k < count; k += PN_T) {
            const double v = part[a * pcap + k];
            t = op == 0 ? t + v : op == 1 ? fmin(t, v) : fmax(t, v);
        }
        sh[threadIdx.x] = t;
        __syncthreads();
        for (int o = PN_T / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                const double u = sh[threadIdx.x], v = sh[threadIdx.x + o];
                sh[threadIdx.x] = op == 0 ? u + v : op == 1 ? fmin(u, v) : fmax(u, v);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            scal[a] = sh[0];
            if (a == 0 && rho_on) scal[3] = rho / sh[0];
        }
        __syncthreads();
    }
}

// what: 0: x = 1, y = 1;  1: p = Z + beta p (:358);  2: y = y + gamma * (alpha p) (:370 :375), gamma = scal[0], alpha = scal[3];  3: x = x * y, y = 1 (:383)
__global__ __launch_bounds__(PN_T) void k_vec(int m, int what, PnVec s, double beta, const double *__restrict__ scal) {
    const int i = blockIdx.x * PN_T + threadIdx.x;
    if (i >= m) return;
    if (what == 0) { s.x[i] = 1.0; s.y[i] = 1.0; }
    else if (what == 1) s.p[i] = s.Z[i] + beta * s.p[i];
    else if (what == 2) { const double ap = scal[3] * s.p[i]; s.y[i] = s.y[i] + scal[0] * ap; }
    else { s.x[i] = s.x[i] * s.y[i]; s.y[i] = 1.0; }
}

// ------------------------------------------------------------------ bnewt of a small block inside one workgroup
struct SmallRed { double a[PN_SW], b[PN_SW], c[PN_SW]; };

// op: 0 sum, 1 min, 2 max; every thread gets the result (waves folded in index order)
__device__ __forceinline__ double wg_fold(double v, int op, double *sh) {
    v = op == 0 ? wave_sum_f64(v) : op == 1 ? wave_min_f64(v) : wave_max_f64(v);
    if (lane_id() == 0) sh[threadIdx.x / HHX_WAVE] = v;
    __syncthreads();
    double t = sh[0];
    for (int k = 1; k < PN_SW; ++k) t = op == 0 ? t + sh[k] : op == 1 ? fmin(t, sh[k]) : fmax(t, sh[k]);
    __syncthreads();
    return t;
}

// block b of `list`: the whole of bnewt :291-404, the workgroup's threads in lock step (every scalar comes out of wg_fold, the same in all)
__global__ __launch_bounds__(PN_ST) void k_bnewt_small(const i32 *__restrict__ counts, i64 n, const i32 *__restrict__ list, const i32 *__restrict__ blo,
                                                       const i32 *__restrict__ bhi, PnVec g, i32 *__restrict__ outer, i64 *__restrict__ mvp,
                                                       i32 *__restrict__ status) {
    __shared__ SmallRed sh;
    const int blk = list[blockIdx.x], lo = blo[blk], m = bhi[blk] - lo;
    const int tid = threadIdx.x, wv = tid / HHX_WAVE, lane = lane_id();
    const i32 *base = counts + (i64)lo * n + lo;
    PnVec s{g.x + lo, g.v + lo, g.rk + lo, g.Z + lo, g.p + lo, g.w + lo, g.y + lo, g.y2 + lo};
    for (int i = tid; i < m; i += PN_ST) { s.x[i] = 1.0; s.y[i] = 1.0; }
    __syncthreads();
    double rr, rz;
    auto residual = [&]() {
        double c0 = 0.0, c1 = 0.0;
        for (int i = wv; i < m; i += PN_SW) {
            const double d = row_dot(base + (i64)i * n, m, s.x, nullptr, lane);
            const double v = s.x[i] * d, rk = 1.0 - v, Z = rk / v;
            if (lane == 0) { s.v[i] = v; s.rk[i] = rk; s.Z[i] = Z; s.p[i] = Z; c0 += rk * rk; c1 += rk * Z; }
        }
        rr = wg_fold(c0, 0, sh.a); rz = wg_fold(c1, 0, sh.b);
    };
    residual();
    const double rt = PN_TOL * PN_TOL, stop_tol = PN_TOL * 0.5;
    double eta = PN_ETAMAX, rho_km1 = rr, rho_km2 = 0.0, rout = rr, rold = rr;
    i64 MVP = 0;
    int nn = 0, st = 0;
    while (rout > rt) {
        if (++nn > PN_MAX_OUTER) { st = 1; break; }
        int k = 0, mm = 0;
        const double innertol = fmax(eta * eta * rout, rt);
        while (rho_km1 > innertol) {
            if (++mm > PN_MAX_INNER) { st = 1; break; }
            ++k;
            if (k == 1) rho_km1 = rz;
            else {
                const double beta = rho_km1 / rho_km2;
                for (int i = tid; i < m; i += PN_ST) s.p[i] = s.Z[i] + beta * s.p[i];
                __syncthreads();
            }
            double c0 = 0.0;
            for (int i = wv; i < m; i += PN_SW) {
                const double d = row_dot(base + (i64)i * n, m, s.x, s.p, lane);
                const double p = s.p[i], w = s.x[i] * d + s.v[i] * p;
                if (lane == 0) { s.w[i] = w; c0 += p * w; }
            }
            const double alpha = rho_km1 / wg_fold(c0, 0, sh.a);
            double mn = INFINITY, mx = -INFINITY;
            for (int i = tid; i < m; i += PN_ST) {
                const double yn = s.y[i] + alpha * s.p[i];
                s.y2[i] = yn;
                mn = fmin(mn, yn); mx = fmax(mx, yn);
            }
            mn = wg_fold(mn, 1, sh.a); mx = wg_fold(mx, 2, sh.b);
            if (mn <= PN_DELTA || mx >= PN_DELTA_UP) {
                const int up = !(mn <= PN_DELTA);
                const double bound = up ? PN_DELTA_UP : PN_DELTA;
                double gm = INFINITY;
                for (int i = tid; i < m; i += PN_ST) {
                    const double ap = alpha * s.p[i];
                    if (up ? s.y2[i] > bound : ap < 0.0) gm = fmin(gm, (bound - s.y[i]) / ap);
                }
                gm = wg_fold(gm, 1, sh.c);
                if (!(gm < INFINITY)) { st = 2; break; }
                for (int i = tid; i < m; i += PN_ST) { const double ap = alpha * s.p[i]; s.y[i] = s.y[i] + gm * ap; }
                break;
            }
            double c1 = 0.0;
            for (int i = tid; i < m; i += PN_ST) {
                const double rk = s.rk[i] - alpha * s.w[i], Z = rk / s.v[i];
                s.y[i] = s.y2[i]; s.rk[i] = rk; s.Z[i] = Z;
                c1 += rk * Z;
            }
            rho_km2 = rho_km1;
            rho_km1 = wg_fold(c1, 0, sh.c);
        }
        if (st) break;
        for (int i = tid; i < m; i += PN_ST) { s.x[i] = s.x[i] * s.y[i]; s.y[i] = 1.0; }
        __syncthreads();
        residual();
        rho_km1 = rr; rout = rr;
        MVP += k + 1;
        const double rat = rout / rold, res_norm = sqrt(rout), eta_o = eta;
        rold = rout;
        eta = PN_G * rat;
        if (PN_G * eta_o * eta_o > 0.1) eta = fmax(eta, PN_G * eta_o * eta_o);
        eta = fmax(fmin(eta, PN_ETAMAX), stop_tol / res_norm);
    }
    if (tid == 0) { outer[blk] = nn - (st == 1 && nn > PN_MAX_OUTER); mvp[blk] = MVP; status[blk] = st; }
}

// ------------------------------------------------------------------ upload, apply, gather, select
__global__ __launch_bounds__(PN_T) void k_narrow(const i64 *__restrict__ in, i64 cells, i32 *__restrict__ out, long long *__restrict__ mnmx) {
    i64 mn = INT64_MAX, mx = INT64_MIN;
    for (i64 k = (i64)blockIdx.x * PN_T + threadIdx.x; k < cells; k += (i64)gridDim.x * PN_T) {
        const i64 v = in[k];
        out[k] = (i32)v;
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const i64 a = __shfl_down(mn, o, HHX_WAVE), b = __shfl_down(mx, o, HHX_WAVE);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if (lane_id() == 0) { atomicMin(&mnmx[0], (long long)mn); atomicMax(&mnmx[1], (long long)mx); }
}

__global__ __launch_bounds__(PN_T) void k_asym(const i32 *__restrict__ c, i64 n, int *__restrict__ flag) {
    const i64 j = (i64)blockIdx.x * 16 + (threadIdx.x & 15), i = (i64)blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i < n && j < n && i < j && c[i * n + j] != c[j * n + i]) atomicOr(flag, 1);
}

__global__ __launch_bounds__(PN_T) void k_apply(const i32 *__restrict__ c, i64 n, i64 row0, i64 cells, const i32 *__restrict__ blk_of,
                                                const double *__restrict__ xa, const double *__restrict__ xb, double *__restrict__ out) {
    for (i64 k = (i64)blockIdx.x * PN_T + threadIdx.x; k < cells; k += (i64)gridDim.x * PN_T) {
        const i64 i = row0 + k / n, j = k % n;
        const i32 v = c[row0 * n + k];
        double r = 0.0;
        if (v != 0) {
            const i32 g = blk_of[i];
            const double *x = g >= 0 && g == blk_of[j] ? xb : xa;
            r = (x[i] * ((double)v + PN_EPS)) * x[j];
        }
        out[k] = r;
    }
}

// one workgroup per bin i of a block: the block row's off-diagonal cells, in the reference's list order (:447-450 / :482-485)
__global__ __launch_bounds__(PN_T) void k_gather(const i32 *__restrict__ c, i64 n, const i32 *__restrict__ blk_of, const i32 *__restrict__ blo,
                                                 const i32 *__restrict__ bhi, const i64 *__restrict__ off, const double *__restrict__ xb, int kr,
                                                 u64 *__restrict__ out) {
    const i64 i = blockIdx.x;
    const i32 g = blk_of[i];
    if (g < 0) return;
    const i32 lo = blo[g], m = bhi[g] - lo;
    u64 *dst = out + off[g] + (i64)(i - lo) * (m - 1);
    for (i32 jj = threadIdx.x; jj < m - 1; jj += PN_T) {
        const i64 j = lo + jj + (lo + jj >= i);
        const i32 v = c[i * n + j];
        dst[jj] = kr ? (u64)__double_as_longlong((xb[i] * ((double)v + PN_EPS)) * xb[j]) : (u64)v;
    }
}

// digit histogram of the values whose bits above shift + 8 equal those of `prefix`
__global__ __launch_bounds__(PN_T) void k_digits(const u64 *__restrict__ v, i64 count, int shift, u64 prefix, unsigned long long *__restrict__ hist) {
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u64 hi_mask = shift + 8 >= 64 ? 0ull : ~0ull << (shift + 8);
    for (i64 k = (i64)blockIdx.x * PN_T + threadIdx.x; k < count; k += (i64)gridDim.x * PN_T) {
        const u64 x = v[k];
        if ((x & hi_mask) == (prefix & hi_mask)) atomicAdd(&h[(x >> shift) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

unsigned grid_for(i64 items, i64 per_block, i64 cap = 8192) { return (unsigned)std::max<i64>(1, std::min<i64>((items + per_block - 1) / per_block, cap)); }

// the value of rank k (0-based) among `count` device values
int select_rank(const u64 *vals, i64 count, i64 k, u64 *out) {
    DevBuf<unsigned long long> hist;
    if (hist.alloc(256)) return 1;
    u64 prefix = 0;
    unsigned long long h[256];
    for (int shift = 56; shift >= 0; shift -= 8) {
        HHX_HIP(hipMemsetAsync(hist.p, 0, sizeof h, g_stream));
        k_digits<<<grid_for(count, PN_T * 8), PN_T, 0, g_stream>>>(vals, count, shift, prefix, hist.p);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(h, hist.p, sizeof h, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        int d = 0;
        for (; d < 256; ++d) {
            if (k < (i64)h[d]) break;
            k -= (i64)h[d];
        }
        if (d == 256) return fail("hhx_plotnorm: radix select lost its rank");
        prefix |= (u64)d << shift;
    }
    *out = prefix;
    return 0;
}

int select_middle(const u64 *vals, i64 count, u64 *lo, u64 *hi) {
    *lo = *hi = 0;
    if (count <= 0) return 0;
    HHX_TRY(select_rank(vals, count, (count - 1) / 2, lo));
    if (count & 1) *hi = *lo;
    else HHX_TRY(select_rank(vals, count, count / 2, hi));
    return 0;
}

// measurement knobs (hhx_tune): the largest block of the one-workgroup path, the cells of an upload / apply chunk.  Defaults: the constants above.
i32 small_limit() { return (i32)std::max<i64>(0, std::min<i64>(PN_SMALL, tune_get("plotnorm_small", PN_SMALL))); }
i64 chunk_cells() { return std::max<i64>(1, tune_get("plotnorm_chunk_cells", PN_CHUNK_CELLS)); }

PnVec vecs_of(hhx_plotnorm *h, double *x, i32 lo) {
    double *w = h->vec.p + lo;
    const i64 n = h->n;
    return PnVec{x + lo, w, w + n, w + 2 * n, w + 3 * n, w + 4 * n, w + 5 * n, w + 6 * n};
}

int read_scal(hhx_plotnorm *h, double *s) {
    HHX_HIP(hipMemcpyAsync(s, h->scal.p, 4 * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

// bnewt :291-404 on [lo, lo + m) with the control flow on the host: one read-back of (p@w, min, max, rk@Z | alpha) per inner step
int bnewt_grid(hhx_plotnorm *h, double *x, i32 lo, i32 m, i32 *outer, i64 *mvp, i32 *status) {
    PnVec s = vecs_of(h, x, lo);
    const i32 *base = h->counts.p + (i64)lo * h->n + lo;
    const int pcap = (h->n + PN_ROWS - 1) / PN_ROWS;
    const unsigned g_rows = (unsigned)((m + PN_ROWS - 1) / PN_ROWS), g_vec = (unsigned)((m + PN_T - 1) / PN_T);
    double *part = h->part.p, *scal = h->scal.p, sc[4];
    double rr = 0.0, rz = 0.0;
    auto residual = [&]() -> int {
        k_matvec<<<g_rows, PN_T, 0, g_stream>>>(base, (i64)h->n, m, 0, s, nullptr, nullptr, part, pcap);
        k_fold<<<1, PN_T, 0, g_stream>>>(part, pcap, (int)g_rows, 2, 0, 0, 0, 0, 0.0, scal);
        HHX_LAUNCH_CHECK();
        HHX_TRY(read_scal(h, sc));
        rr = sc[0]; rz = sc[1];
        return 0;
    };
    k_vec<<<g_vec, PN_T, 0, g_stream>>>(m, 0, s, 0.0, scal);
    HHX_TRY(residual());
    const double rt = PN_TOL * PN_TOL, stop_tol = PN_TOL * 0.5;
    double eta = PN_ETAMAX, rho_km1 = rr, rho_km2 = 0.0, rout = rr, rold = rr;
    i64 MVP = 0;
    int nn = 0, st = 0;
    while (rout > rt) {
        if (++nn > PN_MAX_OUTER) { st = 1; --nn; break; }
        int k = 0, mm = 0;
        const double innertol = std::max(eta * eta * rout, rt);
        while (rho_km1 > innertol) {
            if (++mm > PN_MAX_INNER) { st = 1; break; }
            ++k;
            if (k == 1) rho_km1 = rz;
            else k_vec<<<g_vec, PN_T, 0, g_stream>>>(m, 1, s, rho_km1 / rho_km2, scal);
            {
                KTimer kt("plotnorm_matvec");
                k_matvec<<<g_rows, PN_T, 0, g_stream>>>(base, (i64)h->n, m, 1, s, nullptr, nullptr, part, pcap);
            }
            k_fold<<<1, PN_T, 0, g_stream>>>(part, pcap, (int)g_rows, 1, 0, 0, 0, 1, rho_km1, scal);         // scal[3] = alpha
            k_update<<<g_vec, PN_T, 0, g_stream>>>(m, s, scal, part, pcap);
            k_fold<<<1, PN_T, 0, g_stream>>>(part, pcap, (int)g_vec, 3, 1, 2, 0, 0, 0.0, scal);
            HHX_LAUNCH_CHECK();
            HHX_TRY(read_scal(h, sc));
            const double mn = sc[0], mx = sc[1];
            if (mn <= PN_DELTA || mx >= PN_DELTA_UP) {
                const int up = !(mn <= PN_DELTA);
                k_gamma<<<g_vec, PN_T, 0, g_stream>>>(m, s, scal, up ? PN_DELTA_UP : PN_DELTA, up, part);
                k_fold<<<1, PN_T, 0, g_stream>>>(part, pcap, (int)g_vec, 1, 1, 0, 0, 0, 0.0, scal);         // scal[0] = gamma
                HHX_LAUNCH_CHECK();
                HHX_TRY(read_scal(h, sc));
                if (!(sc[0] < INFINITY)) { st = 2; break; }
                k_vec<<<g_vec, PN_T, 0, g_stream>>>(m, 2, s, 0.0, scal);
                break;
            }
            std::swap(s.y, s.y2);
            rho_km2 = rho_km1;
            rho_km1 = sc[2];
        }
        if (st) break;
        k_vec<<<g_vec, PN_T, 0, g_stream>>>(m, 3, s, 0.0, scal);
        HHX_TRY(residual());
        rho_km1 = rr; rout = rr;
        MVP += k + 1;
        const double rat = rout / rold, res_norm = std::sqrt(rout), eta_o = eta;
        rold = rout;
        eta = PN_G * rat;
        if (PN_G * eta_o * eta_o > 0.1) eta = std::max(eta, PN_G * eta_o * eta_o);
        eta = std::max(std::min(eta, PN_ETAMAX), stop_tol / res_norm);
    }
    prof_count("plotnorm_matvecs", MVP);
    *outer = nn; *mvp = MVP; *status = st;
    return 0;
}

}  // namespace

extern "C" int hhx_plotnorm_create(const i64 *matrix, i32 n, hhx_plotnorm **out, i64 *max, i64 *min, i32 *symmetric) {
    if (!out) return fail("null pointer");
    if (n <= 0 || !matrix) return fail("hhx_plotnorm_create: bad arguments");
    hhx_plotnorm *h = new hhx_plotnorm();
    h->n = n;
    const i64 cells = (i64)n * n, rows_per = std::max<i64>(1, chunk_cells() / n);
    DevBuf<i64> stage;
    DevBuf<long long> mnmx;
    DevBuf<int> flag;
    long long init[2] = {INT64_MAX, INT64_MIN}, got[2];
    int asym = 0;
    auto run = [&]() -> int {
        if (h->counts.alloc((size_t)cells) || stage.alloc((size_t)(rows_per * n)) || mnmx.alloc(2) || flag.alloc(1) || h->x_all.alloc(n) ||
            h->x_blk.alloc(n) || h->vec.alloc((size_t)7 * n) || h->part.alloc((size_t)3 * ((n + PN_ROWS - 1) / PN_ROWS)) || h->scal.alloc(4) ||
            h->blk_of.alloc(n))
            return 1;
        HHX_HIP(hipMemcpyAsync(mnmx.p, init, sizeof init, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), g_stream));
        HHX_HIP(hipMemsetAsync(h->blk_of.p, 0xff, sizeof(i32) * n, g_stream));
        HHX_HIP(hipMemsetAsync(h->x_blk.p, 0, sizeof(double) * n, g_stream));
        for (i64 r = 0; r < n; r += rows_per) {
            const i64 c = std::min<i64>(rows_per, n - r) * n;
            HHX_HIP(hipMemcpyAsync(stage.p, matrix + r * n, sizeof(i64) * c, hipMemcpyHostToDevice, g_stream));
            k_narrow<<<grid_for(c, PN_T * 8), PN_T, 0, g_stream>>>(stage.p, c, h->counts.p + r * n, mnmx.p);
            HHX_LAUNCH_CHECK();
            HHX_HIP(hipStreamSynchronize(g_stream));          // the staging block is reused
        }
        const unsigned t = (unsigned)((n + 15) / 16);
        k_asym<<<dim3(t, t), PN_T, 0, g_stream>>>(h->counts.p, (i64)n, flag.p);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(got, mnmx.p, sizeof got, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(&asym, flag.p, sizeof asym, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        return 0;
    };
    if (run()) { delete h; return 1; }
    h->valid = got[0] >= 0 && got[1] <= INT32_MAX;           // otherwise the int32 copy is not the matrix: every later call refuses
    if (max) *max = got[1];
    if (min) *min = got[0];
    if (symmetric) *symmetric = !asym;
    *out = h;
    return 0;
}

extern "C" int hhx_plotnorm_set_blocks(hhx_plotnorm *h, i32 n_blocks, const i32 *lo, const i32 *hi) {
    if (!h) return fail("null handle");
    if (n_blocks < 0 || (n_blocks && (!lo || !hi))) return fail("hhx_plotnorm_set_blocks: bad arguments");
    i32 at = 0;
    std::vector<i32> of((size_t)h->n, -1);
    std::vector<i64> off((size_t)n_blocks + 1, 0);
    for (i32 g = 0; g < n_blocks; ++g) {
        if (lo[g] < at || hi[g] < lo[g] || hi[g] > h->n) return fail("hhx_plotnorm_set_blocks: block %d = [%d, %d) of %d bins", g, lo[g], hi[g], h->n);
        at = hi[g];
        for (i32 i = lo[g]; i < hi[g]; ++i) of[i] = g;
        const i64 m = hi[g] - lo[g];
        off[g + 1] = off[g] + m * (m - 1);
    }
    h->n_blocks = n_blocks;
    h->lo.assign(lo, lo + n_blocks); h->hi.assign(hi, hi + n_blocks); h->off = off;
    h->balanced = false;
    if (h->d_lo.alloc(n_blocks) || h->d_hi.alloc(n_blocks) || h->d_off.alloc((size_t)n_blocks + 1)) return 1;
    HHX_HIP(hipMemcpyAsync(h->blk_of.p, of.data(), sizeof(i32) * h->n, hipMemcpyHostToDevice, g_stream));
    if (n_blocks) {
        HHX_HIP(hipMemcpyAsync(h->d_lo.p, lo, sizeof(i32) * n_blocks, hipMemcpyHostToDevice, g_stream));
        HHX_HIP(hipMemcpyAsync(h->d_hi.p, hi, sizeof(i32) * n_blocks, hipMemcpyHostToDevice, g_stream));
    }
    HHX_HIP(hipMemcpyAsync(h->d_off.p, off.data(), sizeof(i64) * (n_blocks + 1), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_plotnorm_balance(hhx_plotnorm *h, i32 *outer, i64 *mvp, i32 *status) {
    if (!h) return fail("null handle");
    if (!outer || !mvp || !status) return fail("null pointer");
    if (!h->valid) return fail("hhx_plotnorm_balance: the matrix holds a negative count or one beyond int32");
    const i32 nb = h->n_blocks;
    for (i32 g = 0; g <= nb; ++g) { outer[g] = 0; mvp[g] = 0; status[g] = 0; }
    HHX_HIP(hipMemsetAsync(h->x_blk.p, 0, sizeof(double) * h->n, g_stream));
    const i32 small_max = small_limit();
    std::vector<i32> small;
    for (i32 g = 0; g < nb; ++g)
        if (h->hi[g] > h->lo[g] && h->hi[g] - h->lo[g] <= small_max) small.push_back(g);
    if (!small.empty()) {
        DevBuf<i32> list, d_outer, d_status;
        DevBuf<i64> d_mvp;
        if (list.alloc(small.size()) || d_outer.alloc(nb) || d_status.alloc(nb) || d_mvp.alloc(nb)) return 1;
        HHX_HIP(hipMemcpyAsync(list.p, small.data(), sizeof(i32) * small.size(), hipMemcpyHostToDevice, g_stream));
        {
            KTimer kt("plotnorm_small_blocks");
            k_bnewt_small<<<(unsigned)small.size(), PN_ST, 0, g_stream>>>(h->counts.p, (i64)h->n, list.p, h->d_lo.p, h->d_hi.p, vecs_of(h, h->x_blk.p, 0),
                                                                          d_outer.p, d_mvp.p, d_status.p);
        }
        HHX_LAUNCH_CHECK();
        std::vector<i32> o(nb), s(nb);
        std::vector<i64> v(nb);
        HHX_HIP(hipMemcpyAsync(o.data(), d_outer.p, sizeof(i32) * nb, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(s.data(), d_status.p, sizeof(i32) * nb, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(v.data(), d_mvp.p, sizeof(i64) * nb, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        bool bad = false;
        for (i32 g : small) { outer[g] = o[g]; mvp[g] = v[g]; status[g] = s[g]; bad |= s[g] != 0; }
        if (bad) return 0;
    }
    for (i32 g = 0; g < nb; ++g)
        if (h->hi[g] - h->lo[g] > small_max) {
            HHX_TRY(bnewt_grid(h, h->x_blk.p, h->lo[g], h->hi[g] - h->lo[g], &outer[g], &mvp[g], &status[g]));
            if (status[g]) return 0;
        }
    HHX_TRY(bnewt_grid(h, h->x_all.p, 0, h->n, &outer[nb], &mvp[nb], &status[nb]));
    h->balanced = status[nb] == 0;
    return 0;
}

extern "C" int hhx_plotnorm_fetch_x(hhx_plotnorm *h, double *x_all, double *x_blocks) {
    if (!h) return fail("null handle");
    if (x_all) HHX_HIP(hipMemcpyAsync(x_all, h->x_all.p, sizeof(double) * h->n, hipMemcpyDeviceToHost, g_stream));
    if (x_blocks) HHX_HIP(hipMemcpyAsync(x_blocks, h->x_blk.p, sizeof(double) * h->n, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_plotnorm_apply(hhx_plotnorm *h, double *out_host) {
    if (!h) return fail("null handle");
    if (!out_host) return fail("null pointer");
    if (!h->balanced) return fail("hhx_plotnorm_apply: no balancing has converged on this handle");
    const i64 n = h->n, rows_per = std::max<i64>(1, chunk_cells() / n);
    DevBuf<double> stage;
    if (stage.alloc((size_t)(rows_per * n))) return 1;
    for (i64 r = 0; r < n; r += rows_per) {
        const i64 c = std::min<i64>(rows_per, n - r) * n;
        k_apply<<<grid_for(c, PN_T * 4, 65536), PN_T, 0, g_stream>>>(h->counts.p, n, r, c, h->blk_of.p, h->x_all.p, h->x_blk.p, stage.p);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(out_host + r * n, stage.p, sizeof(double) * c, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
    }
    return 0;
}

extern "C" int hhx_plotnorm_median(hhx_plotnorm *h, i32 kr, i64 *count, u64 *lo, u64 *hi) {
    if (!h) return fail("null handle");
    if (!count || !lo || !hi) return fail("null pointer");
    if (!h->valid) return fail("hhx_plotnorm_median: the matrix holds a negative count or one beyond int32");
    if (kr && !h->balanced) return fail("hhx_plotnorm_median: no balancing has converged on this handle");
    const i64 total = h->off.empty() ? 0 : h->off.back();
    *count = total; *lo = *hi = 0;
    if (!total) return 0;
    DevBuf<u64> vals;
    if (vals.alloc((size_t)total)) return 1;
    k_gather<<<(unsigned)h->n, PN_T, 0, g_stream>>>(h->counts.p, (i64)h->n, h->blk_of.p, h->d_lo.p, h->d_hi.p, h->d_off.p, h->x_blk.p, kr ? 1 : 0, vals.p);
    HHX_LAUNCH_CHECK();
    return select_middle(vals.p, total, lo, hi);
}

extern "C" int hhx_plotnorm_matvec(hhx_plotnorm *h, i32 lo, i32 hi, const double *v, double *out) {
    if (!h) return fail("null handle");
    if (!v || !out) return fail("null pointer");
    if (lo < 0 || hi <= lo || hi > h->n) return fail("hhx_plotnorm_matvec: bad range [%d, %d) of %d bins", lo, hi, h->n);
    if (!h->valid) return fail("hhx_plotnorm_matvec: the matrix holds a negative count or one beyond int32");
    const i32 m = hi - lo;
    double *a = h->vec.p, *o = h->vec.p + h->n;
    HHX_HIP(hipMemcpyAsync(a, v, sizeof(double) * m, hipMemcpyHostToDevice, g_stream));
    k_matvec<<<(unsigned)((m + PN_ROWS - 1) / PN_ROWS), PN_T, 0, g_stream>>>(h->counts.p + (i64)lo * h->n + lo, (i64)h->n, m, 2, PnVec{}, a, o, nullptr, 0);
    HHX_LAUNCH_CHECK();
    HHX_HIP(hipMemcpyAsync(out, o, sizeof(double) * m, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_plotnorm_destroy(hhx_plotnorm *h) {
    delete h;
    return 0;
}

extern "C" int hhx_select_middle_u64(const u64 *vals, i64 count, u64 *lo, u64 *hi) {
    if (!lo || !hi || (count > 0 && !vals)) return fail("null pointer");
    if (count < 0) return fail("hhx_select_middle_u64: negative count");
    *lo = *hi = 0;
    if (!count) return 0;
    DevBuf<u64> d;
    if (d.alloc((size_t)count)) return 1;
    HHX_HIP(hipMemcpyAsync(d.p, vals, sizeof(u64) * count, hipMemcpyHostToDevice, g_stream));
    return select_middle(d.p, count, lo, hi);
}
