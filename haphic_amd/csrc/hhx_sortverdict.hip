// `haphic sort`, fast sorting vs ALLHiC (HapHiC_sort.py compare_fast_sort_and_allhic :645-724): the weighted longest-increasing-subsequence sums of
// every rotation of the fast-sort tour, s[r] = max(find_lis(forward), find_lis(reverse)) :707-710, r = 0 .. n - 2.
//
// The reference spends O(n^2) per rotation (dp[i] = len_i + max over the earlier j of its class with a smaller signed value :662-669).  Here a
// rotation is one wavefront and the max over "earlier and smaller" is a prefix maximum of a Fenwick tree indexed by the element's RANK inside its class:
// the host ranks the positive elements by ascending position in the ALLHiC tour and the negative ones by descending position (a signed value
// -(pos + 1) grows as pos falls), so both classes ask the same question, "the best dp among ranks below mine", of two trees that share one array of
// n + 1 cells: cells 1 .. P the positive class, P + 1 .. n the negative one.  Values of one class are distinct, so "strictly smaller" is "rank below".
//
// One element is one step of the wave: lane b reads the query node of set bit b of the rank (rank & ~(2^b - 1)) and, in the same issue, the update node
// of zero bit b - 1 (rank | (2^b - 1), lane 0: the rank itself); a DPP max over the 16-lane rows and two lane reads join the query; the update lanes write
// max(old, dp).  Ranks stay below 2^18, so lanes 0 .. 18 of the wave carry a step and the others idle: the step is bound by the latency of its chain
// (LDS read -> max -> LDS write), not by lanes, and a CU hides it behind the other rotations it holds.  Elements reach the wave 64 at a time (one
// coalesced read of the ranks and the lengths, then a lane read per step).
//
// Two forms of the same loop.  LDS: the tree of a rotation lives in the LDS of its one-wave workgroup, (n + 1) cells of 4 bytes when the lengths sum to
// less than 2^32 (any chromosome-sized group) and of 8 bytes otherwise; n <= 40959 / 20479 would fit the 160 KiB of a CU.  HBM: every workgroup owns
// a slab of n + 1 cells in a scratch buffer of at most 1 GiB and takes its rotations one after the other (grid stride), so the scratch is bounded
// whatever n; the lanes of the wave then meet through memory, hence the workgroup barrier per step.  The seam between them is where the LDS form stops
// paying: a step is latency, a CU hides it behind the other rotations it holds, and the LDS form holds 160 KiB / tree of them.  Measured
// (profiles/sort_verdict_bench.json): n = 1000 LDS 0.27 ms, HBM 0.44 ms; n = 4000 2.2 and 2.0 ms; n = 16000 (two trees per CU) LDS 104 ms, HBM 31 ms.
// So by default a tree of up to 16 KiB (ten rotations per CU and more) stays in LDS: n <= 4095 / 2047; hhx_tune "sort_verdict_lds_n" moves the
// seam anywhere up to what fits.  Only maxima of exact integer sums leave the kernel: both forms and both cell widths give the same integers.
#include <algorithm>

#include "hhx_common.h"

using namespace hhx;

namespace {
constexpr int SV_T = HHX_WAVE;                  // one wave per workgroup: no barrier in the LDS form
constexpr int SV_LDS_BYTES = 160 * 1024;
constexpr int SV_LDS_DEFAULT_BYTES = 16 * 1024;   // the largest tree that stays in LDS unless the knob says otherwise (head of this file)
constexpr i32 SV_MAX_N = HHX_SORT_VERDICT_MAX_N;
constexpr i64 SV_SCRATCH_BYTES = 1ll << 30;
constexpr i64 SV_HBM_GRID = 4096;
constexpr u32 SV_NEG = 0x80000000u;             // class bit of an encoded rank
}  // namespace

// DPP controls: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror — after the four, every lane of a 16-lane row holds the row's max
template <int CTRL>
__device__ __forceinline__ u32 sv_dpp(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ u64 sv_dpp(u64 v) { return ((u64)sv_dpp<CTRL>((u32)(v >> 32)) << 32) | sv_dpp<CTRL>((u32)v); }
__device__ __forceinline__ u32 sv_lane(u32 v, int lane) { return (u32)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ u64 sv_lane(u64 v, int lane) { return ((u64)sv_lane((u32)(v >> 32), lane) << 32) | sv_lane((u32)v, lane); }
__device__ __forceinline__ i32 sv_lane(i32 v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

template <class V>
__device__ __forceinline__ V sv_mx(V a, V b) { return a > b ? a : b; }

// the max over lanes 0 .. 31, the same in every lane; all 64 lanes call it
template <class V>
__device__ __forceinline__ V sv_max32(V m) {
    m = sv_mx(m, sv_dpp<0xB1>(m));
    m = sv_mx(m, sv_dpp<0x4E>(m));
    m = sv_mx(m, sv_dpp<0x141>(m));
    m = sv_mx(m, sv_dpp<0x140>(m));
    return sv_mx(sv_lane(m, 0), sv_lane(m, 16));
}

// enc[i]: rank of element i of the fast-sort tour inside its class | SV_NEG for the negative class; len[i]: its weight.  Workgroup b takes the
// rotations r0 + b, r0 + b + gridDim.x, ... below r1; sums[r - r0] = the largest dp of rotation r.
template <class V, bool LDS>
static __global__ __launch_bounds__(SV_T) void k_sv_rotations(i32 n, i32 n_pos, const i32 *__restrict__ enc, const V *__restrict__ len, i32 r0, i32 r1,
                                                             V *scratch, i64 *__restrict__ sums) {
    extern __shared__ __align__(8) unsigned char sv_lds[];
    V *T = LDS ? (V *)sv_lds : scratch + (i64)blockIdx.x * ((i64)n + 1);
    const int lane = threadIdx.x;
    const u32 below = (1u << (lane & 31)) - 1u;         // the bits under this lane's bit
    const bool low = lane < 32;
    for (i32 r = r0 + (i32)blockIdx.x; r < r1; r += (i32)gridDim.x) {
        for (i32 k = lane; k <= n; k += SV_T) T[k] = 0;
        if (LDS) __builtin_amdgcn_wave_barrier();
        else __syncthreads();
        V best = 0;
        for (i32 k0 = 0; k0 < n; k0 += SV_T) {
            const i32 idx = k0 + lane;
            i32 src = r + idx;                            // r < n, idx < n + 64: no wrap of int32 for n <= 2^18
            if (src >= n) src -= n;
            const i32 my_e = idx < n ? enc[src] : 0;
            const V my_w = idx < n ? len[src] : (V)0;
            const int cnt = min(SV_T, n - k0);
            for (int t = 0; t < cnt; ++t) {
                const u32 e = (u32)sv_lane(my_e, t);
                const V w = sv_lane(my_w, t);
                const u32 q = e & ~SV_NEG;                // 0-based rank: the query is the prefix of q cells, the update cell q + 1
                const u32 base = (e & SV_NEG) ? (u32)n_pos : 0u, size = (e & SV_NEG) ? (u32)(n - n_pos) : (u32)n_pos;
                const u32 un = q | below;
                const bool ask = low && ((q >> (lane & 31)) & 1u);
                const bool upd = low && (lane == 0 || !((q >> ((lane - 1) & 31)) & 1u)) && un < size;
                V m = ask ? T[base + (q & ~below)] : (V)0;
                const V old = upd ? T[base + un + 1] : (V)0;
                m = sv_max32(m);
                const V dp = m + w;
                if (upd) T[base + un + 1] = sv_mx(old, dp);
                best = sv_mx(best, dp);
                if (LDS) __builtin_amdgcn_wave_barrier();  // LDS serves a wave's accesses in program order: only the compiler must keep it
                else __syncthreads();                      // the next step's lanes read what other lanes of the wave stored: through memory
            }
        }
        if (lane == 0) sums[r - r0] = (i64)best;
    }
}

template <class V>
static int sv_run(i32 n, i32 n_pos, const std::vector<i32> &enc, const int64_t *len, i32 r0, i32 r1, int64_t *sums, i64 *stats) {
    const i32 R = r1 - r0;
    std::vector<V> hlen((size_t)n);
    for (i32 i = 0; i < n; ++i) hlen[i] = (V)len[i];
    DevBuf<i32> d_enc;
    DevBuf<V> d_len, scratch;
    DevBuf<i64> d_sums;
    if (d_enc.alloc(n) || d_len.alloc(n) || d_sums.alloc(R)) return 1;
    HHX_HIP(hipMemcpyAsync(d_enc.p, enc.data(), (size_t)n * sizeof(i32), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_len.p, hlen.data(), (size_t)n * sizeof(V), hipMemcpyHostToDevice, g_stream));
    const i64 cap = SV_LDS_BYTES / (i64)sizeof(V) - 1;          // the largest n whose n + 1 cells fit
    const i64 lds_n = std::max<i64>(0, std::min<i64>(tune_get("sort_verdict_lds_n", SV_LDS_DEFAULT_BYTES / (i64)sizeof(V) - 1), cap));
    const bool lds = n <= lds_n;
    const size_t bytes = ((size_t)n + 1) * sizeof(V);
    if (lds) {
        HHX_TRY((raise_dynamic_lds<k_sv_rotations<V, true>>(SV_LDS_BYTES)));
        KTimer kt("sort_verdict");
        k_sv_rotations<V, true><<<(unsigned)R, SV_T, bytes, g_stream>>>(n, n_pos, d_enc.p, d_len.p, r0, r1, nullptr, d_sums.p);
        HHX_LAUNCH_CHECK();
    } else {
        const i64 grid = std::min<i64>(R, std::max<i64>(1, std::min<i64>(SV_SCRATCH_BYTES / (i64)bytes, SV_HBM_GRID)));
        if (scratch.alloc((size_t)grid * ((size_t)n + 1))) return 1;
        KTimer kt("sort_verdict");
        k_sv_rotations<V, false><<<(unsigned)grid, SV_T, 0, g_stream>>>(n, n_pos, d_enc.p, d_len.p, r0, r1, scratch.p, d_sums.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(sums, d_sums.p, (size_t)R * sizeof(i64), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));                   // enc, hlen and the caller's arrays
    if (stats) {
        stats[lds ? 0 : 1] = R;
        stats[2] = (i64)sizeof(V);
    }
    return 0;
}

extern "C" int hhx_sort_verdict_sums(int32_t n, const int32_t *value, const int64_t *len, int32_t r0, int32_t r1, int64_t *sums, int64_t *stats) {
    if (stats) for (int k = 0; k < HHX_SORT_VERDICT_N_STATS; ++k) stats[k] = 0;
    if (n < 2) return fail("hhx_sort_verdict_sums: n = %d (two contigs at least: a tour of one has no rotation to look at)", n);
    if (n > SV_MAX_N) {
        fail("hhx_sort_verdict_sums: n = %d is beyond the %d contigs served", n, SV_MAX_N);
        return HHX_UNSUPPORTED;
    }
    if (!value || !len) return fail("hhx_sort_verdict_sums: null value or len");
    if (r0 < 0 || r1 < r0 || r1 > n - 1) return fail("hhx_sort_verdict_sums: rotations [%d, %d) outside [0, %d)", r0, r1, n - 1);
    if (r1 > r0 && !sums) return fail("hhx_sort_verdict_sums: null sums");
    std::vector<i32> at((size_t)n, -1), enc((size_t)n);
    u64 total = 0;
    for (i32 i = 0; i < n; ++i) {
        const i64 v = value[i], p = (v < 0 ? -v : v) - 1;
        if (v == 0 || p >= n) return fail("hhx_sort_verdict_sums: value[%d] = %lld (a signed position, 1 .. %d in magnitude)", i, (long long)v, n);
        if (at[p] >= 0) return fail("hhx_sort_verdict_sums: position %lld is taken by elements %d and %d", (long long)p + 1, at[p], i);
        at[p] = i;
        if (len[i] < 0) return fail("hhx_sort_verdict_sums: len[%d] = %lld", i, (long long)len[i]);
        if ((u64)len[i] >= 1ull << 62 || (total += (u64)len[i]) >= 1ull << 62) return fail("hhx_sort_verdict_sums: the lengths sum to 2^62 or more");
    }
    i32 n_pos = 0, n_neg = 0;
    for (i32 p = 0; p < n; ++p)
        if (value[at[p]] > 0) enc[at[p]] = n_pos++;
    for (i32 p = n - 1; p >= 0; --p)
        if (value[at[p]] < 0) enc[at[p]] = (i32)((u32)n_neg++ | SV_NEG);
    if (r1 == r0) return 0;
    return total < 1ull << 32 ? sv_run<u32>(n, n_pos, enc, len, r0, r1, sums, stats) : sv_run<u64>(n, n_pos, enc, len, r0, r1, sums, stats);
}

// ---------------------------------------------------------------- `haphic refsort`: both LIS sums of many sequences (HapHiC_refsort.py find_lis :175-214)
// The same wave step as k_sv_rotations on a batch: one wavefront per (sequence, class), a job.  The forward class of a sequence is its elements with
// value >= 0, the reverse class those with value <= 0 (:182-185); inside a class an element whose value stood earlier in the sequence is dropped
// (:186-187) and the rest are ranked by ascending signed value, so "strictly increasing" is "rank below" and a job owns one tree of m + 1 cells, m its
// kept elements.  Ranking and dropping repeats are done HERE, by the entry's host code (a sort of each class; the kernel sees ranks and weights only):
// neither on the device nor by the caller.  The tree of a job lives in LDS up to the seam of hhx_sort_verdict_sums (the same knob
// "sort_verdict_lds_n", the same 4-byte cells while every sequence's weights sum to less than 2^32 and 8-byte cells otherwise) and in a
// per-workgroup slab of HBM scratch above it; the jobs of either form are taken grid-stride by one launch each.
template <class V, bool LDS>
static __global__ __launch_bounds__(SV_T) void k_lis_jobs(i32 n_jobs, const i32 *__restrict__ job, const i64 *__restrict__ jptr, const i32 *__restrict__ rank,
                                                         const V *__restrict__ len, i64 slab_cells, V *scratch, i64 *__restrict__ sums) {
    extern __shared__ __align__(8) unsigned char sv_lds[];
    V *T = LDS ? (V *)sv_lds : scratch + (i64)blockIdx.x * slab_cells;
    const int lane = threadIdx.x;
    const u32 below = (1u << (lane & 31)) - 1u;
    const bool low = lane < 32;
    for (i32 jj = (i32)blockIdx.x; jj < n_jobs; jj += (i32)gridDim.x) {
        const i32 j = job[jj];
        const i64 a = jptr[j];
        const i32 m = (i32)(jptr[j + 1] - a);
        for (i32 k = lane; k <= m; k += SV_T) T[k] = 0;
        if (LDS) __builtin_amdgcn_wave_barrier();
        else __syncthreads();
        V best = 0;
        for (i32 k0 = 0; k0 < m; k0 += SV_T) {
            const i32 idx = k0 + lane;
            const i32 my_q = idx < m ? rank[a + idx] : 0;
            const V my_w = idx < m ? len[a + idx] : (V)0;
            const int cnt = min(SV_T, m - k0);
            for (int t = 0; t < cnt; ++t) {
                const u32 q = (u32)sv_lane(my_q, t);          // 0-based rank: the query is the prefix of q cells, the update cell q + 1
                const V w = sv_lane(my_w, t);
                const u32 un = q | below;
                const bool ask = low && ((q >> (lane & 31)) & 1u);
                const bool upd = low && (lane == 0 || !((q >> ((lane - 1) & 31)) & 1u)) && un < (u32)m;
                V mx = ask ? T[q & ~below] : (V)0;
                const V old = upd ? T[un + 1] : (V)0;
                mx = sv_max32(mx);
                const V dp = mx + w;
                if (upd) T[un + 1] = sv_mx(old, dp);
                best = sv_mx(best, dp);
                if (LDS) __builtin_amdgcn_wave_barrier();
                else __syncthreads();
            }
        }
        if (lane == 0) sums[j] = (i64)best;
    }
}

template <class V>
static int lis_run(const std::vector<i64> &jptr, const std::vector<i32> &rank, const std::vector<i64> &w64, std::vector<i64> &sums) {
    const i32 n_jobs = (i32)jptr.size() - 1;
    const i64 cap = SV_LDS_BYTES / (i64)sizeof(V) - 1;
    const i64 lds_n = std::max<i64>(0, std::min<i64>(tune_get("sort_verdict_lds_n", SV_LDS_DEFAULT_BYTES / (i64)sizeof(V) - 1), cap));
    std::vector<i32> jobs[2];                                   // 0: LDS, 1: HBM
    i64 m_max[2] = {0, 0};
    for (i32 j = 0; j < n_jobs; ++j) {
        const i64 m = jptr[(size_t)j + 1] - jptr[(size_t)j];
        if (m == 0) continue;                                    // an empty class: 0 (:192-193)
        const int form = m <= lds_n ? 0 : 1;
        jobs[form].push_back(j);
        m_max[form] = std::max(m_max[form], m);
    }
    if (jobs[0].empty() && jobs[1].empty()) return 0;
    std::vector<V> hw(w64.size());
    for (size_t i = 0; i < w64.size(); ++i) hw[i] = (V)w64[i];
    DevBuf<i64> d_jptr, d_sums;
    DevBuf<i32> d_rank, d_jobs[2];
    DevBuf<V> d_w, scratch;
    if (d_jptr.alloc(jptr.size()) || d_sums.alloc((size_t)n_jobs) || d_rank.alloc(rank.size()) || d_w.alloc(hw.size())) return 1;
    HHX_HIP(hipMemcpyAsync(d_jptr.p, jptr.data(), jptr.size() * sizeof(i64), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_rank.p, rank.data(), rank.size() * sizeof(i32), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(d_w.p, hw.data(), hw.size() * sizeof(V), hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemsetAsync(d_sums.p, 0, (size_t)n_jobs * sizeof(i64), g_stream));
    for (int form = 0; form < 2; ++form) {
        if (jobs[form].empty()) continue;
        if (d_jobs[form].alloc(jobs[form].size())) return 1;
        HHX_HIP(hipMemcpyAsync(d_jobs[form].p, jobs[form].data(), jobs[form].size() * sizeof(i32), hipMemcpyHostToDevice, g_stream));
    }
    if (!jobs[0].empty()) {
        HHX_TRY((raise_dynamic_lds<k_lis_jobs<V, true>>(SV_LDS_BYTES)));
        const i64 grid = std::min<i64>((i64)jobs[0].size(), (i64)1 << 20);
        KTimer kt("lis_sums");
        k_lis_jobs<V, true><<<(unsigned)grid, SV_T, ((size_t)m_max[0] + 1) * sizeof(V), g_stream>>>((i32)jobs[0].size(), d_jobs[0].p, d_jptr.p, d_rank.p,
                                                                                                     d_w.p, 0, nullptr, d_sums.p);
        HHX_LAUNCH_CHECK();
    }
    if (!jobs[1].empty()) {
        const i64 cells = m_max[1] + 1, bytes = cells * (i64)sizeof(V);
        const i64 grid = std::min<i64>((i64)jobs[1].size(), std::max<i64>(1, std::min<i64>(SV_SCRATCH_BYTES / bytes, SV_HBM_GRID)));
        if (scratch.alloc((size_t)(grid * cells))) return 1;
        KTimer kt("lis_sums");
        k_lis_jobs<V, false><<<(unsigned)grid, SV_T, 0, g_stream>>>((i32)jobs[1].size(), d_jobs[1].p, d_jptr.p, d_rank.p, d_w.p, cells, scratch.p, d_sums.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(sums.data(), d_sums.p, (size_t)n_jobs * sizeof(i64), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

static int lis_unsupported(const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return HHX_UNSUPPORTED;
}

extern "C" int hhx_lis_sums(int64_t n_seq, const int64_t *ptr, const int64_t *value, const int64_t *len, int64_t *sums_f, int64_t *sums_r) {
    if (n_seq < 0 || (n_seq && (!ptr || !sums_f || !sums_r))) return fail("hhx_lis_sums: bad argument");
    if (n_seq == 0) return 0;
    if (n_seq >= (i64)1 << 30) return lis_unsupported("hhx_lis_sums: %lld sequences", (long long)n_seq);
    if (ptr[0] != 0) return fail("hhx_lis_sums: ptr[0] = %lld", (long long)ptr[0]);
    for (i64 s = 0; s < n_seq; ++s) {
        if (ptr[s + 1] < ptr[s]) return fail("hhx_lis_sums: ptr runs backwards at sequence %lld", (long long)s);
        if (ptr[s + 1] - ptr[s] > SV_MAX_N)
            return lis_unsupported("hhx_lis_sums: sequence %lld has %lld elements, beyond the %d served", (long long)s, (long long)(ptr[s + 1] - ptr[s]), SV_MAX_N);
    }
    if (ptr[n_seq] && (!value || !len)) return fail("hhx_lis_sums: null value or len");
    bool wide = false;
    for (i64 s = 0; s < n_seq; ++s) {
        u64 total = 0;
        for (i64 i = ptr[s]; i < ptr[s + 1]; ++i) {
            if (len[i] <= 0) return lis_unsupported("hhx_lis_sums: len[%lld] = %lld (a weight is positive)", (long long)i, (long long)len[i]);
            if ((u64)len[i] >= 1ull << 62 || (total += (u64)len[i]) >= 1ull << 62)
                return lis_unsupported("hhx_lis_sums: the weights of sequence %lld sum to 2^62 or more", (long long)s);
        }
        wide = wide || total >= 1ull << 32;
    }
    // job 2 s: the forward class of sequence s, job 2 s + 1: its reverse class; kept elements in sequence order with their rank
    std::vector<i64> jptr(1, 0), w;
    std::vector<i32> rank;
    std::vector<std::pair<i64, i32>> order;                      // (value, position among the kept)
    for (i64 s = 0; s < n_seq; ++s)
        for (int cls = 0; cls < 2; ++cls) {
            order.clear();
            for (i64 i = ptr[s]; i < ptr[s + 1]; ++i)
                if (cls == 0 ? value[i] >= 0 : value[i] <= 0) order.emplace_back(value[i], (i32)(i - ptr[s]));
            std::sort(order.begin(), order.end());               // equal values: the earliest first, the others are the repeats
            const size_t at = rank.size();
            std::vector<std::pair<i32, i32>> kept;               // (position, rank)
            i32 r = 0;
            for (size_t k = 0; k < order.size(); ++k)
                if (k == 0 || order[k].first != order[k - 1].first) kept.emplace_back(order[k].second, r++);
            std::sort(kept.begin(), kept.end());
            rank.resize(at + kept.size());
            w.resize(at + kept.size());
            for (size_t k = 0; k < kept.size(); ++k) {
                rank[at + k] = kept[k].second;
                w[at + k] = len[ptr[s] + kept[k].first];
            }
            jptr.push_back((i64)rank.size());
        }
    std::vector<i64> sums((size_t)(2 * n_seq), 0);
    HHX_TRY(wide ? lis_run<u64>(jptr, rank, w, sums) : lis_run<u32>(jptr, rank, w, sums));
    for (i64 s = 0; s < n_seq; ++s) {
        sums_f[s] = sums[(size_t)(2 * s)];
        sums_r[s] = sums[(size_t)(2 * s + 1)];
    }
    return 0;
}
