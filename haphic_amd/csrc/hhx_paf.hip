// The PAF reader of `haphic refsort`: parse_paf, scripts/HapHiC_refsort.py:81-134.
//
// reference, per line of the text file (universal newlines: '\n', '\r\n' and a lone '\r' end a line):
//       if not line.strip(): continue; cols = line.split()                             :88-90
//       int(cols[11]), cols[0], int(cols[2]), int(cols[3]), cols[5], cols[4] == '+', int(cols[7]), int(cols[8])   :91-107
// A line of `minimap2 -c` carries a cg:Z: tag of kilobytes to megabytes behind field 11 and the reference cuts all of it into Python strings.  No lane
// walks a line here.  The whole text lies in HBM in one piece.  A FIELD START is a byte that is no whitespace and whose left neighbour is whitespace
// (or the start of the text); line breaks are whitespace, so the field starts of the FILE, numbered from 0, are the fields of its lines one after
// the other: field j of a line is field start g0 + j of the file, g0 being the number of field starts in front of the line, and the line has
// g0(next line) - g0 fields.  Passes:
//   1. k_paf_count: per TX_BLOCK (4 KB) block the line breaks, the field starts and whether any byte is >= 0x80 (16 bytes per lane); both counts scanned;
//   2. k_write_starts (hhx_textscan.h): the line starts;
//   3. k_paf_line_fields, one wave per line: g0 of every line (the scanned count of its block + at most TX_BLOCK / WAVE_STEP wave steps inside it);
//      k_paf_mark / k_paf_compact: the lines with a field (not blank under line.strip()), scanned and compacted into the list of records;
//   4. k_paf_fields, one wave per record: field starts g0 + {0, 2, 3, 4, 5, 7, 8, 11} by select_field() — a binary search in the scanned block counts
//      and a wave scan inside the one block, the same ~17 probes behind a tag of 3 MB as behind one of 30 bytes — then lane j reads its field: a name up
//      to NAME_BYTES_MAX bytes, an integer of 1..DIGITS_MAX digits that the next whitespace (or the end of the text) ends, or the one byte '+'.
//      Fields 1, 6, 9, 10 and everything behind field 11 are never looked at;
//   5. the name table: the 2 n_rec names (query, target, query, ...) go into an open-addressing table keyed by their bytes; a slot keeps the SMALLEST
//      index among the equal names that met in it (compare-and-swap to claim, min to settle, bytes compared before either), so the names number in
//      first-seen order whatever order the lanes ran in: k_paf_insert, k_paf_unique, scan, k_paf_ids, scan of the lengths, k_paf_names.
// One read of the text in pass 1, one in pass 2; passes 3-5 touch a few cache lines per line.  What leaves the device is the table.
// Ranking and repeat handling of the LIS step live in hhx_sortverdict.hip (hhx_lis_sums), not here.
#include <sys/stat.h>

#include <memory>

#include "hhx_internal.h"
#include "hhx_textscan.h"

using namespace hhx;
using namespace hhx::textscan;

namespace {

constexpr int SLACK = 64;                      // readable bytes behind the text
constexpr int WAVE_STEP = HHX_WAVE * 16;       // bytes a wave looks at per step inside a block
constexpr int NAME_BYTES_MAX = 255;
constexpr int DIGITS_MAX = 18;                 // below 10^18 < 2^63
constexpr int N_WANTED = 8;                    // fields 0, 2, 3, 4, 5, 7, 8, 11
constexpr int N_INTS = 5;                      // fields 2, 3, 7, 8, 11
constexpr int N_FIELDS_MIN = 12;
// device bytes per line at most: starts, g0, rec, rid, rec_line (40), name_at, name_len (32), vals (40), plus (1), the slot table (at most 8 slots
// of 8 bytes), slot_of, uniq, uid (48), ids (8), u_at, u_len, name_off (48), the names themselves counted with the text
constexpr double TABLE_BYTES_PER_LINE = 288;

enum { E_FIELDS = 1, E_NAME0 = 2, E_NAME5 = 3, E_INT = 4 /* + slot 0..4 */, E_NONE = 15 };
constexpr unsigned long long NO_ERROR = ~0ull;
constexpr unsigned long long EMPTY = ~0ull;

// workgroups of every pass at most (HHX_PAF_GRID, read at every launch: the tests walk the grid-stride loops on 1 and 2 workgroups)
inline unsigned paf_grid(i64 work, int per_block) {
    const unsigned g = grid_for(work, per_block);
    const char *e = getenv("HHX_PAF_GRID");
    const long long cap = e ? atoll(e) : 0;
    return cap > 0 && (unsigned long long)cap < g ? (unsigned)cap : g;
}

// bit k set: byte base + k begins a field (base a multiple of 16, base < n; t is 16-byte aligned with SLACK readable bytes behind n).  *high collects
// the bytes' 0x80 bits
__device__ __forceinline__ u32 field_mask16(const unsigned char *__restrict__ t, i64 base, i64 n, u32 *high) {
    u32 ws = 0, h = 0, valid = 0xffffu;
    if (base + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(t + base);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        h = v.x | v.y | v.z | v.w;
#pragma unroll
        for (int k = 0; k < 16; ++k) ws |= (u32)is_ws((unsigned char)((w[k >> 2] >> (8 * (k & 3))) & 0xffu)) << k;
    } else {
        valid = (1u << (int)(n - base)) - 1u;
        for (int k = 0; base + k < n; ++k) {
            const unsigned char c = t[base + k];
            h |= c;
            ws |= (u32)is_ws(c) << k;
        }
    }
    if (high) *high |= h & 0x80808080u;
    const u32 left = (ws << 1) | (u32)(base == 0 || is_ws(t[base - 1]));
    return ~ws & left & valid;
}

__global__ __launch_bounds__(256) void k_paf_count(const unsigned char *__restrict__ t, i64 n, i64 n_blocks, i64 *__restrict__ breaks, i64 *__restrict__ fields,
                                                   u32 *__restrict__ flag) {
    __shared__ i32 ws[2][4];
    const bool aligned = ((uintptr_t)t & 15) == 0;
    u32 high = 0;
    for (i64 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const i64 base = b * TX_BLOCK + (i64)threadIdx.x * 16;
        i32 cb = __popc(break_mask(t, base, n, aligned)), cf = base < n ? __popc(field_mask16(t, base, n, &high)) : 0;
        cb = wave_sum_i32(cb);
        cf = wave_sum_i32(cf);
        if (lane_id() == 0) { ws[0][threadIdx.x / HHX_WAVE] = cb; ws[1][threadIdx.x / HHX_WAVE] = cf; }
        __syncthreads();
        if (threadIdx.x == 0) {
            breaks[b] = (i64)ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
            fields[b] = (i64)ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
        }
        __syncthreads();
    }
    if (high) flag[0] = 1;
}

// field starts of the file in front of byte p (p <= n), by the whole wave
__device__ __forceinline__ i64 fields_before(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ pre_f, i64 n_blocks, i64 p) {
    if (p >= n) return pre_f[n_blocks];
    const i64 b = p / TX_BLOCK;
    i32 c = 0;
    for (i64 base = b * TX_BLOCK + (i64)lane_id() * 16; base < p; base += WAVE_STEP) {
        u32 m = field_mask16(t, base, n, nullptr);
        if (p - base < 16) m &= (1u << (int)(p - base)) - 1;
        c += __popc(m);
    }
    return pre_f[b] + wave_sum_i32(c);
}

// the position of field start g of the file (g < pre_f[n_blocks]), by the whole wave; g is the same in every lane
__device__ __forceinline__ i64 select_field(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ pre_f, i64 n_blocks, i64 g) {
    i64 lo = 0, hi = n_blocks - 1;                               // the last block with pre_f[b] <= g: pre_f[b + 1] > g, the field start lies in it
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (pre_f[mid] <= g) lo = mid; else hi = mid - 1;
    }
    i32 r = (i32)(g - pre_f[lo]);
    for (int s = 0; s < TX_BLOCK / WAVE_STEP; ++s) {
        const i64 base = lo * TX_BLOCK + (i64)s * WAVE_STEP + (i64)lane_id() * 16;
        u32 m = base < n ? field_mask16(t, base, n, nullptr) : 0;
        const i32 c = __popc(m);
        i32 incl = c;
#pragma unroll
        for (int o = 1; o < HHX_WAVE; o <<= 1) {
            const i32 v = __shfl_up(incl, o, HHX_WAVE);
            if (lane_id() >= o) incl += v;
        }
        const i32 tot = __shfl(incl, HHX_WAVE - 1, HHX_WAVE);
        if (r < tot) {
            const bool hit = r >= incl - c && r < incl;          // one lane
            i64 pos = 0;
            if (hit) {
                for (int q = r - (incl - c); q > 0; --q) m &= m - 1;
                pos = base + __ffs(m) - 1;
            }
            const int src = __ffsll((unsigned long long)__ballot(hit)) - 1;
            return __shfl(pos, src, HHX_WAVE);
        }
        r -= tot;
    }
    return n;                                                    // (the counts of pass 1 say it is there)
}

// one wave per line: g0[k] = field starts in front of line k; g0[n_lines] = all of them
__global__ __launch_bounds__(256) void k_paf_line_fields(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ starts, i64 n_lines,
                                                         const i64 *__restrict__ pre_f, i64 n_blocks, i64 *__restrict__ g0) {
    const i64 n_waves = (i64)gridDim.x * (256 / HHX_WAVE);
    for (i64 k = (i64)blockIdx.x * (256 / HHX_WAVE) + threadIdx.x / HHX_WAVE; k <= n_lines; k += n_waves) {
        const i64 v = k < n_lines ? fields_before(t, n, pre_f, n_blocks, starts[k]) : pre_f[n_blocks];
        if (lane_id() == 0) g0[k] = v;
    }
}

__global__ __launch_bounds__(256) void k_paf_mark(const i64 *__restrict__ g0, i64 n_lines, i64 *__restrict__ rec) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n_lines; k += (i64)gridDim.x * blockDim.x) rec[k] = g0[k + 1] > g0[k];
}

__global__ __launch_bounds__(256) void k_paf_compact(const i64 *__restrict__ rec, const i64 *__restrict__ rid, i64 n_lines, i64 *__restrict__ rec_line) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n_lines; k += (i64)gridDim.x * blockDim.x)
        if (rec[k]) rec_line[rid[k]] = k;
}

// one wave per record.  name_at / name_len [2 n_rec]: fields 0 and 5 of record r at 2 r and 2 r + 1; vals [N_INTS n_rec]: fields 2, 3, 7, 8, 11 of
// record r at slot * n_rec + r; plus[r]: field 4 is exactly "+".  err: the smallest (line << 4 | reason) of the records that are not served
__global__ __launch_bounds__(256) void k_paf_fields(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ g0, const i64 *__restrict__ rec_line,
                                                    i64 n_rec, const i64 *__restrict__ pre_f, i64 n_blocks, i64 *__restrict__ name_at,
                                                    i64 *__restrict__ name_len, i64 *__restrict__ vals, unsigned char *__restrict__ plus,
                                                    unsigned long long *__restrict__ err) {
    const i64 n_waves = (i64)gridDim.x * (256 / HHX_WAVE);
    const int lane = lane_id();
    for (i64 r = (i64)blockIdx.x * (256 / HHX_WAVE) + threadIdx.x / HHX_WAVE; r < n_rec; r += n_waves) {
        const i64 k = rec_line[r], g = g0[k];
        int code = E_NONE;
        i64 my = n, out = 0;
        if (g0[k + 1] - g < N_FIELDS_MIN) {
            code = E_FIELDS;
        } else {
            const int want[N_WANTED] = {0, 2, 3, 4, 5, 7, 8, 11};
#pragma unroll
            for (int j = 0; j < N_WANTED; ++j) {
                const i64 p = select_field(t, n, pre_f, n_blocks, g + want[j]);
                if (lane == j) my = p;
            }
            if (lane == 0 || lane == 4) {                        // a name: up to the next whitespace
                i64 q = my;
                while (q < n && !is_ws(t[q]) && q - my <= NAME_BYTES_MAX) ++q;
                out = q - my;
                if (out > NAME_BYTES_MAX) code = lane == 0 ? E_NAME0 : E_NAME5;
            } else if (lane == 3) {
                out = my < n && t[my] == '+' && (my + 1 >= n || is_ws(t[my + 1]));
            } else if (lane < N_WANTED) {                        // an integer: 1..DIGITS_MAX digits and nothing else
                u64 v = 0;
                int nd = 0;
                i64 q = my;
                while (q < n && t[q] >= '0' && t[q] <= '9' && nd <= DIGITS_MAX) { v = v * 10 + (u64)(t[q] - '0'); ++nd; ++q; }
                out = (i64)v;
                if (nd == 0 || nd > DIGITS_MAX || (q < n && !is_ws(t[q]))) code = E_INT + (lane < 3 ? lane - 1 : lane - 3);
            }
        }
        int worst = code;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) worst = min(worst, __shfl_xor(worst, o, HHX_WAVE));
        const bool ok = worst == E_NONE;
        if (lane == 0) {
            name_at[2 * r] = my;
            name_len[2 * r] = ok ? out : 0;
            if (!ok) atomicMin(err, ((unsigned long long)k << 4) | (unsigned long long)worst);
        } else if (lane == 4) {
            name_at[2 * r + 1] = my;
            name_len[2 * r + 1] = ok ? out : 0;
        } else if (lane == 3) {
            plus[r] = (unsigned char)(ok ? out : 0);
        } else if (lane < N_WANTED) {
            vals[(i64)(lane < 3 ? lane - 1 : lane - 3) * n_rec + r] = ok ? out : 0;
        }
    }
}

__device__ __forceinline__ bool same_bytes(const unsigned char *__restrict__ t, i64 a, i64 b, i64 m) {
    for (i64 q = 0; q < m; ++q)
        if (t[a + q] != t[b + q]) return false;
    return true;
}

// slot[s]: the smallest index of the names that met in slot s (EMPTY: none); slot_of[i]: where name i went
__global__ __launch_bounds__(256) void k_paf_insert(const unsigned char *__restrict__ t, const i64 *__restrict__ name_at, const i64 *__restrict__ name_len,
                                                    i64 n_names, unsigned long long *slot, u64 mask, i64 *__restrict__ slot_of) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_names; i += (i64)gridDim.x * blockDim.x) {
        const i64 a = name_at[i], m = name_len[i];
        u64 h = HASH_SEED;
        for (i64 q = 0; q < m; ++q) h = hash_step(h, t[a + q]);
        u64 s = h & mask;
        for (;;) {
            unsigned long long cur = __hip_atomic_load(&slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == EMPTY) {
                cur = atomicCAS(&slot[s], EMPTY, (unsigned long long)i);
                if (cur == EMPTY) break;
            }
            // whoever holds the slot now or later has the bytes of `cur`: a slot only ever changes hands among equal names
            if (name_len[cur] == m && same_bytes(t, a, name_at[cur], m)) {
                atomicMin(&slot[s], (unsigned long long)i);
                break;
            }
            s = (s + 1) & mask;
        }
        slot_of[i] = (i64)s;
    }
}

__global__ __launch_bounds__(256) void k_paf_unique(const unsigned long long *__restrict__ slot, const i64 *__restrict__ slot_of, i64 n_names,
                                                    i64 *__restrict__ uniq) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_names; i += (i64)gridDim.x * blockDim.x) uniq[i] = slot[slot_of[i]] == (unsigned long long)i;
}

__global__ __launch_bounds__(256) void k_paf_ids(const unsigned long long *__restrict__ slot, const i64 *__restrict__ slot_of, const i64 *__restrict__ uid,
                                                 const i64 *__restrict__ name_at, const i64 *__restrict__ name_len, i64 n_names, i32 *__restrict__ id,
                                                 i64 *__restrict__ u_at, i64 *__restrict__ u_len) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_names; i += (i64)gridDim.x * blockDim.x) {
        const i64 first = (i64)slot[slot_of[i]], u = uid[first];
        id[i] = (i32)u;
        if (first == i) { u_at[u] = name_at[i]; u_len[u] = name_len[i]; }
    }
}

__global__ __launch_bounds__(256) void k_paf_names(const unsigned char *__restrict__ t, const i64 *__restrict__ u_at, const i64 *__restrict__ name_off,
                                                   i64 n_uniq, unsigned char *__restrict__ out) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n_uniq; r += (i64)gridDim.x * blockDim.x) {
        const i64 a = u_at[r], o = name_off[r], m = name_off[r + 1] - o;
        for (i64 q = 0; q < m; ++q) out[o + q] = t[a + q];
    }
}

int unsupported(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return HHX_UNSUPPORTED;
}

int fits(i64 n, const char *who) {
    size_t free_b = 0, total_b = 0;
    HHX_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((double)n > (double)total_b / 2)
        return unsupported("%s: %lld bytes of text do not fit in half of the device's memory (%lld bytes)", who, (long long)n, (long long)total_b);
    return 0;
}

}  // namespace

struct hhx_paf {
    i64 n_rec = 0, n_names = 0;
    std::vector<i64> name_off, vals;            // vals: fields 2, 3, 7, 8, 11, n_rec of each
    std::vector<i32> ids;                       // query, target, query, ...
    std::vector<unsigned char> names, plus;
};

namespace {

// t[0, n) is the text, with SLACK bytes behind it
int parse(hhx_paf *g, const unsigned char *t, i64 n) {
    g->name_off.assign(1, 0);
    if (n == 0) return 0;
    const i64 n_blocks = (n + TX_BLOCK - 1) / TX_BLOCK;
    DevBuf<u32> flag;
    DevBuf<unsigned long long> err;
    DevBuf<i64> cnt_b, cnt_f, pre_b, pre_f, starts;
    if (flag.alloc(1) || err.alloc(1) || cnt_b.alloc((size_t)n_blocks) || cnt_f.alloc((size_t)n_blocks) || pre_b.alloc((size_t)n_blocks + 1) ||
        pre_f.alloc((size_t)n_blocks + 1)) return 1;
    HHX_HIP(hipMemsetAsync(flag.p, 0, sizeof(u32), g_stream));
    HHX_HIP(hipMemsetAsync(err.p, 0xff, sizeof(unsigned long long), g_stream));
    { KTimer kt("paf_count");
    k_paf_count<<<paf_grid(n_blocks, 1), 256, 0, g_stream>>>(t, n, n_blocks, cnt_b.p, cnt_f.p, flag.p); }
    HHX_LAUNCH_CHECK();
    i64 n_breaks = 0, n_fields = 0;
    HHX_TRY(exclusive_scan_i64(cnt_b.p, pre_b.p, n_blocks, &n_breaks));
    HHX_TRY(exclusive_scan_i64(cnt_f.p, pre_f.p, n_blocks, &n_fields));
    u32 high = 0;
    HHX_HIP(hipMemcpyAsync(&high, flag.p, sizeof high, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (high) return unsupported("hhx_paf: the text holds a byte >= 0x80 (the reference decodes it by the locale)");
    if (n_fields == 0) return 0;
    {                                                            // the tables of the passes below: up to TABLE_BYTES_PER_LINE per line, beside the text
        size_t free_b = 0, total_b = 0;
        HHX_HIP(hipMemGetInfo(&free_b, &total_b));
        if ((double)(n_breaks + 1) * TABLE_BYTES_PER_LINE > (double)total_b / 2 - (double)n)
            return unsupported("hhx_paf: the tables of %lld lines do not fit beside the text in half of the device's memory (%lld bytes)",
                               (long long)(n_breaks + 1), (long long)total_b);
    }
    if (starts.alloc((size_t)n_breaks + 2)) return 1;
    { KTimer kt("paf_starts");
    k_write_starts<<<paf_grid(n_blocks, 1), 256, 0, g_stream>>>(t, n, n_blocks, pre_b.p, starts.p); }
    HHX_LAUNCH_CHECK();

    const i64 n_lines = n_breaks + 1;                            // the last one may be empty
    DevBuf<i64> g0, rec, rid, rec_line;
    if (g0.alloc((size_t)n_lines + 1) || rec.alloc((size_t)n_lines) || rid.alloc((size_t)n_lines + 1)) return 1;
    { KTimer kt("paf_lines", 2);
    k_paf_line_fields<<<paf_grid(n_lines + 1, 256 / HHX_WAVE), 256, 0, g_stream>>>(t, n, starts.p, n_lines, pre_f.p, n_blocks, g0.p);
    k_paf_mark<<<paf_grid(n_lines, 256), 256, 0, g_stream>>>(g0.p, n_lines, rec.p); }
    HHX_LAUNCH_CHECK();
    i64 n_rec = 0;
    HHX_TRY(exclusive_scan_i64(rec.p, rid.p, n_lines, &n_rec));
    if (n_rec == 0) return 0;
    if (2 * n_rec >= (i64)1 << 31) return unsupported("hhx_paf: %lld lines (the name ids are 32 bits)", (long long)n_rec);
    const i64 n_tok = 2 * n_rec;
    DevBuf<i64> name_at, name_len, vals;
    DevBuf<unsigned char> plus;
    if (rec_line.alloc((size_t)n_rec) || name_at.alloc((size_t)n_tok) || name_len.alloc((size_t)n_tok) || vals.alloc((size_t)(N_INTS * n_rec)) ||
        plus.alloc((size_t)n_rec)) return 1;
    { KTimer kt("paf_lines");
    k_paf_compact<<<paf_grid(n_lines, 256), 256, 0, g_stream>>>(rec.p, rid.p, n_lines, rec_line.p); }
    HHX_LAUNCH_CHECK();
    { KTimer kt("paf_fields");
    k_paf_fields<<<paf_grid(n_rec, 256 / HHX_WAVE), 256, 0, g_stream>>>(t, n, g0.p, rec_line.p, n_rec, pre_f.p, n_blocks, name_at.p, name_len.p, vals.p,
                                                                         plus.p, err.p); }
    HHX_LAUNCH_CHECK();
    unsigned long long first = NO_ERROR;
    HHX_HIP(hipMemcpyAsync(&first, err.p, sizeof first, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (first != NO_ERROR) {
        const long long line = (long long)(first >> 4) + 1;
        const int code = (int)(first & 15);
        static const int int_field[N_INTS] = {2, 3, 7, 8, 11};
        if (code == E_FIELDS) return unsupported("hhx_paf: line %lld: fewer than %d fields (the reference raises IndexError)", line, N_FIELDS_MIN);
        if (code == E_NAME0 || code == E_NAME5)
            return unsupported("hhx_paf: line %lld: field %d is a name longer than %d bytes", line, code == E_NAME0 ? 0 : 5, NAME_BYTES_MAX);
        return unsupported("hhx_paf: line %lld: field %d is not 1 to %d digits (Python's int() decides)", line, int_field[code - E_INT], DIGITS_MAX);
    }

    u64 cap = 16;
    while (cap < 2 * (u64)n_tok + 2) cap <<= 1;
    DevBuf<unsigned long long> slot;
    DevBuf<i64> slot_of, uniq, uid, u_at, u_len, name_off;
    DevBuf<i32> ids;
    if (slot.alloc((size_t)cap) || slot_of.alloc((size_t)n_tok) || uniq.alloc((size_t)n_tok) || uid.alloc((size_t)n_tok + 1) || ids.alloc((size_t)n_tok)) return 1;
    HHX_HIP(hipMemsetAsync(slot.p, 0xff, sizeof(unsigned long long) * (size_t)cap, g_stream));
    { KTimer kt("paf_names", 2);
    k_paf_insert<<<paf_grid(n_tok, 256), 256, 0, g_stream>>>(t, name_at.p, name_len.p, n_tok, slot.p, cap - 1, slot_of.p);
    k_paf_unique<<<paf_grid(n_tok, 256), 256, 0, g_stream>>>(slot.p, slot_of.p, n_tok, uniq.p); }
    HHX_LAUNCH_CHECK();
    i64 n_uniq = 0, n_name_bytes = 0;
    HHX_TRY(exclusive_scan_i64(uniq.p, uid.p, n_tok, &n_uniq));
    if (u_at.alloc((size_t)n_uniq) || u_len.alloc((size_t)n_uniq) || name_off.alloc((size_t)n_uniq + 1)) return 1;
    { KTimer kt("paf_names");
    k_paf_ids<<<paf_grid(n_tok, 256), 256, 0, g_stream>>>(slot.p, slot_of.p, uid.p, name_at.p, name_len.p, n_tok, ids.p, u_at.p, u_len.p); }
    HHX_LAUNCH_CHECK();
    HHX_TRY(exclusive_scan_i64(u_len.p, name_off.p, n_uniq, &n_name_bytes));
    DevBuf<unsigned char> names;
    if (names.alloc((size_t)n_name_bytes + 1)) return 1;
    { KTimer kt("paf_names");
    k_paf_names<<<paf_grid(n_uniq, 256), 256, 0, g_stream>>>(t, u_at.p, name_off.p, n_uniq, names.p); }
    HHX_LAUNCH_CHECK();
    g->n_rec = n_rec;
    g->n_names = n_uniq;
    g->name_off.resize((size_t)n_uniq + 1);
    g->vals.resize((size_t)(N_INTS * n_rec));
    g->ids.resize((size_t)n_tok);
    g->plus.resize((size_t)n_rec);
    g->names.resize((size_t)n_name_bytes);
    HHX_HIP(hipMemcpyAsync(g->name_off.data(), name_off.p, sizeof(i64) * ((size_t)n_uniq + 1), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(g->vals.data(), vals.p, sizeof(i64) * (size_t)(N_INTS * n_rec), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(g->ids.data(), ids.p, sizeof(i32) * (size_t)n_tok, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(g->plus.data(), plus.p, (size_t)n_rec, hipMemcpyDeviceToHost, g_stream));
    if (n_name_bytes) HHX_HIP(hipMemcpyAsync(g->names.data(), names.p, (size_t)n_name_bytes, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

}  // namespace

extern "C" int hhx_paf_open_bytes(const uint8_t *text, int64_t n_bytes, hhx_paf **out) {
    if (!out || n_bytes < 0 || (n_bytes && !text)) return fail("hhx_paf_open_bytes: bad argument");
    HHX_TRY(fits(n_bytes, "hhx_paf_open_bytes"));
    std::unique_ptr<hhx_paf> g(new hhx_paf());
    DevBuf<unsigned char> t;
    if (t.alloc((size_t)n_bytes + SLACK)) return 1;
    { KTimer kt("paf_h2d");
    if (n_bytes) HHX_HIP(hipMemcpyAsync(t.p, text, (size_t)n_bytes, hipMemcpyHostToDevice, g_stream)); }
    HHX_HIP(hipStreamSynchronize(g_stream));
    HHX_TRY(parse(g.get(), t.p, n_bytes));
    *out = g.release();
    return 0;
}

extern "C" int hhx_paf_open(const char *path, hhx_paf **out) {
    if (!out || !path) return fail("hhx_paf_open: bad argument");
    struct stat sb;
    if (::stat(path, &sb) != 0) return fail("cannot open %s: %s", path, strerror(errno));
    if (!S_ISREG(sb.st_mode)) return unsupported("hhx_paf_open: %s is not a regular file", path);
    const i64 n = (i64)sb.st_size;
    HHX_TRY(fits(n, "hhx_paf_open"));
    std::unique_ptr<hhx_paf> g(new hhx_paf());
    DevBuf<unsigned char> t;
    if (t.alloc((size_t)n + SLACK)) return 1;
    if (n > 0) {                                                 // raw chunks from the pinned read-ahead buffers of the text reader, as they come
        hhx_text_reader *r = nullptr;
        HHX_TRY(hhx_text_reader_open_raw(path, (i64)64 << 20, 4, &r));
        int rc = 0;
        i64 at = 0;
        for (;;) {
            const uint8_t *host = nullptr;
            i64 m = 0;
            if ((rc = hhx_text_reader_next(r, &host, &m)) != 0 || m == 0) break;
            if (at + m > n) { rc = fail("hhx_paf_open: %s grew while it was read", path); break; }
            hipError_t e = hipMemcpyAsync(t.p + at, host, (size_t)m, hipMemcpyHostToDevice, g_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
            if (e != hipSuccess) { rc = fail("hhx_paf_open: %s", hipGetErrorString(e)); break; }
            at += m;
        }
        if (!rc && at != n) rc = fail("hhx_paf_open: %s shrank while it was read", path);
        const std::string err = g_err;
        (void)hhx_text_reader_close(r);
        if (rc) { g_err = err; return rc; }
    }
    HHX_TRY(parse(g.get(), t.p, n));
    *out = g.release();
    return 0;
}

extern "C" int hhx_paf_counts(const hhx_paf *g, int64_t *n_rec, int64_t *n_names, int64_t *n_name_bytes) {
    if (!g) return fail("hhx_paf_counts: null handle");
    if (n_rec) *n_rec = g->n_rec;
    if (n_names) *n_names = g->n_names;
    if (n_name_bytes) *n_name_bytes = g->name_off.back();
    return 0;
}

extern "C" int hhx_paf_table(const hhx_paf *g, int64_t *name_off, uint8_t *names, int32_t *query, int32_t *target, int64_t *query_start,
                             int64_t *query_end, int64_t *target_start, int64_t *target_end, int64_t *mapq, uint8_t *plus) {
    if (!g) return fail("hhx_paf_table: null handle");
    const size_t n = (size_t)g->n_rec;
    if (name_off) memcpy(name_off, g->name_off.data(), sizeof(i64) * ((size_t)g->n_names + 1));
    if (names && !g->names.empty()) memcpy(names, g->names.data(), g->names.size());
    for (size_t r = 0; r < n; ++r) {
        if (query) query[r] = g->ids[2 * r];
        if (target) target[r] = g->ids[2 * r + 1];
    }
    int64_t *const cols[N_INTS] = {query_start, query_end, target_start, target_end, mapq};
    for (int c = 0; c < N_INTS; ++c)
        if (cols[c] && n) memcpy(cols[c], g->vals.data() + (size_t)c * n, sizeof(i64) * n);
    if (plus && n) memcpy(plus, g->plus.data(), n);
    return 0;
}

extern "C" int hhx_paf_close(hhx_paf *g) {
    delete g;
    return 0;
}
