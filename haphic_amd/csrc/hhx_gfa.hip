// The GFA reader of `haphic cluster` / `haphic reassign`: parse_gfa, scripts/HapHiC_cluster.py:150-185.
//
// reference, per line of the text file (universal newlines: '\n', '\r\n' and a lone '\r' end a line):
//       if line.startswith('S\t'): cols = line.split('\t')                             :160-161
//           ctg = cols[1]; ctg_len = int(cols[3].split(':')[-1]); read_depth = int(cols[4].split(':')[-1])   :162-164
// An S line of hifiasm carries the whole sequence of the contig as field 2, so a line is anything between 10 bytes and hundreds of megabytes, and the
// A / L lines behind it come by the million.  No lane walks a line here.  The whole text lies in HBM in one piece.  Passes:
//   1. k_gfa_count: per TX_BLOCK (4 KB) block the line breaks, the TABs and whether any byte is >= 0x80 (16 bytes per lane); both counts are scanned;
//   2. k_write_starts (hhx_textscan.h): the line starts;
//   3. k_gfa_mark / k_gfa_compact: the lines that begin with "S\t", scanned and compacted into the list of records;
//   4. k_gfa_fields, one wave per record: the TABs of a file are numbered by the scan of pass 1, so the TAB that ends field j of a record is TAB
//      g1 + j - 1 of the FILE, g1 being the number of the record's first TAB.  tabs_before() counts the TABs of one block in front of a byte (at most
//      TX_BLOCK / WAVE_STEP wave steps), select_tab() finds TAB g by a binary search in the scanned block counts — a sequence of 300 MB costs the same
//      17 probes as one of 30 bytes — and a wave scan inside the one block that holds it.  A TAB found behind the end of the record's line belongs to
//      a later line: the record has too few fields, and is refused rather than repaired.  The two integers are read backwards from the end of their
//      field: 1..DIGITS_MAX digits, in front of them ':' or the field's start;
//   5. k_gfa_names: the names one after the other.
// One read of the text in pass 1, one in pass 2; passes 3-5 touch a few cache lines per record.  What leaves the device is the table: names, lengths, depths.
#include <sys/stat.h>

#include <memory>

#include "hhx_internal.h"
#include "hhx_textscan.h"

using namespace hhx;
using namespace hhx::textscan;

namespace {

constexpr int SLACK = 64;                      // readable bytes behind the text
constexpr int WAVE_STEP = HHX_WAVE * 16;       // bytes a wave looks at per step inside a block (TX_BLOCK / WAVE_STEP = 4 steps per block)
constexpr int NAME_BYTES_MAX = 255;            // bytes of a name that is served
constexpr int DIGITS_MAX = 18;                 // digits of an integer that is served (below 10^18 < 2^63)

enum { E_FIELDS = 1, E_NAME = 2, E_LEN = 3, E_DEPTH = 4 };
constexpr unsigned long long NO_ERROR = ~0ull;

// workgroups of every pass at most (HHX_GFA_GRID, read at every launch: the tests walk the grid-stride loops on 1 and 2 workgroups)
inline unsigned gfa_grid(i64 work, int per_block) {
    const unsigned g = grid_for(work, per_block);
    const char *e = getenv("HHX_GFA_GRID");
    const long long cap = e ? atoll(e) : 0;
    return cap > 0 && (unsigned long long)cap < g ? (unsigned)cap : g;
}

// bit k set: byte base + k is a TAB (base a multiple of 16, base < n; t is 16-byte aligned with SLACK readable bytes behind n).  *high collects the
// bytes' 0x80 bits
__device__ __forceinline__ u32 tab_mask16(const unsigned char *__restrict__ t, i64 base, i64 n, u32 *high) {
    u32 m = 0, h = 0;
    if (base + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(t + base);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        h = v.x | v.y | v.z | v.w;
#pragma unroll
        for (int k = 0; k < 16; ++k) m |= (u32)(((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == '\t') << k;
    } else {
        for (int k = 0; base + k < n; ++k) {
            const unsigned char c = t[base + k];
            h |= c;
            m |= (u32)(c == '\t') << k;
        }
    }
    if (high) *high |= h & 0x80808080u;
    return m;
}

__global__ __launch_bounds__(256) void k_gfa_count(const unsigned char *__restrict__ t, i64 n, i64 n_blocks, i64 *__restrict__ breaks, i64 *__restrict__ tabs,
                                                   u32 *__restrict__ flag) {
    __shared__ i32 ws[2][4];
    const bool aligned = ((uintptr_t)t & 15) == 0;
    u32 high = 0;
    for (i64 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const i64 base = b * TX_BLOCK + (i64)threadIdx.x * 16;
        i32 cb = __popc(break_mask(t, base, n, aligned)), ct = base < n ? __popc(tab_mask16(t, base, n, &high)) : 0;
        cb = wave_sum_i32(cb);
        ct = wave_sum_i32(ct);
        if (lane_id() == 0) { ws[0][threadIdx.x / HHX_WAVE] = cb; ws[1][threadIdx.x / HHX_WAVE] = ct; }
        __syncthreads();
        if (threadIdx.x == 0) {
            breaks[b] = (i64)ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
            tabs[b] = (i64)ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
        }
        __syncthreads();
    }
    if (high) flag[0] = 1;
}

// line k = [starts[k], starts[k + 1]) (the last one: up to n).  rec[k] = 1: it begins with "S\t"
__global__ __launch_bounds__(256) void k_gfa_mark(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ starts, i64 n_lines, i64 *__restrict__ rec) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n_lines; k += (i64)gridDim.x * blockDim.x) {
        const i64 a = starts[k], e = k + 1 < n_lines ? starts[k + 1] : n;
        rec[k] = a + 1 < e && t[a] == 'S' && t[a + 1] == '\t';
    }
}

__global__ __launch_bounds__(256) void k_gfa_compact(const i64 *__restrict__ rec, const i64 *__restrict__ rid, i64 n_lines, i64 *__restrict__ rec_line) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n_lines; k += (i64)gridDim.x * blockDim.x)
        if (rec[k]) rec_line[rid[k]] = k;
}

// TABs of the file in front of byte p (p < n), by the whole wave: the scanned count of p's block and the TABs of the block in front of p
__device__ __forceinline__ i64 tabs_before(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ pre_t, i64 p) {
    const i64 b = p / TX_BLOCK;
    i32 c = 0;
    for (i64 base = b * TX_BLOCK + (i64)lane_id() * 16; base < p; base += WAVE_STEP) {
        u32 m = tab_mask16(t, base, n, nullptr);
        if (p - base < 16) m &= (1u << (int)(p - base)) - 1;
        c += __popc(m);
    }
    return pre_t[b] + wave_sum_i32(c);
}

// the position of TAB g of the file (n: the file has no such TAB), by the whole wave; g is the same in every lane
__device__ __forceinline__ i64 select_tab(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ pre_t, i64 n_blocks, i64 g) {
    if (g >= pre_t[n_blocks]) return n;
    i64 lo = 0, hi = n_blocks - 1;                               // the last block with pre_t[b] <= g: pre_t[b + 1] > g, the TAB lies in it
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (pre_t[mid] <= g) lo = mid; else hi = mid - 1;
    }
    i32 r = (i32)(g - pre_t[lo]);
    for (int s = 0; s < TX_BLOCK / WAVE_STEP; ++s) {
        const i64 base = lo * TX_BLOCK + (i64)s * WAVE_STEP + (i64)lane_id() * 16;
        u32 m = base < n ? tab_mask16(t, base, n, nullptr) : 0;
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

// int(field.split(':')[-1]) on t[s, e) as far as it is served: 1..DIGITS_MAX digits at the end, in front of them ':' or the field's start
__device__ __forceinline__ bool tail_int(const unsigned char *__restrict__ t, i64 s, i64 e, i64 *out) {
    u64 val = 0, mul = 1;
    int nd = 0;
    i64 q = e;
    while (q > s) {
        const unsigned char c = t[q - 1];
        if (c < '0' || c > '9') break;
        if (nd == DIGITS_MAX) return false;
        val += (u64)(c - '0') * mul;
        mul *= 10;
        ++nd;
        --q;
    }
    if (nd == 0 || (q > s && t[q - 1] != ':')) return false;
    *out = (i64)val;
    return true;
}

// one wave per record.  err: the smallest (line << 3 | reason) of the records that are not served
__global__ __launch_bounds__(256) void k_gfa_fields(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ starts, i64 n_lines,
                                                    const i64 *__restrict__ rec_line, i64 n_rec, const i64 *__restrict__ pre_t, i64 n_blocks,
                                                    i64 *__restrict__ name_at, i64 *__restrict__ name_len, i64 *__restrict__ val_len,
                                                    i64 *__restrict__ val_depth, unsigned long long *__restrict__ err) {
    const i64 n_waves = (i64)gridDim.x * (256 / HHX_WAVE);
    for (i64 r = (i64)blockIdx.x * (256 / HHX_WAVE) + threadIdx.x / HHX_WAVE; r < n_rec; r += n_waves) {
        const i64 k = rec_line[r], a = starts[k], e = k + 1 < n_lines ? starts[k + 1] : n;
        i64 ce = e;                                              // the end of the line without its line break
        if (k + 1 < n_lines) {
            ce = e - 1;
            if (t[ce] == '\n' && ce > a && t[ce - 1] == '\r') --ce;
        }
        const i64 g1 = tabs_before(t, n, pre_t, a + 1);          // the number of the TAB at a + 1
        i64 p[5] = {a + 1, n, n, n, n};                          // the TABs that end fields 0..4
        for (int j = 1; j < 5; ++j) {
            p[j] = select_tab(t, n, pre_t, n_blocks, g1 + j);
            if (p[j] >= ce) break;                               // the TAB of a later line, or none
        }
        int code = 0;
        i64 nlen = 0, v3 = 0, v4 = 0;
        if (p[3] >= ce) code = E_FIELDS;
        else if ((nlen = p[1] - (a + 2)) > NAME_BYTES_MAX) code = E_NAME;
        else if (!tail_int(t, p[2] + 1, p[3], &v3)) code = E_LEN;
        else if (!tail_int(t, p[3] + 1, p[4] < ce ? p[4] : ce, &v4)) code = E_DEPTH;
        if (lane_id() == 0) {
            name_at[r] = a + 2;
            name_len[r] = code ? 0 : nlen;
            val_len[r] = v3;
            val_depth[r] = v4;
            if (code) atomicMin(err, ((unsigned long long)k << 3) | (unsigned long long)code);
        }
    }
}

__global__ __launch_bounds__(256) void k_gfa_names(const unsigned char *__restrict__ t, const i64 *__restrict__ name_at, const i64 *__restrict__ name_off,
                                                   i64 n_rec, unsigned char *__restrict__ out) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (i64)gridDim.x * blockDim.x) {
        const i64 a = name_at[r], o = name_off[r], m = name_off[r + 1] - o;
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

struct hhx_gfa {
    i64 n_rec = 0;
    std::vector<i64> name_off, len, depth;
    std::vector<unsigned char> names;
};

namespace {

// t[0, n) is the text, with SLACK bytes behind it
int parse(hhx_gfa *g, const unsigned char *t, i64 n) {
    g->name_off.assign(1, 0);
    if (n == 0) return 0;
    const i64 n_blocks = (n + TX_BLOCK - 1) / TX_BLOCK;
    DevBuf<u32> flag;
    DevBuf<unsigned long long> err;
    DevBuf<i64> cnt_b, cnt_t, pre_b, pre_t, starts;
    if (flag.alloc(1) || err.alloc(1) || cnt_b.alloc((size_t)n_blocks) || cnt_t.alloc((size_t)n_blocks) || pre_b.alloc((size_t)n_blocks + 1) ||
        pre_t.alloc((size_t)n_blocks + 1)) return 1;
    HHX_HIP(hipMemsetAsync(flag.p, 0, sizeof(u32), g_stream));
    HHX_HIP(hipMemsetAsync(err.p, 0xff, sizeof(unsigned long long), g_stream));
    { KTimer kt("gfa_count");
    k_gfa_count<<<gfa_grid(n_blocks, 1), 256, 0, g_stream>>>(t, n, n_blocks, cnt_b.p, cnt_t.p, flag.p); }
    HHX_LAUNCH_CHECK();
    i64 n_breaks = 0, n_tabs = 0;
    HHX_TRY(exclusive_scan_i64(cnt_b.p, pre_b.p, n_blocks, &n_breaks));
    HHX_TRY(exclusive_scan_i64(cnt_t.p, pre_t.p, n_blocks, &n_tabs));
    u32 high = 0;
    HHX_HIP(hipMemcpyAsync(&high, flag.p, sizeof high, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (high) return unsupported("hhx_gfa: the text holds a byte >= 0x80 (the reference decodes it by the locale)");
    if (starts.alloc((size_t)n_breaks + 2)) return 1;
    { KTimer kt("gfa_starts");
    k_write_starts<<<gfa_grid(n_blocks, 1), 256, 0, g_stream>>>(t, n, n_blocks, pre_b.p, starts.p); }
    HHX_LAUNCH_CHECK();

    const i64 n_lines = n_breaks + 1;                            // the last one may be empty
    DevBuf<i64> rec, rid, rec_line;
    if (rec.alloc((size_t)n_lines) || rid.alloc((size_t)n_lines + 1)) return 1;
    { KTimer kt("gfa_mark");
    k_gfa_mark<<<gfa_grid(n_lines, 256), 256, 0, g_stream>>>(t, n, starts.p, n_lines, rec.p); }
    HHX_LAUNCH_CHECK();
    i64 n_rec = 0;
    HHX_TRY(exclusive_scan_i64(rec.p, rid.p, n_lines, &n_rec));
    if (n_rec == 0) return 0;
    DevBuf<i64> name_at, name_len, name_off, val_len, val_depth;
    if (rec_line.alloc((size_t)n_rec) || name_at.alloc((size_t)n_rec) || name_len.alloc((size_t)n_rec) || name_off.alloc((size_t)n_rec + 1) ||
        val_len.alloc((size_t)n_rec) || val_depth.alloc((size_t)n_rec)) return 1;
    { KTimer kt("gfa_mark");
    k_gfa_compact<<<gfa_grid(n_lines, 256), 256, 0, g_stream>>>(rec.p, rid.p, n_lines, rec_line.p); }
    HHX_LAUNCH_CHECK();
    { KTimer kt("gfa_fields");
    k_gfa_fields<<<gfa_grid(n_rec, 256 / HHX_WAVE), 256, 0, g_stream>>>(t, n, starts.p, n_lines, rec_line.p, n_rec, pre_t.p, n_blocks, name_at.p, name_len.p,
                                                                         val_len.p, val_depth.p, err.p); }
    HHX_LAUNCH_CHECK();
    unsigned long long first = NO_ERROR;
    HHX_HIP(hipMemcpyAsync(&first, err.p, sizeof first, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (first != NO_ERROR) {
        const long long line = (long long)(first >> 3) + 1;
        switch ((int)(first & 7)) {
        case E_FIELDS: return unsupported("hhx_gfa: line %lld: an S record with fewer than five fields (the reference raises IndexError)", line);
        case E_NAME: return unsupported("hhx_gfa: line %lld: a name longer than %d bytes", line, NAME_BYTES_MAX);
        case E_LEN: return unsupported("hhx_gfa: line %lld: field 3 does not end in ':' and 1 to %d digits (Python's int() decides)", line, DIGITS_MAX);
        default: return unsupported("hhx_gfa: line %lld: field 4 does not end in ':' and 1 to %d digits (Python's int() decides)", line, DIGITS_MAX);
        }
    }
    i64 n_name_bytes = 0;
    HHX_TRY(exclusive_scan_i64(name_len.p, name_off.p, n_rec, &n_name_bytes));
    DevBuf<unsigned char> names;
    if (names.alloc((size_t)n_name_bytes + 1)) return 1;
    { KTimer kt("gfa_names");
    k_gfa_names<<<gfa_grid(n_rec, 256), 256, 0, g_stream>>>(t, name_at.p, name_off.p, n_rec, names.p); }
    HHX_LAUNCH_CHECK();
    g->n_rec = n_rec;
    g->name_off.resize((size_t)n_rec + 1);
    g->len.resize((size_t)n_rec);
    g->depth.resize((size_t)n_rec);
    g->names.resize((size_t)n_name_bytes);
    HHX_HIP(hipMemcpyAsync(g->name_off.data(), name_off.p, sizeof(i64) * ((size_t)n_rec + 1), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(g->len.data(), val_len.p, sizeof(i64) * (size_t)n_rec, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(g->depth.data(), val_depth.p, sizeof(i64) * (size_t)n_rec, hipMemcpyDeviceToHost, g_stream));
    if (n_name_bytes) HHX_HIP(hipMemcpyAsync(g->names.data(), names.p, (size_t)n_name_bytes, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

}  // namespace

extern "C" int hhx_gfa_open_bytes(const uint8_t *text, int64_t n_bytes, hhx_gfa **out) {
    if (!out || n_bytes < 0 || (n_bytes && !text)) return fail("hhx_gfa_open_bytes: bad argument");
    HHX_TRY(fits(n_bytes, "hhx_gfa_open_bytes"));
    std::unique_ptr<hhx_gfa> g(new hhx_gfa());
    DevBuf<unsigned char> t;
    if (t.alloc((size_t)n_bytes + SLACK)) return 1;
    { KTimer kt("gfa_h2d");
    if (n_bytes) HHX_HIP(hipMemcpyAsync(t.p, text, (size_t)n_bytes, hipMemcpyHostToDevice, g_stream)); }
    HHX_HIP(hipStreamSynchronize(g_stream));
    HHX_TRY(parse(g.get(), t.p, n_bytes));
    *out = g.release();
    return 0;
}

extern "C" int hhx_gfa_open(const char *path, hhx_gfa **out) {
    if (!out || !path) return fail("hhx_gfa_open: bad argument");
    struct stat sb;
    if (::stat(path, &sb) != 0) return fail("cannot open %s: %s", path, strerror(errno));
    if (!S_ISREG(sb.st_mode)) return unsupported("hhx_gfa_open: %s is not a regular file", path);
    const i64 n = (i64)sb.st_size;
    HHX_TRY(fits(n, "hhx_gfa_open"));
    std::unique_ptr<hhx_gfa> g(new hhx_gfa());
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
            if (at + m > n) { rc = fail("hhx_gfa_open: %s grew while it was read", path); break; }
            hipError_t e = hipMemcpyAsync(t.p + at, host, (size_t)m, hipMemcpyHostToDevice, g_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
            if (e != hipSuccess) { rc = fail("hhx_gfa_open: %s", hipGetErrorString(e)); break; }
            at += m;
        }
        if (!rc && at != n) rc = fail("hhx_gfa_open: %s shrank while it was read", path);
        const std::string err = g_err;
        (void)hhx_text_reader_close(r);
        if (rc) { g_err = err; return rc; }
    }
    HHX_TRY(parse(g.get(), t.p, n));
    *out = g.release();
    return 0;
}

extern "C" int hhx_gfa_counts(const hhx_gfa *g, int64_t *n_rec, int64_t *n_name_bytes) {
    if (!g) return fail("hhx_gfa_counts: null handle");
    if (n_rec) *n_rec = g->n_rec;
    if (n_name_bytes) *n_name_bytes = g->name_off.back();
    return 0;
}

extern "C" int hhx_gfa_table(const hhx_gfa *g, int64_t *name_off, uint8_t *names, int64_t *len, int64_t *depth) {
    if (!g) return fail("hhx_gfa_table: null handle");
    const size_t n = (size_t)g->n_rec;
    if (name_off) memcpy(name_off, g->name_off.data(), sizeof(i64) * (n + 1));
    if (names && !g->names.empty()) memcpy(names, g->names.data(), g->names.size());
    if (len && n) memcpy(len, g->len.data(), sizeof(i64) * n);
    if (depth && n) memcpy(depth, g->depth.data(), sizeof(i64) * n);
    return 0;
}

extern "C" int hhx_gfa_close(hhx_gfa *g) {
    delete g;
    return 0;
}
