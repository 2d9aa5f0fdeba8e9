// paired_links.clm -> split_clms/<group>.clm on the device: split_clm_file (scripts/HapHiC_reassign.py:581-622).
//
//   reference, per line of the text file (universal newlines: '\n', '\r\n' and a lone '\r' end a line, the line reaches the loop with
//   '\n' as its terminator, a last line without a break has none):
//       cols = line.split()                                                          :616
//       ctg_1, ctg_2 = cols[0][:-1], cols[1][:-1]                                    :617   (IndexError with fewer than two tokens; the
//                                                                                           last CHARACTER goes, whatever it is)
//       if both are keys of ctg_group_dict and map to the same group: fp_dict[group].write(line)     :618-619
//
// Domain, as for the .pairs tokeniser (hhx_text.hip): whitespace is the ASCII subset of str.split()'s (\t \n \v \f \r \x1c-\x1f and
// space), bytes >= 0x80 are name bytes, the input is valid UTF-8 without the non-ASCII characters str.split() treats as whitespace.
//
// The text arrives as pushes that may cut it ANYWHERE (hhx_clm_split_push; hhx_clm_split_file pushes raw fixed-size chunks of the file).
// A CLM line carries every link of a contig pair and is megabytes long at times, so a line is never held whole.  State across a cut:
//   - the line in progress with its fate decided (keep into group g, or drop): what follows up to the next break is a CONTINUATION
//     segment and leaves, or is dropped, as it arrives;
//   - the HEAD of a line whose first two tokens are not complete yet (the second token counts as complete once a whitespace byte follows
//     it): the only bytes that are buffered; they are put in front of the next push.  The first two tokens must end within HEAD_MAX
//     bytes of the line's start — a clear failure otherwise, whether or not a cut falls there;
//   - a '\r' on the last byte of a push: held back and put in front of the next push, where a following '\n' makes it one break.
// Per push, on the device:
//   1. line breaks per 4 KB block, scanned, segment starts written (the passes of hhx_textscan.h);
//   2. one thread per segment finds the first two tokens, drops the last character of each, resolves both through the byte-verified name table
//      and maps id -> group (k_clm_parse): (source start, output length, gets '\n') with the group as sort key, G for "no output";
//   3. stable radix sort by group (hhx_sort.h): stream order is kept inside a group; an exclusive scan of the lengths in that order gives
//      every segment its offset in ONE group-major output buffer, and the first / last segment of a group give the group's span;
//   4. the byte gather (k_clm_gather), balanced by OUTPUT bytes: a workgroup owns GATHER_TILE destination bytes and finds its segments by
//      binary search in the scanned offsets, every thread assembles 16 destination-aligned bytes in registers — from two 16-byte source
//      loads funnel-shifted by the source/destination misalignment when the 16 bytes lie inside one segment, byte by byte where they
//      straddle segments or take the '\n' that stands for a "\r\n" / '\r' — and stores them with one 16-byte store.  A 5 MB line is
//      copied by hundreds of workgroups, 200 ten-byte lines by one.
// The buffer goes to one of two pinned host buffers; the library's writer lanes (hhx_jobs.hip) append every group's span to its file
// (G descriptors, as the reference keeps), even groups on one lane, odd groups on the other.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <condition_variable>
#include <memory>

#include "hhx_sort.h"
#include "hhx_textscan.h"

using namespace hhx;
using namespace hhx::textscan;

namespace {

constexpr int GATHER_TILE = 16 * 1024;         // destination bytes per workgroup step of the gather (256 threads x 4 x 16 bytes)
constexpr i64 HEAD_MAX = 64 * 1024;            // bound of the carried head of a line (its first two tokens and what surrounds them)
constexpr i64 PIECE_MAX = (i64)1 << 30;        // a push is worked off in pieces of at most this: segment starts and lengths are packed in 31 / 32 bits
constexpr int SLACK = 64;                      // bytes behind the work buffer that the 16-byte source loads may touch

enum { ST_ERR = 0, ST_OPEN_KIND, ST_OPEN_GROUP, ST_OPEN_START, ST_LINES, ST_KEPT, ST_CONT, ST_OUT, ST_MULTI, ST_SPAN, ST_N };
enum { OPEN_NONE = 0, OPEN_HEAD = 1, OPEN_DECIDED = 2 };
enum { ERR_INDEX = 0, ERR_HEAD = 1 };         // st[ST_ERR] = (segment << 1 | kind) of the first segment that fails

// segment k = [starts[k], starts[k + 1]) (the last one: up to n, without a break).  key[k]: its group, or n_groups when nothing leaves;
// val[k]: source start | output length << 31 | gets '\n' << 63
__global__ __launch_bounds__(256) void k_clm_parse(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ starts, i64 n_breaks, int first_is_cont,
                                                   i32 cont_group, int final, NameTable T, const i32 *__restrict__ group_of, i32 n_groups,
                                                   u64 *__restrict__ key, u64 *__restrict__ val, unsigned long long *__restrict__ st) {
    const HbmText rd{t};
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k <= n_breaks; k += (i64)gridDim.x * blockDim.x) {
        const bool has_break = k < n_breaks;
        const i64 a = starts[k], e = has_break ? starts[k + 1] : n;
        i64 ce = e;                                              // end of the content: the break bytes go, '\n' comes back in the gather
        if (has_break) ce = (t[e - 1] == '\n' && e - 2 >= a && t[e - 2] == '\r') ? e - 2 : e - 1;
        i32 g = -1;
        int open_kind = OPEN_NONE;
        if (k == 0 && first_is_cont) {
            g = cont_group;
            open_kind = OPEN_DECIDED;
            if (e > a) atomicAdd(&st[ST_CONT], 1ull);
        } else if (has_break || ce > a) {                        // (an open segment without bytes is no line)
            // the first two tokens must end within HEAD_MAX bytes of the line's start, wherever the cuts fall: nothing is read beyond that
            const i64 lim = ce - a > HEAD_MAX + 1 ? a + HEAD_MAX + 1 : ce;
            i64 p = a;
            Tok tok[2] = {{0, 0}, {0, 0}};
            int nt = 0;
            for (; nt < 2; ++nt) {
                while (p < lim && is_ws(rd(p))) ++p;
                if (p >= lim) break;
                tok[nt].s = p;
                while (p < lim && !is_ws(rd(p))) ++p;
                tok[nt].len = (i32)(p - tok[nt].s);
            }
            const bool ended = nt == 2 && p < lim;               // a whitespace byte follows the second token
            if (!ended && lim < ce) {
                atomicMin(&st[ST_ERR], ((unsigned long long)k << 1) | ERR_HEAD);
            } else if (!has_break && !final && !ended) {
                open_kind = OPEN_HEAD;                           // the second token may still grow: the bytes wait for the next push
            } else if (nt < 2) {
                atomicMin(&st[ST_ERR], ((unsigned long long)k << 1) | ERR_INDEX);
            } else {
                for (int q = 0; q < 2; ++q) {                    // cols[0][:-1], cols[1][:-1]: the last CHARACTER goes, with its UTF-8 continuation bytes
                    i32 last = tok[q].len - 1;
                    while (last > 0 && (rd(tok[q].s + last) & 0xC0) == 0x80) --last;
                    tok[q].len = last;
                }
                const i32 id1 = lookup(T, rd, tok[0]), id2 = lookup(T, rd, tok[1]);
                const i32 g1 = id1 >= 0 ? group_of[id1] : -1, g2 = id2 >= 0 ? group_of[id2] : -1;
                g = (g1 >= 0 && g1 == g2) ? g1 : -1;
                open_kind = OPEN_DECIDED;
                atomicAdd(&st[ST_LINES], 1ull);
                if (g >= 0) atomicAdd(&st[ST_KEPT], 1ull);
            }
        }
        const i64 len = (g >= 0 && open_kind == OPEN_DECIDED) ? (ce - a) + (has_break ? 1 : 0) : 0;
        key[k] = len > 0 ? (u64)g : (u64)n_groups;
        val[k] = (u64)a | ((u64)len << 31) | ((u64)(has_break ? 1 : 0) << 63);
        if (len > 0) atomicAdd(&st[ST_OUT], 1ull);
        if (!has_break) {
            st[ST_OPEN_KIND] = (unsigned long long)open_kind;
            st[ST_OPEN_GROUP] = (unsigned long long)(long long)g;
            st[ST_OPEN_START] = (unsigned long long)a;
        }
    }
}

__global__ __launch_bounds__(256) void k_clm_lengths(const u64 *__restrict__ val, i64 n, i64 *__restrict__ len) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) len[k] = (i64)((val[k] >> 31) & 0xffffffffull);
}

// span[2 g], span[2 g + 1]: where the bytes of group g begin and end in the output buffer (both 0 for a group that receives nothing)
__global__ __launch_bounds__(256) void k_clm_spans(const u64 *__restrict__ key, const i64 *__restrict__ off, i64 n, i32 n_groups, i64 *__restrict__ span) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) {
        const u64 g = key[k];
        if (g >= (u64)n_groups) continue;
        if (k == 0 || key[k - 1] != g) span[2 * g] = off[k];
        if (k + 1 == n || key[k + 1] != g) span[2 * g + 1] = off[k + 1];
    }
}

// the first segment i of [lo, hi] with off[i + 1] > d (d < off[hi + 1])
__device__ __forceinline__ i64 seg_of(const i64 *__restrict__ off, i64 lo, i64 hi, i64 d) {
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (off[mid + 1] > d) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// out[0, total): the segments in sorted order, one after the other.  t is 16-byte aligned with SLACK readable bytes behind it, out is 16-byte aligned
// with room up to the next multiple of 16.
__global__ __launch_bounds__(256) void k_clm_gather(const unsigned char *__restrict__ t, const u64 *__restrict__ val, const i64 *__restrict__ off, i64 n_seg,
                                                    i64 total, unsigned char *__restrict__ out, unsigned long long *__restrict__ st) {
    __shared__ i64 s_range[2];
    const i64 n_tiles = (total + GATHER_TILE - 1) / GATHER_TILE;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 d0 = tile * GATHER_TILE, d1 = d0 + GATHER_TILE < total ? d0 + GATHER_TILE : total;
        if (threadIdx.x == 0) {
            const i64 i0 = seg_of(off, 0, n_seg - 1, d0), i1 = seg_of(off, i0, n_seg - 1, d1 - 1);
            s_range[0] = i0;
            s_range[1] = i1;
            if (i1 > i0) atomicAdd(&st[ST_MULTI], 1ull);                                     // a tile that holds more than one line
            if (off[i1] >= d0 && off[i1 + 1] > d1) atomicAdd(&st[ST_SPAN], 1ull);            // a line that begins here and goes on in the next tile
        }
        __syncthreads();
        const i64 i0 = s_range[0], i1 = s_range[1];
        for (int j = 0; j < GATHER_TILE / (256 * 16); ++j) {
            const i64 d = d0 + ((i64)j * 256 + threadIdx.x) * 16;
            if (d >= d1) break;
            i64 i = seg_of(off, i0, i1, d);
            const u64 v = val[i];
            const i64 o = off[i], content_end = off[i + 1] - (i64)(v >> 63);
            uint4 r;
            if (d + 16 <= content_end) {
                const i64 src = (i64)(v & 0x7fffffffull) + (d - o), base = src & ~(i64)15;
                const int sh = (int)(src & 15);
                const uint4 lo = *reinterpret_cast<const uint4 *>(t + base);
                if (sh == 0) r = lo;
                else {
                    const uint4 hi = *reinterpret_cast<const uint4 *>(t + base + 16);
                    u64 a0 = (u64)lo.x | ((u64)lo.y << 32), a1 = (u64)lo.z | ((u64)lo.w << 32), a2 = (u64)hi.x | ((u64)hi.y << 32);
                    const u64 a3 = (u64)hi.z | ((u64)hi.w << 32);
                    int s = sh * 8;
                    if (s >= 64) { a0 = a1; a1 = a2; a2 = a3; s -= 64; }
                    const u64 r0 = s ? (a0 >> s) | (a1 << (64 - s)) : a0, r1 = s ? (a1 >> s) | (a2 << (64 - s)) : a1;
                    r = make_uint4((u32)r0, (u32)(r0 >> 32), (u32)r1, (u32)(r1 >> 32));
                }
            } else {                                             // the 16 bytes take a '\n', cross into the next segments or pass the end
                u64 r0 = 0, r1 = 0;
                i64 lo_i = o, hi_i = off[i + 1], src0 = (i64)(v & 0x7fffffffull);
                i64 nl = (i64)(v >> 63);
                for (int q = 0; q < 16 && d + q < total; ++q) {
                    const i64 x = d + q;
                    while (x >= hi_i) {
                        ++i;
                        const u64 vv = val[i];
                        lo_i = hi_i;
                        hi_i = off[i + 1];
                        src0 = (i64)(vv & 0x7fffffffull);
                        nl = (i64)(vv >> 63);
                    }
                    const u64 c = x < hi_i - nl ? t[src0 + (x - lo_i)] : (unsigned char)'\n';
                    if (q < 8) r0 |= c << (8 * q); else r1 |= c << (8 * (q - 8));
                }
                r = make_uint4((u32)r0, (u32)(r0 >> 32), (u32)r1, (u32)(r1 >> 32));
            }
            *reinterpret_cast<uint4 *>(out + d) = r;
        }
        __syncthreads();
    }
}

}  // namespace

struct hhx_clm_split {
    NameTableBuf table;
    DevBuf<i32> group_of;
    i32 n_groups = 0;
    std::vector<std::string> paths;
    std::vector<int> fd;
    // state across a cut
    int open_kind = OPEN_NONE;               // OPEN_DECIDED: the line in progress leaves into open_group (-1: is dropped); OPEN_HEAD: `head` holds its bytes so far
    i32 open_group = -1;
    std::vector<unsigned char> head;
    bool pending_cr = false;
    bool failed = false, finished = false;
    i64 stat[HHX_CLM_SPLIT_N_STATS] = {0, 0, 0, 0, 0, 0, 0};
    std::vector<i64> bytes_per_group;
    DevBuf<unsigned char> work, out;
    DevBuf<unsigned long long> st;
    // the output leaves through two pinned host buffers used in turn: the writer lanes empty buffer k while the next push is worked off
    unsigned char *pin[2] = {nullptr, nullptr};
    size_t pin_cap[2] = {0, 0};
    int pin_jobs[2] = {0, 0};                // writer jobs that still read pin[k]
    int pin_next = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::string write_err;                   // the first failure of a writer job

    void close_files() {
        for (int &f : fd) if (f >= 0) { ::close(f); f = -1; }
    }
    ~hhx_clm_split() {
        close_files();
        for (int k = 0; k < 2; ++k) if (pin[k]) (void)hipHostFree(pin[k]);
    }
};

namespace {

enum { C_LINES = 0, C_KEPT, C_HEADS, C_SEAMS, C_CONT, C_MULTI, C_SPAN };

int write_all(int fd, const unsigned char *p, size_t n) {
    while (n) {
        const ssize_t k = ::write(fd, p, n);
        if (k < 0) { if (errno == EINTR) continue; return errno ? errno : EIO; }
        p += k;
        n -= (size_t)k;
    }
    return 0;
}

// the spans of the groups g = parity (mod 2) of pin[b] appended to their files on a writer lane
void submit_writes(hhx_clm_split *s, int b, std::shared_ptr<std::vector<i64>> span) {
    for (int parity = 0; parity < 2; ++parity) {
        bool any = false;
        for (i32 g = parity; g < s->n_groups; g += 2) any |= (*span)[2 * g + 1] > (*span)[2 * g];
        if (!any) continue;
        { std::lock_guard<std::mutex> lk(s->mu); ++s->pin_jobs[b]; }
        files_submit("split_clms", s, [s, b, span, parity]() {
            for (i32 g = parity; g < s->n_groups; g += 2) {
                const i64 lo = (*span)[2 * g], hi = (*span)[2 * g + 1];
                if (hi <= lo) continue;
                const int e = write_all(s->fd[g], s->pin[b] + lo, (size_t)(hi - lo));
                if (e) {
                    std::lock_guard<std::mutex> lk(s->mu);
                    if (s->write_err.empty()) s->write_err = "writing " + s->paths[g] + " failed: " + strerror(e);
                    break;
                }
            }
            { std::lock_guard<std::mutex> lk(s->mu); --s->pin_jobs[b]; }
            s->cv.notify_all();
            return 0;                                            // the failure is reported by hhx_clm_split_finish
        }, parity);
    }
}

const char *const k_head_msg = "hhx_clm_split: the first two tokens of a line do not end within %lld bytes (not a CLM file?)";

// one piece of text (n < 2^30 + HEAD_MAX) behind what is carried; final: nothing follows, the open line is a whole line
int process(hhx_clm_split *s, const unsigned char *text, i64 n, bool on_device, bool final) {
    unsigned char ends[2] = {0, 0};                              // first and last byte of the piece
    if (n > 0) {
        if (on_device) {
            HHX_HIP(hipMemcpyAsync(&ends[0], text, 1, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipMemcpyAsync(&ends[1], text + n - 1, 1, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipStreamSynchronize(g_stream));
        } else { ends[0] = text[0]; ends[1] = text[n - 1]; }
    }
    if (n > 0 && s->pending_cr && ends[0] == '\n') ++s->stat[C_SEAMS];
    const bool hold_cr = !final && n > 0 && ends[1] == '\r';    // whether it is a break of its own is known with the next byte
    const i64 n_use = hold_cr ? n - 1 : n;
    const i64 n_head = (i64)s->head.size(), n_cr = s->pending_cr ? 1 : 0;
    const i64 m = n_head + n_cr + n_use;
    if (m == 0 || (n == 0 && !final)) { s->pending_cr = s->pending_cr || hold_cr; return 0; }
    if (s->work.n < (size_t)m + SLACK && s->work.alloc((size_t)(m + m / 4) + SLACK)) return 1;
    unsigned char *t = s->work.p;
    { KTimer kt("clm_h2d");
    if (n_head) HHX_HIP(hipMemcpyAsync(t, s->head.data(), (size_t)n_head, hipMemcpyHostToDevice, g_stream));
    if (n_cr) HHX_HIP(hipMemsetAsync(t + n_head, '\r', 1, g_stream));
    if (n_use) HHX_HIP(hipMemcpyAsync(t + n_head + n_cr, text, (size_t)n_use, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, g_stream)); }

    const i64 n_blocks = (m + TX_BLOCK - 1) / TX_BLOCK;
    DevBuf<i64> cnt, pre, starts;
    if (cnt.alloc((size_t)n_blocks) || pre.alloc((size_t)n_blocks + 1)) return 1;
    { KTimer kt("clm_breaks");
    k_count_breaks<<<grid_for(n_blocks, 1), 256, 0, g_stream>>>(t, m, n_blocks, cnt.p); }
    HHX_LAUNCH_CHECK();
    i64 n_breaks = 0;
    HHX_TRY(exclusive_scan_i64(cnt.p, pre.p, n_blocks, &n_breaks));          // (synchronises: the host copies of the head and of a pageable text are done with)
    s->head.clear();
    s->pending_cr = hold_cr;
    if (starts.alloc((size_t)n_breaks + 2)) return 1;
    { KTimer kt("clm_breaks");
    k_write_starts<<<grid_for(n_blocks, 1), 256, 0, g_stream>>>(t, m, n_blocks, pre.p, starts.p); }
    HHX_LAUNCH_CHECK();

    const i64 n_seg = n_breaks + 1;
    DevBuf<u64> key, val, skey, sval;
    if (key.alloc((size_t)n_seg) || val.alloc((size_t)n_seg)) return 1;
    unsigned long long st[ST_N];
    memset(st, 0, sizeof st);
    st[ST_ERR] = ~0ull;
    HHX_HIP(hipMemcpyAsync(s->st.p, st, sizeof st, hipMemcpyHostToDevice, g_stream));
    { KTimer kt("clm_parse");
    k_clm_parse<<<grid_for(n_seg, 256), 256, 0, g_stream>>>(t, m, starts.p, n_breaks, s->open_kind == OPEN_DECIDED ? 1 : 0, s->open_group, final ? 1 : 0,
                                                              s->table.view(), s->group_of.p, s->n_groups, key.p, val.p, s->st.p); }
    HHX_LAUNCH_CHECK();
    HHX_HIP(hipMemcpyAsync(st, s->st.p, sizeof st, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (st[ST_ERR] != ~0ull && (st[ST_ERR] & 1) == ERR_INDEX) return fail("IndexError: list index out of range");
    if (st[ST_ERR] != ~0ull) return fail(k_head_msg, (long long)HEAD_MAX);
    s->stat[C_LINES] += (i64)st[ST_LINES];
    s->stat[C_KEPT] += (i64)st[ST_KEPT];
    s->stat[C_CONT] += (i64)st[ST_CONT];
    s->open_kind = (int)st[ST_OPEN_KIND];
    s->open_group = (i32)(long long)st[ST_OPEN_GROUP];
    if (s->open_kind == OPEN_HEAD) {
        const i64 a = (i64)st[ST_OPEN_START];
        if (m - a > HEAD_MAX) return fail(k_head_msg, (long long)HEAD_MAX);
        s->head.resize((size_t)(m - a));
        HHX_HIP(hipMemcpyAsync(s->head.data(), t + a, (size_t)(m - a), hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        ++s->stat[C_HEADS];
    }
    if (st[ST_OUT] == 0) return 0;

    int bits = 1;
    while (((i64)1 << bits) <= (i64)s->n_groups) ++bits;
    DevBuf<i64> len, off, span;
    if (skey.alloc((size_t)n_seg) || sval.alloc((size_t)n_seg) || len.alloc((size_t)n_seg) || off.alloc((size_t)n_seg + 1) || span.alloc(2 * (size_t)s->n_groups)) return 1;
    i64 total = 0;
    { KTimer kt("clm_partition");
    HHX_TRY(stable_sort_pairs_u64(key.p, skey.p, val.p, sval.p, n_seg, bits));
    k_clm_lengths<<<grid_for(n_seg, 256), 256, 0, g_stream>>>(sval.p, n_seg, len.p);
    HHX_LAUNCH_CHECK();
    HHX_TRY(exclusive_scan_i64(len.p, off.p, n_seg, &total));
    HHX_HIP(hipMemsetAsync(span.p, 0, sizeof(i64) * 2 * (size_t)s->n_groups, g_stream));
    k_clm_spans<<<grid_for(n_seg, 256), 256, 0, g_stream>>>(skey.p, off.p, n_seg, s->n_groups, span.p); }
    HHX_LAUNCH_CHECK();
    const size_t room = ((size_t)total + 15) & ~(size_t)15;
    if (s->out.n < room && s->out.alloc(room + room / 4)) return 1;
    { KTimer kt("clm_gather");
    k_clm_gather<<<grid_for((total + GATHER_TILE - 1) / GATHER_TILE, 1), 256, 0, g_stream>>>(t, sval.p, off.p, n_seg, total, s->out.p, s->st.p); }
    HHX_LAUNCH_CHECK();

    const int b = s->pin_next;
    s->pin_next ^= 1;
    {
        std::unique_lock<std::mutex> lk(s->mu);
        s->cv.wait(lk, [&] { return s->pin_jobs[b] == 0; });
    }
    if ((size_t)total > s->pin_cap[b]) {
        if (s->pin[b]) (void)hipHostFree(s->pin[b]);
        s->pin[b] = nullptr;
        s->pin_cap[b] = (size_t)total + (size_t)total / 4 + 4096;
        HHX_HIP(hipHostMalloc((void **)&s->pin[b], s->pin_cap[b], hipHostMallocDefault));
    }
    auto host_span = std::make_shared<std::vector<i64>>(2 * (size_t)s->n_groups);
    { KTimer kt("clm_d2h");
    HHX_HIP(hipMemcpyAsync(s->pin[b], s->out.p, (size_t)total, hipMemcpyDeviceToHost, g_stream)); }
    HHX_HIP(hipMemcpyAsync(host_span->data(), span.p, sizeof(i64) * 2 * (size_t)s->n_groups, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(st, s->st.p, sizeof st, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    s->stat[C_MULTI] += (i64)st[ST_MULTI];
    s->stat[C_SPAN] += (i64)st[ST_SPAN];
    for (i32 g = 0; g < s->n_groups; ++g) s->bytes_per_group[(size_t)g] += (*host_span)[2 * g + 1] - (*host_span)[2 * g];
    submit_writes(s, b, host_span);
    return 0;
}

}  // namespace

extern "C" int hhx_clm_split_create(int32_t n_names, const uint8_t *names_blob, const int64_t *name_off, const int32_t *group_of_name, int32_t n_groups,
                                    const uint8_t *paths_blob, const int64_t *path_off, hhx_clm_split **out) {
    if (n_names < 0 || n_groups < 0 || !out || (n_names && (!names_blob || !name_off || !group_of_name)) || (n_groups && (!paths_blob || !path_off)))
        return fail("hhx_clm_split_create: bad argument");
    for (i32 k = 0; k < n_names; ++k)
        if (group_of_name[k] < -1 || group_of_name[k] >= n_groups) return fail("hhx_clm_split_create: name %d is in group %d of %d", k, group_of_name[k], n_groups);
    std::unique_ptr<hhx_clm_split> s(new hhx_clm_split());
    s->n_groups = n_groups;
    s->bytes_per_group.assign((size_t)n_groups, 0);
    if (s->table.build(n_names, names_blob, name_off, "hhx_clm_split_create") || s->group_of.alloc((size_t)n_names + 1) || s->st.alloc(ST_N)) return 1;
    if (n_names) HHX_HIP(hipMemcpyAsync(s->group_of.p, group_of_name, sizeof(i32) * (size_t)n_names, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    s->fd.assign((size_t)n_groups, -1);
    for (i32 g = 0; g < n_groups; ++g) {
        s->paths.emplace_back((const char *)paths_blob + path_off[g], (size_t)(path_off[g + 1] - path_off[g]));
        s->fd[(size_t)g] = ::open(s->paths.back().c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (s->fd[(size_t)g] < 0) return fail("cannot open %s: %s", s->paths.back().c_str(), strerror(errno));
    }
    *out = s.release();
    return 0;
}

extern "C" int hhx_clm_split_push(hhx_clm_split *s, const uint8_t *text, int64_t n_bytes, int on_device) {
    if (!s) return fail("hhx_clm_split_push: null handle");
    if (n_bytes < 0 || (n_bytes && !text)) return fail("hhx_clm_split_push: bad argument");
    if (s->failed || s->finished) return fail("hhx_clm_split_push: the split has %s", s->failed ? "failed" : "been finished");
    for (i64 at = 0; at < n_bytes; at += PIECE_MAX)
        if (process(s, text + at, std::min<i64>(PIECE_MAX, n_bytes - at), on_device != 0, false)) { s->failed = true; return 1; }
    return 0;
}

extern "C" int hhx_clm_split_file(hhx_clm_split *s, const char *clm_path, int64_t chunk_bytes, int n_threads) {
    if (!s) return fail("hhx_clm_split_file: null handle");
    if (!clm_path || chunk_bytes <= 0) return fail("hhx_clm_split_file: bad argument");
    hhx_text_reader *r = nullptr;
    HHX_TRY(hhx_text_reader_open_raw(clm_path, std::min<i64>(chunk_bytes, PIECE_MAX), n_threads, &r));
    int rc = 0;
    for (;;) {
        const uint8_t *host = nullptr;
        i64 n = 0;
        if ((rc = hhx_text_reader_next(r, &host, &n)) != 0 || n == 0) break;
        if ((rc = hhx_clm_split_push(s, host, n, 0)) != 0) break;
    }
    const std::string err = g_err;
    (void)hhx_text_reader_close(r);
    if (rc) g_err = err;
    return rc;
}

extern "C" int hhx_clm_split_finish(hhx_clm_split *s, int64_t *n_lines, int64_t *n_kept, int64_t *bytes_per_group) {
    if (!s) return fail("hhx_clm_split_finish: null handle");
    int rc = 0;
    if (!s->failed && !s->finished && (!s->head.empty() || s->pending_cr)) rc = process(s, nullptr, 0, false, true);
    if (rc) s->failed = true;
    const std::string err = g_err;
    s->finished = true;
    files_wait_handle(s);
    s->close_files();
    if (rc) { g_err = err; return rc; }
    if (s->failed) return fail("hhx_clm_split_finish: the split has failed");
    if (!s->write_err.empty()) return fail("%s", s->write_err.c_str());
    if (n_lines) *n_lines = s->stat[C_LINES];
    if (n_kept) *n_kept = s->stat[C_KEPT];
    if (bytes_per_group) for (i32 g = 0; g < s->n_groups; ++g) bytes_per_group[g] = s->bytes_per_group[(size_t)g];
    return 0;
}

extern "C" int hhx_clm_split_stats(hhx_clm_split *s, int64_t *values) {
    if (!s || !values) return fail("hhx_clm_split_stats: null pointer");
    for (int k = 0; k < HHX_CLM_SPLIT_N_STATS; ++k) values[k] = s->stat[k];
    return 0;
}

extern "C" int hhx_clm_split_destroy(hhx_clm_split *s) {
    if (!s) return 0;
    files_wait_handle(s);
    delete s;
    return 0;
}
