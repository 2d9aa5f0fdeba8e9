// `haphic build` on the device: the FASTA reader (parse_fasta, scripts/HapHiC_cluster.py:87-113) and the scaffold writer
// (build_final_scaffolds, scripts/HapHiC_build.py:153-168).
//
// Reader.  reference, per line of the text file (universal newlines: '\n', '\r\n' and a lone '\r' end a line):
//       if not line.strip(): continue                                                :95
//       if line.startswith('>'): ctg = line.split()[0][1:]; fa_dict[ctg] = list()    :97-99   (the FIRST RAW byte decides; '>' alone and '> x' name '')
//       else: fa_dict[ctg].append(line.strip() [.upper()])                           :101-104 (inner whitespace stays; UnboundLocalError before the first header)
//   and ''.join per contig :108.  Whitespace is the ASCII part of str.strip()'s (\t \n \v \f \r \x1c-\x1f and space); a byte >= 0x80 is refused
//   (the reference decodes by locale), so str.upper() is the fold of a-z.
// The whole text lies in HBM in one piece.  Passes:
//   1. k_fa_high: any byte >= 0x80 (16 bytes per lane);
//   2. line breaks per 4 KB block, scanned, line starts written (the passes of hhx_textscan.h);
//   3. k_fa_classify: a group of 8 lanes per line finds the strip range from both ends and, on a header line, the end of the first token:
//      (kept length, header flag, first kept byte, name length) per line;
//   4. exclusive scans of the kept lengths (where a line's bytes go) and of the header flags (the contig id of a line); k_fa_tables: seq_off and the
//      name span per contig, and the flag for a sequence line in front of every header; seq_len from the neighbours;
//   5. k_fa_copy, balanced by OUTPUT bytes: a workgroup owns COPY_TILE destination bytes and finds its lines by binary search in the scanned
//      offsets, every lane assembles 16 destination-aligned bytes — two 16-byte source loads funnel-shifted where the 16 bytes lie inside one
//      line, byte by byte where they straddle lines — folds a-z and stores them with one 16-byte store.  A line of 10 MB is copied by hundreds of
//      workgroups, the many lines that keep nothing (headers, blanks) vanish in the search.
// 1 + 1 + 1 bytes read per text byte (passes 1, 2 twice from L2 / HBM), one read and one write per kept byte in pass 5; the tables are 56 bytes per line.
//
// Writer.  The file is a function of its byte offset: record r ('>name\n', then the sequence in lines of max_width bytes, each followed by '\n') begins at
// rec_off[r] (int64 scan of 1 + name + 1 + len + ceil(len / max_width)); the sequence of a record is a run of segments (contig forward, contig
// reversed and complemented through ATCGNatcgn -> TAGCNtagcn, gap of Ns 'N') with scanned ends.  k_fa_emit: every lane produces 16 consecutive file
// bytes and stores them with one aligned 16-byte store: binary search for the record, ONE 64-bit division for (line, column) where the lane begins
// inside a sequence, binary search for the segment, then it steps run by run (to the end of the line, of the segment or of its 16 bytes).  A run is
// fetched with aligned 8-byte loads and shifted into place; a reversed run is the forward fetch of the same bytes (the lanes of a wave walk one
// cache line downwards), byte-swapped and complemented 8 bytes at a time.  No atomics, no LDS.  One sequence byte read and one file byte written per
// output byte; the searches hit L2.
// The file is produced slab by slab (hhx_tune "fasta_slab") into two device buffers on a stream of the call's own: the kernel of slab k + 1 runs
// while FileSink copies slab k to pinned memory and its threads write it.  What bounds the step is the file system, then PCIe.
#include <sys/stat.h>

#include <memory>

#include "hhx_filesink.h"
#include "hhx_internal.h"
#include "hhx_textscan.h"

using namespace hhx;
using namespace hhx::textscan;

typedef unsigned __int128 u128;

namespace {

constexpr int COPY_TILE = 16 * 1024;           // destination bytes per workgroup step of the compaction copy (256 lanes x 4 x 16 bytes)
constexpr int SLACK = 64;                      // bytes behind the text that the 16-byte source loads may touch
constexpr int SEQ_PAD = 32;                    // bytes in front of and behind the compacted sequences that the 8-byte loads of the writer may touch
constexpr int LINE_LANES = 8;                  // lanes that share one line in k_fa_classify
constexpr i64 SLAB_MIN = 256;
constexpr i64 SLAB_DEFAULT = (i64)FileSink::PIECE;
constexpr i64 SPAN_MAX = (i64)1 << 60;         // max_width beyond it is "one line"; a scaffold beyond it is refused

enum { FL_HIGH = 0, FL_ORPHAN = 1, FL_N = 2 };

__global__ __launch_bounds__(256) void k_fa_high(const unsigned char *__restrict__ t, i64 n, u32 *__restrict__ flag) {
    const i64 n16 = n >> 4, stride = (i64)gridDim.x * blockDim.x, me = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 acc = 0;
    for (i64 k = me; k < n16; k += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(t)[k];
        acc |= v.x | v.y | v.z | v.w;
    }
    for (i64 p = (n16 << 4) + me; p < n; p += stride) acc |= t[p];
    if (acc & 0x80808080u) flag[FL_HIGH] = 1;
}

// line k = [starts[k], starts[k + 1]) (the last one: up to n).  kept[k]: bytes of a sequence line that stay; hdr[k]: 1 on a header line;
// first[k]: the first kept byte, on a header line the first byte of the name; nlen[k]: bytes of the name
__global__ __launch_bounds__(256) void k_fa_classify(const unsigned char *__restrict__ t, i64 n, const i64 *__restrict__ starts, i64 n_lines,
                                                     i64 *__restrict__ kept, i64 *__restrict__ hdr, i64 *__restrict__ first, i64 *__restrict__ nlen) {
    const int gl = threadIdx.x & (LINE_LANES - 1), sh = lane_id() & ~(LINE_LANES - 1);
    const i64 n_groups = (i64)gridDim.x * (256 / LINE_LANES);
    for (i64 k = (i64)blockIdx.x * (256 / LINE_LANES) + threadIdx.x / LINE_LANES; k < n_lines; k += n_groups) {
        const i64 a = starts[k], e = k + 1 < n_lines ? starts[k + 1] : n;
        i64 s = e;                                               // the first byte that is no whitespace
        for (i64 b = a; b < e; b += LINE_LANES) {
            const i64 p = b + gl;
            const u32 m = (u32)(__ballot(p < e && !is_ws(t[p])) >> sh) & ((1u << LINE_LANES) - 1);
            if (m) { s = b + __ffs(m) - 1; break; }
        }
        i64 len = 0, is_hdr = 0, name_len = 0, from = s;
        if (s < e) {
            i64 last = s;                                        // the last one
            for (i64 b = e; b > s; b -= LINE_LANES) {
                const i64 p = b - 1 - gl;
                const u32 m = (u32)(__ballot(p >= s && !is_ws(t[p])) >> sh) & ((1u << LINE_LANES) - 1);
                if (m) { last = b - 1 - (__ffs(m) - 1); break; }
            }
            if (t[a] == '>') {                                   // line.split()[0][1:]: up to the first whitespace byte
                i64 te = last + 1;
                for (i64 b = a + 1; b <= last; b += LINE_LANES) {
                    const i64 p = b + gl;
                    const u32 m = (u32)(__ballot(p <= last && is_ws(t[p])) >> sh) & ((1u << LINE_LANES) - 1);
                    if (m) { te = b + __ffs(m) - 1; break; }
                }
                is_hdr = 1;
                from = a + 1;
                name_len = te - (a + 1);
            } else len = last + 1 - s;
        }
        if (gl == 0) { kept[k] = len; hdr[k] = is_hdr; first[k] = from; nlen[k] = name_len; }
    }
}

__global__ __launch_bounds__(256) void k_fa_tables(i64 n_lines, const i64 *__restrict__ kept, const i64 *__restrict__ hdr, const i64 *__restrict__ first,
                                                   const i64 *__restrict__ nlen, const i64 *__restrict__ koff, const i64 *__restrict__ hid,
                                                   i64 *__restrict__ seq_off, i64 *__restrict__ name_at, i64 *__restrict__ name_len, u32 *__restrict__ flag) {
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n_lines; k += (i64)gridDim.x * blockDim.x) {
        if (hdr[k]) {
            const i64 c = hid[k];
            seq_off[c] = koff[k];
            name_at[c] = first[k];
            name_len[c] = nlen[k];
        } else if (kept[k] > 0 && hid[k] == 0) flag[FL_ORPHAN] = 1;   // fa_dict[ctg] before any ctg: the reference raises
    }
}

__global__ __launch_bounds__(256) void k_fa_lens(const i64 *__restrict__ seq_off, i64 n_ctg, i64 total, i64 *__restrict__ seq_len) {
    for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctg; c += (i64)gridDim.x * blockDim.x)
        seq_len[c] = (c + 1 < n_ctg ? seq_off[c + 1] : total) - seq_off[c];
}

__global__ __launch_bounds__(256) void k_fa_names(const unsigned char *__restrict__ t, const i64 *__restrict__ name_at, const i64 *__restrict__ name_off,
                                                  i64 n_ctg, unsigned char *__restrict__ out) {
    for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < n_ctg; c += (i64)gridDim.x * blockDim.x) {
        const i64 a = name_at[c], o = name_off[c], m = name_off[c + 1] - o;
        for (i64 q = 0; q < m; ++q) out[o + q] = t[a + q];
    }
}

// the first i of [lo, hi] with off[i + 1] > d (d < off[hi + 1])
__device__ __forceinline__ i64 first_above(const i64 *__restrict__ off, i64 lo, i64 hi, i64 d) {
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (off[mid + 1] > d) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// a-z -> A-Z in the 8 bytes of w, all below 0x80 (no carry leaves a byte)
__device__ __forceinline__ u64 fold8(u64 w) {
    const u64 ones = 0x0101010101010101ull;
    const u64 ge_a = w + ones * (0x80 - 'a'), gt_z = w + ones * (0x80 - 'z' - 1);
    return w - (((ge_a & ~gt_z) & (ones * 0x80)) >> 2);
}

// out[0, total): the kept bytes of the lines one after the other.  t is 16-byte aligned with SLACK readable bytes behind it, out is 16-byte aligned with
// room up to the next multiple of 16
__global__ __launch_bounds__(256) void k_fa_copy(const unsigned char *__restrict__ t, const i64 *__restrict__ first, const i64 *__restrict__ off, i64 n_lines,
                                                 i64 total, int fold, unsigned char *__restrict__ out) {
    __shared__ i64 s_range[2];
    const i64 n_tiles = (total + COPY_TILE - 1) / COPY_TILE;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 d0 = tile * COPY_TILE, d1 = d0 + COPY_TILE < total ? d0 + COPY_TILE : total;
        if (threadIdx.x == 0) {
            const i64 i0 = first_above(off, 0, n_lines - 1, d0);
            s_range[0] = i0;
            s_range[1] = first_above(off, i0, n_lines - 1, d1 - 1);
        }
        __syncthreads();
        const i64 i0 = s_range[0], i1 = s_range[1];
        for (int j = 0; j < COPY_TILE / (256 * 16); ++j) {
            const i64 d = d0 + ((i64)j * 256 + threadIdx.x) * 16;
            if (d >= d1) break;
            i64 i = first_above(off, i0, i1, d);
            const i64 o = off[i];
            u64 r0 = 0, r1 = 0;
            if (d + 16 <= off[i + 1]) {
                const i64 src = first[i] + (d - o), base = src & ~(i64)15;
                const int sh = (int)(src & 15);
                const uint4 lo = *reinterpret_cast<const uint4 *>(t + base);
                r0 = (u64)lo.x | ((u64)lo.y << 32);
                r1 = (u64)lo.z | ((u64)lo.w << 32);
                if (sh) {
                    const uint4 hi = *reinterpret_cast<const uint4 *>(t + base + 16);
                    u64 a0 = r0, a1 = r1, a2 = (u64)hi.x | ((u64)hi.y << 32);
                    const u64 a3 = (u64)hi.z | ((u64)hi.w << 32);
                    int s = sh * 8;
                    if (s >= 64) { a0 = a1; a1 = a2; a2 = a3; s -= 64; }
                    r0 = s ? (a0 >> s) | (a1 << (64 - s)) : a0;
                    r1 = s ? (a1 >> s) | (a2 << (64 - s)) : a1;
                }
            } else {                                             // the 16 bytes cross into the next lines or pass the end
                i64 lo_i = o, hi_i = off[i + 1], src0 = first[i];
                for (int q = 0; q < 16 && d + q < total; ++q) {
                    const i64 x = d + q;
                    while (x >= hi_i) {
                        ++i;
                        lo_i = hi_i;
                        hi_i = off[i + 1];
                        src0 = first[i];
                    }
                    const u64 c = t[src0 + (x - lo_i)];
                    if (q < 8) r0 |= c << (8 * q); else r1 |= c << (8 * (q - 8));
                }
            }
            if (fold) { r0 = fold8(r0); r1 = fold8(r1); }
            *reinterpret_cast<uint4 *>(out + d) = make_uint4((u32)r0, (u32)(r0 >> 32), (u32)r1, (u32)(r1 >> 32));
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- writer
struct EmitTab {
    i64 n_rec;
    const i64 *rec_off;                      // [n_rec + 1] first file byte of a record
    const i64 *rec_slen;                     // [n_rec] bytes of its sequence
    const i64 *rec_seg0;                     // [n_rec + 1] its segments
    const i64 *name_off;                     // [n_rec + 1] its name in `names`
    const unsigned char *names;
    const i64 *seg_end;                      // end of a segment in the coordinates of its record's sequence (its start: the end before it, 0 for the first)
    const i64 *seg_src;                      // first byte of the contig in seq | reversed << 62; -1: a gap
    i64 width;
};

// ATCGNatcgn -> TAGCNtagcn in the 8 bytes of w, all below 0x80: A ^ T = 0x15, C ^ G = 0x04, case kept, everything else unchanged
__device__ __forceinline__ u64 complement8(u64 w) {
    const u64 ones = 0x0101010101010101ull, low7 = ones * 0x7f, high = ones * 0x80;
    const u64 u = w & (ones * 0xdf);
    const u64 zA = u ^ (ones * 'A'), zT = u ^ (ones * 'T'), zC = u ^ (ones * 'C'), zG = u ^ (ones * 'G');
    const u64 at = (~((zA + low7) | zA) | ~((zT + low7) | zT)) & high, cg = (~((zC + low7) | zC) | ~((zG + low7) | zG)) & high;
    return w ^ ((at >> 7) * 0x15) ^ ((cg >> 7) * 0x04);
}

// bytes [lo, lo + m) of seq (1 <= m <= 16) in the low bytes of the result, by aligned 8-byte loads; what lies above them is not defined
__device__ __forceinline__ u128 fetch_run(const unsigned char *__restrict__ seq, i64 lo) {
    const u64 *w = reinterpret_cast<const u64 *>(seq + (lo & ~(i64)7));
    const int s = (int)(lo & 7) * 8;
    u128 v = (((u128)w[1] << 64) | w[0]) >> s;
    if (s) v |= (u128)w[2] << (128 - s);
    return v;
}

// file bytes [g0, g1) into out[0, g1 - g0) (g0 a multiple of 16, out 16-byte aligned with room up to the next multiple of 16); seq has SEQ_PAD
// readable bytes on both sides
__global__ __launch_bounds__(256) void k_fa_emit(EmitTab T, const unsigned char *__restrict__ seq, i64 g0, i64 g1, unsigned char *__restrict__ out) {
    const i64 n_gran = (g1 - g0 + 15) >> 4, W = T.width;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < n_gran; idx += (i64)gridDim.x * blockDim.x) {
        const i64 g = g0 + idx * 16;
        const int cnt = g1 - g < 16 ? (int)(g1 - g) : 16;
        i64 r = first_above(T.rec_off, 0, T.n_rec - 1, g);
        i64 p = g - T.rec_off[r], rlen = T.rec_off[r + 1] - T.rec_off[r], hdr = T.name_off[r + 1] - T.name_off[r] + 2, slen = T.rec_slen[r];
        i64 x = 0, col = 0, seg = -1;
        if (p > hdr) {                                           // inside the sequence lines: the one division of the lane
            const i64 q = p - hdr, line = q / (W + 1);
            col = q - line * (W + 1);
            x = line * W + col;
        }
        u128 acc = 0;
        int pos = 0;
        while (pos < cnt) {
            if (p >= rlen) {
                ++r;
                p = 0; x = 0; col = 0; seg = -1;
                rlen = T.rec_off[r + 1] - T.rec_off[r];
                hdr = T.name_off[r + 1] - T.name_off[r] + 2;
                slen = T.rec_slen[r];
                continue;
            }
            if (p < hdr) {
                const unsigned char c = p == 0 ? '>' : p == hdr - 1 ? '\n' : T.names[T.name_off[r] + p - 1];
                acc |= (u128)c << (8 * pos);
                ++pos; ++p;
                continue;
            }
            if (col == W || x == slen) {
                acc |= (u128)'\n' << (8 * pos);
                col = 0;
                ++pos; ++p;
                continue;
            }
            const i64 s0 = T.rec_seg0[r];
            if (seg < 0) seg = s0 + first_above(T.seg_end + s0 - 1, 0, T.rec_seg0[r + 1] - s0 - 1, x);
            else while (T.seg_end[seg] <= x) ++seg;
            const i64 sbeg = seg == s0 ? 0 : T.seg_end[seg - 1], send = T.seg_end[seg], src = T.seg_src[seg];
            i64 m = cnt - pos;
            if (W - col < m) m = W - col;
            if (send - x < m) m = send - x;
            u128 v;
            if (src < 0) v = ((u128)0x4e4e4e4e4e4e4e4eull << 64) | 0x4e4e4e4e4e4e4e4eull;
            else if (!(src >> 62)) v = fetch_run(seq, src + (x - sbeg));
            else {                                               // output byte o of the piece is contig byte len - 1 - o: the run's bytes, read upwards, turned round
                const i64 lo = (src & (((i64)1 << 62) - 1)) + (send - x) - m;
                const u128 f = fetch_run(seq, lo);
                const u64 f0 = complement8((u64)f), f1 = complement8((u64)(f >> 64));
                v = (((u128)__builtin_bswap64(f0) << 64) | __builtin_bswap64(f1)) >> (8 * (16 - (int)m));
            }
            if (m < 16) v &= ((u128)1 << (8 * (int)m)) - 1;
            acc |= v << (8 * pos);
            pos += (int)m; p += m; x += m; col += m;
        }
        *reinterpret_cast<uint4 *>(out + idx * 16) = make_uint4((u32)acc, (u32)(acc >> 32), (u32)(acc >> 64), (u32)(acc >> 96));
    }
}

// a stream and two events of one hhx_fasta_emit call; waits for the stream before it goes
struct EmitStream {
    hipStream_t s = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int open() {
        HHX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        for (auto &e : ev) HHX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return 0;
    }
    ~EmitStream() {
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    }
};

template <class T>
int upload(DevBuf<T> &d, const std::vector<T> &h) {
    if (d.alloc(h.size())) return 1;
    if (!h.empty()) HHX_HIP(hipMemcpyAsync(d.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, g_stream));
    return 0;
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

i64 slab_bytes() { return std::max<i64>(SLAB_MIN, std::min<i64>(SLAB_DEFAULT, tune_get("fasta_slab", SLAB_DEFAULT))) & ~(i64)15; }

}  // namespace

struct hhx_fasta {
    i64 n_ctg = 0, n_seq = 0;
    DevBuf<unsigned char> seq;               // SEQ_PAD | the sequences of the contigs in file order, nothing between them | SEQ_PAD
    DevBuf<i64> seq_off, seq_len;
    std::vector<i64> h_seq_off, h_seq_len, h_name_off;
    std::vector<unsigned char> h_names;
    const unsigned char *bases() const { return seq.p + SEQ_PAD; }
};

namespace {

// text + sequences + one slab of output within half of the device's memory
int fits(i64 n, const char *who) {
    size_t free_b = 0, total_b = 0;
    HHX_HIP(hipMemGetInfo(&free_b, &total_b));
    if (2 * (double)n + (double)slab_bytes() > (double)total_b / 2)
        return unsupported("%s: %lld bytes of text, as many of sequence and an output slab do not fit in half of the device's memory (%lld bytes)", who,
                           (long long)n, (long long)total_b);
    return 0;
}

// t[0, n) is the text, with SLACK bytes behind it
int parse(hhx_fasta *f, const unsigned char *t, i64 n, bool keep_case) {
    f->h_name_off.assign(1, 0);
    if (f->seq.alloc(2 * SEQ_PAD + 16)) return 1;
    if (n == 0) return 0;
    DevBuf<u32> flag;
    if (flag.alloc(FL_N)) return 1;
    HHX_HIP(hipMemsetAsync(flag.p, 0, sizeof(u32) * FL_N, g_stream));
    { KTimer kt("fa_high");
    k_fa_high<<<grid_for(n >> 4, 256 * 4), 256, 0, g_stream>>>(t, n, flag.p); }
    HHX_LAUNCH_CHECK();
    const i64 n_blocks = (n + TX_BLOCK - 1) / TX_BLOCK;
    DevBuf<i64> cnt, pre, starts;
    if (cnt.alloc((size_t)n_blocks) || pre.alloc((size_t)n_blocks + 1)) return 1;
    { KTimer kt("fa_breaks");
    k_count_breaks<<<grid_for(n_blocks, 1), 256, 0, g_stream>>>(t, n, n_blocks, cnt.p); }
    HHX_LAUNCH_CHECK();
    i64 n_breaks = 0;
    HHX_TRY(exclusive_scan_i64(cnt.p, pre.p, n_blocks, &n_breaks));
    u32 fl[FL_N] = {0, 0};
    HHX_HIP(hipMemcpyAsync(fl, flag.p, sizeof fl, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (fl[FL_HIGH]) return unsupported("hhx_fasta: the text holds a byte >= 0x80 (the reference decodes it by the locale)");
    if (starts.alloc((size_t)n_breaks + 2)) return 1;
    { KTimer kt("fa_breaks");
    k_write_starts<<<grid_for(n_blocks, 1), 256, 0, g_stream>>>(t, n, n_blocks, pre.p, starts.p); }
    HHX_LAUNCH_CHECK();

    const i64 n_lines = n_breaks + 1;                            // the last one may be empty
    DevBuf<i64> kept, hdr, first, nlen, koff, hid;
    if (kept.alloc((size_t)n_lines) || hdr.alloc((size_t)n_lines) || first.alloc((size_t)n_lines) || nlen.alloc((size_t)n_lines) ||
        koff.alloc((size_t)n_lines + 1) || hid.alloc((size_t)n_lines + 1)) return 1;
    { KTimer kt("fa_classify");
    k_fa_classify<<<grid_for(n_lines, 256 / LINE_LANES), 256, 0, g_stream>>>(t, n, starts.p, n_lines, kept.p, hdr.p, first.p, nlen.p); }
    HHX_LAUNCH_CHECK();
    i64 total = 0, n_ctg = 0;
    HHX_TRY(exclusive_scan_i64(kept.p, koff.p, n_lines, &total));
    HHX_TRY(exclusive_scan_i64(hdr.p, hid.p, n_lines, &n_ctg));
    DevBuf<i64> name_at, name_len, name_off;
    if (f->seq_off.alloc((size_t)n_ctg + 1) || f->seq_len.alloc((size_t)n_ctg + 1) || name_at.alloc((size_t)n_ctg + 1) || name_len.alloc((size_t)n_ctg + 1) ||
        name_off.alloc((size_t)n_ctg + 2)) return 1;
    { KTimer kt("fa_tables");
    k_fa_tables<<<grid_for(n_lines, 256), 256, 0, g_stream>>>(n_lines, kept.p, hdr.p, first.p, nlen.p, koff.p, hid.p, f->seq_off.p, name_at.p, name_len.p, flag.p);
    HHX_LAUNCH_CHECK();
    k_fa_lens<<<grid_for(n_ctg, 256), 256, 0, g_stream>>>(f->seq_off.p, n_ctg, total, f->seq_len.p); }
    HHX_LAUNCH_CHECK();
    HHX_HIP(hipMemcpyAsync(fl, flag.p, sizeof fl, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (fl[FL_ORPHAN]) return unsupported("hhx_fasta: a sequence line stands in front of the first header (the reference raises UnboundLocalError)");
    i64 n_name_bytes = 0;
    HHX_TRY(exclusive_scan_i64(name_len.p, name_off.p, n_ctg, &n_name_bytes));

    const size_t room = ((size_t)total + 15) & ~(size_t)15;
    if (f->seq.alloc(room + 2 * SEQ_PAD)) return 1;
    DevBuf<unsigned char> names;
    if (names.alloc((size_t)n_name_bytes + 1)) return 1;
    if (total > 0) {
        KTimer kt("fa_copy");
        k_fa_copy<<<grid_for((total + COPY_TILE - 1) / COPY_TILE, 1), 256, 0, g_stream>>>(t, first.p, koff.p, n_lines, total, keep_case ? 0 : 1,
                                                                                              f->seq.p + SEQ_PAD);
    }
    HHX_LAUNCH_CHECK();
    if (n_ctg > 0) k_fa_names<<<grid_for(n_ctg, 256), 256, 0, g_stream>>>(t, name_at.p, name_off.p, n_ctg, names.p);
    HHX_LAUNCH_CHECK();
    f->n_ctg = n_ctg;
    f->n_seq = total;
    f->h_seq_off.resize((size_t)n_ctg);
    f->h_seq_len.resize((size_t)n_ctg);
    f->h_name_off.resize((size_t)n_ctg + 1);
    f->h_names.resize((size_t)n_name_bytes);
    if (n_ctg) {
        HHX_HIP(hipMemcpyAsync(f->h_seq_off.data(), f->seq_off.p, sizeof(i64) * (size_t)n_ctg, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(f->h_seq_len.data(), f->seq_len.p, sizeof(i64) * (size_t)n_ctg, hipMemcpyDeviceToHost, g_stream));
    }
    HHX_HIP(hipMemcpyAsync(f->h_name_off.data(), name_off.p, sizeof(i64) * ((size_t)n_ctg + 1), hipMemcpyDeviceToHost, g_stream));
    if (n_name_bytes) HHX_HIP(hipMemcpyAsync(f->h_names.data(), names.p, (size_t)n_name_bytes, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

}  // namespace

extern "C" int hhx_fasta_open_bytes(const uint8_t *text, int64_t n_bytes, int keep_letter_case, hhx_fasta **out) {
    if (!out || n_bytes < 0 || (n_bytes && !text)) return fail("hhx_fasta_open_bytes: bad argument");
    HHX_TRY(fits(n_bytes, "hhx_fasta_open_bytes"));
    std::unique_ptr<hhx_fasta> f(new hhx_fasta());
    DevBuf<unsigned char> t;
    if (t.alloc((size_t)n_bytes + SLACK)) return 1;
    { KTimer kt("fa_h2d");
    if (n_bytes) HHX_HIP(hipMemcpyAsync(t.p, text, (size_t)n_bytes, hipMemcpyHostToDevice, g_stream)); }
    HHX_HIP(hipStreamSynchronize(g_stream));
    HHX_TRY(parse(f.get(), t.p, n_bytes, keep_letter_case != 0));
    *out = f.release();
    return 0;
}

extern "C" int hhx_fasta_open(const char *path, int keep_letter_case, hhx_fasta **out) {
    if (!out || !path) return fail("hhx_fasta_open: bad argument");
    struct stat sb;
    if (::stat(path, &sb) != 0) return fail("cannot open %s: %s", path, strerror(errno));
    if (!S_ISREG(sb.st_mode)) return unsupported("hhx_fasta_open: %s is not a regular file", path);
    const i64 n = (i64)sb.st_size;
    HHX_TRY(fits(n, "hhx_fasta_open"));
    std::unique_ptr<hhx_fasta> f(new hhx_fasta());
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
            if (at + m > n) { rc = fail("hhx_fasta_open: %s grew while it was read", path); break; }
            hipError_t e = hipMemcpyAsync(t.p + at, host, (size_t)m, hipMemcpyHostToDevice, g_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
            if (e != hipSuccess) { rc = fail("hhx_fasta_open: %s", hipGetErrorString(e)); break; }
            at += m;
        }
        if (!rc && at != n) rc = fail("hhx_fasta_open: %s shrank while it was read", path);
        const std::string err = g_err;
        (void)hhx_text_reader_close(r);
        if (rc) { g_err = err; return rc; }
    }
    HHX_TRY(parse(f.get(), t.p, n, keep_letter_case != 0));
    *out = f.release();
    return 0;
}

extern "C" int hhx_fasta_counts(const hhx_fasta *f, int64_t *n_ctg, int64_t *n_seq_bytes, int64_t *n_name_bytes) {
    if (!f) return fail("hhx_fasta_counts: null handle");
    if (n_ctg) *n_ctg = f->n_ctg;
    if (n_seq_bytes) *n_seq_bytes = f->n_seq;
    if (n_name_bytes) *n_name_bytes = f->h_name_off.back();
    return 0;
}

extern "C" int hhx_fasta_table(const hhx_fasta *f, int64_t *seq_off, int64_t *seq_len, int64_t *name_off, uint8_t *names) {
    if (!f) return fail("hhx_fasta_table: null handle");
    const size_t n = (size_t)f->n_ctg;
    if (seq_off && n) memcpy(seq_off, f->h_seq_off.data(), sizeof(i64) * n);
    if (seq_len && n) memcpy(seq_len, f->h_seq_len.data(), sizeof(i64) * n);
    if (name_off) memcpy(name_off, f->h_name_off.data(), sizeof(i64) * (n + 1));
    if (names && !f->h_names.empty()) memcpy(names, f->h_names.data(), f->h_names.size());
    return 0;
}

extern "C" int hhx_fasta_sequences(hhx_fasta *f, uint8_t *out) {
    if (!f) return fail("hhx_fasta_sequences: null handle");
    if (f->n_seq && !out) return fail("hhx_fasta_sequences: null pointer");
    if (f->n_seq) HHX_HIP(hipMemcpyAsync(out, f->bases(), (size_t)f->n_seq, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

// count_RE_sites :75-84 on the sequences where they lie: behind the n_seq bytes stand SEQ_PAD readable ones, which the matcher's core asks for
extern "C" int hhx_fasta_re_counts(hhx_fasta *f, int64_t n_seg, const int64_t *seg_off, const int64_t *seg_len, int32_t n_sites, const uint8_t *sites,
                                   const int32_t *site_len, int64_t *counts_host) {
    if (!f) return fail("hhx_fasta_re_counts: null handle");
    return hhx_count_re_sites_device("hhx_fasta_re_counts", f->bases(), f->n_seq, n_seg, seg_off, seg_len, n_sites, sites, site_len, counts_host);
}

extern "C" int hhx_fasta_fetch(hhx_fasta *f, int64_t off, int64_t len, uint8_t *out_host) {
    if (!f) return fail("hhx_fasta_fetch: null handle");
    if (off < 0 || len < 0 || len > f->n_seq || off > f->n_seq - len)
        return fail("hhx_fasta_fetch: bytes [%lld, +%lld) of %lld", (long long)off, (long long)len, (long long)f->n_seq);
    if (len == 0) return 0;
    if (!out_host) return fail("hhx_fasta_fetch: null pointer");
    HHX_HIP(hipMemcpyAsync(out_host, f->bases() + off, (size_t)len, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

namespace {

// the file of both emits from its tables: rec_off [n_rec + 1], rec_slen and rec_seg0 [n_rec + 1], seg_end with entry -1 in front, seg_src with one
// entry behind (EmitTab); slab by slab, each written while the next is produced
int emit_file(hhx_fasta *f, const char *path, i64 n_rec, const uint8_t *rec_names, const int64_t *rec_name_off, const std::vector<i64> &rec_off,
              const std::vector<i64> &rec_slen, const std::vector<i64> &rec_seg0, const std::vector<i64> &seg_end, const std::vector<i64> &seg_src, i64 W,
              int64_t *n_bytes) {
    const i64 total = rec_off[(size_t)n_rec];
    const i64 slab = std::min<i64>(slab_bytes(), std::max<i64>(16, (total + 15) & ~(i64)15));

    DevBuf<i64> d_rec_off, d_rec_slen, d_rec_seg0, d_name_off, d_seg_end, d_seg_src;
    DevBuf<unsigned char> d_names, buf[2];
    const std::vector<i64> name_off(rec_name_off, rec_name_off + (n_rec ? n_rec + 1 : 0));
    const std::vector<unsigned char> names(rec_names, rec_names + (n_rec ? rec_name_off[n_rec] : 0));
    if (total > 0) {
        if (upload(d_rec_off, rec_off) || upload(d_rec_slen, rec_slen) || upload(d_rec_seg0, rec_seg0) || upload(d_name_off, name_off) ||
            upload(d_seg_end, seg_end) || upload(d_seg_src, seg_src) || upload(d_names, names) || buf[0].alloc((size_t)slab) || buf[1].alloc((size_t)slab)) return 1;
        HHX_HIP(hipStreamSynchronize(g_stream));                 // the tables are up, and what the stream still did with recycled blocks is done
    }
    EmitStream es;                                               // (declared behind the buffers: it waits for its stream before they go back to the pool)
    FileSink sink;
    HHX_TRY(sink.open(path));
    int rc = 0;
    if (total > 0) {
        rc = es.open();
        const EmitTab T{n_rec, d_rec_off.p, d_rec_slen.p, d_rec_seg0.p, d_name_off.p, d_names.p, d_seg_end.p + 1, d_seg_src.p, W};
        const i64 n_slabs = (total + slab - 1) / slab;
        hipStream_t const caller = g_stream;
        auto launch = [&](i64 k) -> int {
            const i64 g0 = k * slab, g1 = std::min<i64>(total, g0 + slab);
            g_stream = es.s;                                     // (the timer records on the stream the kernel runs on)
            { KTimer kt("fa_emit");
            k_fa_emit<<<grid_for((g1 - g0 + 15) >> 4, 256), 256, 0, es.s>>>(T, f->bases(), g0, g1, buf[k & 1].p); }
            g_stream = caller;
            HHX_LAUNCH_CHECK();
            HHX_HIP(hipEventRecord(es.ev[k & 1], es.s));
            return 0;
        };
        if (!rc) rc = launch(0);
        for (i64 k = 0; k < n_slabs && !rc; ++k) {
            if (k + 1 < n_slabs) rc = launch(k + 1);             // its buffer was read last by the copy of slab k - 1, which write_device has waited for
            if (!rc && hipStreamWaitEvent(g_stream, es.ev[k & 1], 0) != hipSuccess) rc = fail("hhx_fasta_emit: hipStreamWaitEvent failed");
            if (!rc) rc = sink.write_device(buf[k & 1].p, (size_t)(std::min<i64>(total, (k + 1) * slab) - k * slab));
        }
    }
    const std::string err = g_err;
    const int rc_close = sink.close();
    if (rc) g_err = err;
    if (rc || rc_close) { (void)::unlink(path); return rc ? rc : rc_close; }
    if (n_bytes) *n_bytes = total;
    return 0;
}

}  // namespace

extern "C" int hhx_fasta_emit(hhx_fasta *f, const char *path, int64_t n_rec, const uint8_t *rec_names, const int64_t *rec_name_off, const int64_t *piece_off,
                              const int32_t *piece_ctg, const uint8_t *piece_rev, int64_t Ns, int64_t max_width, int64_t *n_bytes) {
    if (!f) return fail("hhx_fasta_emit: null handle");
    if (!path || n_rec < 0 || (n_rec && (!rec_name_off || !piece_off))) return fail("hhx_fasta_emit: bad argument");
    if (max_width < 1) return unsupported("hhx_fasta_emit: max_width %lld (the reference's range() raises or writes nothing)", (long long)max_width);
    if (Ns < 0 || Ns > SPAN_MAX >> 20) return unsupported("hhx_fasta_emit: Ns %lld", (long long)Ns);
    const i64 W = std::min<i64>(max_width, SPAN_MAX);
    const i64 n_pieces = n_rec ? piece_off[n_rec] : 0;
    if (n_rec && (rec_name_off[0] != 0 || piece_off[0] != 0 || (rec_name_off[n_rec] && !rec_names) || (n_pieces && (!piece_ctg || !piece_rev))))
        return fail("hhx_fasta_emit: bad argument");
    std::vector<i64> rec_off((size_t)n_rec + 1, 0), rec_slen((size_t)n_rec + 1, 0), rec_seg0((size_t)n_rec + 1, 0), seg_end, seg_src;
    seg_end.push_back(0);                                        // entry -1 of the first record's search
    for (i64 r = 0; r < n_rec; ++r) {
        const i64 name_len = rec_name_off[r + 1] - rec_name_off[r], np = piece_off[r + 1] - piece_off[r];
        if (name_len < 0 || np < 0) return fail("hhx_fasta_emit: offsets of record %lld run backwards", (long long)r);
        i64 x = 0;
        rec_seg0[(size_t)r] = (i64)seg_src.size();
        for (i64 k = piece_off[r]; k < piece_off[r + 1]; ++k) {
            const i64 c = piece_ctg[k];
            if (c < 0 || c >= f->n_ctg) return fail("hhx_fasta_emit: piece %lld names contig %lld of %lld", (long long)k, (long long)c, (long long)f->n_ctg);
            if (k > piece_off[r] && Ns > 0) { x += Ns; seg_end.push_back(x); seg_src.push_back(-1); }
            x += f->h_seq_len[(size_t)c];
            seg_end.push_back(x);
            seg_src.push_back(f->h_seq_off[(size_t)c] | ((i64)(piece_rev[k] ? 1 : 0) << 62));
            if (x > SPAN_MAX) return unsupported("hhx_fasta_emit: record %lld is longer than 2^60 bytes", (long long)r);
        }
        rec_slen[(size_t)r] = x;
        rec_off[(size_t)r + 1] = rec_off[(size_t)r] + name_len + 2 + x + (x + W - 1) / W;
        if (rec_off[(size_t)r + 1] > SPAN_MAX) return unsupported("hhx_fasta_emit: the file is longer than 2^60 bytes");
    }
    rec_seg0[(size_t)n_rec] = (i64)seg_src.size();
    seg_src.push_back(-1);                                       // seg_src is read as seg_end + 1 is: one entry behind
    return emit_file(f, path, n_rec, rec_names, rec_name_off, rec_off, rec_slen, rec_seg0, seg_end, seg_src, W, n_bytes);
}

// the FASTA half of order_and_orient_groups, scripts/HapHiC_refsort.py:269-342: the tables of k_fa_emit from sub-ranges and N runs, no joiner
extern "C" int hhx_fasta_emit_segments(hhx_fasta *f, const char *path, int64_t n_rec, const uint8_t *rec_names, const int64_t *rec_name_off,
                                       const int64_t *piece_off, const int32_t *piece_ctg, const int64_t *piece_start, const int64_t *piece_len,
                                       const uint8_t *piece_rev, int64_t max_width, int64_t *n_bytes) {
    if (!f) return fail("hhx_fasta_emit_segments: null handle");
    if (!path || n_rec < 0 || (n_rec && (!rec_name_off || !piece_off))) return fail("hhx_fasta_emit_segments: bad argument");
    if (max_width < 1) return unsupported("hhx_fasta_emit_segments: max_width %lld (the reference's range() raises or writes nothing)", (long long)max_width);
    const i64 W = std::min<i64>(max_width, SPAN_MAX);
    const i64 n_pieces = n_rec ? piece_off[n_rec] : 0;
    if (n_rec && (rec_name_off[0] != 0 || piece_off[0] != 0 || (rec_name_off[n_rec] && !rec_names) ||
                  (n_pieces && (!piece_ctg || !piece_start || !piece_len || !piece_rev))))
        return fail("hhx_fasta_emit_segments: bad argument");
    std::vector<i64> rec_off((size_t)n_rec + 1, 0), rec_slen((size_t)n_rec + 1, 0), rec_seg0((size_t)n_rec + 1, 0), seg_end, seg_src;
    seg_end.push_back(0);                                        // entry -1 of the first record's search
    for (i64 r = 0; r < n_rec; ++r) {
        const i64 name_len = rec_name_off[r + 1] - rec_name_off[r], np = piece_off[r + 1] - piece_off[r];
        if (name_len < 0 || np < 0) return fail("hhx_fasta_emit_segments: offsets of record %lld run backwards", (long long)r);
        i64 x = 0;
        rec_seg0[(size_t)r] = (i64)seg_src.size();
        for (i64 k = piece_off[r]; k < piece_off[r + 1]; ++k) {
            const i64 c = piece_ctg[k], m = piece_len[k];
            if (m < 0) return unsupported("hhx_fasta_emit_segments: piece %lld has length %lld", (long long)k, (long long)m);
            if (m > SPAN_MAX) return unsupported("hhx_fasta_emit_segments: record %lld is longer than 2^60 bytes", (long long)r);
            i64 src = -1;
            if (c >= 0) {
                if (c >= f->n_ctg) return fail("hhx_fasta_emit_segments: piece %lld names contig %lld of %lld", (long long)k, (long long)c, (long long)f->n_ctg);
                const i64 s = piece_start[k];
                if (s < 0 || s > f->h_seq_len[(size_t)c] || m > f->h_seq_len[(size_t)c] - s)
                    return unsupported("hhx_fasta_emit_segments: piece %lld, bytes [%lld, %lld + %lld), lies outside its contig of %lld bytes", (long long)k,
                                       (long long)s, (long long)s, (long long)m, (long long)f->h_seq_len[(size_t)c]);
                src = (f->h_seq_off[(size_t)c] + s) | ((i64)(piece_rev[k] ? 1 : 0) << 62);
            } else if (c != -1) {
                return fail("hhx_fasta_emit_segments: piece %lld names contig %lld (-1: a run of N)", (long long)k, (long long)c);
            }
            if (m == 0) continue;                                // contributes nothing: no segment
            x += m;
            if (x > SPAN_MAX) return unsupported("hhx_fasta_emit_segments: record %lld is longer than 2^60 bytes", (long long)r);
            seg_end.push_back(x);
            seg_src.push_back(src);
        }
        rec_slen[(size_t)r] = x;
        rec_off[(size_t)r + 1] = rec_off[(size_t)r] + name_len + 2 + x + (x + W - 1) / W;
        if (rec_off[(size_t)r + 1] > SPAN_MAX) return unsupported("hhx_fasta_emit_segments: the file is longer than 2^60 bytes");
    }
    rec_seg0[(size_t)n_rec] = (i64)seg_src.size();
    seg_src.push_back(-1);                                       // seg_src is read as seg_end + 1 is: one entry behind
    return emit_file(f, path, n_rec, rec_names, rec_name_off, rec_off, rec_slen, rec_seg0, seg_end, seg_src, W, n_bytes);
}

extern "C" int hhx_fasta_close(hhx_fasta *f) {
    delete f;
    return 0;
}
