// full_links.pkl / HT_links.pkl read back into the arrays they were written from (HapHiC_reassign.py parse_pickle :38-50 is `pickle.load`).
//
// The accepted stream (DESIGN.md "Reading the link pickles"): PROTO 4 | 5, an optional FRAME, the construction of
// collections.defaultdict(builtins.int) exactly as the pickler and csrc/hhx_files.hip spell it (memo slots 0-7), then the body
//     ( FRAME | MARK | SETITEMS | SETITEM | MEMOIZE | name name TUPLE2 value )*  STOP
// name = SHORT_BINUNICODE, or BINGET / LONG_BINGET of a slot a name literal was memoised into; value = BININT1 / BININT2 / BININT /
// LONG1 of at most 8 bytes / BINFLOAT.  The body is validated token by token with the state a sequential reader would hold (item
// phase, open MARK, items since the last MARK / SETITEM(S), the token before a MEMOIZE); whatever does not fit is reported as
// HHX_PICKLE_NOT_OURS and the caller runs pickle.load.
//
// Opcode boundaries: payloads hold every opcode byte, so where an opcode starts is only known from the start of the body.  The body is cut
// into chunks of C bytes (hhx_tune "pkl_chunk").  No accepted opcode is longer than 257 bytes, so a chunk is entered at one of the offsets
// 0 .. 256.  k_chunk_table builds, per chunk and in LDS, next[p] = p + (length of the opcode that would start at p) and squares that map
// until every p points past the chunk (pointer doubling, ceil(log2 C) rounds); the exits of the 257 possible entries are kept: F_c.
// The true entry of chunk c + 1 is F_c[entry_c]; the chain is followed in two levels (k_compose: the composition over 256 chunks for all
// 257 entries; k_chain: one thread over those; k_entries: back down).  k_walk then walks every chunk from its true entry, one thread per
// chunk, first to count tokens, then — with the running counts and the reader state at every chunk's entry scanned on the host — to
// validate and emit them.
//
// Every length read from the text is speculative until the walk gets there: it is at most 257 and checked against the end of the text
// before a byte is loaded through it.  Every walk moves at least one byte per step and stops at its chunk's end.  Every probe loop of the
// two hash tables is bounded.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <memory>

#include "hhx_internal.h"
#include "hhx_sort.h"
#include "hhx_textscan.h"

using namespace hhx;
using hhx::textscan::grid_for;
using hhx::textscan::hash_step;
using hhx::textscan::HASH_SEED;

namespace {

constexpr int N_ENTRY = 257;                  // offsets at which an opcode can reach into a chunk: 0 .. 256
constexpr int SUPER = 256;                    // chunks per step of the second level
constexpr int MAX_PROBE = 1 << 14;
constexpr i64 READ_CHUNK = (i64)64 << 20;
constexpr u64 EMPTY = ~0ull;

enum : u32 { ST_OPCODE = 1, ST_TRUNCATED = 2, ST_GRAMMAR = 4, ST_MEMO = 8, ST_PROBE = 16, ST_DUPLICATE = 32 };
enum : int { K_NONE, K_LIT, K_GET, K_TUPLE, K_VALUE, K_MARK, K_SETITEMS, K_SETITEM, K_MEMO, K_STOP, K_FRAME, K_BAD };

struct ChunkSum {                             // what the counting walk leaves per chunk
    i32 n_body, n_memo, n_frame;
    i32 since;                                // body tokens after the chunk's last MARK / SETITEM(S) (all of them if it has none)
    i64 last_pos;                             // the chunk's last token that is no FRAME ...
    i64 stop_pos;                             // where the walk met STOP, -1
    i32 last_kind;                            // ... K_NONE: the chunk has none
    i32 last_struct;                          // K_MARK / K_SETITEMS / K_SETITEM, K_NONE: none in this chunk
};
struct ChunkIn {                              // the reader's state at a chunk's entry
    i64 body_base, memo_base, frame_base, prev_pos;
    i32 since, last_struct, prev_kind, pad;
};

__device__ __forceinline__ int op_len(unsigned b0, unsigned b1) {
    switch (b0) {
    case 0x8c: case 0x8a: return 2 + (int)b1;             // SHORT_BINUNICODE, LONG1
    case 'h': case 'K': return 2;                         // BINGET, BININT1
    case 'M': return 3;                                   // BININT2
    case 'j': case 'J': return 5;                         // LONG_BINGET, BININT
    case 'G': case 0x95: return 9;                        // BINFLOAT, FRAME
    default: return 1;
    }
}
__device__ __forceinline__ int op_kind(unsigned b0, unsigned b1) {
    switch (b0) {
    case 0x8c: return K_LIT;
    case 'h': case 'j': return K_GET;
    case 0x86: return K_TUPLE;
    case 'K': case 'M': case 'J': case 'G': return K_VALUE;
    case 0x8a: return b1 <= 8 ? K_VALUE : K_BAD;
    case '(': return K_MARK;
    case 'u': return K_SETITEMS;
    case 's': return K_SETITEM;
    case 0x94: return K_MEMO;
    case '.': return K_STOP;
    case 0x95: return K_FRAME;
    default: return K_BAD;
    }
}

// F[c][e] = where the opcode chain that enters chunk c at offset e leaves it, as an offset into chunk c + 1
__global__ __launch_bounds__(256) void k_chunk_table(const unsigned char *__restrict__ t, i64 n, int C, i64 n_chunks, int rounds,
                                                     unsigned short *__restrict__ F) {
    extern __shared__ unsigned short jump[];
    for (i64 c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const i64 base = c * C;
        for (int p = threadIdx.x; p < C; p += 256) {
            const i64 g = base + p;
            int nxt = C;                                  // past the end of the text: nothing to walk
            if (g < n) nxt = p + op_len(t[g], g + 1 < n ? t[g + 1] : 0u);          // <= C + 256
            jump[p] = (unsigned short)nxt;
        }
        __syncthreads();
        // a value read while its owner replaces it is the old or the new one: both lie on the chain of p, the new one further along
        for (int r = 0; r < rounds; ++r) {
            for (int p = threadIdx.x; p < C; p += 256) {
                const int j = jump[p];
                if (j < C) jump[p] = jump[j];
            }
            __syncthreads();
        }
        for (int e = threadIdx.x; e < N_ENTRY; e += 256) {
            const int j = jump[e];
            F[c * N_ENTRY + e] = (unsigned short)(j >= C ? min(j - C, N_ENTRY - 1) : 0);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_compose(const unsigned short *__restrict__ F, i64 n_chunks, i64 n_super, unsigned short *__restrict__ G) {
    for (i64 id = (i64)blockIdx.x * 256 + threadIdx.x; id < n_super * N_ENTRY; id += (i64)gridDim.x * 256) {
        const i64 sc = id / N_ENTRY;
        int x = (int)(id - sc * N_ENTRY);
        const i64 c1 = min(n_chunks, (sc + 1) * SUPER);
        for (i64 c = sc * SUPER; c < c1; ++c) x = F[c * N_ENTRY + x];
        G[id] = (unsigned short)x;
    }
}
__global__ void k_chain(const unsigned short *__restrict__ G, i64 n_super, unsigned short *__restrict__ entry_super) {
    if (blockIdx.x || threadIdx.x) return;
    int x = 0;
    for (i64 sc = 0; sc < n_super; ++sc) { entry_super[sc] = (unsigned short)x; x = G[sc * N_ENTRY + x]; }
}
__global__ __launch_bounds__(256) void k_entries(const unsigned short *__restrict__ F, i64 n_chunks, i64 n_super, const unsigned short *__restrict__ entry_super,
                                                 unsigned short *__restrict__ entry) {
    for (i64 sc = (i64)blockIdx.x * 256 + threadIdx.x; sc < n_super; sc += (i64)gridDim.x * 256) {
        int x = entry_super[sc];
        const i64 c1 = min(n_chunks, (sc + 1) * SUPER);
        for (i64 c = sc * SUPER; c < c1; ++c) { entry[c] = (unsigned short)x; x = F[c * N_ENTRY + x]; }
    }
}

struct EmitOut {
    i64 *tok;                                 // [2 * key + side]: position of the name literal, or -(slot - 8) - 1 of a memo reference
    i64 *val;                                 // the value's 64 bits (two's complement, or IEEE-754)
    unsigned char *isf;
    i64 *memo_src;                            // per memo slot from 8 on: position of the literal it holds, -1 a tuple
    i64 *frames;                              // (position, length) of every FRAME
    u32 *info;                                // [0] status bits, [1] any float
};

// one thread per chunk.  EMIT = false: the counts and the chunk's last tokens; EMIT = true: the same walk with the reader's state at the entry
template <bool EMIT>
__global__ __launch_bounds__(256) void k_walk(const unsigned char *__restrict__ t, i64 n, int C, i64 n_chunks, const unsigned short *__restrict__ entry,
                                              ChunkSum *__restrict__ sums, const ChunkIn *__restrict__ ins, EmitOut o, u32 *__restrict__ status) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < n_chunks; c += (i64)gridDim.x * 256) {
        const i64 end = min(n, (c + 1) * C);
        i64 p = c * C + entry[c];
        u32 st = 0;
        i32 n_body = 0, n_memo = 0, n_frame = 0, since = 0, last_kind = K_NONE, last_struct = K_NONE;
        i64 last_pos = -1, stop_pos = -1;
        i64 b = 0, m = 0, f = 0;
        if (EMIT) {
            const ChunkIn in = ins[c];
            b = in.body_base; m = in.memo_base; f = in.frame_base;
            since = in.since; last_struct = in.last_struct; last_kind = in.prev_kind; last_pos = in.prev_pos;
        }
        while (p < end) {
            const unsigned b0 = t[p], b1 = p + 1 < n ? t[p + 1] : 0u;
            const int len = op_len(b0, b1);
            if (p + len > n) { st |= ST_TRUNCATED; break; }
            const int kind = op_kind(b0, b1);
            if (kind == K_BAD) { st |= ST_OPCODE; break; }
            if (EMIT) {
                const int role = (int)(b & 3);
                const bool batch = last_struct == K_MARK;
                switch (kind) {
                case K_LIT: case K_GET: {
                    if (role > 1 || (role == 0 && !batch && since != 0)) st |= ST_GRAMMAR;
                    i64 tok = p;
                    if (kind == K_GET) {
                        i64 slot = b1;
                        if (b0 == 'j') slot = (i64)((u32)t[p + 1] | (u32)t[p + 2] << 8 | (u32)t[p + 3] << 16 | (u32)t[p + 4] << 24);
                        if (slot < 8 || slot - 8 >= m) { st |= ST_MEMO; slot = 8; }
                        tok = -(slot - 8) - 1;
                    }
                    o.tok[2 * (b >> 2) + (role & 1)] = tok;
                    break;
                }
                case K_TUPLE:
                    if (role != 2) st |= ST_GRAMMAR;
                    break;
                case K_VALUE: {
                    if (role != 3) st |= ST_GRAMMAR;
                    u64 v = 0;
                    unsigned char isf = 0;
                    if (b0 == 'K') v = b1;
                    else if (b0 == 'M') v = (u64)b1 | (u64)t[p + 2] << 8;
                    else if (b0 == 'J') v = (u64)(i64)(i32)((u32)b1 | (u32)t[p + 2] << 8 | (u32)t[p + 3] << 16 | (u32)t[p + 4] << 24);
                    else if (b0 == 'G') { for (int q = 0; q < 8; ++q) v = v << 8 | t[p + 1 + q]; isf = 1; }
                    else {                                                        // LONG1: little-endian two's complement of b1 <= 8 bytes
                        for (int q = 0; q < (int)b1; ++q) v |= (u64)t[p + 2 + q] << (8 * q);
                        if (b1 > 0 && b1 < 8 && (t[p + 1 + b1] & 0x80)) v |= ~0ull << (8 * b1);
                    }
                    o.val[b >> 2] = (i64)v;
                    o.isf[b >> 2] = isf;
                    if (isf) o.info[1] = 1;
                    break;
                }
                case K_MARK:
                    if (role != 0 || batch || since != 0) st |= ST_GRAMMAR;
                    break;
                case K_SETITEMS:
                    if (role != 0 || !batch) st |= ST_GRAMMAR;
                    break;
                case K_SETITEM:
                    if (role != 0 || batch || since != 4) st |= ST_GRAMMAR;
                    break;
                case K_MEMO:
                    if (last_kind != K_LIT && last_kind != K_TUPLE) st |= ST_GRAMMAR;
                    o.memo_src[m] = last_kind == K_LIT ? last_pos : -1;
                    break;
                case K_STOP:
                    if (role != 0 || batch || since != 0) st |= ST_GRAMMAR;
                    break;
                case K_FRAME: {
                    u64 v = 0;
                    for (int q = 7; q >= 0; --q) v = v << 8 | t[p + 1 + q];
                    o.frames[2 * f] = p;
                    o.frames[2 * f + 1] = (i64)min(v, (u64)INT64_MAX);
                    break;
                }
                }
            }
            if (kind == K_FRAME) { ++n_frame; ++f; }
            else {
                if (kind <= K_VALUE) { ++n_body; ++b; if (since < (1 << 30)) ++since; }
                else if (kind == K_MEMO) { ++n_memo; ++m; }
                else if (kind != K_STOP) { last_struct = kind; since = 0; }
                last_kind = kind;
                last_pos = p;
            }
            p += len;                                                             // len >= 1
            if (kind == K_STOP) { stop_pos = p - 1; break; }
        }
        if (!EMIT) sums[c] = ChunkSum{n_body, n_memo, n_frame, since, last_pos, stop_pos, last_kind, last_struct};
        if (st) atomicOr(status, st);
    }
}

__device__ __forceinline__ u64 name_hash(const unsigned char *__restrict__ t, i64 pos) {
    const int len = t[pos + 1];
    u64 h = HASH_SEED;
    for (int q = 0; q < len; q += 8) {
        u64 w = 0;
        for (int r = 0; r < 8 && q + r < len; ++r) w |= (u64)t[pos + 2 + q + r] << (8 * r);
        h = hash_step(h, w);
    }
    return hash_step(h, (u64)len);
}
__device__ __forceinline__ bool same_name(const unsigned char *__restrict__ t, i64 a, i64 b) {
    if (a == b) return true;
    const int len = t[a + 1];
    if (t[b + 1] != len) return false;
    for (int q = 0; q < len; ++q)
        if (t[a + 2 + q] != t[b + 2 + q]) return false;
    return true;
}

// slots[s] = the smallest literal position among the literals of one content (byte-verified; EMPTY: free)
__global__ __launch_bounds__(256) void k_name_insert(const unsigned char *__restrict__ t, const i64 *__restrict__ tok, i64 n_tok, unsigned long long *slots, u32 mask,
                                                     u32 *info) {
    for (i64 id = (i64)blockIdx.x * 256 + threadIdx.x; id < n_tok; id += (i64)gridDim.x * 256) {
        const i64 pos = tok[id];
        if (pos < 0) continue;
        u32 s = (u32)name_hash(t, pos) & mask;
        bool done = false;
        for (int probe = 0; probe < MAX_PROBE && !done; ++probe, s = (s + 1) & mask) {
            u64 cur = __atomic_load_n(&slots[s], __ATOMIC_RELAXED);
            if (cur == EMPTY) {
                cur = atomicCAS(&slots[s], (unsigned long long)EMPTY, (unsigned long long)pos);
                if (cur == EMPTY) { atomicAdd(&info[2], 1u); done = true; break; }
            }
            if (same_name(t, (i64)cur, pos)) {
                if ((u64)pos < cur) atomicMin(&slots[s], (unsigned long long)pos);
                done = true;
            }
        }
        if (!done) atomicOr(&info[0], ST_PROBE);
    }
}
// every name token -> the smallest literal position of its content
__global__ __launch_bounds__(256) void k_name_canon(const unsigned char *__restrict__ t, i64 *__restrict__ tok, i64 n_tok, const i64 *__restrict__ memo_src,
                                                    const unsigned long long *__restrict__ slots, u32 mask, u32 *info) {
    for (i64 id = (i64)blockIdx.x * 256 + threadIdx.x; id < n_tok; id += (i64)gridDim.x * 256) {
        i64 pos = tok[id];
        if (pos < 0) pos = memo_src[-pos - 1];
        if (pos < 0) { atomicOr(&info[0], ST_MEMO); tok[id] = 0; continue; }                 // the slot holds a tuple
        u32 s = (u32)name_hash(t, pos) & mask;
        i64 found = -1;
        for (int probe = 0; probe < MAX_PROBE; ++probe, s = (s + 1) & mask) {
            const u64 cur = slots[s];
            if (cur == EMPTY) break;
            if (same_name(t, (i64)cur, pos)) { found = (i64)cur; break; }
        }
        if (found < 0) { atomicOr(&info[0], ST_PROBE); found = 0; }
        tok[id] = found;
    }
}
__global__ __launch_bounds__(256) void k_collect(const unsigned long long *__restrict__ slots, i64 cap, i64 *__restrict__ list, i64 n_list, u32 *info) {
    for (i64 s = (i64)blockIdx.x * 256 + threadIdx.x; s < cap; s += (i64)gridDim.x * 256)
        if (slots[s] != EMPTY) {
            const u32 at = atomicAdd(&info[3], 1u);
            if ((i64)at < n_list) list[at] = (i64)slots[s];
        }
}
// name id = rank of the canonical position among the sorted distinct ones: the order of first appearance
__global__ __launch_bounds__(256) void k_rank(const i64 *__restrict__ tok, i64 n_keys, const i64 *__restrict__ uniq, i64 n_uniq, i32 *__restrict__ id_i,
                                              i32 *__restrict__ id_j) {
    for (i64 id = (i64)blockIdx.x * 256 + threadIdx.x; id < 2 * n_keys; id += (i64)gridDim.x * 256) {
        const i64 pos = tok[id];
        i64 lo = 0, hi = n_uniq;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (uniq[mid] < pos) lo = mid + 1; else hi = mid;
        }
        ((id & 1) ? id_j : id_i)[id >> 1] = (i32)min(lo, n_uniq - 1);
    }
}
__global__ __launch_bounds__(256) void k_name_len(const unsigned char *__restrict__ t, const i64 *__restrict__ uniq, i64 n_uniq, i32 *__restrict__ len) {
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < n_uniq; k += (i64)gridDim.x * 256) len[k] = t[uniq[k] + 1];
}
__global__ __launch_bounds__(256) void k_name_gather(const unsigned char *__restrict__ t, const i64 *__restrict__ uniq, i64 n_uniq, const i64 *__restrict__ off,
                                                     unsigned char *__restrict__ blob) {
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < n_uniq; k += (i64)gridDim.x * 256) {
        const i64 a = uniq[k] + 2, d = off[k];
        const int len = (int)(off[k + 1] - d);
        for (int q = 0; q < len; ++q) blob[d + q] = t[a + q];
    }
}
// a key written twice would be one entry of the dict: not a file this reader answers
__global__ __launch_bounds__(256) void k_dup_keys(const i32 *__restrict__ id_i, const i32 *__restrict__ id_j, i64 n_keys, unsigned long long *set, u64 mask, u32 *info) {
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < n_keys; k += (i64)gridDim.x * 256) {
        const u64 key = (u64)(u32)id_i[k] << 32 | (u32)id_j[k];
        u64 s = hash_step(HASH_SEED, key) & mask;
        bool done = false;
        for (int probe = 0; probe < MAX_PROBE && !done; ++probe, s = (s + 1) & mask) {
            const u64 old = atomicCAS(&set[s], (unsigned long long)EMPTY, (unsigned long long)key);
            if (old == EMPTY) done = true;
            else if (old == key) { atomicOr(&info[0], ST_DUPLICATE); done = true; }
        }
        if (!done) atomicOr(&info[0], ST_PROBE);
    }
}

const unsigned char k_head[] = "\x8c\x0b" "collections" "\x94" "\x8c\x0b" "defaultdict" "\x94" "\x93" "\x94"      // STACK_GLOBAL, memo 0-2
                               "\x8c\x08" "builtins" "\x94" "\x8c\x03" "int" "\x94" "\x93" "\x94"                 // memo 3-5
                               "\x85\x94" "R\x94";                                                                // TUPLE1 (6), REDUCE (7)
constexpr size_t HEAD_LEN = sizeof k_head - 1;

int not_ours(const char *why) {
    fail("not a link pickle this reader answers: %s", why);
    return HHX_PICKLE_NOT_OURS;
}
int status_not_ours(u32 st) {
    return not_ours(st & ST_TRUNCATED ? "the file ends inside an opcode" : st & ST_OPCODE ? "an opcode outside the link-table grammar"
                    : st & ST_MEMO ? "a memo reference to something that is no name" : st & ST_DUPLICATE ? "a key is written twice"
                    : "the opcodes do not form name, name, TUPLE2, value items in MARK .. SETITEMS batches");
}

}  // namespace

struct hhx_pickle {
    i64 n_keys = 0, names_bytes = 0;
    i32 n_names = 0;
    int any_float = 0;
    DevBuf<i32> id_i, id_j;
    DevBuf<i64> val;
    DevBuf<unsigned char> isf, blob;
    std::vector<i64> name_off;
    // the last hhx_pickle_group_heads: the group's edges in the reference's order
    i64 heads_n = 0;
    DevBuf<i32> heads_i, heads_j;
    DevBuf<u64> heads_w;
};

static int pickle_read(const char *path, hhx_pickle *h) {
    struct stat sb;
    if (::stat(path, &sb) != 0) return fail("cannot open %s: %s", path, strerror(errno));
    const i64 size = (i64)sb.st_size;
    size_t mem_free = 0, mem_total = 0;
    HHX_HIP(hipMemGetInfo(&mem_free, &mem_total));
    if (size > (i64)(mem_total / 2)) return not_ours("the file is larger than half of the device's memory");
    if (size < (i64)(2 + HEAD_LEN + 1)) return not_ours("the file is shorter than the header of a defaultdict(int)");

    // the file into HBM through the pinned read-ahead
    DevBuf<unsigned char> text;
    if (text.alloc((size_t)size)) return 1;
    unsigned char head[2 + 9 + HEAD_LEN];
    {
        hhx_text_reader *r = nullptr;
        HHX_TRY(hhx_text_reader_open_raw(path, std::min<i64>(READ_CHUNK, size), 0, &r));
        i64 at = 0;
        int rc = 0;
        for (;;) {
            const uint8_t *host = nullptr;
            i64 nb = 0;
            if ((rc = hhx_text_reader_next(r, &host, &nb)) != 0 || nb == 0) break;
            if (at + nb > size) { rc = fail("%s grew while it was read", path); break; }
            if (at < (i64)sizeof head) memcpy(head + at, host, (size_t)std::min<i64>(nb, (i64)sizeof head - at));
            if (hipMemcpyAsync(text.p + at, host, (size_t)nb, hipMemcpyHostToDevice, g_stream) != hipSuccess || hipStreamSynchronize(g_stream) != hipSuccess) {
                rc = fail("copying %s to the device failed: %s", path, hipGetErrorString(hipGetLastError()));
                break;
            }
            at += nb;
        }
        const std::string err = g_err;
        (void)hhx_text_reader_close(r);
        if (rc) { g_err = err; return rc; }
        if (at != size) return fail("%s shrank while it was read", path);
    }

    // PROTO, an optional FRAME, the construction of the defaultdict: host
    if (head[0] != 0x80 || (head[1] != 4 && head[1] != 5)) return not_ours("not pickle protocol 4 or 5");
    std::vector<i64> frames;                                                       // (absolute position, length) ...
    i64 body0 = 2;
    if (head[2] == 0x95) {
        if (size < (i64)sizeof head) return not_ours("the file is shorter than the header of a defaultdict(int)");
        u64 v = 0;
        for (int q = 7; q >= 0; --q) v = v << 8 | head[3 + q];
        frames.push_back(2);
        frames.push_back((i64)std::min<u64>(v, (u64)INT64_MAX));
        body0 = 11;
    }
    if (memcmp(head + body0, k_head, HEAD_LEN) != 0) return not_ours("the object is not built as collections.defaultdict(builtins.int)");
    body0 += (i64)HEAD_LEN;

    const unsigned char *t = text.p + body0;
    const i64 n = size - body0;
    if (n < 1) return not_ours("the file ends before STOP");
    const int C = (int)std::min<i64>(16384, std::max<i64>(512, tune_get("pkl_chunk", 4096)));
    const i64 n_chunks = (n + C - 1) / C, n_super = (n_chunks + SUPER - 1) / SUPER;
    int rounds = 1;
    while ((1 << rounds) < C) ++rounds;

    DevBuf<unsigned short> entry;
    DevBuf<u32> info;
    if (entry.alloc((size_t)n_chunks) || info.alloc(4)) return 1;
    HHX_HIP(hipMemsetAsync(info.p, 0, 4 * sizeof(u32), g_stream));
    {
        DevBuf<unsigned short> F, G, entry_super;
        if (F.alloc((size_t)n_chunks * N_ENTRY) || G.alloc((size_t)n_super * N_ENTRY) || entry_super.alloc((size_t)n_super)) return 1;
        KTimer kt("pkl_boundaries", 4);
        k_chunk_table<<<grid_for(n_chunks, 1), 256, (size_t)C * sizeof(unsigned short), g_stream>>>(t, n, C, n_chunks, rounds, F.p);
        HHX_LAUNCH_CHECK();
        k_compose<<<grid_for(n_super * N_ENTRY, 256), 256, 0, g_stream>>>(F.p, n_chunks, n_super, G.p);
        k_chain<<<1, 64, 0, g_stream>>>(G.p, n_super, entry_super.p);
        k_entries<<<grid_for(n_super, 256), 256, 0, g_stream>>>(F.p, n_chunks, n_super, entry_super.p, entry.p);
        HHX_LAUNCH_CHECK();
    }

    // the counting walk, and the reader's state at every chunk's entry
    DevBuf<ChunkSum> sums;
    DevBuf<ChunkIn> ins;
    if (sums.alloc((size_t)n_chunks) || ins.alloc((size_t)n_chunks)) return 1;
    std::vector<ChunkSum> hs((size_t)n_chunks);
    u32 hinfo[4] = {0, 0, 0, 0};
    {
        KTimer kt("pkl_walk");
        k_walk<false><<<grid_for(n_chunks, 256), 256, 0, g_stream>>>(t, n, C, n_chunks, entry.p, sums.p, nullptr, EmitOut{}, info.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipMemcpyAsync(hs.data(), sums.p, sizeof(ChunkSum) * (size_t)n_chunks, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (hinfo[0]) return status_not_ours(hinfo[0]);
    std::vector<ChunkIn> hi((size_t)n_chunks);
    i64 n_body = 0, n_memo = 0, n_frame = 0, since = 0, prev_pos = -1, stop_pos = -1;
    i32 last_struct = K_NONE, prev_kind = K_NONE;                                 // (the REDUCE's MEMOIZE ends the header: a MEMOIZE first in the body has no token to hold)
    for (i64 c = 0; c < n_chunks; ++c) {
        const ChunkSum &s = hs[(size_t)c];
        hi[(size_t)c] = ChunkIn{n_body, n_memo, n_frame, prev_pos, (i32)std::min<i64>(since, 8), last_struct, prev_kind, 0};
        if (stop_pos >= 0) return not_ours("bytes after STOP");
        n_body += s.n_body; n_memo += s.n_memo; n_frame += s.n_frame;
        if (s.last_struct != K_NONE) { last_struct = s.last_struct; since = s.since; } else since += s.n_body;
        if (s.last_kind != K_NONE) { prev_kind = s.last_kind; prev_pos = s.last_pos; }
        stop_pos = s.stop_pos;
    }
    if (stop_pos < 0) return not_ours("the file ends before STOP");
    if (stop_pos != n - 1) return not_ours("bytes after STOP");
    if (n_body & 3) return not_ours("the opcodes do not form name, name, TUPLE2, value items");
    const i64 n_keys = n_body >> 2;
    if (n_memo > (i64)UINT32_MAX - 8) return not_ours("more memo slots than LONG_BINGET addresses");

    // the validating walk
    DevBuf<i64> tok, memo_src, dframes;
    if (tok.alloc((size_t)(2 * n_keys)) || h->val.alloc((size_t)n_keys) || h->isf.alloc((size_t)n_keys) || memo_src.alloc((size_t)n_memo) ||
        dframes.alloc((size_t)(2 * n_frame)))
        return 1;
    HHX_HIP(hipMemcpyAsync(ins.p, hi.data(), sizeof(ChunkIn) * (size_t)n_chunks, hipMemcpyHostToDevice, g_stream));
    {
        KTimer kt("pkl_walk");
        k_walk<true><<<grid_for(n_chunks, 256), 256, 0, g_stream>>>(t, n, C, n_chunks, entry.p, nullptr, ins.p,
                                                                    EmitOut{tok.p, h->val.p, h->isf.p, memo_src.p, dframes.p, info.p}, info.p);
        HHX_LAUNCH_CHECK();
    }
    const size_t frames_head = frames.size();
    frames.resize(frames_head + (size_t)(2 * n_frame));
    if (n_frame) HHX_HIP(hipMemcpyAsync(frames.data() + frames_head, dframes.p, sizeof(i64) * (size_t)(2 * n_frame), hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (hinfo[0]) return status_not_ours(hinfo[0]);
    h->any_float = (int)hinfo[1];
    // frames, if the file has any, must tile it from the byte after PROTO to its end
    for (size_t k = frames_head; k < frames.size(); k += 2) frames[k] += body0;
    for (size_t k = 0; k < frames.size(); k += 2) {
        const i64 pos = frames[k], len = frames[k + 1];
        const i64 next = k + 2 < frames.size() ? frames[k + 2] : size;
        if ((k == 0 && pos != 2) || len > size || pos + 9 + len != next) return not_ours("the frames do not tile the file");
    }

    // names: one id per distinct content, in order of first appearance
    std::vector<i64> uniq;
    {
        KTimer kt("pkl_names");
        u64 want = 16;
        while (want < 2 * (u64)(2 * n_keys) + 2) want <<= 1;                       // every name token a literal of its own: the table is never more than half full
        DevBuf<unsigned long long> slots;
        u64 cap = std::min<u64>(want, (u64)1 << 21);
        for (;;) {
            if (slots.alloc((size_t)cap)) return 1;
            HHX_HIP(hipMemsetAsync(slots.p, 0xff, sizeof(u64) * (size_t)cap, g_stream));
            HHX_HIP(hipMemsetAsync(info.p, 0, 4 * sizeof(u32), g_stream));
            if (n_keys) k_name_insert<<<grid_for(2 * n_keys, 256), 256, 0, g_stream>>>(t, tok.p, 2 * n_keys, slots.p, (u32)(cap - 1), info.p);
            HHX_LAUNCH_CHECK();
            HHX_HIP(hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipStreamSynchronize(g_stream));
            if (!(hinfo[0] & ST_PROBE) && (u64)hinfo[2] * 2 <= cap) break;
            if (cap >= want) return fail("hhx_pickle_open: the name table of %llu slots overflowed", (unsigned long long)cap);
            cap = std::min<u64>(want, cap << 3);                                  // more distinct names than the first table holds well
        }
        const i64 n_uniq = (i64)hinfo[2];
        if (n_uniq > INT32_MAX) return not_ours("more than 2^31 names");
        if (n_keys) k_name_canon<<<grid_for(2 * n_keys, 256), 256, 0, g_stream>>>(t, tok.p, 2 * n_keys, memo_src.p, slots.p, (u32)(cap - 1), info.p);
        DevBuf<i64> list;
        if (list.alloc((size_t)n_uniq)) return 1;
        k_collect<<<grid_for((i64)cap, 256), 256, 0, g_stream>>>(slots.p, (i64)cap, list.p, n_uniq, info.p);
        HHX_LAUNCH_CHECK();
        uniq.resize((size_t)n_uniq);
        if (n_uniq) HHX_HIP(hipMemcpyAsync(uniq.data(), list.p, sizeof(i64) * (size_t)n_uniq, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        if (hinfo[0] & ST_PROBE) return fail("hhx_pickle_open: a name is missing from the name table");
        if (hinfo[0]) return status_not_ours(hinfo[0]);
        if ((i64)hinfo[3] != n_uniq) return fail("hhx_pickle_open: the name table holds %u names, %lld were counted", hinfo[3], (long long)n_uniq);
        std::sort(uniq.begin(), uniq.end());
        // ids, name lengths and bytes
        DevBuf<i64> duniq, doff;
        DevBuf<i32> dlen;
        if (duniq.alloc((size_t)n_uniq) || doff.alloc((size_t)n_uniq + 1) || dlen.alloc((size_t)n_uniq) || h->id_i.alloc((size_t)n_keys) || h->id_j.alloc((size_t)n_keys)) return 1;
        std::vector<i32> len((size_t)n_uniq);
        h->name_off.assign((size_t)n_uniq + 1, 0);
        if (n_uniq) {
            HHX_HIP(hipMemcpyAsync(duniq.p, uniq.data(), sizeof(i64) * (size_t)n_uniq, hipMemcpyHostToDevice, g_stream));
            if (n_keys) k_rank<<<grid_for(2 * n_keys, 256), 256, 0, g_stream>>>(tok.p, n_keys, duniq.p, n_uniq, h->id_i.p, h->id_j.p);
            k_name_len<<<grid_for(n_uniq, 256), 256, 0, g_stream>>>(t, duniq.p, n_uniq, dlen.p);
            HHX_LAUNCH_CHECK();
            HHX_HIP(hipMemcpyAsync(len.data(), dlen.p, sizeof(i32) * (size_t)n_uniq, hipMemcpyDeviceToHost, g_stream));
            HHX_HIP(hipStreamSynchronize(g_stream));
            for (i64 k = 0; k < n_uniq; ++k) h->name_off[(size_t)k + 1] = h->name_off[(size_t)k] + len[(size_t)k];
        }
        h->names_bytes = h->name_off[(size_t)n_uniq];
        if (h->blob.alloc((size_t)h->names_bytes)) return 1;
        if (n_uniq) {
            HHX_HIP(hipMemcpyAsync(doff.p, h->name_off.data(), sizeof(i64) * ((size_t)n_uniq + 1), hipMemcpyHostToDevice, g_stream));
            k_name_gather<<<grid_for(n_uniq, 256), 256, 0, g_stream>>>(t, duniq.p, n_uniq, doff.p, h->blob.p);
            HHX_LAUNCH_CHECK();
            HHX_HIP(hipStreamSynchronize(g_stream));                              // doff / duniq are read until here
        }
        h->n_names = (i32)n_uniq;
    }
    h->n_keys = n_keys;
    if (n_keys) {
        KTimer kt("pkl_keys");
        u64 cap = 16;
        while (cap < 2 * (u64)n_keys + 2) cap <<= 1;
        DevBuf<unsigned long long> set;
        if (set.alloc((size_t)cap)) return 1;
        HHX_HIP(hipMemsetAsync(set.p, 0xff, sizeof(u64) * (size_t)cap, g_stream));
        HHX_HIP(hipMemsetAsync(info.p, 0, 4 * sizeof(u32), g_stream));
        k_dup_keys<<<grid_for(n_keys, 256), 256, 0, g_stream>>>(h->id_i.p, h->id_j.p, n_keys, set.p, cap - 1, info.p);
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
        if (hinfo[0] & ST_PROBE) return fail("hhx_pickle_open: the key table of %llu slots overflowed", (unsigned long long)cap);
        if (hinfo[0]) return status_not_ours(hinfo[0]);
    }
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}

extern "C" int hhx_pickle_open(const char *path, hhx_pickle **out) {
    if (!path || !out) return fail("hhx_pickle_open: null pointer");
    *out = nullptr;
    std::unique_ptr<hhx_pickle> h(new hhx_pickle());
    const int rc = pickle_read(path, h.get());
    if (rc) return rc;
    *out = h.release();
    return 0;
}

extern "C" int hhx_pickle_sizes(hhx_pickle *p, int64_t *n_keys, int32_t *n_names, int64_t *names_bytes, int *any_float) {
    if (!p) return fail("hhx_pickle_sizes: null handle");
    if (n_keys) *n_keys = p->n_keys;
    if (n_names) *n_names = p->n_names;
    if (names_bytes) *names_bytes = p->names_bytes;
    if (any_float) *any_float = p->any_float;
    return 0;
}

extern "C" int hhx_pickle_fetch(hhx_pickle *p, int32_t *name_i, int32_t *name_j, int64_t *value_bits, uint8_t *is_float, uint8_t *names_blob, int64_t *name_off) {
    if (!p) return fail("hhx_pickle_fetch: null handle");
    const size_t n = (size_t)p->n_keys;
    if (n && name_i) HHX_HIP(hipMemcpyAsync(name_i, p->id_i.p, sizeof(i32) * n, hipMemcpyDeviceToHost, g_stream));
    if (n && name_j) HHX_HIP(hipMemcpyAsync(name_j, p->id_j.p, sizeof(i32) * n, hipMemcpyDeviceToHost, g_stream));
    if (n && value_bits) HHX_HIP(hipMemcpyAsync(value_bits, p->val.p, sizeof(i64) * n, hipMemcpyDeviceToHost, g_stream));
    if (n && is_float) HHX_HIP(hipMemcpyAsync(is_float, p->isf.p, n, hipMemcpyDeviceToHost, g_stream));
    if (p->names_bytes && names_blob) HHX_HIP(hipMemcpyAsync(names_blob, p->blob.p, (size_t)p->names_bytes, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    if (name_off) memcpy(name_off, p->name_off.data(), sizeof(i64) * p->name_off.size());
    return 0;
}

extern "C" int hhx_pickle_free(hhx_pickle *p) {
    delete p;
    return 0;
}

// ------------------------------------------------------------------ the handle of the reassignment rounds from the open table
// What parse_link_dict's mirror (haphic_amd/reassign.py) decides on host arrays before it builds a handle — a key that names one contig twice, totals
// that leave the exact range of float64 — decided here in one pass over id_i / id_j / val / isf where they lie.  The total cannot wrap: the low and
// the high 32 bits of the non-negative integer values are added apart, each sum below 2^63 for fewer than 2^31 keys, and put together on the host.
namespace {

constexpr int RC_T = 256;
constexpr unsigned RC_GRID = 256 * 8;         // eight workgroups a CU keep the three streams in flight (hhx_tune "reassign_check_grid": fewer)
enum { RC_LO = 0, RC_HI, RC_FLAGS, RC_WORDS };

__global__ __launch_bounds__(RC_T) void k_reassign_check(const i32 *__restrict__ id_i, const i32 *__restrict__ id_j, const i64 *__restrict__ val,
                                                         const unsigned char *__restrict__ isf, i64 n, unsigned long long *__restrict__ out) {
    __shared__ i64 s_lo[RC_T / HHX_WAVE], s_hi[RC_T / HHX_WAVE];
    __shared__ i32 s_fl[RC_T / HHX_WAVE];
    i64 lo = 0, hi = 0;
    i32 fl = 0;
    for (i64 k = (i64)blockIdx.x * RC_T + threadIdx.x; k < n; k += (i64)gridDim.x * RC_T) {
        const i64 v = val[k];
        if (isf[k]) fl |= HHX_REFUSED_FLOAT;                     // v holds the bits of a double
        else if (v < 0) fl |= HHX_REFUSED_NEGATIVE;
        else { lo += v & 0xffffffffll; hi += v >> 32; }
        if (id_i[k] == id_j[k]) fl |= HHX_REFUSED_SELF_KEY;
    }
    lo = wave_sum_i64(lo);
    hi = wave_sum_i64(hi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fl |= __shfl_down(fl, o, HHX_WAVE);
    if (lane_id() == 0) { s_lo[threadIdx.x / HHX_WAVE] = lo; s_hi[threadIdx.x / HHX_WAVE] = hi; s_fl[threadIdx.x / HHX_WAVE] = fl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RC_T / HHX_WAVE; ++w) { lo += s_lo[w]; hi += s_hi[w]; fl |= s_fl[w]; }
        if (lo) atomicAdd(&out[RC_LO], (unsigned long long)lo);
        if (hi) atomicAdd(&out[RC_HI], (unsigned long long)hi);
        if (fl) atomicOr(&out[RC_FLAGS], (unsigned long long)fl);
    }
}

}  // namespace

extern "C" int hhx_reassign_create_from_pickle(hhx_pickle *p, int32_t n_ctg, const int32_t *group_host, int32_t n_groups, int *refused, hhx_reassign **out) {
    if (!p) return fail("hhx_reassign_create_from_pickle: null handle");
    if (!refused || !out) return fail("hhx_reassign_create_from_pickle: null pointer");
    *refused = 0;
    *out = nullptr;
    if (n_ctg < p->n_names) return fail("hhx_reassign_create_from_pickle: %d contigs, the table names %d", n_ctg, p->n_names);
    const i64 n = p->n_keys;
    if (n >= (i64)1 << 31) {                                     // the pass adds 32-bit halves in 64-bit words
        fail("reassign: not the device's table: 2^31 keys and more;");
        *refused = HHX_REFUSED_KEYS;
        return 0;
    }
    unsigned long long acc[RC_WORDS] = {0, 0, 0};
    if (n) {
        DevBuf<unsigned long long> d_acc;
        if (d_acc.alloc(RC_WORDS)) return 1;
        HHX_HIP(hipMemsetAsync(d_acc.p, 0, sizeof acc, g_stream));
        const unsigned grid = std::min(grid_for(n, RC_T), (unsigned)std::min<i64>(RC_GRID, std::max<i64>(1, tune_get("reassign_check_grid", RC_GRID))));
        { KTimer kt("reassign_check");
        k_reassign_check<<<grid, RC_T, 0, g_stream>>>(p->id_i.p, p->id_j.p, p->val.p, p->isf.p, n, d_acc.p); }
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, g_stream));
        HHX_HIP(hipStreamSynchronize(g_stream));
    }
    int why = (int)acc[RC_FLAGS];
    const unsigned __int128 total = ((unsigned __int128)acc[RC_HI] << 32) + acc[RC_LO];
    if (total >= (unsigned __int128)1 << 52) why |= HHX_REFUSED_TOTAL;            // 2 * total reaches 2^53
    if (why) {
        fail("reassign: not the device's table:%s%s%s%s", why & HHX_REFUSED_SELF_KEY ? " a key names one contig twice;" : "",
             why & HHX_REFUSED_FLOAT ? " a value is a float;" : "", why & HHX_REFUSED_NEGATIVE ? " a value is negative;" : "",
             why & HHX_REFUSED_TOTAL ? " twice the total of the values reaches 2^53;" : "");
        *refused = why;
        return 0;
    }
    return hhx_reassign_create_device("hhx_reassign_create_from_pickle", n, p->id_i.p, p->id_j.p, p->val.p, n_ctg, group_host, n_groups, out);
}

// ------------------------------------------------------------------ one group's H/T links from the open table
// HapHiC_sort.py get_sub_HT_dict :117-143 for one group of run() :912-920, on id_i / id_j / val as hhx_pickle_open left them (the rule: include/haphic_hip.h).
// The caller numbers the names: slot[name id] = 2 * position + suffix for the 2 n names ctg + '_H' / '_T' the file holds, -1 for every other name, and
// rank[position] = the contig's place among the sorted names.  k_heads_pass streams the keys, four per lane as two 16-byte loads: both ends are tested
// against a bitmap of the slotted names held in LDS (hhx_tune "heads_bitmap"; as hhx_partition.h does for frag_set) before the slots are gathered, and the
// value is loaded for a key of two slotted names of two contigs only.  Every wavefront owns one contiguous range of the table, walks it in steps of 64
// quads with the next step's ids loaded ahead, and compacts its survivors (key of the reference's insertion order, value) with ballot and prefix.  No
// counter is shared between wavefronts — atomics of the whole grid on one address would bound the pass — so the pass runs twice: once to
// count per wavefront, then, after a scan of those counts, to write at the wavefront's own running offset.  The stable radix sort of hhx_sort.h then puts
// the survivors in the reference's order on as many bits as the order key has — the keys are distinct — and k_heads_finish turns every order key into
// its two indices.
namespace {

constexpr int HD_T = 256, HD_PER = 4, HD_WAVES = HD_T / HHX_WAVE;
constexpr i64 HD_BITMAP_BYTES = 64 << 10;     // the most names (2^19) whose bitmap a workgroup holds in LDS; more: the plain gather
constexpr unsigned HD_GRID = 256 * 6;         // six workgroups a CU: what fits beside a bitmap of 25 KB each; every workgroup reads the whole bitmap once (hhx_tune "heads_grid": fewer)

// member bit (id & 63) of word (id >> 6): slot[id] >= 0
__global__ __launch_bounds__(HD_T) void k_heads_bitmap(const i32 *__restrict__ slot, i64 n_names, i64 n_words, u64 *__restrict__ member) {
    for (i64 base = (i64)blockIdx.x * HD_T; base < n_words * 64; base += (i64)gridDim.x * HD_T) {
        const i64 id = base + threadIdx.x;
        const u64 m = __ballot(id < n_names && slot[id] >= 0);
        if (lane_id() == 0 && (id >> 6) < n_words) member[id >> 6] = m;
    }
}

__device__ __forceinline__ bool bit_of(const u64 *bits, i32 id) { return (bits[id >> 6] >> (id & 63)) & 1ull; }

// wavefront w of the grid takes the quads (four keys) [w * per_wave, (w + 1) * per_wave), 64 consecutive quads per step.  EMIT = false: counts[w] = its
// survivors; EMIT = true: they are written from offs[w] on (offs: the exclusive scan of counts, so every position lies below the total)
template <bool BITMAP, bool EMIT>
__global__ __launch_bounds__(HD_T) void k_heads_pass(const i32 *__restrict__ id_i, const i32 *__restrict__ id_j, const i64 *__restrict__ val, i64 n_keys,
                                                     i64 per_wave, const i32 *__restrict__ slot, const i32 *__restrict__ rank, i64 n,
                                                     const u64 *__restrict__ member, i64 n_words, i64 *__restrict__ counts, const i64 *__restrict__ offs,
                                                     u64 *__restrict__ okey, u64 *__restrict__ oval) {
    extern __shared__ u64 bits[];
    if (BITMAP) {
        for (i64 w = threadIdx.x; w < n_words; w += HD_T) bits[w] = member[w];
        __syncthreads();
    }
    const int lane = lane_id();
    const u64 lt = (1ull << lane) - 1ull;
    const i64 wave = (i64)blockIdx.x * HD_WAVES + threadIdx.x / HHX_WAVE;
    const i64 q0 = wave * per_wave, q1 = min((n_keys + HD_PER - 1) / HD_PER, q0 + per_wave);
    i64 at = EMIT ? offs[wave] : 0;                                                                      // the same in every lane
    // the ids of the quad (-1: past the range or the table); id_i / id_j start on 16-byte boundaries
    auto load = [&](i64 quad, int4 &va, int4 &vb) {
        const i64 k0 = quad * HD_PER;
        if (quad < q1 && k0 + HD_PER <= n_keys) {
            va = *reinterpret_cast<const int4 *>(id_i + k0);
            vb = *reinterpret_cast<const int4 *>(id_j + k0);
        } else {
            i32 x[HD_PER], y[HD_PER];
#pragma unroll
            for (int q = 0; q < HD_PER; ++q) {
                const bool in = quad < q1 && k0 + q < n_keys;
                x[q] = in ? id_i[k0 + q] : -1;
                y[q] = in ? id_j[k0 + q] : -1;
            }
            va = make_int4(x[0], x[1], x[2], x[3]);
            vb = make_int4(y[0], y[1], y[2], y[3]);
        }
    };
    int4 na = make_int4(-1, -1, -1, -1), nb = na;
    if (q0 < q1) load(q0 + lane, na, nb);
    for (i64 base = q0; base < q1; base += HHX_WAVE) {                                                   // the bound is the same for the whole wavefront
        const i64 k0 = (base + lane) * HD_PER;
        const i32 a[HD_PER] = {na.x, na.y, na.z, na.w}, b[HD_PER] = {nb.x, nb.y, nb.z, nb.w};
        if (base + HHX_WAVE < q1) load(base + HHX_WAVE + lane, na, nb);                                 // the next step's ids are on their way while this one's slots are gathered
#pragma unroll
        for (int q = 0; q < HD_PER; ++q) {
            bool keep = false;
            u64 key = 0;
            i64 v = 0;
            if (a[q] >= 0 && (!BITMAP || (bit_of(bits, a[q]) && bit_of(bits, b[q])))) {
                const i32 sa = slot[a[q]];
                const i32 sb = sa >= 0 ? slot[b[q]] : -1;
                if (sb >= 0) {
                    const i64 pa = sa >> 1, pb = sb >> 1;                                                // positions in ctgs, below n
                    if (pa != pb && rank[pa] < rank[pb]) {                                              // two contigs, the smaller name first
                        v = val[k0 + q];
                        key = (u64)(min(pa, pb) * n + max(pa, pb)) << 2 | (u64)(2 * (sa & 1) + (sb & 1));
                        keep = v != 0;
                    }
                }
            }
            const u64 m = __ballot(keep);
            if (EMIT && keep) {
                const i64 pos = at + __popcll(m & lt);
                okey[pos] = key;
                oval[pos] = (u64)v;
            }
            at += __popcll(m);
        }
    }
    if (!EMIT && lane == 0) counts[wave] = at;
}

// lo_H = 0, hi_H = 1, hi_T = 2, lo_T = 3 for lo, hi = sorted(ctgs[:2]); ctgs[k]_H = 2 k, ctgs[k]_T = 2 k + 1 from k = 2 on
__device__ __forceinline__ i32 head_index(i64 pos, int suffix, int lo_pos) {
    if (pos >= 2) return (i32)(2 * pos + suffix);
    return pos == lo_pos ? (suffix ? 3 : 0) : (suffix ? 2 : 1);
}
__global__ __launch_bounds__(HD_T) void k_heads_finish(const u64 *__restrict__ key, i64 m, i64 n, const i32 *__restrict__ rank, int lo_pos, i32 *__restrict__ ei,
                                                       i32 *__restrict__ ej) {
    for (i64 t = (i64)blockIdx.x * HD_T + threadIdx.x; t < m; t += (i64)gridDim.x * HD_T) {
        const u64 k = key[t];
        const i64 cell = (i64)(k >> 2), a = cell / n, b = cell - a * n;                                  // a < b < n by construction
        const bool a_first = rank[a] < rank[b];
        ei[t] = head_index(a_first ? a : b, (int)(k >> 1) & 1, lo_pos);
        ej[t] = head_index(a_first ? b : a, (int)k & 1, lo_pos);
    }
}

}  // namespace

extern "C" int hhx_pickle_group_heads(hhx_pickle *p, int32_t n_ctg, const int32_t *slot, const int32_t *rank, int64_t *n_edges) {
    if (!p) return fail("hhx_pickle_group_heads: null handle");
    if (!slot || !rank || !n_edges) return fail("hhx_pickle_group_heads: null pointer");
    *n_edges = 0;
    p->heads_n = 0;
    if (n_ctg < 2 || n_ctg >= (1 << 30)) return fail("hhx_pickle_group_heads: %d contigs (2 .. 2^30 - 1 are served)", n_ctg);
    if (p->any_float) return fail("hhx_pickle_group_heads: the table holds float values");
    const i64 n = n_ctg, n_names = p->n_names, n_keys = p->n_keys;
    // what the kernels index with: every slot below 2 n, rank a permutation of 0 .. n - 1
    for (i64 k = 0; k < n_names; ++k)
        if (slot[k] < -1 || slot[k] >= 2 * n) return fail("hhx_pickle_group_heads: slot[%lld] = %d is outside -1 .. %lld", (long long)k, slot[k], (long long)(2 * n - 1));
    {
        std::vector<unsigned char> seen((size_t)n, 0);
        for (i64 k = 0; k < n; ++k) {
            if (rank[k] < 0 || rank[k] >= n || seen[(size_t)rank[k]]) return fail("hhx_pickle_group_heads: rank is no permutation of 0 .. %lld", (long long)(n - 1));
            seen[(size_t)rank[k]] = 1;
        }
    }
    if (n_keys == 0 || n_names == 0) return 0;

    const i64 n_words = (n_names + 63) / 64;
    const bool bitmap = tune_get("heads_bitmap", 1) != 0 && n_words * (i64)sizeof(u64) <= HD_BITMAP_BYTES;
    const i64 n_quads = (n_keys + HD_PER - 1) / HD_PER;
    const unsigned grid = std::min(grid_for(n_quads, HD_T), (unsigned)std::min<i64>(HD_GRID, std::max<i64>(1, tune_get("heads_grid", HD_GRID))));
    const i64 n_waves = (i64)grid * HD_WAVES;
    const i64 per_wave = ((n_quads + n_waves - 1) / n_waves + HHX_WAVE - 1) / HHX_WAVE * HHX_WAVE;         // whole steps: every wavefront's range starts on a 1 KiB boundary
    DevBuf<i32> dslot, drank;
    DevBuf<u64> member, key, value;
    DevBuf<i64> counts, offs;
    if (dslot.alloc((size_t)n_names) || drank.alloc((size_t)n) || member.alloc((size_t)n_words) || counts.alloc((size_t)n_waves) || offs.alloc((size_t)n_waves + 1))
        return 1;
    HHX_HIP(hipMemcpyAsync(dslot.p, slot, sizeof(i32) * (size_t)n_names, hipMemcpyHostToDevice, g_stream));
    HHX_HIP(hipMemcpyAsync(drank.p, rank, sizeof(i32) * (size_t)n, hipMemcpyHostToDevice, g_stream));
    const size_t lds = bitmap ? (size_t)n_words * sizeof(u64) : 0;
    i64 m = 0;
    {
        KTimer kt("heads_pass", bitmap ? 2 : 1);
        if (bitmap) {
            k_heads_bitmap<<<grid_for(n_words * 64, HD_T), HD_T, 0, g_stream>>>(dslot.p, n_names, n_words, member.p);
            k_heads_pass<true, false><<<grid, HD_T, lds, g_stream>>>(p->id_i.p, p->id_j.p, p->val.p, n_keys, per_wave, dslot.p, drank.p, n, member.p, n_words, counts.p,
                                                                    nullptr, nullptr, nullptr);
        } else {
            k_heads_pass<false, false><<<grid, HD_T, 0, g_stream>>>(p->id_i.p, p->id_j.p, p->val.p, n_keys, per_wave, dslot.p, drank.p, n, nullptr, 0, counts.p, nullptr,
                                                                   nullptr, nullptr);
        }
        HHX_LAUNCH_CHECK();
    }
    HHX_TRY(exclusive_scan_i64(counts.p, offs.p, n_waves, &m));                    // synchronises: m is the number of survivors
    prof_count("heads_keys", n_keys);
    if (m == 0) return 0;
    if (m > n_keys) return fail("hhx_pickle_group_heads: %lld survivors of %lld keys", (long long)m, (long long)n_keys);
    if (key.alloc((size_t)m) || value.alloc((size_t)m)) return 1;
    {
        KTimer kt("heads_pass");
        if (bitmap)
            k_heads_pass<true, true><<<grid, HD_T, lds, g_stream>>>(p->id_i.p, p->id_j.p, p->val.p, n_keys, per_wave, dslot.p, drank.p, n, member.p, n_words, nullptr,
                                                                   offs.p, key.p, value.p);
        else
            k_heads_pass<false, true><<<grid, HD_T, 0, g_stream>>>(p->id_i.p, p->id_j.p, p->val.p, n_keys, per_wave, dslot.p, drank.p, n, nullptr, 0, nullptr, offs.p,
                                                                  key.p, value.p);
        HHX_LAUNCH_CHECK();
    }
    int bits = 2;                                                                  // 2 * ceil(log2 n) + 2
    while ((1ll << ((bits - 2) / 2)) < n) bits += 2;
    DevBuf<u64> skey;
    if (skey.alloc((size_t)m) || p->heads_w.alloc((size_t)m) || p->heads_i.alloc((size_t)m) || p->heads_j.alloc((size_t)m)) return 1;
    {
        KTimer kt("heads_sort", 2 * ((bits + 7) / 8) + 1);
        HHX_TRY(stable_sort_pairs_u64(key.p, skey.p, value.p, p->heads_w.p, m, bits));
        k_heads_finish<<<grid_for(m, HD_T), HD_T, 0, g_stream>>>(skey.p, m, n, drank.p, rank[0] < rank[1] ? 0 : 1, p->heads_i.p, p->heads_j.p);
        HHX_LAUNCH_CHECK();
    }
    HHX_HIP(hipStreamSynchronize(g_stream));                                       // skey / drank are read until here
    p->heads_n = m;
    *n_edges = m;
    return 0;
}

extern "C" int hhx_pickle_group_heads_fetch(hhx_pickle *p, int32_t *ei, int32_t *ej, int64_t *w) {
    if (!p) return fail("hhx_pickle_group_heads_fetch: null handle");
    const size_t m = (size_t)p->heads_n;
    if (m && ei) HHX_HIP(hipMemcpyAsync(ei, p->heads_i.p, sizeof(i32) * m, hipMemcpyDeviceToHost, g_stream));
    if (m && ej) HHX_HIP(hipMemcpyAsync(ej, p->heads_j.p, sizeof(i32) * m, hipMemcpyDeviceToHost, g_stream));
    if (m && w) HHX_HIP(hipMemcpyAsync(w, p->heads_w.p, sizeof(i64) * m, hipMemcpyDeviceToHost, g_stream));
    HHX_HIP(hipStreamSynchronize(g_stream));
    return 0;
}
