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
