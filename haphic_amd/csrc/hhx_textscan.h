// What the text passes share (hhx_text.hip: .pairs lines, hhx_clmsplit.hip: CLM lines): the universal-newline line-break passes, the byte
// reader over HBM, the token type and the byte-verified name table with its host-side builder.  Whitespace is the ASCII subset of
// str.split()'s (\t \n \v \f \r \x1c-\x1f and space); bytes >= 0x80 are name bytes.
#pragma once
#include <algorithm>

#include "hhx_common.h"

namespace hhx {
namespace textscan {

constexpr int TX_BLOCK = 4096;                 // bytes per workgroup step of the line-break passes

// name hash over the 8-byte words of the name (last word zero-padded), so that a lane hashes a 35-byte contig
// name in 5 steps; the table is byte-verified, the hash only has to spread
__host__ __device__ __forceinline__ u64 hash_step(u64 h, u64 w) { h = (h ^ w) * 0x9E3779B97F4A7C15ull; return h ^ (h >> 29); }
constexpr u64 HASH_SEED = 1469598103934665603ull;
__device__ __forceinline__ bool is_ws(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }

// bit k set: byte base + k ends a line ('\n', or a '\r' that is not followed by '\n'); 16 bytes per thread
__device__ __forceinline__ u32 break_mask(const unsigned char *__restrict__ t, i64 base, i64 n, bool aligned) {
    u32 m = 0;
    if (aligned && base + 16 < n) {                              // one 16-byte load + the look-ahead byte
        const uint4 v = *reinterpret_cast<const uint4 *>(t + base);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        unsigned char nxt = t[base + 16];
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            const unsigned char ch = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
            m |= (u32)(ch == '\n' || (ch == '\r' && nxt != '\n')) << k;
            nxt = ch;
        }
    } else {
        for (int k = 0; k < 16 && base + k < n; ++k) {
            const unsigned char ch = t[base + k];
            m |= (u32)(ch == '\n' || (ch == '\r' && (base + k + 1 >= n || t[base + k + 1] != '\n'))) << k;
        }
    }
    return m;
}

static __global__ __launch_bounds__(256) void k_count_breaks(const unsigned char *__restrict__ t, i64 n, i64 n_blocks, i64 *__restrict__ counts) {
    __shared__ i32 wsum[4];
    const bool aligned = ((uintptr_t)t & 15) == 0;
    for (i64 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        i32 c = __popc(break_mask(t, b * TX_BLOCK + (i64)threadIdx.x * 16, n, aligned));
        c = wave_sum_i32(c);
        if (lane_id() == 0) wsum[threadIdx.x / HHX_WAVE] = c;
        __syncthreads();
        if (threadIdx.x == 0) counts[b] = (i64)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// starts[1 + r] = p + 1 for the r-th break (starts[0] = 0 is written by thread 0 of block 0)
static __global__ __launch_bounds__(256) void k_write_starts(const unsigned char *__restrict__ t, i64 n, i64 n_blocks,
                                                      const i64 *__restrict__ prefix, i64 *__restrict__ starts) {
    __shared__ i32 wsum[4];
    const bool aligned = ((uintptr_t)t & 15) == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
    for (i64 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const i64 base = b * TX_BLOCK + (i64)threadIdx.x * 16;
        u32 m = break_mask(t, base, n, aligned);
        const i32 c = __popc(m);
        i32 incl = c;                                            // inclusive wave scan
#pragma unroll
        for (int o = 1; o < HHX_WAVE; o <<= 1) {
            const i32 v = __shfl_up(incl, o, HHX_WAVE);
            if (lane_id() >= o) incl += v;
        }
        if (lane_id() == HHX_WAVE - 1) wsum[threadIdx.x / HHX_WAVE] = incl;
        __syncthreads();
        i64 at = prefix[b] + incl - c;
        for (int w = 0; w < (int)(threadIdx.x / HHX_WAVE); ++w) at += wsum[w];
        while (m) {
            const int k = __ffs(m) - 1;
            m &= m - 1;
            starts[1 + at++] = base + k + 1;
        }
        __syncthreads();
    }
}

struct HbmText {
    const unsigned char *t;
    __device__ __forceinline__ unsigned char operator()(i64 p) const { return t[p]; }
    __device__ __forceinline__ u64 word(i64 p, int nb) const {
        u64 w = 0;
        for (int q = 0; q < nb; ++q) w |= (u64)t[p + q] << (8 * q);
        return w;
    }
};

struct Tok { i64 s; i32 len; };

struct NameTable {
    const u64 *names;                                            // every name padded with zeros to whole 8-byte words
    const i64 *name_off;                                         // in words; name_len in bytes
    const i32 *name_len;
    const u64 *slot_hash;
    const i32 *slot_id;
    u32 mask;
};

template <class RD>
__device__ __forceinline__ u64 tok_word(const RD &rd, const Tok &k, int q) {
    return rd.word(k.s + 8 * (i64)q, k.len - 8 * q < 8 ? k.len - 8 * q : 8);
}
template <class RD>
__device__ __forceinline__ i32 lookup(const NameTable &T, const RD &rd, const Tok &k) {
    constexpr int MAXW = 8;                                      // the words of names up to 64 bytes stay in registers
    const int nw = (k.len + 7) >> 3;
    u64 w[MAXW];
    u64 h = HASH_SEED;
#pragma unroll
    for (int q = 0; q < MAXW; ++q)
        if (q < nw) { w[q] = tok_word(rd, k, q); h = hash_step(h, w[q]); }
    for (int q = MAXW; q < nw; ++q) h = hash_step(h, tok_word(rd, k, q));
    for (u32 s = (u32)h & T.mask;; s = (s + 1) & T.mask) {
        const i32 id = T.slot_id[s];
        if (id < 0) return -1;
        if (T.slot_hash[s] != h || T.name_len[id] != k.len) continue;
        const u64 *nm = T.names + T.name_off[id];
        u64 diff = 0;
#pragma unroll
        for (int q = 0; q < MAXW; ++q)
            if (q < nw) diff |= nm[q] ^ w[q];
        for (int q = MAXW; q < nw; ++q) diff |= nm[q] ^ tok_word(rd, k, q);
        if (!diff) return id;
    }
}

inline unsigned grid_for(i64 work, int per_block) { return (unsigned)std::max<i64>(1, std::min<i64>((work + per_block - 1) / per_block, 256 * 32)); }

// the table on the device, built from n_names strings (concatenated, name_off[n_names + 1]) on the calling thread's stream
struct NameTableBuf {
    i32 n_names = 0;
    u32 mask = 0;
    DevBuf<u64> names;
    DevBuf<i64> name_off;
    DevBuf<i32> name_len;
    DevBuf<u64> slot_hash;
    DevBuf<i32> slot_id;
    NameTable view() const { return NameTable{names.p, name_off.p, name_len.p, slot_hash.p, slot_id.p, mask}; }
    int build(i32 n, const uint8_t *blob, const i64 *blob_off, const char *who) {
        n_names = n;
        u32 cap = 16;
        while (cap < 2u * (u32)n + 2) cap <<= 1;
        mask = cap - 1;
        std::vector<u64> sh(cap, 0);
        std::vector<i32> si(cap, -1), len((size_t)n + 1, 0);
        std::vector<i64> off((size_t)n + 1, 0);
        for (i32 k = 0; k < n; ++k) { len[k] = (i32)(blob_off[k + 1] - blob_off[k]); off[k + 1] = off[k] + (len[k] + 7) / 8; }
        std::vector<u64> words((size_t)off[n] + 1, 0);
        for (i32 k = 0; k < n; ++k) {
            if (len[k]) memcpy(&words[(size_t)off[k]], blob + blob_off[k], (size_t)len[k]);
            u64 h = HASH_SEED;
            for (i64 q = off[k]; q < off[k + 1]; ++q) h = hash_step(h, words[(size_t)q]);
            u32 s = (u32)h & mask;
            while (si[s] >= 0) s = (s + 1) & mask;
            si[s] = k;
            sh[s] = h;
        }
        if (names.alloc(words.size()) || name_off.alloc(off.size()) || name_len.alloc(len.size()) || slot_hash.alloc(cap) || slot_id.alloc(cap)) return 1;
        hipError_t e = hipMemcpyAsync(names.p, words.data(), sizeof(u64) * words.size(), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(name_off.p, off.data(), sizeof(i64) * off.size(), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(name_len.p, len.data(), sizeof(i32) * len.size(), hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(slot_hash.p, sh.data(), sizeof(u64) * cap, hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(slot_id.p, si.data(), sizeof(i32) * cap, hipMemcpyHostToDevice, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        if (e != hipSuccess) return fail("%s: %s", who, hipGetErrorString(e));
        return 0;
    }
};

}  // namespace textscan
}  // namespace hhx
