// Radix partition of (w0: u64, w1: u32 | u64 | nothing) records into 2^total_bits buckets, in levels of at most
// 8-9 bits.  Shared by the link-table group-by (hhx_ingest.hip: bucket = hash of the key) and by the link
// matrix build (hhx_matrix.hip: bucket = matrix row).
//
// Per level: a COUNT pass (LDS histogram per 4096-record tile -> global histogram), an exclusive scan, and
// a SCATTER pass.  The scatter stages a tile in LDS grouped by bucket (LDS histogram rank + tile-local
// exclusive scan) and then writes it out linearly, so every (tile, bucket) group is one contiguous,
// coalesced run of records; one global atomicAdd per (tile, bucket) reserves the run.  Scattering single
// 8/4-byte stores instead (first version) measured 4-5x write amplification in the HBM counters
// (profiles/r01_pmc_c3.txt).  Nothing here is stable or needs to be: records carry what they need.
//
// The scatter's tile loop is a pipeline (k_part_scatter has the phases): the loads of a workgroup's NEXT tile and the
// reservation atomics of the current one are in flight while the current tile is scanned and staged, four LDS barriers
// a tile; and a source whose whole next tile fits the registers runs 1024 threads on a tile twice as long (8192 records
// of 12 B), because the length of the runs a tile writes — tile / buckets of the level — is what bounds these passes
// once the loads are hidden.  The count pass keeps its own 512-thread tiles: the two need not agree.
#pragma once
#include <type_traits>
#include "hhx_common.h"

namespace hhx {

constexpr int PT = 512, P_MAX_BINS = 512;
struct NoPayload {};       // w1_t of a source whose records are the bare 64-bit word
template <class W1> struct PartW1 { static constexpr bool HAS = true; static constexpr size_t BYTES = sizeof(W1); };
template <> struct PartW1<NoPayload> { static constexpr bool HAS = false; static constexpr size_t BYTES = 0; };
// records per thread and tile: 8 records of 12 B, 7 of 16 B, 14 of 8 B.  With 512 threads a tile stages in < 80 KB of LDS (two
// workgroups per CU), with the 1024 of part_scatter_threads() in < 152 KB (one: the same sixteen waves).  The longer the tile, the
// longer the contiguous run a (tile, bucket) pair writes.
template <class W1> struct PartTile { static constexpr int ITEMS = !PartW1<W1>::HAS ? 14 : (sizeof(W1) == 4 ? 8 : 7), TILE = PT * ITEMS; };

struct PartLevel {
    int total_bits;     // buckets = 2^total_bits; bucket id comes from the Dig functor
    int shift;          // digit of this level = bucket >> shift
    int lds_bits;       // low lds_bits of the digit index the LDS histogram; the rest ("group") is constant
                        // within a tile except where a tile straddles two buckets of the previous level
};

// A record source is read through get(idx, w0, w1) -> "the record exists".  A BATCHED source also hands its loads out one step at a
// time, without a branch between them: load1(idx, raw) (idx valid: the caller clamps it), load2(raw) (the gathers that depend on
// load1's words) and decode(idx, raw, w0, w1), which touches no memory.  The kernels issue load1 for a CHUNK of records, then load2
// for all of them, then decode: with get() in the per-record loop every load sat in a basic block of its own behind the LDS atomic of
// the record before it, each followed by s_waitcnt vmcnt(0) — one round trip per load and record (read off the ISA), which is why
// these passes ran at a third of the stream rate.
template <class W1>
struct SrcRecs {
    typedef W1 w1_t;
    static constexpr bool MARK = false;
    static constexpr bool BATCHED = true;
    static constexpr int CHUNK = 16, CHUNK_SCATTER = 16, PREFETCH = 2;
    const u64 *w0;
    const W1 *w1;
    struct Raw { u64 a; W1 b; };
    static __device__ __forceinline__ void pin(Raw &r) {
        asm volatile("" : "+v"(r.a));
        if constexpr (PartW1<W1>::HAS) asm volatile("" : "+v"(r.b));
    }
    __device__ __forceinline__ void load1(i64 idx, Raw &r) const {
        r.a = w0[idx];
        if constexpr (PartW1<W1>::HAS) r.b = w1[idx];
    }
    __device__ __forceinline__ void load2(Raw &) const {}
    __device__ __forceinline__ bool decode(i64, const Raw &r, u64 &a, W1 &b) const {
        a = r.a;
        if constexpr (PartW1<W1>::HAS) b = r.b;
        return true;
    }
    __device__ __forceinline__ bool get(i64 idx, u64 &a, W1 &b) const {
        a = w0[idx];
        if constexpr (PartW1<W1>::HAS) b = w1[idx];
        return true;
    }
};

// A source may keep a small READ-ONLY TABLE IN LDS, one copy per workgroup (hhx_matrix.hip: the membership bitmap of
// SrcDirectedPacked<true>, so that a membership test is an LDS read instead of a divergent gather).  It says so with
//     static constexpr bool LDS_TABLE = true;  static constexpr size_t LDS_TABLE_MAX = <bytes at most>;
//     size_t lds_table_bytes() const;          (host: bytes of this object's table)
//     Src lds_table(void *at) const;           (device, every thread of the workgroup: copies the table to `at`, 16-byte aligned,
//                                               and returns a copy of the source that reads it there; the caller runs the barrier)
// k_part_count and k_part_scatter place the table in dynamic LDS — the scatter behind its staging arrays, which never reach it —
// fill it once per workgroup in front of the tile loop and read through the returned copy; the host driver adds the bytes to the
// launch.  A source without the declaration compiles to the code it had before.
template <class Src, class = void> struct PartLds { static constexpr bool HAS = false; static constexpr size_t MAX = 0; };
template <class Src> struct PartLds<Src, std::void_t<decltype(Src::LDS_TABLE)>> {
    static constexpr bool HAS = Src::LDS_TABLE;
    static constexpr size_t MAX = HAS ? (Src::LDS_TABLE_MAX + 15) / 16 * 16 : 0;
};
template <class Src> inline size_t part_lds_table_bytes(const Src &src) {
    if constexpr (PartLds<Src>::HAS) return (src.lds_table_bytes() + 15) / 16 * 16;
    else return 0;
}

template <class Src, class Dig>
__device__ __forceinline__ u32 tile_group(const Src &src, const Dig &dig, i64 first, i64 n, const PartLevel &L) {
    if (L.shift + L.lds_bits >= L.total_bits) return 0;          // first level: the LDS histogram spans the whole digit
    u64 w0; typename Src::w1_t w1;
    (void)src.get(first < n ? first : n - 1, w0, w1);            // later levels read compact records: never invalid
    return (dig(w0) >> L.shift) >> L.lds_bits;
}

template <class Src, class Dig>
__global__ __launch_bounds__(PT) void k_part_count(Src src_arg, Dig dig, i64 n, PartLevel L, unsigned long long *__restrict__ ghist) {
    constexpr int P_ITEMS = PartTile<typename Src::w1_t>::ITEMS, P_TILE = PartTile<typename Src::w1_t>::TILE;
    __shared__ u32 hist[P_MAX_BINS];
    __shared__ u32 s_grp;
    extern __shared__ __attribute__((aligned(16))) unsigned char count_smem[];      // the source's LDS table, if it has one: nothing else
    const int tid = threadIdx.x, nb = 1 << L.lds_bits;
    for (int t = tid; t < nb; t += PT) hist[t] = 0;
    Src src = src_arg;
    if constexpr (PartLds<Src>::HAS) {
        src = src_arg.lds_table(count_smem);
        lds_barrier();
    }
    u32 cur = 0xffffffffu;
    u32 marked = 0;                                              // (MARK) what the side effect counts for this thread: mark_apply, mark_flush
    const i64 n_tiles = (n + P_TILE - 1) / P_TILE;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 base = tile * P_TILE;
        if (tid == 0) s_grp = tile_group(src, dig, base, n, L);
        lds_barrier();
        const u32 tg = s_grp;
        if (tg != cur) {                                         // flush the histogram of the previous group
            if (cur != 0xffffffffu)
                for (int t = tid; t < nb; t += PT) {
                    if (hist[t]) atomicAdd(&ghist[((u64)cur << L.lds_bits) | (u64)t], (unsigned long long)hist[t]);
                    hist[t] = 0;
                }
            cur = tg;
            lds_barrier();
        }
        if constexpr (Src::BATCHED) {
            // the loads of a chunk of records, then the gathers that depend on them — for a source with a side effect per record
            // (MARK: mark_load / mark_apply, mark_flush at the kernel's end) the load the side effect needs rides with those gathers — then the histogram and the
            // side effect's (rare) atomics: an atomic inside the load loop would pin the loads of the following records behind it
            constexpr int CH = Src::CHUNK < P_ITEMS ? Src::CHUNK : P_ITEMS;
#pragma unroll
            for (int h = 0; h < P_ITEMS; h += CH) {
                typename Src::Raw raw[CH];
                u64 seen[CH];
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) {
                        const i64 idx = base + (i64)(h + k) * PT + tid;
                        src.load1(idx < n ? idx : n - 1, raw[k]);
                    }
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) {
                        src.load2(raw[k]);
                        if constexpr (Src::MARK) seen[k] = src.mark_load(base + (i64)(h + k) * PT + tid, raw[k]);
                    }
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) {
                        const i64 idx = base + (i64)(h + k) * PT + tid;
                        u64 w0, extra = 0;
                        bool ok;
                        if constexpr (Src::MARK) ok = src.decode_marked(idx, raw[k], w0, extra);
                        else { typename Src::w1_t w1; ok = src.decode(idx, raw[k], w0, w1); }
                        if (idx < n && ok) {
                            if constexpr (Src::MARK) src.mark_apply(w0, extra, seen[k], marked);
                            const u32 d = dig(w0) >> L.shift;
                            if ((d >> L.lds_bits) == tg) atomicAdd(&hist[d & (u32)(nb - 1)], 1u);
                            else atomicAdd(&ghist[d], 1ull);
                        }
                    }
            }
        } else {
            static_assert(!Src::MARK, "a source with a side effect per record is a BATCHED one");
#pragma unroll
        for (int k = 0; k < P_ITEMS; ++k) {
            const i64 idx = base + (i64)k * PT + tid;
            u64 w0; typename Src::w1_t w1;
            if (idx < n && src.get(idx, w0, w1)) {
                const u32 d = dig(w0) >> L.shift;
                if ((d >> L.lds_bits) == tg) atomicAdd(&hist[d & (u32)(nb - 1)], 1u);
                else atomicAdd(&ghist[d], 1ull);
            }
        }
        }
        lds_barrier();
    }
    if (cur != 0xffffffffu)
        for (int t = tid; t < nb; t += PT)
            if (hist[t]) atomicAdd(&ghist[((u64)cur << L.lds_bits) | (u64)t], (unsigned long long)hist[t]);
    if constexpr (Src::MARK) src.mark_flush(marked);             // one sum per wave (every thread is here)
}

template <class W1, int T>
constexpr size_t part_scatter_lds() {
    return (size_t)PartTile<W1>::ITEMS * T * (8 + PartW1<W1>::BYTES + 2) + (size_t)P_MAX_BINS * (4 + 4 + 8) + 16;
}
// where a source's LDS table starts in the scatter's dynamic LDS: behind s_bin, the last of the staging arrays
template <class W1, int T>
constexpr size_t part_scatter_table_at() { return (part_scatter_lds<W1, T>() + 15) / 16 * 16; }

// what k_part_scatter keeps in flight for the NEXT tile of a workgroup while it scans, reserves and stages the current one (a BATCHED
// source says so in PREFETCH): 0 nothing, 1 the load1 words, 2 the load1 words and the load2 gathers; Src::pin(raw) names the
// registers of that prefetch, so that the wait for them can be put where it belongs (see the kernel)
template <class Src, bool B = Src::BATCHED> struct PartRaw { struct type {}; static constexpr int PF = 0; };
template <class Src> struct PartRaw<Src, true> { typedef typename Src::Raw type; static constexpr int PF = Src::PREFETCH; };

// The tile loop, four LDS barriers a tile:
//   top   decode the tile's records from the registers the previous iteration (or the prologue) loaded; rank them with one LDS
//         atomic each (the histogram is clear: see below); THEN issue the loads of tile + gridDim.x
//   (1)   scan: thread t reads bin t — and clears it for the next tile, nobody else reads it — wave scan
//   (2)   tile-local bases to LDS; the global reservation atomic of bin t is ISSUED, its result stays in a register
//   (3)   stage the tile in LDS grouped by bucket (needs the local bases only); behind the staging the reserved base goes to LDS —
//         the one place that waits for global memory: the reservation's round trip and the next tile's loads (issued before it,
//         vmcnt retires in order) have had the scan, the bases and the staging to come back.  The prefetched registers are pinned
//         here, BEFORE the write-out's stores are issued: the waitcnt pass is static and the write-out has a data-dependent trip
//         count, so a wait placed behind it (where the next iteration consumes the registers) is vmcnt(0) and drains the stores too
//   (4)   write-out: linear sweep over the staged tile, lanes write consecutive addresses inside a run.  No barrier ends the tile:
//         what the write-out reads (staged records, bins, both bases, the count) is next written behind barrier (2) of the next
//         tile, and no wave passes (1) before every wave has left its write-out.
// The group of a later level's tile (tile_group) comes from a load of the tile's first record that every thread issues with the
// prefetch (one line per wave) instead of a read by thread 0, an LDS word and a barrier.  A prefetch past the last tile reads
// record n - 1 (the clamp the tile's own tail uses) and is never decoded.
template <class Src, class Dig, int T>
__global__ __launch_bounds__(T) void k_part_scatter(Src src_arg, Dig dig, i64 n, PartLevel L, unsigned long long *__restrict__ cursor,
                                                     u64 *__restrict__ out_w0, typename Src::w1_t *__restrict__ out_w1) {
    typedef typename Src::w1_t W1;
    typedef typename PartRaw<Src>::type RawT;
    constexpr int P_ITEMS = PartTile<W1>::ITEMS, P_TILE = PartTile<W1>::ITEMS * T, PF = PartRaw<Src>::PF;
    static_assert(P_TILE <= 0x10000 && P_MAX_BINS <= 0x8000, "bin and rank of a record share one register");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *s_w0 = (u64 *)smem;                                     // [P_TILE] tile grouped by bucket
    unsigned long long *gbase = (unsigned long long *)(s_w0 + P_TILE);   // [P_MAX_BINS] reserved global run of every bucket
    W1 *s_w1 = (W1 *)(gbase + P_MAX_BINS);                       // [P_TILE] (nothing for payload-free records)
    u32 *hist = (u32 *)((unsigned char *)s_w1 + (size_t)P_TILE * PartW1<W1>::BYTES);   // [P_MAX_BINS]
    u32 *lbase = hist + P_MAX_BINS;                              // [P_MAX_BINS] tile-local exclusive prefix
    u32 *s_misc = lbase + P_MAX_BINS;                            // [4]: [1] records staged by the tile
    unsigned short *s_bin = (unsigned short *)(s_misc + 4);      // [P_TILE]
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / HHX_WAVE, nb = 1 << L.lds_bits;
    __shared__ u32 wsum[T / HHX_WAVE];
    const i64 n_tiles = (n + P_TILE - 1) / P_TILE;
    if ((i64)blockIdx.x >= n_tiles) return;                      // (also n == 0: the clamp below needs a record)
    const bool later = L.shift + L.lds_bits < L.total_bits;      // a level whose tiles have a group (tile_group)
    for (int t = tid; t < nb; t += T) hist[t] = 0;
    // the source's LDS table lies behind s_bin[P_TILE]: the staging writes s_bin[s] for s < P_TILE only, so it outlives every tile
    Src src = src_arg;
    if constexpr (PartLds<Src>::HAS) src = src_arg.lds_table(smem + part_scatter_table_at<W1, T>());
    lds_barrier();
    [[maybe_unused]] auto prefetch = [&](const i64 pbase, RawT (&raw)[P_ITEMS], u64 &gw) {
        if constexpr (PF > 0) {
#pragma unroll
            for (int k = 0; k < P_ITEMS; ++k) {
                const i64 idx = pbase + (i64)k * T + tid;
                src.load1(idx < n ? idx : n - 1, raw[k]);
            }
            if constexpr (PF > 1) {
#pragma unroll
                for (int k = 0; k < P_ITEMS; ++k) src.load2(raw[k]);
            }
            if (later) { W1 gw1; (void)src.get(pbase < n ? pbase : n - 1, gw, gw1); }   // later levels read compact records: never invalid
        }
    };
    [[maybe_unused]] auto pin = [&](RawT (&raw)[P_ITEMS], u64 &gw) {
        if constexpr (PF > 0) {
#pragma unroll
            for (int k = 0; k < P_ITEMS; ++k) Src::pin(raw[k]);
            asm volatile("" : "+v"(gw));
        }
    };
    // the loop is entered with the first tile's registers DEFINED, not pending (k_aggregate has the reason)
    [[maybe_unused]] RawT raw_c[P_ITEMS];
    [[maybe_unused]] u64 gw_c = 0;
    prefetch((i64)blockIdx.x * P_TILE, raw_c, gw_c);
    pin(raw_c, gw_c);
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 base = tile * P_TILE;
        u32 tg = 0;
        if constexpr (PF > 0) { if (later) tg = (dig(gw_c) >> L.shift) >> L.lds_bits; }
        else tg = tile_group(src, dig, base, n, L);
        u64 w0[P_ITEMS];
        W1 w1[P_ITEMS];
        u32 lr[P_ITEMS];                                             // bin << 16 | rank in the bin; all ones: not staged
        bool have[P_ITEMS];
        if constexpr (PF > 0) {
            constexpr int CH = PF > 1 ? P_ITEMS : (Src::CHUNK_SCATTER < P_ITEMS ? Src::CHUNK_SCATTER : P_ITEMS);
#pragma unroll
            for (int h = 0; h < P_ITEMS; h += CH) {
                if constexpr (PF == 1) {
#pragma unroll
                    for (int k = 0; k < CH; ++k)
                        if (h + k < P_ITEMS) src.load2(raw_c[h + k]);
                }
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) {
                        const i64 idx = base + (i64)(h + k) * T + tid;
                        const bool ok = src.decode(idx, raw_c[h + k], w0[h + k], w1[h + k]);
                        have[h + k] = idx < n && ok;
                    }
            }
        } else if constexpr (Src::BATCHED) {                         // every load of a chunk in flight before the first is consumed (see SrcRecs)
            constexpr int CH = Src::CHUNK_SCATTER < P_ITEMS ? Src::CHUNK_SCATTER : P_ITEMS;
#pragma unroll
            for (int h = 0; h < P_ITEMS; h += CH) {
                RawT raw[CH];
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) {
                        const i64 idx = base + (i64)(h + k) * T + tid;
                        src.load1(idx < n ? idx : n - 1, raw[k]);
                    }
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) src.load2(raw[k]);
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    if (h + k < P_ITEMS) {
                        const i64 idx = base + (i64)(h + k) * T + tid;
                        const bool ok = src.decode(idx, raw[k], w0[h + k], w1[h + k]);
                        have[h + k] = idx < n && ok;
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < P_ITEMS; ++k) {
            const i64 idx = base + (i64)k * T + tid;
            lr[k] = 0xffffffffu;
            if constexpr (!Src::BATCHED) have[k] = idx < n && src.get(idx, w0[k], w1[k]);
            if (have[k]) {
                const u32 d = dig(w0[k]) >> L.shift;
                if ((d >> L.lds_bits) == tg) {
                    const u32 loc = d & (u32)(nb - 1);
                    lr[k] = (loc << 16) | atomicAdd(&hist[loc], 1u);
                } else {                                         // straddling record: reserve its slot directly
                    const unsigned long long pos = atomicAdd(&cursor[d], 1ull);
                    out_w0[pos] = w0[k];
                    if constexpr (PartW1<W1>::HAS) out_w1[pos] = w1[k];
                }
            }
        }
        [[maybe_unused]] RawT raw_n[P_ITEMS];
        [[maybe_unused]] u64 gw_n = 0;
        prefetch(base + (i64)gridDim.x * P_TILE, raw_n, gw_n);
        lds_barrier();                                               // (1)
        // tile-local exclusive scan of the histogram (one bin per thread, nb <= T)
        const u32 c = tid < nb ? hist[tid] : 0;
        if (tid < nb) hist[tid] = 0;
        u32 incl = c;
#pragma unroll
        for (int o = 1; o < HHX_WAVE; o <<= 1) {
            const u32 v = __shfl_up(incl, o, HHX_WAVE);
            if (lane >= o) incl += v;
        }
        if (lane == HHX_WAVE - 1) wsum[wave] = incl;
        lds_barrier();                                               // (2)
        u32 woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        unsigned long long gb = 0;
        if (tid < nb) {
            lbase[tid] = woff + incl - c;
            if (c) gb = atomicAdd(&cursor[((u64)tg << L.lds_bits) | (u64)tid], (unsigned long long)c);
        }
        if (tid == T - 1) s_misc[1] = woff + incl;              // records staged by this tile
        lds_barrier();                                               // (3)
#pragma unroll
        for (int k = 0; k < P_ITEMS; ++k)
            if (lr[k] != 0xffffffffu) {
                const u32 loc = lr[k] >> 16;
                const u32 s = lbase[loc] + (lr[k] & 0xffffu);
                s_w0[s] = w0[k];
                if constexpr (PartW1<W1>::HAS) s_w1[s] = w1[k];
                s_bin[s] = (unsigned short)loc;
            }
        if (c) gbase[tid] = gb;                                      // (c != 0 implies tid < nb)
        pin(raw_n, gw_n);
        lds_barrier();                                               // (4)
        const u32 staged = s_misc[1];
        for (u32 s = tid; s < staged; s += T) {                 // linear sweep: lanes write consecutive addresses inside a run
            const u32 b = s_bin[s];
            const unsigned long long pos = gbase[b] + (s - lbase[b]);
            out_w0[pos] = s_w0[s];
            if constexpr (PartW1<W1>::HAS) out_w1[pos] = s_w1[s];
        }
        if constexpr (PF > 0) {
#pragma unroll
            for (int k = 0; k < P_ITEMS; ++k) raw_c[k] = raw_n[k];
            gw_c = gw_n;
        }
    }
}

// threads of a scatter workgroup: a source whose whole next tile is prefetched runs ONE workgroup of 1024 threads a CU instead of two of
// 512 — the same sixteen waves, but a tile twice as long, so every (tile, bucket) run it writes is twice as long
template <class Src> constexpr int part_scatter_threads() { return PartRaw<Src>::PF == 2 ? 2 * PT : PT; }

// workgroups of the count and scatter passes at most (HHX_PART_GRID, read at every launch: a test gives one workgroup several tiles
// of a few tens of thousands of records)
inline i64 part_grid_cap() { const char *e = getenv("HHX_PART_GRID"); return e && atoll(e) > 0 ? atoll(e) : 256 * 4; }

void u64_copy_async(const unsigned long long *src, unsigned long long *dst, i64 n);   // hhx_runtime.hip

// Host driver.  Partitions the records of `src` (n items, the source may drop some) into 2^total_bits buckets.
// Outputs: w0/w1 (bucket-grouped records), base[2^total_bits + 1] (device, record offsets), n_valid.
template <class W1>
struct Partitioned {
    DevBuf<u64> w0;
    DevBuf<W1> w1;
    DevBuf<i64> base;
    i64 n_valid = 0;
    u32 n_buckets = 1;
};

inline int part_levels(int total_bits, int max_bits, int *bits /* [4] */) {
    int n = total_bits <= 0 ? 1 : (total_bits + max_bits - 1) / max_bits;
    if (n > 4) n = 4;
    int left = total_bits;
    // the FIRST level gets the smaller share: its (tile, bucket) runs are scattered over the whole output, so they should be
    // long; a later level writes inside one bucket of the previous one, a region the L2 / Infinity Cache merges
    static const bool ascending = !getenv("HHX_PART_DESC");
    for (int l = 0; l < n; ++l) {
        bits[l] = ascending ? left / (n - l) : (left + (n - l) - 1) / (n - l);
        left -= bits[l];
    }
    return n;
}

// count_src (optional): the source object the level-1 COUNT pass reads through instead of src — same records, but its
// get() may carry a side effect that has to happen exactly once per record (hhx_matrix.hip: first positions).
// hist0 (optional): the level-1 histogram already counted by whoever produced the records (hhx_ingest.hip: k_map_records) —
// 2^bits[0] counts of the digit `bucket >> (total_bits - bits[0])` over the valid records; the level's COUNT pass is skipped.
template <class Src, class Dig>
int partition_records(const Src &src, const Dig &dig, i64 n_items, int total_bits, int max_bits_per_level,
                      Partitioned<typename Src::w1_t> *out, const char *timer_prefix, const Src *count_src = nullptr,
                      const unsigned long long *hist0 = nullptr) {
    typedef typename Src::w1_t W1;
    constexpr int T1 = part_scatter_threads<Src>(), TN = part_scatter_threads<SrcRecs<W1>>();      // first level, later levels
    static int attr_dev = -1;           // the attribute is per device: keyed on the current ordinal (one static per instantiation)
    int dev = 0;
    HHX_HIP(hipGetDevice(&dev));
    if (attr_dev != dev) {
        HHX_HIP(hipFuncSetAttribute((const void *)k_part_scatter<Src, Dig, T1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(part_scatter_table_at<W1, T1>() + PartLds<Src>::MAX)));
        if constexpr (PartLds<Src>::HAS)
            HHX_HIP(hipFuncSetAttribute((const void *)k_part_count<Src, Dig>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PartLds<Src>::MAX));
        HHX_HIP(hipFuncSetAttribute((const void *)k_part_scatter<SrcRecs<W1>, Dig, TN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)part_scatter_lds<W1, TN>()));
        attr_dev = dev;
    }
    if (max_bits_per_level > 9) max_bits_per_level = 9;          // P_MAX_BINS
    int bits[4];
    const int n_levels = part_levels(total_bits, max_bits_per_level, bits);
    int used = 0;
    for (int l = 0; l < n_levels; ++l) used += bits[l];
    if (used != total_bits) return fail("partition: %d bits do not fit %d levels", total_bits, n_levels);
    const size_t table_bytes = part_lds_table_bytes(src);        // the source's LDS table (level 1 reads through the source): 0 without one
    if (table_bytes > PartLds<Src>::MAX) return fail("partition: an LDS table of %zu bytes exceeds the %zu its source declares", table_bytes, PartLds<Src>::MAX);
    out->n_buckets = 1u << total_bits;
    DevBuf<u64> cur_w0, nxt_w0;
    DevBuf<W1> cur_w1, nxt_w1;
    DevBuf<i64> base;
    i64 n_cur = n_items;
    int done_bits = 0;
    char tname[64];
    for (int l = 0; l < n_levels; ++l) {
        done_bits += bits[l];
        const u32 nbk = 1u << done_bits;                         // buckets after this level
        const PartLevel L{total_bits, total_bits - done_bits, bits[l]};
        DevBuf<unsigned long long> hist, cursor;
        DevBuf<i64> nbase;
        if (hist.alloc((size_t)nbk + 1) || cursor.alloc((size_t)nbk + 1) || nbase.alloc((size_t)nbk + 2)) return 1;
        HHX_HIP(hipMemsetAsync(hist.p, 0, sizeof(unsigned long long) * ((size_t)nbk + 1), g_stream));
        const i64 tile = l == 0 ? PartTile<W1>::TILE : PartTile<W1>::TILE;
        const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>((n_cur + tile - 1) / tile, part_grid_cap()));
        const SrcRecs<W1> rs{cur_w0.p, cur_w1.p};
        snprintf(tname, sizeof tname, "%s_count%d", timer_prefix, l + 1);
        { KTimer kt(tname);
        if (l == 0 && hist0) u64_copy_async(hist0, hist.p, (i64)nbk);
        else if (l == 0) k_part_count<Src, Dig><<<grid, PT, table_bytes, g_stream>>>(count_src ? *count_src : src, dig, n_cur, L, hist.p);
        else k_part_count<SrcRecs<W1>, Dig><<<grid, PT, 0, g_stream>>>(rs, dig, n_cur, L, hist.p); }
        HHX_LAUNCH_CHECK();
        i64 n_valid = 0;
        HHX_TRY(exclusive_scan_i64((const i64 *)hist.p, nbase.p, nbk, &n_valid));
        if (l == 0) out->n_valid = n_valid;
        if (n_valid == 0) {
            out->n_valid = 0;
            out->base = std::move(nbase);
            return 0;
        }
        if (nxt_w0.alloc((size_t)n_valid) || (PartW1<W1>::HAS && nxt_w1.alloc((size_t)n_valid))) return 1;
        u64_copy_async((const unsigned long long *)nbase.p, cursor.p, (i64)nbk + 1);
        snprintf(tname, sizeof tname, "%s_scatter%d", timer_prefix, l + 1);
        { KTimer kt(tname);
        const i64 stile = (i64)PartTile<W1>::ITEMS * (l == 0 ? T1 : TN);
        const unsigned sgrid = (unsigned)std::max<i64>(1, std::min<i64>((n_cur + stile - 1) / stile, part_grid_cap()));
        if (l == 0) k_part_scatter<Src, Dig, T1><<<sgrid, T1, part_scatter_table_at<W1, T1>() + table_bytes, g_stream>>>(src, dig, n_cur, L, cursor.p, nxt_w0.p, nxt_w1.p);
        else k_part_scatter<SrcRecs<W1>, Dig, TN><<<sgrid, TN, part_scatter_lds<W1, TN>(), g_stream>>>(rs, dig, n_cur, L, cursor.p, nxt_w0.p, nxt_w1.p); }
        HHX_LAUNCH_CHECK();
        HHX_HIP(hipStreamSynchronize(g_stream));                 // hist / cursor die here; the previous level's records too
        cur_w0 = std::move(nxt_w0);
        cur_w1 = std::move(nxt_w1);
        base = std::move(nbase);
        n_cur = n_valid;
    }
    out->w0 = std::move(cur_w0);
    out->w1 = std::move(cur_w1);
    out->base = std::move(base);
    return 0;
}

}  // namespace hhx
