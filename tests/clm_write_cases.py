"""A seeded corpus for the device writer of paired_links.clm (ingest_write_clm_fd in haphic_amd/csrc/hhx_pairs.hip, FileSink in
hhx_filesink.h), the contract it answers to, and a host mirror of where it cuts its work.

The contract is the oracle: oracle.ingest(..., bins=False, want_clm=True) followed by oracle.clm_text, the few-line restatement
of update_clm_dict / output_clm (scripts/HapHiC_cluster.py:376-401).  tests/golden/clm_write.npz holds what the reference's own
two functions wrote for the same streams.  Every case is (names, lengths, id1, p1, id2, p2, cuts of the pushes) with id1 != id2,
as pairs_generator_inter_ctgs :1562-1583 hands the read pairs over; positions are 0-based.

plan() takes the contract's per-line data and follows the writer: the kept contig pairs cut into chunks of `clm_chunk` distances
(whole pairs, upper_bound with its equality, at least one pair), the blocks of CW_T distances of a chunk and the span
b1 - (b0 & ~15) that decides staged / direct, and the pieces the text leaves in.  It is written from the constants below, which
mirror the .hip file; the GPU tests compare its counts with the device's counters, so a constant that moves there fails a test
instead of turning the boundary cases into ordinary ones.  Seeded; no GPU and no reference checkout needed."""
import bisect
import functools

import numpy as np

from oracle import oracle as orc

# constants of hhx_pairs.hip / hhx_filesink.h
CW_T = 256                      # distances per workgroup step of k_clm_write
CW_OUT_CAP = 24 * 1024          # bytes of its LDS window
CLM_CHUNK = 1 << 27             # distances per chunk (hhx_tune "clm_chunk", clamped to [4, CLM_CHUNK])
PIECE = 64 << 20                # bytes per piece of FileSink::write_device (hhx_tune "sink_piece", clamped to [4096, PIECE])
NBUF = 4                        # its pinned buffers
I32_MAX = 2 ** 31 - 1
FLANK = 10_000


def clamp_chunk(v):
    return CLM_CHUNK if v is None else max(4, min(CLM_CHUNK, int(v)))


def clamp_piece(v):
    return PIECE if v is None else max(4096, min(PIECE, int(v)))


# ------------------------------------------------------------------ cases and the contract
class Case:
    def __init__(self, name, names, lengths, id1, p1, id2, p2, cuts=()):
        self.name, self.names = name, list(names)
        self.lengths = np.asarray(lengths, np.int64)
        self.id1, self.id2 = np.asarray(id1, np.int32), np.asarray(id2, np.int32)
        self.p1, self.p2 = np.asarray(p1, np.int64), np.asarray(p2, np.int64)
        self.cuts = tuple(int(c) for c in cuts)
        n = len(self.names)
        assert len(set(self.names)) == n == len(self.lengths) and self.lengths.max() <= I32_MAX
        assert len(self.id1) == len(self.id2) == len(self.p1) == len(self.p2)
        assert (self.id1 != self.id2).all() and list(self.cuts) == sorted(set(self.cuts)) and all(0 < c < len(self.id1) for c in self.cuts)

    def __repr__(self):
        return 'Case(%s, %d contigs, %d pairs)' % (self.name, len(self.names), len(self.id1))

    @functools.cached_property
    def table(self):
        n = len(self.names)
        order = sorted(range(n), key=self.names.__getitem__)
        rank = np.empty(n, np.int32)
        rank[order] = np.arange(n, dtype=np.int32)
        return orc.FragTable(rank, self.lengths, np.arange(n, dtype=np.int32), np.zeros(n, np.uint8), 0, rank, self.lengths, np.ones(n, np.uint8))

    def pushes(self):
        """[(id1, p1, id2, p2)] of the case's pushes; the positions as int32 (every one fits)"""
        edges = (0,) + self.cuts + (len(self.id1),)
        return [(self.id1[a:b], self.p1[a:b].astype(np.int32), self.id2[a:b], self.p2[a:b].astype(np.int32)) for a, b in zip(edges, edges[1:])]

    @functools.cached_property
    def want(self):
        return orc.ingest(self.table, self.id1, self.p1, self.id2, self.p2, FLANK, bins=False, want_clm=True)

    @functools.cached_property
    def text(self):
        """the bytes of paired_links.clm"""
        w = self.want
        return orc.clm_text(self.names, w['full_i'], w['full_j'], w['clm_ptr'], w['clm'])

    @functools.cached_property
    def kept(self):
        return kept_groups(self.want)

    def name_len(self):
        return np.array([len(n.encode()) for n in self.names], np.int64)

    def plan(self, clm_chunk=None, sink_piece=None):
        return plan(self.kept, self.name_len(), clm_chunk, sink_piece)


def kept_groups(want):
    """[(contig i, contig j, read pairs c, int64 [4, c]: the distances of the four lines, ascending)] of the contig pairs output_clm :385 keeps,
    in dict order — the contract's per-line data"""
    out = []
    ptr, clm = want['clm_ptr'], want['clm']
    for k, (a, b) in enumerate(zip(want['full_i'].tolist(), want['full_j'].tolist())):
        v = clm[ptr[k]:ptr[k + 1]]
        if len(v) < 8:
            continue
        out.append((a, b, len(v) // 4, np.sort(v.reshape(-1, 4).T.astype(np.int64), axis=1)))
    return out


def n_digits(v):
    """decimal digits of non-negative int64 values (dlen of the .hip file)"""
    v = np.asarray(v, np.int64)
    assert (v >= 0).all()
    d = np.ones(v.shape, np.int64)
    for k in range(1, 19):
        d += v >= 10 ** k
    return d


# ------------------------------------------------------------------ the device's route, on the host
class Chunk:
    """groups [kr0, kr1) of one chunk: E distances, B bytes, the first element of every line, the blocks' (b0, b1, span), whether the cut
    fell on upper_bound's equality, whether it is one group larger than the chunk"""


def plan(kept, name_len, clm_chunk=None, sink_piece=None):
    """-> dict: chunks [Chunk], n_chunks, direct (blocks written straight into HBM, per chunk), staged, pieces (bytes of every piece), n_bytes,
    n_lines"""
    chunk, piece = clamp_chunk(clm_chunk), clamp_piece(sink_piece)
    eoff = [0]
    for g in kept:
        eoff.append(eoff[-1] + g[2])
    nk = len(kept)
    chunks, pieces = [], []
    kr0 = 0
    while kr0 < nk:
        limit = eoff[kr0] + chunk // 4
        kr1 = bisect.bisect_right(eoff, limit, kr0 + 1) - 1           # std::upper_bound(eoff + kr0 + 1, end, limit) - eoff - 1
        c = Chunk()
        c.oversize = kr1 <= kr0
        if kr1 <= kr0:
            kr1 = kr0 + 1
        c.kr0, c.kr1 = kr0, kr1
        c.equality = not c.oversize and eoff[kr1] == limit
        lens, starts = [], []
        e = 0
        for a, b, cnt, dist in kept[kr0:kr1]:
            hdr = int(name_len[a] + name_len[b]) + 5 + len(str(2 * cnt))      # "{ctg_i}{s} {ctg_j}{s}\t{2c}\t"
            ln = 2 * n_digits(dist) + 2                                      # "{d} {d}" and a blank or the line break
            ln[:, 0] += hdr
            lens.append(ln.reshape(-1))
            starts += [e + n * cnt for n in range(4)]
            e += 4 * cnt
        off = np.concatenate([[0], np.cumsum(np.concatenate(lens))])
        c.E, c.B, c.line_starts = e, int(off[-1]), starts
        assert c.E == 4 * (eoff[kr1] - eoff[kr0])
        c.blocks = []
        for e0 in range(0, c.E, CW_T):
            b0, b1 = int(off[e0]), int(off[min(e0 + CW_T, c.E)])
            c.blocks.append((b0, b1, b1 - (b0 & ~15)))
        c.direct = sum(1 for _b0, _b1, span in c.blocks if span > CW_OUT_CAP)
        chunks.append(c)
        pieces += [min(piece, c.B - o) for o in range(0, c.B, piece)]
        kr0 = kr1
    return dict(chunks=chunks, n_chunks=len(chunks), direct=[c.direct for c in chunks], staged=[len(c.blocks) - c.direct for c in chunks],
                pieces=pieces, n_bytes=sum(c.B for c in chunks), n_lines=4 * nk)


def counters(p):
    """what the profile counters of one file must read"""
    return dict(clm_chunks=p['n_chunks'], clm_blocks_direct=sum(p['direct']), sink_pieces=len(p['pieces']))


COUNTERS = ('clm_chunks', 'clm_blocks_direct', 'sink_pieces')


def first_difference(case, got, clm_chunk=None):
    """where the first byte that differs from the contract lies: a line for the assertion message"""
    want = case.text
    n = next((k for k, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    p, at = case.plan(clm_chunk), 0
    for ci, c in enumerate(p['chunks']):
        if n < at + c.B:
            bi = next(k for k, (b0, b1, _s) in enumerate(c.blocks) if n - at < b1)
            return 'byte %d of %d / %d: chunk %d (groups %d..%d) block %d, line %d; got %r want %r' % (
                n, len(got), len(want), ci, c.kr0, c.kr1, bi, want[:n].count(b'\n'), got[max(0, n - 20):n + 20], want[max(0, n - 20):n + 20])
        at += c.B
    return 'byte %d of %d / %d (past the last chunk)' % (n, len(got), len(want))


# ------------------------------------------------------------------ the corpus
def _name(k, length):
    """a name of `length` bytes whose order among its siblings is that of k, whatever the lengths"""
    base = 'n%03d' % k
    assert length >= len(base)
    return base + ('_' + 'ACGTacgt0123456789.|:' * 20)[:length - len(base)]


def _stream(rng, groups):
    """groups: [(u, v, [(pos on u, pos on v)])] -> id1, p1, id2, p2 with the groups interleaved, the two ends of a pair in either order, and the
    first pair of every group up front in the order given — dict order, which need not be key order"""
    head, rest = [], []
    for u, v, pos in groups:
        head.append((u, pos[0][0], v, pos[0][1]))
        rest += [(u, a, v, c) for a, c in pos[1:]]
    rest = [rest[k] for k in rng.permutation(len(rest))] if rest else []
    rows = np.array(head + rest, np.int64).reshape(-1, 4)
    swap = rng.random(len(rows)) < 0.5
    rows[swap] = rows[swap][:, [2, 3, 0, 1]]
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def _random_pos(rng, lu, lv, c):
    return list(zip(rng.integers(0, lu, c).tolist(), rng.integers(0, lv, c).tolist()))


GROUP_SIZES = (256, 255, 1, 2, 3, 63, 64, 65, 257, 1000)        # 256 then 255: a line header on the first and on the last element of a block


def group_sizes():
    rng = np.random.default_rng(8100)
    n = 14
    names = [_name(n - 1 - k, (4, 9, 17, 30)[k % 4]) for k in range(n)]          # ids descend in name order: the ends are swapped by the sort :1629
    lengths = rng.integers(5_000, 3_000_000, n)
    pairs = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13), (0, 2), (1, 3), (4, 6)]
    groups = []
    for (u, v), c in zip(pairs, GROUP_SIZES):
        pos = _random_pos(rng, lengths[u], lengths[v], c)
        pos[c // 2:c // 2 + 3] = [pos[c // 2]] * len(pos[c // 2:c // 2 + 3])   # equal distances inside a line
        groups.append((u, v, pos))
    s = _stream(rng, groups)
    m = len(s[0])
    return Case('group_sizes', names, lengths, *s, cuts=(m // 7, m // 7 + 1234))


DIGIT_COUNTS = (2, 4, 5, 49, 50, 499, 500)
DIGIT_LEN = 1_500_000_000
DIGIT_VALUES = tuple(sorted({v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)} | {0}))


def digit_targets():
    """{orientation n: {distance: (a, c)}}: 0-based positions on two contigs of DIGIT_LEN that give the distance on line n"""
    L = DIGIT_LEN
    out = {0: {}, 1: {}, 2: {}, 3: {}}
    for v in DIGIT_VALUES:
        if v >= 1:
            out[0][v] = (L - v, 0) if v <= L else (0, v - L)                       # len_i - a + c
            out[3][v] = (0, L - v) if v <= L else (v - L, 0)                       # a + len_j - c
        if v >= 2:
            out[1][v] = (L - v // 2, L - (v - v // 2))                              # len_i - a + len_j - c
        out[2][v] = (v // 2, v - v // 2)                                           # a + c
    return out


def digits():
    rng = np.random.default_rng(8200)
    n = 8
    names = ['d%d' % k for k in range(n)]
    lengths = np.full(n, DIGIT_LEN)
    pairs = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6)]
    wanted = [ac for t in digit_targets().values() for ac in t.values()]
    groups = [(u, v, _random_pos(rng, DIGIT_LEN, DIGIT_LEN, c)) for (u, v), c in zip(pairs, DIGIT_COUNTS)]
    at = [0] * len(groups)
    for k, ac in enumerate(wanted):                                   # dealt round the groups that still have room; the large ones take the rest
        gi = k % len(groups)
        while at[gi] >= DIGIT_COUNTS[gi] - (1 if DIGIT_COUNTS[gi] > 2 else 0):
            gi = (gi + 1) % len(groups)
        groups[gi][2][at[gi]] = ac
        at[gi] += 1
    for gi, c in enumerate(DIGIT_COUNTS):                             # equal distances inside a line
        if c > 2:
            groups[gi][2][c - 1] = groups[gi][2][0]
    s = _stream(rng, groups)
    return Case('digits', names, lengths, *s, cuts=(100, 101, 700))


def longest(max_len=I32_MAX, tag='2p31m1'):
    """two contigs of max_len with read pairs at position 0 and at the last base, and two shorter contigs; the first kept pair is the two longest
    at position 0: the largest distance there is, len_i + len_j"""
    rng = np.random.default_rng(8300)
    names = ['big_a', 'big_b', 'small_c', 'small_d']
    lengths = np.array([max_len, max_len, 1000, 7])
    last = max_len - 1
    groups = [(0, 1, [(0, 0), (last, last), (0, last), (last, 0), (last // 2, last // 2 + 1)]),
              (2, 0, [(0, 0), (999, last), (999, 0)]),
              (3, 1, [(6, last), (0, 0)]),
              (2, 3, [(0, 0), (999, 6)])]
    return Case('longest_' + tag, names, lengths, *_stream(rng, groups), cuts=(3,))


PHASE_NAME = 5


def phase_case(phase):
    """a kept group of two read pairs in front, then a group of 300 whose first line holds the start of the second block: `phase` more bytes in
    that line's header move the byte the block starts on by as many — the 16 cases run b0 & 15 of that block through every residue"""
    rng = np.random.default_rng(8400)
    names = [_name(0, 6), _name(1, 6), _name(2, PHASE_NAME + phase), _name(3, 11), _name(4, 5)]
    lengths = np.array([50_000, 60_000, 70_000, 80_000, 90_000])
    groups = [(0, 1, _random_pos(rng, 50_000, 60_000, 2)), (2, 3, _random_pos(rng, 70_000, 80_000, 300)), (3, 4, _random_pos(rng, 80_000, 90_000, 70))]
    return Case('phase_%02d' % phase, names, lengths, *_stream(rng, groups), cuts=(1,))


def _elements(kept):
    """the bytes of every distance without the headers, and where the headers go: (base [E], first element of every line, its contigs i / j,
    the digits of its count field)"""
    base, starts, ci, cj, cd = [], [], [], [], []
    e = 0
    for a, b, cnt, dist in kept:
        base.append((2 * n_digits(dist) + 2).reshape(-1))
        starts += [e + n * cnt for n in range(4)]
        ci += [a] * 4
        cj += [b] * 4
        cd += [len(str(2 * cnt))] * 4
        e += 4 * cnt
    return np.concatenate(base), np.array(starts), np.array(ci), np.array(cj), np.array(cd)


def _spans(el, name_len):
    base, starts, ci, cj, cd = el
    ln = base.copy()
    ln[starts] += name_len[ci] + name_len[cj] + 5 + cd
    off = np.concatenate([[0], np.cumsum(ln)])
    e0 = np.arange(0, len(base), CW_T)
    b0, b1 = off[e0], off[np.minimum(e0 + CW_T, len(base))]
    return b1 - (b0 & ~15)


# the regions of the `direct` case: (pool of contigs, groups, read pairs of every group).  Groups of two read pairs alone give even spans only
# (every name and every distance is there twice per pair of lines, and a block of 256 distances ends on an even number of such lines), so the
# two regions of the boundary blocks put a group of three across every block seam, eight of its distances before it: three headers on one
# side, one on the other, and a byte more in its names is an odd number of bytes more in either block
# (every contig of M1 / M2 is in one group only: one byte more in its name is one byte more per line of that group)
def _seam_size(e):
    return 3 if e % CW_T in (CW_T - 8, 4) else 2                   # the second one brings the groups of two back onto multiples of 8


_DIRECT_REGIONS = (('S', 16, 70, lambda e: 2), ('L', 15, 100, lambda e: 2), ('M1', 160, 80, _seam_size), ('M2', 160, 80, _seam_size), ('S', 0, 40, lambda e: 2))
DIRECT_BLOCK_AT_CAP, DIRECT_BLOCK_OVER_CAP = 6, 9          # blocks wholly inside M1 / M2


def direct():
    """names of 100 to 300 bytes on groups of two read pairs: blocks beyond the LDS window next to staged ones, and two blocks whose span the
    builder sets to CW_OUT_CAP and CW_OUT_CAP + 1 exactly by walking the lengths of the names of their regions"""
    rng = np.random.default_rng(8500)
    pools, n = {}, 0
    for tag, n_ctg, _g, _c in _DIRECT_REGIONS:
        if n_ctg:
            pools[tag] = list(range(n, n + n_ctg))
            n += n_ctg
    lengths = rng.integers(100_000, 1_000_000, n)
    name_len = np.zeros(n, np.int64)
    name_len[pools['S']] = rng.integers(4, 12, len(pools['S']))
    name_len[pools['L']] = rng.integers(100, 301, len(pools['L']))
    name_len[pools['M1']] = 79
    name_len[pools['M2']] = 79
    groups, used, e, span_of = [], {}, 0, {}
    for tag, _n, n_groups, size in _DIRECT_REGIONS:
        span_of[tag] = [e, None]
        pool = pools[tag]
        free = used.setdefault(tag, [(u, v) for k, u in enumerate(pool) for v in pool[k + 1:]] if tag in 'SL' else list(zip(pool[::2], pool[1::2])))
        for k in range(n_groups):
            u, v = free.pop(int(rng.integers(len(free))))
            groups.append((u, v, _random_pos(rng, lengths[u], lengths[v], size(e))))
            e += 4 * len(groups[-1][2])
        span_of[tag][1] = e
    s = _stream(rng, groups)
    probe = Case('direct_probe', [_name(k, 4) for k in range(n)], lengths, *s)        # the distances do not depend on the names' lengths
    el = _elements(probe.kept)
    for block, target, tag in ((DIRECT_BLOCK_AT_CAP, CW_OUT_CAP, 'M1'), (DIRECT_BLOCK_OVER_CAP, CW_OUT_CAP + 1, 'M2')):
        pool = pools[tag]
        assert span_of[tag][0] <= block * CW_T and (block + 1) * CW_T <= span_of[tag][1]
        for _ in range(20_000):
            d = target - int(_spans(el, name_len)[block])
            if d == 0:
                break
            t = pool[int(rng.integers(len(pool)))]
            step = int(np.sign(d)) if rng.random() < 0.8 else -int(np.sign(d))
            if not 60 <= name_len[t] + step <= 99:
                continue
            name_len[t] += step
            d2 = target - int(_spans(el, name_len)[block])
            if abs(d2) > abs(d) and not (abs(d) < 16 and rng.random() < 0.3):
                name_len[t] -= step
        assert int(_spans(el, name_len)[block]) == target, (tag, d)
    m = len(s[0])
    return Case('direct', [_name(k, int(name_len[k])) for k in range(n)], lengths, *s, cuts=(m // 3, m // 3 + 5))


def short_names(total):
    """one-byte names; E = 4 * total distances in the whole file"""
    rng = np.random.default_rng(8600 + total)
    names = list('abcdefgh')
    lengths = rng.integers(50, 5000, len(names))
    sizes = {10: (2, 3, 5), 64: (2, 3, 5, 54), 1: ()}[total]
    pairs = [(0, 1), (2, 3), (4, 5), (6, 7)]
    groups = [(u, v, _random_pos(rng, lengths[u], lengths[v], c)) for (u, v), c in zip(pairs, sizes)]
    groups.append((0, 7, _random_pos(rng, lengths[0], lengths[7], 1)))           # skipped
    return Case('short_names_E%d' % (4 * total), names, lengths, *_stream(rng, groups), cuts=(2,))


def nothing_kept(one_kept):
    """every contig pair has one read pair (an empty file); one_kept: thousands of them and one pair of two in their middle"""
    rng = np.random.default_rng(8700 + one_kept)
    n = 80 if one_kept else 12
    names = [_name(k, 4 + k % 9) for k in range(n)]
    lengths = rng.integers(1000, 100_000, n)
    all_pairs = [(u, v) for u in range(n) for v in range(u + 1, n)]
    pick = rng.permutation(len(all_pairs))[:3000 if one_kept else 50]
    groups = [(all_pairs[k][0], all_pairs[k][1], _random_pos(rng, lengths[all_pairs[k][0]], lengths[all_pairs[k][1]], 1)) for k in pick]
    if one_kept:
        u, v, pos = groups[1500]
        groups[1500] = (u, v, pos + _random_pos(rng, lengths[u], lengths[v], 1))
    return Case('one_kept_among_thousands' if one_kept else 'nothing_kept', names, lengths, *_stream(rng, groups), cuts=(len(groups) // 2,))


def random_case():
    rng = np.random.default_rng(8800)
    n, m = 40, 20_000
    names = [_name(k * 7 % n, (4, 6, 13, 40, 120)[k % 5]) for k in range(n)]
    lengths = rng.integers(20_000, 3_000_000, n)
    id1 = rng.integers(0, n, m)
    id2 = np.where(rng.random(m) < 0.9, (id1 + 1) % n, (id1 + 1 + rng.integers(0, n - 1, m)) % n)       # heavy groups, and thin ones down to one read pair
    p1 = (rng.random(m) * lengths[id1]).astype(np.int64)
    p2 = (rng.random(m) * lengths[id2]).astype(np.int64)
    p2[::5] = p1[::5] % lengths[id2[::5]]                              # ties
    return Case('random', names, lengths, id1, p1, id2, p2, cuts=(777, 12_345))


def beyond(negative):
    """a small stream with one read position equal to its contig's length (the first the writer refuses); negative: and one so far beyond
    that output_clm prints a negative distance"""
    rng = np.random.default_rng(8900)
    names = ['ctgA', 'ctgB', 'ctgC']
    lengths = np.array([3000, 4000, 5000])
    groups = [(0, 1, _random_pos(rng, 3000, 4000, 5) + [(3000, 17)]), (1, 2, _random_pos(rng, 4000, 5000, 3)), (0, 2, _random_pos(rng, 3000, 5000, 4))]
    if negative:
        groups[2][2].append((3900, 2))                               # len_i - a + c = -898
    return Case('beyond_negative' if negative else 'beyond_edge', names, lengths, *_stream(rng, groups), cuts=(4,))


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith('phase_'):
        return phase_case(int(name[6:]))
    return {'group_sizes': group_sizes, 'digits': digits, 'longest_2p31m1': longest,
            'longest_2p20m1': lambda: longest(2 ** 20 - 1, '2p20m1'), 'longest_2p20': lambda: longest(2 ** 20, '2p20'),
            'direct': direct, 'short_names_E40': lambda: short_names(10), 'short_names_E256': lambda: short_names(64),
            'nothing_kept': lambda: nothing_kept(0), 'one_kept_among_thousands': lambda: nothing_kept(1), 'random': random_case,
            'beyond_edge': lambda: beyond(0), 'beyond_negative': lambda: beyond(1)}[name]()


PHASE_NAMES = tuple('phase_%02d' % p for p in range(16))
CASE_NAMES = ('group_sizes', 'digits', 'longest_2p31m1', 'longest_2p20m1', 'longest_2p20') + PHASE_NAMES + (
    'direct', 'short_names_E40', 'short_names_E256', 'nothing_kept', 'one_kept_among_thousands', 'random')
REFUSED_NAMES = ('beyond_edge', 'beyond_negative')
CHUNK_SWEEP_CASES = ('group_sizes', 'direct', 'random')
PIECE_SWEEP_CASES = ('random', 'direct')


@functools.lru_cache(maxsize=None)
def equality_chunk(name):
    """the smallest "clm_chunk" above 8 at which the case's file is three chunks or more and one of several contig pairs ends exactly on the limit
    (upper_bound's equality); with a contig pair larger than the chunk as well, where the case has one"""
    c = case(name)
    biggest = max(g[2] for g in c.kept)
    found = None
    for m in range(3, sum(g[2] for g in c.kept)):
        p = c.plan(4 * m)
        if p['n_chunks'] >= 3 and any(ch.equality and ch.kr1 - ch.kr0 >= 2 for ch in p['chunks']):
            if any(ch.oversize for ch in p['chunks']) or biggest <= m:
                return 4 * m
            found = found or 4 * m
        if m > 4096 and found:
            break
    return found


def chunk_settings(name):
    return (4, 8, 1024, equality_chunk(name), None)


def piece_settings(name):
    return (4096, 4096 * 3, len(case(name).text), None)


# ------------------------------------------------------------------ tests/golden/clm_write.npz (make_golden_clm_write.py)
GOLDEN_CASES = CASE_NAMES + REFUSED_NAMES
GOLDEN_TEXT_MAX = 100_000          # a text above this is kept as its SHA-256 and length


def golden_outputs(z):
    """{case name: (length, sha256 hex, bytes | None)}: what the reference's own output_clm wrote"""
    out, at = {}, 0
    for k, name in enumerate(z['case_names']):
        n, kept = int(z['text_len'][k]), bool(z['text_kept'][k])
        out[str(name)] = (n, str(z['text_sha256'][k]), z['text'][at:at + n].tobytes() if kept else None)
        at += n if kept else 0
    return out
