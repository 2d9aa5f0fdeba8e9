"""A seeded corpus for the CLM splitter (haphic_amd/csrc/hhx_clmsplit.hip), the contract it answers to, and a host mirror of its
state machine.

split_spec() is the few-line restatement of split_clm_file (scripts/HapHiC_reassign.py:581-622): universal newlines, line.split(),
the last character of the first two tokens dropped, the line written verbatim to its group's file when both names share a group,
IndexError for a line with fewer than two tokens.  Every case is (text, names, group_of_name, n_groups); what it must give is
split_spec on the same bytes (tests/golden/clm_split.npz holds what the reference's own function wrote for them).

simulate() follows a sequence of pushes the way the .hip file does — the held-back '\\r', the carried head, the continuation
segments, the group-major output buffer cut into gather tiles — and returns the counters of hhx_clm_split_stats next to the
bytes.  It is written from the constants below, which mirror the .hip file; the GPU tests compare its counters with the
device's, so a constant that moves there fails a test instead of turning the boundary cases into ordinary ones.
Seeded, no GPU and no reference checkout needed."""
import functools

import numpy as np

from tests.pairs_text_cases import SEPS, in_domain, line_bounds

# constants of hhx_textscan.h / hhx_clmsplit.hip
TX_BLOCK = 4096                 # bytes per workgroup step of the line-break passes
GATHER_TILE = 16 * 1024         # destination bytes per workgroup step of the gather
HEAD_MAX = 64 * 1024            # bound of the carried head of a line
STATS = ('lines', 'kept', 'heads', 'seams', 'continuations', 'multi_line_tiles', 'multi_tile_lines')

WS = frozenset(SEPS + b'\r\n')


# ------------------------------------------------------------------ the contract
def split_spec(text, names, group_of_name, n_groups):
    """[bytes per group], or IndexError: split_clm_file :614-619 on the bytes of the file"""
    text = bytes(text)
    group = {n: g for n, g in zip(names, group_of_name) if g >= 0}
    out = [bytearray() for _ in range(n_groups)]
    b = line_bounds(text)
    for k in range(len(b) - 1):
        raw = text[b[k]:b[k + 1]]
        line = raw[:-2] + b'\n' if raw.endswith(b'\r\n') else raw[:-1] + b'\n' if raw.endswith(b'\r') else raw      # universal newlines
        cols = line.decode('utf-8').split()
        ctg_1, ctg_2 = cols[0][:-1], cols[1][:-1]                     # IndexError: list index out of range
        if ctg_1 in group and ctg_2 in group and group[ctg_1] == group[ctg_2]:
            out[group[ctg_1]] += line
    return [bytes(x) for x in out]


# ------------------------------------------------------------------ the device's route, on the host
def _two_tokens(seg):
    """(tokens found (at most 2), position behind the last one) of the bytes, whitespace as the kernel's is_ws"""
    p, toks = 0, []
    while len(toks) < 2:
        while p < len(seg) and seg[p] in WS:
            p += 1
        if p >= len(seg):
            break
        s = p
        while p < len(seg) and seg[p] not in WS:
            p += 1
        toks.append(seg[s:p])
    return toks, p


def simulate(pieces, names, group_of_name, n_groups):
    """-> ([bytes per group], {counter: value}); IndexError / RuntimeError (head bound) as the library raises them"""
    group = {n.encode(): g for n, g in zip(names, group_of_name)}
    out = [bytearray() for _ in range(n_groups)]
    stat = dict.fromkeys(STATS, 0)
    kind, open_group, head, pending_cr = 0, -1, b'', False          # kind: 0 at a line start, 1 head carried, 2 fate decided
    for piece, final in [(bytes(p), False) for p in pieces] + [(b'', True)]:
        if final and not (head or pending_cr):
            break
        n = len(piece)
        if n and pending_cr and piece[:1] == b'\n':
            stat['seams'] += 1
        hold = not final and n > 0 and piece[-1:] == b'\r'
        work = head + (b'\r' if pending_cr else b'') + (piece[:-1] if hold else piece)
        m = len(work)
        if m == 0 or (n == 0 and not final):
            pending_cr = pending_cr or hold
            continue
        head, pending_cr = b'', hold
        w = np.frombuffer(work, np.uint8)
        nxt = np.append(w[1:], np.uint8(0))
        cut = (np.flatnonzero((w == 10) | ((w == 13) & (nxt != 10))) + 1).tolist()
        emitted = []                                                 # (group, bytes) of this push, in stream order
        for k in range(len(cut) + 1):
            has_break = k < len(cut)
            a, e = (cut[k - 1] if k else 0), (cut[k] if has_break else m)
            ce = e
            if has_break:
                ce = e - 2 if (work[e - 1] == 10 and e - 2 >= a and work[e - 2] == 13) else e - 1
            g, seg_kind = -1, 0
            if k == 0 and kind == 2:
                g, seg_kind = open_group, 2
                stat['continuations'] += int(e > a)
            elif has_break or ce > a:
                lim = min(ce - a, HEAD_MAX + 1)
                toks, p = _two_tokens(work[a:a + lim])
                ended = len(toks) == 2 and p < lim
                if not ended and lim < ce - a:
                    raise RuntimeError('the first two tokens of a line do not end within %d bytes' % HEAD_MAX)
                elif not has_break and not final and not ended:
                    seg_kind = 1
                elif len(toks) < 2:
                    raise IndexError('list index out of range')
                else:
                    g1, g2 = (group.get(t.decode('utf-8')[:-1].encode(), -1) for t in toks)         # the last CHARACTER goes
                    g = g1 if g1 >= 0 and g1 == g2 else -1
                    seg_kind = 2
                    stat['lines'] += 1
                    stat['kept'] += int(g >= 0)
            if g >= 0 and seg_kind == 2 and (ce - a) + int(has_break) > 0:
                emitted.append((g, work[a:ce] + (b'\n' if has_break else b'')))
            if not has_break:
                kind, open_group = seg_kind, g
                if seg_kind == 1:
                    if m - a > HEAD_MAX:
                        raise RuntimeError('the first two tokens of a line do not end within %d bytes' % HEAD_MAX)
                    head = work[a:]
                    stat['heads'] += 1
        emitted.sort(key=lambda x: x[0])                             # stable: stream order inside a group
        off = 0
        tiles = {}
        for g, seg in emitted:
            out[g] += seg
            first, last = off // GATHER_TILE, (off + len(seg) - 1) // GATHER_TILE
            stat['multi_tile_lines'] += int(last > first)
            for t in range(first, last + 1):
                tiles[t] = tiles.get(t, 0) + 1
            off += len(seg)
        stat['multi_line_tiles'] += sum(1 for c in tiles.values() if c > 1)
    return [bytes(x) for x in out], stat


def pushes(text, size):
    return [text[k:k + size] for k in range(0, len(text), size)]


# ------------------------------------------------------------------ the corpus
class Case:
    """kind 'ok': the files equal split_spec.  'error': the reference raises IndexError (bad_line: 1-based).  'head': the library's own
    refusal, a first token beyond HEAD_MAX.  small: under 400 bytes — also run with a cut at every byte offset."""

    def __init__(self, section, name, text, names, group_of_name, n_groups, kind='ok'):
        self.section, self.name, self.text, self.names = section, name, bytes(text), list(names)
        self.group_of_name, self.n_groups, self.kind = list(group_of_name), int(n_groups), kind
        assert len(self.names) == len(self.group_of_name) == len(set(self.names))
        assert all(-1 <= g < self.n_groups for g in self.group_of_name)
        assert in_domain(self.text), name
        self.small = len(self.text) < 400

    @functools.cached_property
    def want(self):
        """[bytes per group], or the IndexError class"""
        try:
            return split_spec(self.text, self.names, self.group_of_name, self.n_groups)
        except IndexError:
            return IndexError

    def args(self):
        return self.names, self.group_of_name, self.n_groups

    def __repr__(self):
        return 'Case(%s/%s, %d bytes, G=%d)' % (self.section, self.name, len(self.text), self.n_groups)


_DIGITS = np.frombuffer(b'0123456789', np.uint8)

NAMES3 = ['ctgA', 'ctgB', 'ctgC', 'ctgD', 'ctgE', 'ctgF', 'lone', 'utg1', 'utg10', 'utg100']
GROUP3 = [0, 0, 1, 1, 2, 2, -1, 0, 0, 1]          # three groups; 'lone' is in none; utg1 / utg10 / utg100 are prefixes of each other


def clm_line(a, b, rng, n_links=None, orient=b'+-', sep=(b' ', b'\t', b' ')):
    """'{a}{o} {b}{o}\\t{n}\\t{d1} {d2} ...' as output_clm writes it (no terminator)"""
    n = int(rng.integers(1, 5)) if n_links is None else n_links
    dists = b' '.join(b'%d' % int(rng.integers(1, 10**6)) for _ in range(n))
    a = a.encode() if isinstance(a, str) else a
    b = b.encode() if isinstance(b, str) else b
    return a + orient[:1] + sep[0] + b + orient[1:2] + sep[1] + (b'%d' % n) + sep[1] + dists


def padded_line(a, b, n, rng, end=b'\n'):
    """a CLM line of exactly n bytes, terminator included: the distances take the slack"""
    headb = a.encode() + b'+ ' + b.encode() + b'-\t7\t'
    fill = n - len(headb) - len(end)
    assert fill > 0, n
    d = bytearray(rng.choice(_DIGITS[1:], fill))
    d[9::10] = b' ' * len(d[9::10])
    if d[-1:] == b' ':
        d[-1:] = b'5'
    return headb + bytes(d) + end


def _line_ends():
    rng = np.random.default_rng(7100)
    pairs = [('ctgA', 'ctgB'), ('ctgC', 'ctgD'), ('ctgA', 'ctgC'), ('ctgE', 'ctgF'), ('lone', 'ctgA'), ('ctgB', 'ctgA')]
    bodies = [clm_line(a, b, rng) for a, b in pairs]
    for tag, ends in (('lf', [b'\n']), ('crlf', [b'\r\n']), ('cr', [b'\r']), ('mixed', [b'\n', b'\r\n', b'\r', b'\r\n', b'\n', b'\r'])):
        text = b''.join(x + ends[k % len(ends)] for k, x in enumerate(bodies))
        yield Case('line_ends', tag, text, NAMES3, GROUP3, 3)
        yield Case('line_ends', tag + '_no_final_break', text + clm_line('ctgD', 'ctgC', rng), NAMES3, GROUP3, 3)
    yield Case('line_ends', 'empty_file', b'', NAMES3, GROUP3, 3)
    yield Case('line_ends', 'one_line', clm_line('ctgE', 'ctgF', rng) + b'\n', NAMES3, GROUP3, 3)
    yield Case('line_ends', 'one_line_cr', clm_line('ctgE', 'ctgF', rng) + b'\r', NAMES3, GROUP3, 3)
    yield Case('line_ends', 'one_line_open', clm_line('ctgE', 'ctgF', rng), NAMES3, GROUP3, 3)
    yield Case('line_ends', 'one_line_two_tokens_open', b'ctgE+ ctgF-', NAMES3, GROUP3, 3)
    yield Case('line_ends', 'crcrlf_between_good_lines', bodies[0] + b'\r\r\n' + bodies[1] + b'\n', NAMES3, GROUP3, 3, 'error')


def _tokens():
    rng = np.random.default_rng(7200)
    lines = [b' ' + clm_line('ctgA', 'ctgB', rng) + b' \n', b'\t\x0b' + clm_line('ctgC', 'ctgD', rng) + b'\x1f\t\r\n']
    yield Case('tokens', 'leading_and_trailing_whitespace', b''.join(lines), NAMES3, GROUP3, 3)
    for k in range(len(SEPS)):
        s = SEPS[k:k + 1]
        text = b''.join(s * r + clm_line('ctgA', 'ctgB', rng, 2, sep=(s * r, s * (r + 1), s)) + s * r + b'\n' for r in (1, 2, 5))
        yield Case('tokens', 'runs_of_sep_%02x' % SEPS[k], text, NAMES3, GROUP3, 3)
    # one-byte tokens: the empty name, which is in no table
    yield Case('tokens', 'one_byte_tokens', b'+ -\t1\t5\nctgA+ ctgB-\t1\t7\n+ ctgA-\n', NAMES3, GROUP3, 3)
    yield Case('tokens', 'exactly_two_tokens', b'ctgA+ ctgB-\nctgC- ctgD+\r\nctgA+ ctgC+\rctgE+ ctgF+', NAMES3, GROUP3, 3)
    # the dropped character is whatever it is, multi-byte ones included
    yield Case('tokens', 'any_orientation_byte', b'ctgAx ctgBy 1 2\nctgA\xc3\xa9 ctgB+ 1 2\nctgA ctgB 1 2\nctgA++ ctgB+ 1 2\n', NAMES3, GROUP3, 3)
    for lo in range(1, 41, 5):                                       # names of 1..40 bytes, with their own prefixes as neighbours in the table
        names = [('N%02d' % L + 'abcdefghijklmnopqrstuvwxyz0123456789_')[:L] if L > 2 else 'NM'[:L] for L in range(lo, lo + 5)]
        names = list(dict.fromkeys(names))
        grp = [k % 2 for k in range(len(names))]
        body = []
        for k, nm in enumerate(names):
            mate = names[(k + 2) % len(names)]
            body.append(clm_line(nm, mate, rng, 1) + b'\n')
            body.append(clm_line(nm + 'x', mate, rng, 1) + b'\n')      # one byte more: absent (or a sibling)
            body.append(clm_line(nm, mate[:-1] or 'q', rng, 1) + b'\n')
        yield Case('tokens', 'names_of_%d_to_%d_bytes' % (lo, lo + 4), b''.join(body), names, grp, 2)
    yield Case('tokens', 'prefix_names', b''.join(clm_line(a, b, rng, 1) + b'\n' for a, b in
                                                  (('utg1', 'utg10'), ('utg10', 'utg100'), ('utg100', 'ctgC'), ('utg1', 'utg1'), ('utg', 'utg1'), ('utg1000', 'utg100'))),
               NAMES3, GROUP3, 3)
    yield Case('tokens', 'absent_and_ungrouped', b''.join(clm_line(a, b, rng, 1) + b'\n' for a, b in
                                                          (('nobody', 'ctgA'), ('ctgA', 'nobody'), ('lone', 'ctgA'), ('ctgA', 'lone'), ('lone', 'lone'), ('ctgA', 'ctgB'))),
               NAMES3, GROUP3, 3)
    yield Case('tokens', 'different_groups_and_same_contig', b''.join(clm_line(a, b, rng, 1) + b'\n' for a, b in
                                                                      (('ctgA', 'ctgC'), ('ctgC', 'ctgE'), ('ctgA', 'ctgA'), ('ctgF', 'ctgF'), ('ctgE', 'ctgB'))),
               NAMES3, GROUP3, 3)
    u8 = ['Ņš', 'ŜŝŞş', 'rŅŠ', 'ŉŊŋŌō']
    text = b''.join(clm_line(a, b, rng, 1) + b'\n' for a, b in ((u8[0], u8[1]), (u8[2], u8[3]), (u8[0], u8[2]), (u8[1], u8[0]), (u8[3], 'Ņ')))
    yield Case('tokens', 'multibyte_names', text, u8, [0, 0, 1, 1], 2)


def _groups():
    rng = np.random.default_rng(7300)
    names = ['c%03d' % k for k in range(24)]
    for G in (1, 3, 70, 300):
        grp = [k % G for k in range(len(names))]
        same = [(a, b) for a in range(len(names)) for b in range(len(names)) if a != b and grp[a] == grp[b]]
        lines = []
        for k in range(6):
            a, b = same[int(rng.integers(len(same)))] if same else (0, 0)
            lines.append(clm_line(names[a], names[b], rng, 1) + b'\n')
            lines.append(clm_line(names[a], names[(a + 1) % len(names)], rng, 1) + b'\n')       # G > 1: another group
        yield Case('groups', 'G_%d' % G, b''.join(lines), names, grp, G)
    yield Case('groups', 'every_line_to_one_group', b''.join(clm_line('ctgC', 'ctgD', rng, 2) + (b'\n', b'\r\n')[k % 2] for k in range(8)), NAMES3, GROUP3, 3)
    yield Case('groups', 'alternating_two_groups', b''.join(clm_line(*(('ctgA', 'ctgB'), ('ctgE', 'ctgF'))[k % 2], rng, 1) + b'\n' for k in range(12)),
               NAMES3, GROUP3, 3)
    yield Case('groups', 'nothing_kept', b''.join(clm_line('ctgA', 'ctgC', rng, 2) + b'\n' for k in range(5)), NAMES3, GROUP3, 3)
    yield Case('groups', 'no_names_no_groups', clm_line('ctgA', 'ctgB', rng, 2) + b'\n', [], [], 0)


BAD_SHAPES = {'empty': b'', 'whitespace_only': b' \t ', 'one_token': b'ctgA+', 'cr_only': None}


def _errors():
    rng = np.random.default_rng(7400)
    good = [clm_line('ctgA', 'ctgB', rng, 2), clm_line('ctgC', 'ctgD', rng, 2), clm_line('ctgE', 'ctgA', rng, 2)]
    for tag, bad in BAD_SHAPES.items():
        for where in ('first', 'middle', 'last'):
            lines = list(good)
            end = b'\n'
            if bad is None:                                          # "\r\r": the second '\r' ends an empty line
                text = {'first': b'\r' + b'\n'.join(good) + b'\n', 'middle': good[0] + b'\r\r' + good[1] + b'\n', 'last': b'\n'.join(good) + b'\n\r'}[where]
            else:
                lines.insert({'first': 0, 'middle': 2, 'last': 3}[where], bad)
                text = end.join(lines) + end
            yield Case('errors', '%s_%s' % (tag, where), text, NAMES3, GROUP3, 3, 'error')
    # the open line at the end of the file: one token, or whitespace alone, without a break
    yield Case('errors', 'open_line_one_token', b'\n'.join(good) + b'\nctgA+', NAMES3, GROUP3, 3, 'error')
    yield Case('errors', 'open_line_whitespace', b'\n'.join(good) + b'\n \t', NAMES3, GROUP3, 3, 'error')


SIZE_LENGTHS = tuple(c + d for c in (TX_BLOCK, GATHER_TILE) for d in (-1, 0, 1))


def size_case(length, phase, shift):
    """one kept line of `length` bytes behind a prefix line that moves it by `phase` bytes mod 16 — a kept prefix (shift='dst') moves source and
    destination alike, a dropped one (shift='src') the source alone — then a CRLF line of the same length and short lines"""
    rng = np.random.default_rng(7500 + length * 32 + phase * 2 + (shift == 'src'))
    parts = []
    if phase:
        a, b = ('ctgA', 'ctgB') if shift == 'dst' else ('ctgA', 'ctgC')
        parts.append(padded_line(a, b, 16 + phase, rng))
    parts.append(padded_line('ctgA', 'ctgB', length, rng))
    parts.append(clm_line('ctgC', 'ctgD', rng, 1) + b'\r\n')
    parts.append(padded_line('ctgB', 'ctgA', length, rng, b'\r\n'))
    parts.append(clm_line('ctgA', 'ctgE', rng, 3) + b'\n')
    parts.append(clm_line('ctgB', 'ctgA', rng, 3))
    return Case('sizes', 'len_%d_%s_phase_%02d' % (length, shift, phase), b''.join(parts), NAMES3, GROUP3, 3)


def _sizes():
    for length in SIZE_LENGTHS:
        for shift in ('dst', 'src'):
            for phase in range(16):
                yield size_case(length, phase, shift)


def long_line_text(kept, n_bytes=300_000):
    """one line of n_bytes (kept, or dropped), then short lines"""
    rng = np.random.default_rng(7600 + kept)
    a, b = ('ctgA', 'ctgB') if kept else ('ctgA', 'ctgC')
    return padded_line(a, b, n_bytes, rng) + b''.join(clm_line(*p, rng, 2) + b'\n' for p in (('ctgA', 'ctgB'), ('ctgC', 'ctgD'), ('ctgA', 'ctgE'), ('ctgF', 'ctgE')))


def head_bound_text():
    """a first token longer than the head bound"""
    return b'ctgA+ ctgB- 1 5\n' + b'x' * (HEAD_MAX + 100) + b'+ ctgB- 1 5\n'


def file_text(n_bytes=2 << 20, first_line_bytes=None):
    """about n_bytes of CLM lines of 40 bytes to 60 KB, a fifth of them ending in "\\r\\n" or '\\r'; first_line_bytes = c + 1 puts the '\\r' of the first
    line's "\\r\\n" on byte c - 1 and its '\\n' on byte c: the two sides of a chunk seam"""
    rng = np.random.default_rng(7700)
    out, size = [], 0
    if first_line_bytes:
        out.append(padded_line('ctgA', 'ctgB', first_line_bytes, rng, b'\r\n'))
        size = first_line_bytes
    while size < n_bytes:
        a, b = NAMES3[int(rng.integers(6))], NAMES3[int(rng.integers(6))]
        n = int(rng.choice([40, 90, 300, 2000, 60_000], p=[0.3, 0.4, 0.2, 0.08, 0.02]))
        end = (b'\r\n', b'\r')[int(rng.integers(2))] if rng.random() < 0.2 else b'\n'
        out.append(padded_line(a, b, n, rng, end))
        size += n
    return b''.join(out)


def seam_inputs():
    """the arguments of split_clm_file for a small run: (text of the CLM file, group_ctg_dict, ctg_group_dict, subdir)"""
    rng = np.random.default_rng(7800)
    groups = {'group1': ['ctgA', 'ctgB', 'utg1'], 'group2': ['ctgC', 'ctgD'], 'group3_empty': ['ctgE'], 'group10': ['ctgF', 'utg10']}
    group_ctg_dict = {g: [set(c), 1000 * len(c)] for g, c in groups.items()}
    ctg_group_dict = {c: g for g, cs in groups.items() for c in cs}
    pairs = [('ctgA', 'ctgB'), ('ctgC', 'ctgD'), ('ctgA', 'ctgC'), ('ctgF', 'utg10'), ('utg1', 'ctgB'), ('lone', 'ctgA'), ('ctgD', 'ctgC'), ('ctgE', 'ctgF'),
             ('utg10', 'ctgF'), ('ctgB', 'utg1')]
    text = b''.join(clm_line(a, b, rng) + (b'\n', b'\r\n', b'\n', b'\r')[k % 4] for k, (a, b) in enumerate(pairs)) + clm_line('ctgB', 'ctgA', rng)
    return text, group_ctg_dict, ctg_group_dict, 'reassigned_groups'


def read_tree(root):
    """{relative path: ('dir',) | ('link', target) | ('file', bytes)} of everything under root"""
    import os
    out = {}
    for dirpath, dirs, files in os.walk(root):
        for n in dirs + files:
            p = os.path.join(dirpath, n)
            rel = os.path.relpath(p, root)
            out[rel] = ('link', os.readlink(p)) if os.path.islink(p) else ('dir',) if os.path.isdir(p) else ('file', open(p, 'rb').read())
    return out


SECTIONS = (('line_ends', _line_ends), ('tokens', _tokens), ('groups', _groups), ('errors', _errors), ('sizes', _sizes))


@functools.lru_cache(maxsize=None)
def section(name):
    return tuple(dict(SECTIONS)[name]())


def cases(sections=None, kind=None):
    out = [c for name, _ in SECTIONS if sections is None or name in sections for c in section(name)]
    return [c for c in out if kind is None or c.kind == kind]


SMALL_SECTIONS = ('line_ends', 'tokens', 'groups', 'errors')


# ------------------------------------------------------------------ tests/golden/clm_split.npz (make_golden_clm_split.py)
def golden_cases(z):
    """[(name, text, names, group_of_name, n_groups, [bytes per group] | IndexError)]: what the reference's own function did"""
    out, at = [], 0
    for k, name in enumerate(z['case_names']):
        text = z['text'][z['text_off'][k]:z['text_off'][k + 1]].tobytes()
        lo, hi = int(z['name_off'][k]), int(z['name_off'][k + 1])
        G = int(z['n_groups'][k])
        want = IndexError
        if not z['raises'][k]:
            lens = z['out_len'][at:at + G]
            base = int(z['out_len'][:at].sum())
            ends = base + np.cumsum(lens)
            want = [z['out'][e - n:e].tobytes() for e, n in zip(ends.tolist(), lens.tolist())]
            at += G
        out.append((str(name), text, [str(n) for n in z['names'][lo:hi]], [int(g) for g in z['group'][lo:hi]], G, want))
    return out


def golden_tree(z):
    """the tree the reference left for seam_inputs(), as read_tree gives it"""
    ends = np.cumsum(z['seam_payload_len']).tolist()
    tree = {}
    for p, kind, e, n in zip(z['seam_paths'], z['seam_kinds'], ends, z['seam_payload_len'].tolist()):
        data = z['seam_payload'][e - n:e].tobytes()
        tree[str(p)] = ('dir',) if kind == 'dir' else ('link', data.decode()) if kind == 'link' else ('file', data)
    return tree
