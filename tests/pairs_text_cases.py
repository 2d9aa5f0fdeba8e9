"""A generated corpus for the .pairs tokeniser (haphic_amd/csrc/hhx_text.hip), and a host mirror of which reader and which BED
path every block of 128 lines takes there.  Every case is (names, text, expectation); the expectation is what
oracle.parse_pairs_text — Python's own `for line in f` / line.split() / int() — returns or raises on the same bytes.  The
corpus stays inside the domain the kernel's header comment states (valid UTF-8, none of the non-ASCII characters
str.split() takes for whitespace, ASCII digits in the integer columns) and asserts so when a case is built.  The mirror is
written from the constants and formulas of the .hip file; the GPU tests compare it with the device's own counters
("text_blocks_*", "bed_blocks_*"), so a capacity that moves under a test makes the test fail instead of silently turning
its boundary cases into ordinary ones.  Seeded, no GPU and no reference checkout needed."""
import functools

import numpy as np

from oracle import oracle as orc

# constants of hhx_text.hip
TX_BLOCK = 4096                 # bytes per workgroup step of the line-break passes
LN_BLOCK = 128                  # lines per workgroup of the parse / BED passes
IN_CAP = 24 * 1024              # LDS bytes for the text of those lines
OUT_CAP = 36 * 1024             # LDS bytes for their BED records

SEPS = b'\t\x0b\x0c\x1c\x1d\x1e\x1f '                                 # in-line whitespace; '\r' and '\n' only end lines
NOT_WS = frozenset('\x85\xa0\u1680\u2028\u2029\u202f\u205f\u3000') | frozenset(chr(c) for c in range(0x2000, 0x200b))
COUNTERS = ('text_blocks_staged', 'text_blocks_direct', 'bed_blocks_lds', 'bed_blocks_direct')

_SEPS = np.frombuffer(SEPS, np.uint8)
_LOWER = np.frombuffer(b'abcdefghijklmnopqrstuvwxyz0123456789_.-|:', np.uint8)
_FIRST = np.frombuffer(b'uvwxyz', np.uint8)

# FASTA names of the small cases: three of every length 1..17, all starting with a capital (generated tokens never do)
BASE_NAMES = [(chr(ord('A') + j) + 'tg%02d_abcdefghijk' % L)[:L] for L in range(1, 18) for j in range(3)]


# ------------------------------------------------------------------ lines, as universal newlines cut them
def line_bounds(text):
    """[n_lines + 1] byte offsets: line k is text[b[k]:b[k + 1]], terminator included ('\\n', '\\r\\n', a lone '\\r')"""
    b = np.frombuffer(bytes(text), np.uint8)
    if b.size == 0:
        return np.zeros(1, np.int64)
    nxt = np.append(b[1:], np.uint8(0))
    cut = np.flatnonzero((b == 10) | ((b == 13) & (nxt != 10))).astype(np.int64) + 1
    if cut.size == 0 or cut[-1] != b.size:
        cut = np.append(cut, b.size)
    return np.concatenate([np.zeros(1, np.int64), cut])


def bed_lengths(text):
    """bytes of the two alignments.bed records of every line (0 for a skipped one), :1557"""
    text = bytes(text)
    b = line_bounds(text)
    out = np.zeros(len(b) - 1, np.int64)
    for k in range(len(out)):
        line = text[b[k]:b[k + 1]].decode('utf-8')
        if not line.strip() or line.startswith('#'):
            continue
        c = line.split()
        out[k] = (2 * len(c[0].encode()) + len(c[1].encode()) + len(c[3].encode()) + 2 * len(str(int(c[2]) - 1))
                  + 2 * len(str(int(c[4]) - 1)) + 24)
    return out


def plan(text, aligned=True, want_bed=True):
    """how many blocks of LN_BLOCK lines take the LDS-staged parser / the HBM parser (k_parse_lines<true / false>: `fits`) and,
    of the blocks that write BED bytes at all, the LDS output path / the direct one (k_bed_write: `out_staged`).
    aligned=False: a device buffer that is not 16-byte aligned — no block stages.  'bed_direct_text_staged' (no device
    counter) counts the blocks of k_bed_write with `staged && !out_staged`."""
    b = line_bounds(text)
    nl = len(b) - 1
    res = dict.fromkeys(COUNTERS + ('bed_direct_text_staged',), 0)
    if len(text) == 0:
        return res
    off = np.concatenate([[0], np.cumsum(bed_lengths(text))]) if want_bed else None
    for k0 in range(0, nl, LN_BLOCK):
        k1 = min(k0 + LN_BLOCK, nl)
        a0, e0 = int(b[k0]), int(b[k1])
        fits = aligned and e0 - (a0 & ~15) <= IN_CAP
        res['text_blocks_staged' if fits else 'text_blocks_direct'] += 1
        if want_bed and off[k1] > off[k0]:
            out_staged = int(off[k1]) - (int(off[k0]) & ~15) <= OUT_CAP
            res['bed_blocks_lds' if out_staged else 'bed_blocks_direct'] += 1
            res['bed_direct_text_staged'] += int(fits and not out_staged)
    return res


def in_domain(text):
    """the domain of the kernel's header comment"""
    s = bytes(text).decode('utf-8')                                   # valid UTF-8, or UnicodeDecodeError
    if NOT_WS.intersection(s):
        return False
    if s.isascii():
        return True
    b = line_bounds(text)
    for k in range(len(b) - 1):
        line = bytes(text[b[k]:b[k + 1]])
        if line.isascii():
            continue
        line = line.decode('utf-8')
        if not line.strip() or line.startswith('#'):
            continue
        c = line.split()
        if not all(x.isascii() for x in c[2:5:2]):
            return False
    return True


class Case:
    """kind 'ok': the device equals the oracle.  'error': the oracle raises, bad_line is the 1-based first offending line.
    'range': a stated limit of the device path — a position outside int32 is refused (ValueError) in narrow mode, in
    wide mode only beyond 2^40 (refused_wide); the oracle itself accepts the line."""

    def __init__(self, section, name, names, text, kind='ok', bad_line=None, refused_wide=False):
        self.section, self.name, self.names, self.text = section, name, list(names), bytes(text)
        self.kind, self.bad_line, self.refused_wide = kind, bad_line, refused_wide
        assert kind in ('ok', 'error', 'range') and (kind == 'ok') == (bad_line is None)
        assert in_domain(self.text), name
        self._want = {}

    def expected(self, wide=False):
        """('ok', (id1, pos1, id2, pos2, bed)) or ('raises', exception type): oracle.parse_pairs_text on the bytes"""
        if wide not in self._want:
            try:
                self._want[wide] = ('ok', orc.parse_pairs_text(self.text, self.names, wide=wide))
            except (IndexError, ValueError) as e:
                self._want[wide] = ('raises', type(e))
        return self._want[wide]

    def __repr__(self):
        return 'Case(%s/%s, %d bytes)' % (self.section, self.name, len(self.text))


def first_bad_line(text, names):
    """1-based number of the first line on which the oracle raises, line by line (None: none does)"""
    text = bytes(text)
    b = line_bounds(text)
    for k in range(len(b) - 1):
        try:
            orc.parse_pairs_text(text[b[k]:b[k + 1]], names)
        except (IndexError, ValueError):
            return k + 1
    return None


# ------------------------------------------------------------------ building blocks
def _ws(rng, n):
    return bytes(rng.choice(_SEPS, int(n)))


def _word(rng, n):
    """a token that is no FASTA name (lower-case first byte) and starts no comment"""
    n = int(n)
    return bytes(rng.choice(_FIRST, 1)) + bytes(rng.choice(_LOWER, n - 1))


def _int(rng, n=None):
    """a position literal; n: of exactly n bytes (zero padded)"""
    v = int(rng.integers(1, 2**31))
    if n is None:
        return b'%d' % v
    return (b'%d' % (v % 10**min(int(n), 10))).rjust(int(n), b'0')


def _name(rng, names, n=None, p_known=0.7):
    if rng.random() < p_known:
        pool = [x for x in names if n is None or len(x.encode()) == n]
        if pool:
            return pool[int(rng.integers(len(pool)))].encode()
    return _word(rng, n if n is not None else rng.integers(1, 18))


def _plain(rng, names, read=None):
    """an ordinary line body (no terminator), at most 48 bytes unless `read` is given"""
    read = _word(rng, rng.integers(2, 9)) if read is None else read
    return b'\t'.join([read, _name(rng, names), _int(rng), _name(rng, names), _int(rng), b'+', b'-'][:5 + int(rng.integers(0, 3))])


def _padded(rng, names, n, end=b'\n'):
    """a line of exactly n bytes, terminator included: the read name takes the slack"""
    tail = b'\t'.join([b'', _name(rng, names, 1, 1.0), _int(rng, 1), _name(rng, names, 1, 1.0), _int(rng, 1)]) + end
    assert n > len(tail), n
    return _word(rng, n - len(tail)) + tail


# ------------------------------------------------------------------ sections
def _alignment():
    u8 = ['Ņ', 'Š', 'ŜŝŞş', 'ŉŊŋŌō', 'rŅŠ', 'ŜxŊyō', 'ŅŠŜŉ']      # continuation bytes 0x85, 0xA0, 0x9C-0x9F, 0x89-0x8D
    ends = (b'\n', b'\r\n')
    for shift in range(16):
        rng = np.random.default_rng(1000 + shift)
        out = [b'', b'\n'][shift] if shift < 2 else b'#' + b'x' * (shift - 2) + b'\n'
        parts = [out]
        for c in range(5):
            for L in range(1, 18):
                for r in range(1, 10):
                    lens = rng.integers(1, 12, 5)
                    lens[c] = L
                    runs = rng.integers(1, 4, 6)
                    runs[c] = r
                    cols = [_word(rng, lens[0]), _name(rng, BASE_NAMES, lens[1]), _int(rng, lens[2]), _name(rng, BASE_NAMES, lens[3]), _int(rng, lens[4])]
                    line = _ws(rng, runs[0]) if c == 0 or rng.random() < 0.3 else b''
                    for q in range(5):
                        line += (_ws(rng, runs[q]) if q else b'') + cols[q]
                    for _ in range(int(rng.integers(0, 7)) if rng.random() < 0.3 else 0):
                        line += _ws(rng, rng.integers(1, 4)) + _word(rng, rng.integers(1, 9))
                    if rng.random() < 0.3:
                        line += _ws(rng, runs[5])
                    parts.append(line + ends[int(rng.integers(2))])
        for n in range(18):                                          # whitespace-only lines, each in front of a short data line
            parts += [_ws(rng, n) + b'\n', b'r\tA\t5\tB\t7\n', _ws(rng, n) + b'\r\n', b'q ' + BASE_NAMES[7].encode() + b' 12 Ct 9 x\n']
        for n in range(7):                                           # extra columns, trailing whitespace
            parts.append(b'rd\tAt\t77\tBt\t88' + b''.join(b'\t' + _word(rng, 3) for _ in range(n)) + _ws(rng, n) + b'\n')
        parts += [b'#r\tA\t5\tB\t7\n', b' #r\tA\t5\tB\t7\n', b'\t#\tA\t5\tB\t7\n', b'#\n', b'# \n', b'r#\tA\t5\tB\t7\n']
        for k, w in enumerate(u8):                                   # multi-byte UTF-8 in read names and in contig names that are no FASTA names
            w, v = w.encode(), u8[(k + 3) % len(u8)].encode()
            parts += [w + b'\tA\t5\tB\t7\n', b'r\t' + w + b'\t5\t' + v + b'\t7\n', _ws(rng, k) + w + v + _ws(rng, 1 + k) + v + b' 15 ' + w + b'x\x1f16\n']
        yield Case('alignment', 'shift%02d' % shift, BASE_NAMES, b''.join(parts))


def _line_ends():
    styles = {'lf': [b'\n'], 'crlf': [b'\r\n'], 'cr': [b'\r'], 'crcrlf': [b'\r\r\n'], 'lfcr': [b'\n\r'], 'mixed': [b'\n', b'\r\n', b'\r', b'\r\r\n', b'\n\r', b'\n\n', b'\r\r']}
    for si, (style, ends) in enumerate(styles.items()):
        rng = np.random.default_rng(2000 + si)
        bodies = [_plain(rng, BASE_NAMES) if rng.random() < 0.9 else b'#' + _word(rng, 5) for _ in range(200)]
        text = b''.join(x + ends[int(rng.integers(len(ends)))] for x in bodies)
        yield Case('line_ends', style, BASE_NAMES, text)
        yield Case('line_ends', style + '_no_final', BASE_NAMES, text + _plain(rng, BASE_NAMES))
        yield Case('line_ends', style + '_last_cr', BASE_NAMES, text + _plain(rng, BASE_NAMES) + b'\r')
    for period, n_lines in ((16, 96), (4096, 12)):                   # '\r' in the last byte of a 16-byte lane / of a 4096-byte block
        rng = np.random.default_rng(2100 + period)
        text = b''
        for k in range(n_lines):
            body = _plain(rng, BASE_NAMES)
            pad = (period - 1 - (len(text) + len(body))) % period
            body = _word(rng, pad) + body if pad else body
            assert (len(text) + len(body)) % period == period - 1
            text += body + (b'\r\n', b'\r', b'\r\r\n', b'\r\n\r')[k % 4]
        yield Case('line_ends', 'cr_at_%dk_minus_1' % period, BASE_NAMES, text)
    rng = np.random.default_rng(2200)
    yield Case('line_ends', 'size_1_lf', BASE_NAMES, b'\n')
    yield Case('line_ends', 'size_1_cr', BASE_NAMES, b'\r')
    yield Case('line_ends', 'size_1_hash', BASE_NAMES, b'#')
    for n in (15, 16, 17, 4095, 4096, 4097, 8192):
        for tag, end in (('none', b''), ('lf', b'\n'), ('cr', b'\r'), ('crlf', b'\r\n')):
            text = b''
            while n - len(text) - len(end) > 100:
                line = _plain(rng, BASE_NAMES) + (b'\n', b'\r\n', b'\r')[int(rng.integers(3))]
                assert len(line) <= 80
                text += line
            text += _padded(rng, BASE_NAMES, n - len(text), end)
            assert len(text) == n
            yield Case('line_ends', 'size_%d_%s' % (n, tag), BASE_NAMES, text)


INT_OK = ['2147483648', '-2147483647', '+0', '-0', '0', '0_0', '+1', '-1', '007', '+007', '-007', '1_0', '+1_2_3', '-1_2_3', '2_147_483_648',
          '00000000000000000000012', '0_0_0_0_1']
INT_BAD = ['1__0', '_1', '1_', '+', '-', '+_1', '-_1', '_', '+_', '1_000_', '--1', '+-1', '1+', '1-', '0x10', '1.0', '1e3', '12a', 'a12', '1__', '__1']


def _integers():
    rng = np.random.default_rng(3000)
    ok = list(INT_OK) + ['0' * k + '1234' for k in range(1, 13)]
    digits = '123456'
    bad = list(INT_BAD)
    for at in range(len(digits) + 1):                                 # an underscore at every position, a doubled one at every interior position
        (ok if 0 < at < len(digits) else bad).append(digits[:at] + '_' + digits[at:])
        if 0 < at < len(digits):
            bad.append(digits[:at] + '__' + digits[at:])
    lines = []
    for k, lit in enumerate(ok):
        lines += [b'r%d\tA\t%s\tB\t%d\n' % (k, lit.encode(), k + 1), b'r%d %s %d\x1c%s\t%s\r\n' % (k, BASE_NAMES[4].encode(), k + 1, BASE_NAMES[9].encode(), lit.encode())]
    text = b''.join(lines)
    yield Case('integers', 'accepted', BASE_NAMES, text)
    filler = [_plain(rng, BASE_NAMES) + b'\n' for _ in range(40)]
    for k, lit in enumerate(bad):
        for col in (2, 4):
            cols = [b'r', b'A', b'5', b'B', b'7']
            cols[col] = lit.encode()
            at = int(rng.integers(len(filler) + 1))
            yield Case('integers', 'malformed_%s_col%d' % (lit, col), BASE_NAMES, b''.join(filler[:at] + [b'\t'.join(cols) + b'\n'] + filler[at:]), 'error', at + 1)
    # the device path's own limits: pos = literal - 1 must fit int32 (narrow) / the literal must not exceed 2^40 (wide)
    for lit, wide_refuses in (('2147483649', False), ('-2147483648', False), ('4294967297', False), ('1099511627776', False), ('-1099511627776', False),
                              ('1099511627777', True), ('-1099511627777', True), ('9999999999999', True), ('10995116277760', True), ('123456789012345678', True)):
        for col in (2, 4):
            cols = [b'r', b'A', b'5', b'B', b'7']
            cols[col] = lit.encode()
            at = int(rng.integers(len(filler) + 1))
            yield Case('integers', 'window_%s_col%d' % (lit, col), BASE_NAMES, b''.join(filler[:at] + [b'\t'.join(cols) + b'\n'] + filler[at:]), 'range', at + 1,
                       refused_wide=wide_refuses)


def _queries(rng, names, queries, extra=0):
    """lines that ask for every query once in column 2 and once in column 4"""
    qs = list(queries)
    order = rng.permutation(len(qs))
    lines = [b'r%d\t%s\t%d\t%s\t%d\n' % (k, qs[k], k + 1, qs[int(order[k])], k + 2) for k in range(len(qs))]
    lines += [_plain(rng, names) + b'\n' for _ in range(extra)]
    return b''.join(lines)


def _names():
    rng = np.random.default_rng(4000)
    some = [x.encode() for x in BASE_NAMES]
    yield Case('names', 'table_of_0', [], _queries(rng, BASE_NAMES, some, 50))
    yield Case('names', 'table_of_1', ['Atg05'], _queries(rng, ['Atg05'], [b'Atg05', b'Atg0', b'Atg05x', b'Atg06', b'A', b'atg05'], 50))
    # lengths 1..80, two names of every length; families that agree in their first 64 / 72 bytes
    table = []
    for L in range(1, 81):
        for j in range(2):
            table.append((chr(ord('A') + j) + 'n%02d' % L + 'abcdefgh' * 10)[:L])
    p64, p72 = 'P' + 'q' * 63, 'S' + 't' * 71
    fam = [p64 + s for s in ('a', 'b', 'ab', 'ba', 'abcdefgh', 'abcdefgi', 'abcdefghi', 'abcdefghj', 'abcdefghijklmnop', 'abcdefghijklmnoq')]
    fam += [p72 + s for s in ('a', 'b', 'ab', 'abcdefgh', 'abcdefgi', 'abcdefghi')] + [p64, p72, p64[:63], p72[:71]]
    table += fam
    assert len(set(table)) == len(table)
    qs = []
    for nm in table:
        b = nm.encode()
        qs += [b, b + b'x', b[:-1] + (b'y' if b[-1:] != b'y' else b'z'), b[:-1] + (b'b' if b[-1:] == b'a' else b'a')] + ([b[:-1]] if len(b) > 1 else [])
    want = {n: i for i, n in enumerate(table)}
    hits = sum(q.decode() in want for q in qs)
    assert len(table) < hits < len(qs) // 2                          # the exact names, and some of the neighbours resolve to a sibling
    yield Case('names', 'lengths_1_to_80_and_shared_prefixes', table, _queries(rng, table, qs))
    # a table of ~50 000 names (the probe sequence of the open-addressing table), few lines
    big = ['scf%d_%s' % (k, 'x' * (k % 23)) for k in range(50_000)] + ['contig_with_a_name_well_beyond_sixty_four_bytes_%s_%06d_%s' % ('y' * (k % 9), k, 'tail' * (k % 5)) for k in range(300)]
    pick = rng.integers(0, len(big), 1500)
    qs = [big[int(k)].encode() for k in pick] + [big[int(k)].encode() + b'0' for k in pick[:200]] + [big[int(k)].encode()[:-1] for k in pick[:200]]
    yield Case('names', 'table_of_50k', big, _queries(rng, big, qs))


def _block(rng, n_bytes, n_lines=LN_BLOCK):
    """n_lines lines of n_bytes bytes altogether"""
    each = n_bytes // n_lines
    return b''.join(_padded(rng, BASE_NAMES, each + (n_bytes - each * n_lines if k == n_lines - 1 else 0)) for k in range(n_lines))


def _bed_block(rng, bed_bytes, n_lines=LN_BLOCK):
    """n_lines lines 'read A 5 B 7' whose BED records take bed_bytes bytes altogether (2 * |read| + 30 a line; an odd byte through the contig name)"""
    each = (bed_bytes // n_lines - 30) // 2
    lines = [_word(rng, each) + b'\tA\t5\tB\t7\n' for _ in range(n_lines - 1)]
    rest = bed_bytes - (n_lines - 1) * (2 * each + 30) - 30
    lines.append(_word(rng, rest // 2) + b'\t' + (b'A' if rest % 2 == 0 else b'uu') + b'\t5\tB\t7\n')
    return b''.join(lines)


IN_CAP_DELTAS = (-16, -15, -1, 0, 1, 15, 16, -8, 8)
OUT_CAP_DELTAS = (-1, 15, 1, 0, -16, 16, -15, 8, -8)


def _blocks():
    rng = np.random.default_rng(5000)
    text = b''
    for d in IN_CAP_DELTAS:                                          # span e0 - (a0 & ~15) = IN_CAP + d
        text += _block(rng, IN_CAP + d - (len(text) & 15))
    yield Case('blocks', 'text_span_around_in_cap', BASE_NAMES, text + _block(rng, 700, 7))
    text, bed = b'', 0
    for d in OUT_CAP_DELTAS:                                         # span b1 - (b0 & ~15) = OUT_CAP + d, from staged text
        text += _bed_block(rng, OUT_CAP + d - (bed & 15))
        bed += OUT_CAP + d - (bed & 15)
    yield Case('blocks', 'bed_span_around_out_cap', BASE_NAMES, text)
    lines = [_padded(rng, BASE_NAMES, int(rng.integers(160, 171))) for _ in range(5 * LN_BLOCK)]      # read names of 150-160 bytes: the text stages, the BED does not
    lines += [_plain(rng, BASE_NAMES, _word(rng, rng.integers(150, 401))) + b'\r\n' for _ in range(4 * LN_BLOCK + 60)]
    yield Case('blocks', 'long_read_names', BASE_NAMES, b''.join(lines))
    for col in (0, 1, 3):                                            # one 30 kB token among short lines
        lines = [_plain(rng, BASE_NAMES) + b'\n' for _ in range(300)]
        cols = [b'big', b'A', b'5', b'B', b'7']
        cols[col] = _word(rng, 30_000)
        lines[200] = b'\t'.join(cols) + b'\n'
        yield Case('blocks', 'one_30k_token_col%d' % col, BASE_NAMES, b''.join(lines))
    for tail in (1, 127):
        yield Case('blocks', 'last_block_of_%d' % tail, BASE_NAMES, b''.join(_plain(rng, BASE_NAMES) + b'\n' for _ in range(LN_BLOCK + tail)))


SHAPES = {'1col': b'r1', '2col': b'r1\tA', '3col_int': b'r1\tA\t5', '3col_bad': b'r1\tA\t5x', '4col_int': b'r1 A\x1c5\tB', '4col_bad': b'r1\tA\t5x\tB',
          '5col_third': b'r1\tA\t5x\tB\t7', '5col_fifth': b' r1\tA\t5\tB\t7_', '5col_both': b'r1\tA\t_5\tB\t7_\textra', '4col_window': b'r1\tA\t99999999999\tB',
          '5col_window_fifth_bad': b'r1\tA\t99999999999\tB\t7x', '3col_window': b'r1\tA\t-2147483648'}
SHAPE_PAIRS = (('1col', '5col_third'), ('4col_int', '5col_fifth'), ('3col_bad', '2col'), ('4col_window', '5col_both'))


def _background(rng, unstaged):
    """300 valid lines = blocks 0, 1, 2; unstaged: line 130 carries a 30 kB read name, so block 1 goes to the HBM reader"""
    lines = [_plain(rng, BASE_NAMES) + (b'\n', b'\r\n')[int(rng.integers(2))] for _ in range(300)]
    if unstaged:
        lines[130] = _plain(rng, BASE_NAMES, _word(rng, 30_000)) + b'\n'
    return lines


def _errors():
    rng = np.random.default_rng(6000)
    blocks = {0: (0, 128), 1: (131, 256), 2: (256, 300)}
    for unstaged in (False, True):
        where = 'unstaged' if unstaged else 'staged'
        for tag, bad in SHAPES.items():
            lines = _background(rng, unstaged)
            at = int(rng.integers(*blocks[1]))
            lines[at] = bad + b'\n'
            yield Case('errors', '%s_%s' % (tag, where), BASE_NAMES, b''.join(lines), 'error', at + 1)
        for a, b in SHAPE_PAIRS:
            for first, second in ((a, b), (b, a)):
                for b1, b2 in ((0, 1), (1, 2), (1, 1), (0, 2)):
                    lines = _background(rng, unstaged)
                    i, j = sorted((int(rng.integers(*blocks[b1])), int(rng.integers(*blocks[b2]))))
                    j += int(i == j)
                    lines[i], lines[j] = SHAPES[first] + b'\n', SHAPES[second] + b'\r\n'
                    yield Case('errors', '%s_then_%s_%s_blocks_%d_%d' % (first, second, where, b1, b2), BASE_NAMES, b''.join(lines), 'error', i + 1)
    # a position outside the window behind / in front of a malformed line: whichever comes first in the file is reported
    lines = _background(rng, True)
    lines[140], lines[20] = b'r1\tA\t5\tB\n', b'r1\tA\t2147483649\tB\t7\n'
    yield Case('errors', 'window_line_21_then_4col_line_141', BASE_NAMES, b''.join(lines), 'range', 21)


SECTIONS = (('alignment', _alignment), ('line_ends', _line_ends), ('integers', _integers), ('names', _names), ('blocks', _blocks), ('errors', _errors))


@functools.lru_cache(maxsize=None)
def section(name):
    return tuple(dict(SECTIONS)[name]())


def cases(kind=None):
    out = [c for name, _ in SECTIONS for c in section(name)]
    return [c for c in out if kind is None or c.kind == kind]
