"""Cases and a numpy engine for `haphic build` on the device (haphic_amd/scaffolds.py, csrc/hhx_fasta.hip).

NumpyFasta has the interface of haphic_amd._lib.Fasta — the reader (parse_fasta, HapHiC_cluster.py:87-113) restated over Python's own text-mode
lines, the writer (build_final_scaffolds, HapHiC_build.py:153-168) restated as array gathers — so the mirrors run without a GPU and the device has a
second statement to agree with.  tests/golden/build.npz (make_golden_build.py) pins both to the reference's bytes on cases()."""
import io
import os
import types

import numpy as np

SLAB_MIN = 256                 # the smallest "fasta_slab" (include/haphic_hip.h)
_COMP = np.arange(256, dtype=np.uint8)
_COMP[list(b'ATCGNatcgn')] = list(b'TAGCNtagcn')


class NumpyFasta:
    class Unsupported(RuntimeError):
        pass

    def __init__(self, source, keep_letter_case=False):
        if isinstance(source, (str, os.PathLike)):
            with open(source, 'rb') as f:
                source = f.read()
        data = bytes(source)
        if any(b >= 0x80 for b in data):
            raise NumpyFasta.Unsupported('a byte >= 0x80')
        names, seqs = [], []
        for line in io.TextIOWrapper(io.BytesIO(data), encoding='ascii', newline=None):
            if not line.strip():
                continue
            if line.startswith('>'):
                names.append(line.split()[0][1:])
                seqs.append([])
            elif not names:
                raise NumpyFasta.Unsupported('a sequence line in front of the first header')
            else:
                seqs[-1].append(line.strip() if keep_letter_case else line.strip().upper())
        joined = [''.join(s) for s in seqs]
        self._names = names
        self.n_ctg = len(names)
        self.seq_len = np.array([len(s) for s in joined], np.int64)
        self.seq_off = np.concatenate([[0], np.cumsum(self.seq_len)[:-1]]).astype(np.int64) if names else np.zeros(0, np.int64)
        self._seq = np.frombuffer(''.join(joined).encode('ascii'), np.uint8)
        self.n_seq_bytes = self._seq.size

    def names(self):
        return list(self._names)

    def sequences(self):
        return self._seq

    def re_counts(self, sites):
        blob = self._seq.tobytes()
        return np.array([sum(blob[o:o + n].count(s) for s in sites) for o, n in zip(self.seq_off.tolist(), self.seq_len.tolist())], np.int64)

    def emit(self, path, rec_names, piece_off, piece_ctg, piece_rev, Ns, max_width):
        if max_width < 1 or Ns < 0:
            raise NumpyFasta.Unsupported('max_width {} / Ns {}'.format(max_width, Ns))
        out = []
        gap = np.full(Ns, ord('N'), np.uint8)
        for r, name in enumerate(rec_names):
            parts = []
            for k in range(piece_off[r], piece_off[r + 1]):
                if parts:
                    parts.append(gap)
                c = int(piece_ctg[k])
                s = self._seq[self.seq_off[c]:self.seq_off[c] + self.seq_len[c]]
                parts.append(_COMP[s][::-1] if piece_rev[k] else s)
            seq = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
            n_lines = -(-seq.size // max_width)
            body = np.full(seq.size + n_lines, ord('\n'), np.uint8)
            at = np.arange(seq.size, dtype=np.int64)
            body[at + at // max_width] = seq
            out.append(b'>' + name.encode() + b'\n' + body.tobytes())
        data = b''.join(out)
        with open(path, 'wb') as f:
            f.write(data)
        return len(data)

    def close(self):
        pass


# ------------------------------------------------------------------ cases
class Case:
    """fasta: bytes of the draft assembly; tours: [(file name, bytes)]; corrected: lines of corrected_ctgs.txt or None; the arguments of haphic build"""

    def __init__(self, name, fasta, tours, corrected=None, Ns=100, max_width=60, sort_by_input=False, keep_letter_case=False, refused=False):
        self.name, self.fasta, self.tours, self.corrected = name, fasta, tours, corrected
        self.Ns, self.max_width, self.sort_by_input, self.keep_letter_case, self.refused = Ns, max_width, sort_by_input, keep_letter_case, refused

    def __repr__(self):
        return self.name

    def write(self, directory):
        """the input files in `directory` -> the args namespace of HapHiC_build.run (prefix `scaffolds`, relative to the working directory)"""
        fasta = os.path.join(directory, 'asm.fa')
        with open(fasta, 'wb') as f:
            f.write(self.fasta)
        paths = []
        for fname, data in self.tours:
            paths.append(os.path.join(directory, fname))
            with open(paths[-1], 'wb') as f:
                f.write(data)
        corrected = None
        if self.corrected is not None:
            corrected = os.path.join(directory, 'corrected_ctgs.txt')
            with open(corrected, 'w') as f:
                f.write(''.join(x + '\n' for x in self.corrected))
        return types.SimpleNamespace(fasta=fasta, raw_fasta=fasta if corrected is None else os.path.join(directory, 'raw.fa'), alignments='aln.bam', tours=paths,
                                     corrected_ctgs=corrected, Ns=self.Ns, max_width=self.max_width, sort_by_input=self.sort_by_input,
                                     keep_letter_case=self.keep_letter_case, prefix='scaffolds')


OUTPUTS = ('scaffolds.fa', 'scaffolds.agp', 'scaffolds.raw.agp')
ALPHABET = b'ACGTacgtNnRYKMSWryBDHVbd'       # bases, soft-masked bases, IUPAC codes (the complement leaves those alone)


def bases(rng, n, alphabet=ALPHABET):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])


def wrap(seq, width, eol=b'\n'):
    return b''.join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def tour(pieces):
    """one tour file: ALLHiC keeps every iteration, the reference takes the last line that is not blank"""
    return ' '.join(c + o for c, o in pieces).encode() + b'\n'


def _tours_over(names, rng, n_groups=3, leave=2):
    """the contigs but the last `leave` dealt to n_groups tours with random orientations"""
    use = [n for n in names if n][:max(len(names) - leave, 0)]
    return [('group%d_x.tour' % (g + 1), tour([(c, '+-'[int(rng.integers(2))]) for c in use[g::n_groups]])) for g in range(n_groups)]


def _text_cases():
    rng = np.random.default_rng(20240611)
    out = []
    seqs = [bases(rng, n) for n in (130, 61, 0, 60, 17, 200)]
    names = ['c%d' % k for k in range(len(seqs))]
    for tag, eols in (('lf', [b'\n']), ('crlf', [b'\r\n']), ('cr', [b'\r']), ('mixed', [b'\n', b'\r\n', b'\r'])):
        text = b''
        for k, (n, s) in enumerate(zip(names, seqs)):
            e = eols[k % len(eols)]
            text += b'>' + n.encode() + b' some description' + e + b''.join(s[i:i + 60] + eols[(k + i) % len(eols)] for i in range(0, len(s), 60))
        out.append(Case('text/eol_' + tag, text, _tours_over(names, rng)))
    out.append(Case('text/no_final_break', out[0].fasta[:-1], _tours_over(names, rng)))
    out.append(Case('text/no_final_break_cr', out[2].fasta + b'ACGT\r', _tours_over(names, rng)))
    blanks = (b'>first_is_empty\n\n \t \n>a desc\twith\ttabs\n  ACGT acgt\tNN  \n\x0b\x0c\n\x1c\x1d\x1e\x1f \nRYKM\t\n \n\n>mid_empty x\n   \n>b\n >not_a_header\n\tac gt\x0c\n'
              b'>\nACGTN\n>c \x1f d\nacgtn\x1c\n>last_is_empty\n\n')
    out.append(Case('text/blanks', blanks, [('g1_a.tour', tour([('a', '-'), ('b', '+'), ('c', '-')])), ('g2_a.tour', tour([('mid_empty', '-'), ('first_is_empty', '+')]))],
                    Ns=3, max_width=7))
    out.append(Case('text/blanks_keep_case', blanks, [('g1_a.tour', tour([('a', '-'), ('b', '-')]))], Ns=1, max_width=5, keep_letter_case=True))
    out.append(Case('text/space_name', b'> x\nACGT\n>y\nGG\n', [('g_1.tour', tour([('y', '-')]))], max_width=1))
    for w in (1, 15, 16, 17, 60):
        text = b''.join(b'>w%d_%d\n' % (w, k) + wrap(bases(rng, n), w) for k, n in enumerate((3 * w + 1, 2 * w, 33)))
        out.append(Case('text/width_%d' % w, text, _tours_over(['w%d_%d' % (w, k) for k in range(3)], rng, 1, 1), Ns=1, max_width=w))
    for n in (4095, 4096, 4097, 10007):
        text = b'>long\n' + bases(rng, n) + b'\n>after\n' + wrap(bases(rng, 100), 60) + b'>long2\n  ' + bases(rng, n) + b' \r\n'
        out.append(Case('text/line_%d' % n, text, [('g_1.tour', tour([('long2', '-'), ('after', '+'), ('long', '-')]))], Ns=100))
    # a break on the last byte of a 16-byte lane granule / of a 4096-byte block, and a "\r\n" cut by each of those seams
    for seam in (16, 4096):
        for tag, eol, at in (('lf_last', b'\n', seam - 1), ('crlf_split', b'\r\n', seam - 1), ('cr_last', b'\r', seam - 1), ('crlf_first', b'\r\n', seam)):
            head = b'>s\n' if seam == 16 else b'>s\n' + wrap(bases(rng, 3900), 60)
            pad = at - len(head)                             # the line's bytes in front of its break
            text = head + bases(rng, pad) + eol + wrap(bases(rng, 70), 16, eol) + b'>t' + eol + bases(rng, 40) + eol
            assert text[at:at + len(eol)] == eol
            out.append(Case('text/seam%d_%s' % (seam, tag), text, [('g_1.tour', tour([('t', '-'), ('s', '-')]))], Ns=0, max_width=16))
    return out


def _emit_cases():
    rng = np.random.default_rng(77)
    out = []
    for W in (1, 7, 60, 100000):
        w = min(W, 60)
        lens = [0, 1, 2, 15, 16, 17, w - 1, w, w + 1, 2 * w, 33, 33, 5, 5, 5]
        names = ['ctg%d' % k for k in range(len(lens))]
        text = b''.join(b'>' + n.encode() + b'\n' + wrap(bases(rng, m), 60) for n, m in zip(names, lens))
        for Ns in (0, 1, 100):
            tours = [('g1_k.tour', tour([(names[k], '+-'[k % 2]) for k in range(0, 7)])),                     # every length, forward and reversed
                     ('g2_k.tour', tour([(names[k], '-+'[k % 2]) for k in range(7, 10)])),
                     ('empty_k.tour', b'\n  \n'),                                                              # header line only, length -Ns in the sort
                     ('eq1_k.tour', tour([(names[10], '-')])), ('eq2_k.tour', tour([(names[11], '+')]))]      # equal lengths: the stable order decides
            out.append(Case('emit/w%d_ns%d' % (W, Ns), text, tours, Ns=Ns, max_width=W))
        out.append(Case('emit/w%d_by_input' % W, text, tours[::-1], Ns=2, max_width=W, sort_by_input=True))
    # a scaffold whose length is an exact multiple of max_width: 2 * 25 + 10 = 60 = 4 * 15 = 1 * 60
    text = b'>p\n' + bases(rng, 25) + b'\n>q\n' + bases(rng, 25) + b'\n>r\n' + bases(rng, 30) + b'\n'
    for W in (15, 60):
        out.append(Case('emit/exact_multiple_w%d' % W, text, [('g_1.tour', tour([('p', '-'), ('q', '+')]))], Ns=10, max_width=W))
    # the last line of a tour file that is not blank counts; corrected contigs
    names = ['utg1:1-500', 'utg1:501-900', 'utg2', 'utg3:1-77']
    text = b''.join(b'>' + n.encode() + b'\n' + wrap(bases(rng, m, b'ACGTacgtn'), 60) for n, m in zip(names, (500, 400, 321, 77)))
    tours = [('g1_c.tour', tour([('utg2', '+'), ('utg1:1-500', '+')]) + b'\n' + tour([('utg1:501-900', '-'), ('utg2', '-'), ('utg1:1-500', '+')]) + b'  \n\n')]
    out.append(Case('emit/last_tour_line_corrected', text, tours, corrected=['utg1:1-500', 'utg1:501-900', 'utg3:1-77'], Ns=100, max_width=60))
    out.append(Case('emit/keep_case', text, tours, corrected=['utg1:1-500', 'utg1:501-900', 'utg3:1-77 '], Ns=100, max_width=60, keep_letter_case=True))
    # reversed pieces and gaps that begin at every offset 0..15 of an output store (one line: 17 + 100 = 5 mod 16 walks all residues), and slab seams
    # (SLAB_MIN) inside headers, on '\n', inside gaps and inside reversed pieces
    names = ['piece_with_a_long_name_%02d' % k for k in range(40)]
    text = b''.join(b'>' + n.encode() + b'\n' + bases(rng, 17, b'ACGTacgt') + b'\n' for n in names)
    tours = [('walk_1.tour', tour([(n, '-') for n in names[:20]])), ('walk2_1.tour', tour([(n, '-+'[k % 3 == 0]) for k, n in enumerate(names[20:36])]))]
    out.append(Case('emit/offsets_one_line', text, tours, Ns=100, max_width=1 << 40))
    out.append(Case('emit/offsets_w60', text, tours, Ns=100, max_width=60))
    out.append(Case('emit/offsets_w7_ns1', text, tours, Ns=1, max_width=7))
    return out


def _refusal_cases():
    ok = b'>a\nACGT\n>b\nGGCC\n'
    t = [('g_1.tour', tour([('a', '-'), ('b', '+')]))]
    return [Case('refuse/high_byte', '>a café\nACGT\n>b\nGGCC\n'.encode('utf-8'), t, refused=True),
            Case('refuse/sequence_first', b'\nACGT\n' + ok, t, refused=True),
            Case('refuse/duplicate_names', b'>a\nAC\n>b\nGGCC\n>a\nTTTTT\n', t, refused=True),
            Case('refuse/max_width_0', ok, t, max_width=0, refused=True),
            Case('refuse/max_width_negative', ok, t, max_width=-3, refused=True)]


def cases():
    return _text_cases() + _emit_cases() + _refusal_cases()


def genome_case(n_bytes=2 << 20, seed=5):
    """a generated genome of about n_bytes: random lengths, orientations and line widths, most contigs in tours"""
    rng = np.random.default_rng(seed)
    lens, total = [], 0
    while total < n_bytes:
        lens.append(int(rng.integers(1, 60000)))
        total += lens[-1]
    names = ['scf%04d' % k for k in range(len(lens))]
    text = b''.join(b'>' + n.encode() + b' len=%d\n' % m + wrap(bases(rng, m, b'ACGTacgtN'), int(rng.choice([50, 60, 61, 80]))) for n, m in zip(names, lens))
    order = rng.permutation(len(names) - 5)
    cut = np.sort(rng.choice(np.arange(1, order.size), 6, replace=False))
    tours = [('chr%d_g.tour' % (g + 1), tour([(names[k], '+-'[int(rng.integers(2))]) for k in part])) for g, part in enumerate(np.split(order, cut))]
    return Case('genome', text, tours, Ns=100, max_width=60)


# ------------------------------------------------------------------ the golden file
def golden(z):
    """{case name: dict} of tests/golden/build.npz"""
    out = {}
    case_names = z['case_names'].tolist()
    blob, off = z['blob'].tobytes(), z['blob_off'].tolist()
    take = iter(range(len(off) - 1))

    def nxt():
        k = next(take)
        return blob[off[k]:off[k + 1]]
    name_list, name_off = z['ctg_names'].tolist(), z['ctg_name_off'].tolist()
    ints, int_off = z['ints'], z['int_off'].tolist()
    q = 0
    for k, cname in enumerate(case_names):
        g = {'raises': str(z['raises'][k]), 'fa_dict': {}}
        for keep in (False, True):
            if z['fa_ok'][k]:
                names = name_list[name_off[q]:name_off[q + 1]]
                nums = ints[int_off[q]:int_off[q + 1]].reshape(2, -1)
                g['fa_dict'][keep] = (names, nums[0], nums[1], nxt())        # names, lengths, RE sites + 1, the sequences back to back
                q += 1
        if not g['raises']:
            g['files'] = {f: nxt() for f in OUTPUTS}
        out[cname] = g
    return out


def parse_tours(tour_files, fa_dict):
    """parse_tours :29-57 restated (the tests run where the reference is absent): group = file name without extension and its last `_` field"""
    from collections import OrderedDict
    tour_dict, output_ctgs = OrderedDict(), set()
    for path in tour_files:
        group = os.path.splitext(os.path.basename(path))[0].rsplit('_', 1)[0]
        last = ''
        with open(path) as f:
            for line in f:
                if line.strip():
                    last = line.strip()
        tour_dict[group] = []
        for tok in last.split():
            assert tok[:-1] in fa_dict and tok[:-1] not in output_ctgs
            output_ctgs.add(tok[:-1])
            tour_dict[group].append((tok[:-1], tok[-1]))
    return tour_dict, output_ctgs


def run_mirrors(case, directory, engine, parse_fasta, build_final_scaffolds, source='path'):
    """run() :272-278 with the two mirrors and `engine` in a fresh directory -> ({file: bytes}, the table parse_fasta returned)"""
    os.makedirs(directory, exist_ok=True)
    args = case.write(directory)
    work = os.path.join(directory, 'run')
    os.mkdir(work)
    fa_dict = parse_fasta(args.fasta if source == 'path' else case.fasta, keep_letter_case=case.keep_letter_case, _engine=engine)
    tour_dict, output_ctgs = parse_tours(args.tours, fa_dict)
    corrected = set(x.rstrip() for x in (case.corrected or []) if x.strip())
    run_in(work, lambda: build_final_scaffolds(tour_dict, fa_dict, output_ctgs, corrected, args))
    return read_outputs(work), fa_dict


NO_CORRECTED = '<none>'


def golden_inputs(z):
    """the cases as the fixture recorded them: what cases() must still generate"""
    blob, off = z['in_blob'].tobytes(), z['in_off'].tolist()
    tour_names, tour_off = z['tour_names'].tolist(), z['tour_off'].tolist()
    out, q = [], 0
    for k, cname in enumerate(z['case_names'].tolist()):
        fasta = blob[off[q]:off[q + 1]]
        q += 1
        tours = []
        for f in tour_names[tour_off[k]:tour_off[k + 1]]:
            tours.append((f, blob[off[q]:off[q + 1]]))
            q += 1
        corrected = str(z['corrected'][k])
        Ns, width, by_input, keep = z['args'][k].tolist()
        out.append(Case(cname, fasta, tours, None if corrected == NO_CORRECTED else corrected.split('\n'), Ns, width, bool(by_input), bool(keep)))
    return out


def run_in(directory, fn):
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        return fn()
    finally:
        os.chdir(cwd)


def read_outputs(directory):
    return {f: open(os.path.join(directory, f), 'rb').read() for f in OUTPUTS}
