"""Cases and host stand-ins for the front of `haphic cluster` on the device (haphic_amd/assembly.py, csrc/hhx_gfa.hip, the view paths of
cluster.stat_fragments and correct.update_bookkeeping).

  * HostGfa: the interface of _lib.Gfa restated over Python's own text-mode lines, str.split and a regular expression;
  * fasta_engine(): a NumpyFasta (tests/build_cases.py) with re_counts_device / fetch / sequences and a record of every call, which keeps no
    reference to its instances (the tests watch them go);
  * gfa_jobs(): the parse_gfa calls — files and fa_dict — with the step each one straddles named beside it;
  * genome() and fragment_combos(): the small assembly and the cross product of stat_fragments arguments;
  * golden(): the reader of tests/golden/assembly.npz (make_golden_assembly.py wrote it from the reference's own functions).

Steps of csrc/hhx_gfa.hip the GFA inputs straddle: LANE = 16 bytes (one lane's load), WAVE_STEP = 1024 bytes (one wave step inside a block),
TX_BLOCK = 4096 bytes (the unit of the scanned line-break and TAB counts; a TAB is found by a binary search over those counts, so a sequence over
many blocks costs more probes of the search, not a longer walk: LONG_BLOCKS = 70 blocks is beyond the 64 entries one wave could hold)."""
import hashlib
import io
import itertools
import json
import os
import re

import numpy as np

from tests import build_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'assembly.npz')
LANE, WAVE_STEP, TX_BLOCK, LONG_BLOCKS = 16, 1024, 4096, 70
NAME_MAX, DIGITS_MAX = 255, 18


# ------------------------------------------------------------------ stand-ins
class HostGfa:
    """_lib.Gfa on the host: what include/haphic_hip.h says of hhx_gfa_open, in Python's own terms"""

    class Unsupported(RuntimeError):
        pass

    opened = 0
    _INT = re.compile(r'[0-9]{1,%d}\Z' % DIGITS_MAX)

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            with open(source, 'rb') as f:
                source = f.read()
        data = bytes(source)
        if any(b >= 0x80 for b in data):
            raise HostGfa.Unsupported('a byte >= 0x80')
        names, lengths, depths = [], [], []
        for k, line in enumerate(io.TextIOWrapper(io.BytesIO(data), encoding='ascii', newline=None), 1):
            if not line.startswith('S\t'):
                continue
            cols = line.split('\t')
            if len(cols) < 5:
                raise HostGfa.Unsupported('line %d: fewer than five fields' % k)
            if len(cols[1]) > NAME_MAX:
                raise HostGfa.Unsupported('line %d: a name longer than %d bytes' % (k, NAME_MAX))
            if len(cols) == 5 and cols[4].endswith('\n'):            # the line break behind the last field
                cols[4] = cols[4][:-1]
            tails = [cols[j].split(':')[-1] for j in (3, 4)]
            if not all(HostGfa._INT.match(t) for t in tails):
                raise HostGfa.Unsupported('line %d: an integer that is not 1..%d digits' % (k, DIGITS_MAX))
            names.append(cols[1])
            lengths.append(int(tails[0]))
            depths.append(int(tails[1]))
        HostGfa.opened += 1
        self._names, self.n_rec = names, len(names)
        self.lengths, self.depths = np.array(lengths, np.int64), np.array(depths, np.int64)

    def names(self):
        return list(self._names)

    def close(self):
        pass


def fasta_engine():
    """a fresh engine class: Engine.fetched lists (off, len) of every fetch, Engine.bulk the sequences() calls, Engine.count_calls the segments of
    every re_counts_device call, Engine.live the number of instances nobody has let go of"""
    class Engine(bc.NumpyFasta):
        class Unsupported(RuntimeError):
            pass

        fetched, bulk, count_calls = [], [], []
        live = 0

        def __init__(self, source, keep_letter_case=False):
            try:
                bc.NumpyFasta.__init__(self, source, keep_letter_case)
            except bc.NumpyFasta.Unsupported as e:
                raise Engine.Unsupported(str(e))
            Engine.live += 1

        def __del__(self):
            Engine.live -= 1

        def re_counts_device(self, sites, seg_off=None, seg_len=None):
            off = self.seq_off if seg_off is None else np.asarray(seg_off, np.int64)
            ln = self.seq_len if seg_len is None else np.asarray(seg_len, np.int64)
            assert off.shape == ln.shape and ((off >= 0) & (ln >= 0) & (off + ln <= self._seq.size)).all()
            Engine.count_calls.append(len(off))
            blob = self._seq.tobytes()
            return np.array([sum(blob[o:o + n].count(s) for s in sites) for o, n in zip(off.tolist(), ln.tolist())], np.int64)

        def fetch(self, off, len):
            assert 0 <= off and 0 <= len and off + len <= self._seq.size
            Engine.fetched.append((off, len))
            return self._seq[off:off + len].tobytes()

        def sequences(self):
            Engine.bulk.append(self._seq.size)
            return self._seq

    return Engine


# ------------------------------------------------------------------ GFA inputs
def rec(name, length, depth, seq='*', eol='\n', ln='LN:i:', rd='rd:i:', extra=''):
    return ('S\t%s\t%s\t%s%s\t%s%s%s%s' % (name, seq, ln, length, rd, depth, extra, eol)).encode('latin-1')


A_LINE = b'A\tutg1\t0\t+\tread1\t0\t15000\tid:i:1\tHG:A:a\n'
L_LINE = b'L\tutg1\t+\tutg2\t-\t0M\tL1:i:3\n'
H_LINE = b'H\tVN:Z:1.0\n'


def at_seam(record, inner, at):
    """filler lines, then `record` placed so that its byte `inner` is byte `at` of the file"""
    pad = at - inner
    assert pad >= 2
    return b'#' + b'x' * (pad - 2) + b'\n' + record


class Job:
    """one parse_gfa call: files (bytes each) and fa_dict as {name: length}; straddles: the step the case is about"""

    def __init__(self, name, files, fa=None, straddles=''):
        self.name, self.files, self.straddles = name, list(files), straddles
        self.fa = dict(fa or {})

    def __repr__(self):
        return self.name

    def write(self, directory):
        paths = []
        for k, data in enumerate(self.files):
            paths.append('f%d.gfa' % k)
            with open(os.path.join(directory, paths[-1]), 'wb') as f:
                f.write(data)
        return paths

    def fa_dict(self):
        return {n: [None, l, 1] for n, l in self.fa.items()}

    def digest(self):
        h = hashlib.sha256()
        for data in self.files:
            h.update(b'%d:' % len(data) + data)
        h.update(json.dumps(list(self.fa.items())).encode())
        return h.hexdigest()


def _seq(rng, n):
    return bc.bases(rng, n, b'ACGT').decode()


def gfa_jobs():
    rng = np.random.default_rng(150185)
    three = rec('utg1', 500, 31) + rec('utg2', 600, 7) + rec('utg3', 7, 0)
    fa3 = {'utg2': 600, 'utg1': 500, 'utg3': 7}
    jobs = [
        # ---- file and line shape
        Job('shape/empty_file', [b'']),
        Job('shape/no_record', [H_LINE + L_LINE + A_LINE]),
        Job('shape/no_record_with_contigs', [H_LINE + L_LINE], fa={'utg1': 5}),
        Job('shape/plain', [three], fa3),
        Job('shape/no_final_newline', [three[:-1]], fa3),
        Job('shape/crlf', [three.replace(b'\n', b'\r\n')], fa3),
        Job('shape/lone_cr', [three.replace(b'\n', b'\r')], fa3),
        Job('shape/lone_cr_no_final', [three.replace(b'\n', b'\r')[:-1]], fa3),
        Job('shape/mixed_breaks', [rec('utg1', 500, 31, eol='\r\n') + A_LINE.replace(b'\n', b'\r') + rec('utg2', 600, 7, eol='\r') + b'\n\r\n' + rec('utg3', 7, 0)], fa3),
        # ---- records
        Job('records/first_and_last_line', [rec('utg1', 500, 31) + H_LINE + A_LINE * 3 + L_LINE + rec('utg2', 600, 7) + A_LINE + L_LINE + rec('utg3', 7, 0)], fa3),
        Job('records/shorter_than_a_lane', [b'S\ta\t*\t1\t2\n' * 1 + b'S\tb\t*\t3\t4\nS\tc\t*\t5\t6\nS\td\t*\t7\t8\nS\te\t*\t9\t0\n'], {'a': 1, 'b': 3, 'c': 5, 'd': 7, 'e': 9},
            straddles='LANE: three records of 10 bytes inside two lanes'),
        Job('records/minimal_refused', [b'S\t\t\t\t1\n'], straddles='the minimal record: field 3 is empty'),
        Job('records/minimal_served', [b'S\ta\t*\t1\t2\n'], {'a': 1}),
        Job('records/empty_name', [rec('', 5, 1) + rec('utg2', 600, 7)], {'': 5, 'utg2': 600}),
        Job('records/names_with_blanks', [rec('ctg 1  x', 5, 1) + rec(' lead', 6, 2) + rec('trail ', 7, 3)], {'ctg 1  x': 5, ' lead': 6, 'trail ': 7}),
        Job('records/no_colon', [b'S\tu\t*\t12345\t678\n'], {'u': 12345}),
        Job('records/many_colons', [b'S\tu\t*\tLN:i::::12\trd:::3\n'], {'u': 12}),
        Job('records/leading_zeros', [rec('u', '0012', '000')], {'u': 12}),
        Job('records/18_digits', [rec('u', '9' * 18, '1' + '0' * 17)]),
        Job('records/name_255', [rec('n' * 255, 5, 1)], {'n' * 255: 5}),
        Job('records/extra_fields', [rec('utg1', 500, 31, extra='\tdp:f:1.5\tXX:Z:a\tb') + rec('utg2', 600, 7, extra='\t')], {'utg1': 500, 'utg2': 600}),
        # ---- the sequence field
        Job('sequence/next_block', [rec('utg1', 5000, 31, seq=_seq(rng, 5000)) + A_LINE * 4 + rec('utg2', 600, 7, seq=_seq(rng, 600))], {'utg1': 5000, 'utg2': 600},
            straddles='TX_BLOCK: the sequence ends in the block after its start'),
        Job('sequence/long', [rec('utg0', 3, 2) + rec('utg1', LONG_BLOCKS * TX_BLOCK + 777, 31, seq=_seq(rng, LONG_BLOCKS * TX_BLOCK + 777)) + A_LINE * 50 +
                              rec('utg2', 9000, 7, seq=_seq(rng, 9000)) + L_LINE],
            {'utg0': 3, 'utg1': LONG_BLOCKS * TX_BLOCK + 777, 'utg2': 9000}, straddles='LONG_BLOCKS: %d blocks without a TAB between two TABs of one record' % LONG_BLOCKS),
        # ---- crediting of TABs
        Job('credit/three_tabs_then_A', [b'S\tx\t*\tLN:i:5\n' + A_LINE + rec('y', 5, 3)], straddles='the A line has TABs: none is credited to the record'),
        Job('credit/two_tabs_last_line', [rec('y', 5, 3) + b'S\tx\t*'], straddles='no TAB behind the record at all'),
        Job('credit/one_tab', [b'S\t\n' + rec('y', 5, 3)]),
        Job('credit/not_records', [b'S x\t*\t1\t2\nSX\ta\t*\t1\t2\ns\ta\t*\t1\t2\n \tS\t*\t1\t2\n' + rec('y', 5, 3) + b'S'], {'y': 5}),
        # ---- duplicates
        Job('duplicates/one_file', [rec('utg1', 500, 31) + rec('utg2', 600, 7) + rec('utg1', 500, 99)], {'utg1': 500, 'utg2': 600}),
        Job('duplicates/two_files', [rec('utg1', 500, 31) + rec('utg2', 600, 7), rec('utg3', 7, 0) + rec('utg1', 500, 99)], fa3),
        Job('files/four', [rec('a%d' % k, 100 + k, k) + A_LINE + rec('b%d' % k, 200 + k, 10 * k) for k in range(4)],
            dict([('b%d' % k, 200 + k) for k in range(4)] + [('a%d' % k, 100 + k) for k in range(4)])),
        Job('files/none', []),
        Job('files/none_with_contigs', [], {'utg1': 5}),
        # ---- mismatches and the warning
        Job('mismatch/length_first_file', [rec('utg1', 500, 31) + rec('utg2', 601, 7) + rec('utg3', 8, 0), rec('utg3', 7, 0)], fa3),
        Job('mismatch/length_second_file', [rec('utg1', 500, 31), rec('utg2', 600, 7) + rec('utg3', 8, 0) + rec('utg1', 1, 1)], fa3),
        Job('mismatch/missing_contig', [rec('utg1', 500, 31) + rec('utg3', 7, 0)], fa3),
        Job('mismatch/two_missing', [rec('utg3', 7, 0)], fa3),
        Job('mismatch/more_records_than_contigs', [three + rec('utg4', 1, 1)], fa3),
        Job('mismatch/refused_second_file', [three, rec('utg4', '+5', 1)], fa3),
    ]
    # ---- refusals, each on its own, in field 3 and in field 4
    spellings = [('float', '12.5'), ('plus', '+5'), ('minus', '-5'), ('underscore', '1_0'), ('blank_before', ' 7'), ('blank_behind', '7 '), ('19_digits', '1' * 19),
                 ('empty', ''), ('letters', 'abc')]
    for tag, text in spellings:
        jobs.append(Job('refuse/%s_depth' % tag, [rec('utg1', 500, 31) + rec('utg2', 600, text) + rec('utg3', 7, 0)]))
        jobs.append(Job('refuse/%s_length' % tag, [rec('utg2', text, 7)]))
        jobs.append(Job('refuse/%s_depth_then_field' % tag, [rec('utg2', 600, text, extra='\tdp:i:1')]))
    jobs += [Job('refuse/depth_is_f', [rec('utg1', 500, '12.5', rd='rd:f:')]),
             Job('refuse/empty_last_field', [b'S\ta\t*\tLN:i:5\t\n']),
             Job('refuse/empty_last_field_no_break', [b'S\ta\t*\tLN:i:5\t']),
             Job('refuse/name_256', [rec('n' * 256, 5, 1)]),
             Job('refuse/byte_0x80_name', [rec('utg\x80', 5, 1)]),
             Job('refuse/byte_0x80_depth', [rec('utg1', 5, '1\xff')]),
             Job('refuse/four_fields', [b'S\ta\t*\tLN:i:5\n']),
             Job('refuse/two_fields', [rec('utg1', 500, 31) + b'S\tb\n'])]
    # ---- a name, a TAB and an integer ending exactly at, and one byte past, a block seam, a wave step and a lane; the same at the end of the file
    r = rec('seam_ctg', 4321, 87)
    inner = {'name_end': 2 + len('seam_ctg') - 1, 'name_tab': 2 + len('seam_ctg'), 'length_end': r.index(b'4321') + 3, 'depth_tab': r.index(b'4321') + 4,
             'depth_end': len(r) - 2, 'line_break': len(r) - 1, 'first_tab': 1}
    for step, step_name in ((TX_BLOCK, 'TX_BLOCK'), (WAVE_STEP + TX_BLOCK, 'WAVE_STEP'), (LANE * 3, 'LANE')):
        for what, k in inner.items():
            for past in (0, 1):
                text = at_seam(r, k, step - 1 + past) + A_LINE + rec('after', 5, 6)
                jobs.append(Job('seam/%s_%s_%s' % (step_name, what, 'past' if past else 'at'), [text], {'seam_ctg': 4321, 'after': 5},
                                straddles='%s: byte %d of the file is the %s' % (step_name, step - 1 + past, what)))
    for size in (TX_BLOCK - 1, TX_BLOCK, TX_BLOCK + 1, 2 * TX_BLOCK, LANE * 4, LANE * 4 + 1):
        for tag, tail in (('no_break', r[:-1]), ('lf', r), ('crlf', r[:-1] + b'\r\n'), ('cr', r[:-1] + b'\r')):
            text = at_seam(tail, len(tail) - 1, size - 1)
            assert len(text) == size
            jobs.append(Job('eof/%d_%s' % (size, tag), [text], {'seam_ctg': 4321}, straddles='the file ends with its byte %d' % (size - 1)))
    # a "\r\n" cut by a block seam behind the last field, and a TAB as the first byte of a block
    jobs.append(Job('seam/crlf_cut', [at_seam(r[:-1] + b'\r\n', len(r) - 1, TX_BLOCK - 1) + rec('after', 5, 6)], {'seam_ctg': 4321, 'after': 5}, straddles='TX_BLOCK'))
    assert len({j.name for j in jobs}) == len(jobs)
    return jobs


def refused_files(job):
    """the indices of the files of a job that the reader hands back (include/haphic_hip.h lists the reasons)"""
    if job.name.startswith('refuse/') or job.name in ('records/minimal_refused', 'credit/three_tabs_then_A', 'credit/two_tabs_last_line', 'credit/one_tab'):
        return {0}
    return {1} if job.name == 'mismatch/refused_second_file' else set()


# ------------------------------------------------------------------ stat_fragments inputs
CONTIG_LENGTHS = (250000, 130000, 100001, 100000, 30011, 12000, 6001, 6000, 5999, 5000, 4097, 2001, 2000, 1999, 700, 3, 0, 10001)
NCHRS = 2                                      # --bin_size < 0: max(min(int(total / 2 / 30), 2000000), 100000) = 100000 bp
RES = ('GATC', 'GATC,AAGCTT,GANTC')
BIN_SIZES = (0, -1, 5)                         # never split; derived (100000 bp: 100001 leaves a bin of one base); 5 kbp
FLANKS = (0, 1, 3)                             # whole fragments; 1000 bp flanks; 3000 bp: larger than half a 5 kbp bin
NXS = (80, 100)
WHITELIST = ('c05', 'c14', 'c02')


def genome(seed=188296):
    """(text, names, lengths) of the assembly of the fragment statistics: lengths on both sides of every bin size and flank rule, soft-masked runs,
    lines of 80 columns"""
    rng = np.random.default_rng(seed)
    names = ['c%02d' % k for k in range(len(CONTIG_LENGTHS))]
    text = b''.join(b'>' + n.encode() + b'\n' + bc.wrap(bc.bases(rng, m, b'ACGTacgtGATCN'), 80) for n, m in zip(names, CONTIG_LENGTHS))
    return text, names, list(CONTIG_LENGTHS)


def depth_dict(names):
    return {n: (k % 2, 10 + 3 * k) for k, n in enumerate(names)}


def fragment_combos():
    """[(key, RE, bin_size, flank, Nx, whitelist, with_depth)]"""
    out = []
    for RE, b, f, nx, wl, dp in itertools.product(RES, BIN_SIZES, FLANKS, NXS, (False, True), (False, True)):
        out.append(('%s|bin%d|flank%d|Nx%d|wl%d|depth%d' % (RE, b, f, nx, wl, dp), RE, b, f, nx, set(WHITELIST) if wl else set(), dp))
    return out


def plain_stat(result, fa_dict, read_depth_dict):
    """the seven return values of stat_fragments, fa_dict and read_depth_dict afterwards as the fixture keeps them (sets sorted: their order is the
    process's hash seed's)"""
    sorted_frag_list, bin_set, bin_size, frag_len_dict, Nx_frag_set, RE_site_dict, split_ctg_set = result
    return {'sorted_frag_list': [list(x) for x in sorted_frag_list], 'bin_set': sorted(bin_set), 'bin_size': bin_size,
            'frag_len_dict': [list(x) for x in frag_len_dict.items()], 'Nx_frag_set': sorted(Nx_frag_set),
            'RE_site_dict': [list(x) for x in RE_site_dict.items()], 'split_ctg_set': sorted(split_ctg_set),
            'fa_dict': [[n] + list(list.__iter__(v)) for n, v in fa_dict.items()], 'read_depth_dict': [[n, list(v)] for n, v in read_depth_dict.items()]}


# ------------------------------------------------------------------ the fixture
def golden():
    """{'gfa': {job: {...}}, 'fragments': {combo: {...}}, 'correction': {...}} of tests/golden/assembly.npz"""
    z = np.load(FIXTURE)
    return json.loads(z['json'].tobytes().decode('utf-8'))
