"""Cases and host engines for the front of `haphic reassign` on the device (haphic_amd/reassign.py bind_fasta, bind_pickle(resident=True) and the
resident branch of parse_link_dict; csrc/hhx_fasta.hip hhx_fasta_re_counts / hhx_fasta_fetch, csrc/hhx_pickleread.hip
hhx_reassign_create_from_pickle).

  * fasta_engine() -> a NumpyFasta (tests/build_cases.py) with re_counts_device / fetch and a record of every fetch;
  * HostLinkPickle: the interface of _lib.LinkPickle over tests/link_pickle_cases.host_reader, counting the copies of its keys;
  * HostReassign: tests/reassign_cases.NumpyReassign with from_pickle, which decides by Python's own integers what the device pass decides;
  * the FASTA cases (the text and refusal cases of tests/build_cases.py and edge_genome() below), the RE strings, and the reader of
    tests/golden/reassign_front.npz (make_golden_reassign_front.py)."""
import os

import numpy as np

from tests import build_cases as bc
from tests import link_pickle_cases as lp
from tests import reassign_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'reassign_front.npz')
RES = ('GATC', 'GATC,GANTC', 'AAGCTT', 'GCGC')
SMALL = 2048                                     # the fixture keeps the sequences of cases up to this many bases


# ------------------------------------------------------------------ engines
def fasta_engine():
    """a fresh engine class: Engine.fetched lists (off, len) of every fetch of every instance, Engine.count_calls the re_counts_device calls"""
    class Engine(bc.NumpyFasta):
        class Unsupported(RuntimeError):
            pass

        fetched = []
        count_calls = []
        opened = []

        def __init__(self, source, keep_letter_case=False):
            try:
                bc.NumpyFasta.__init__(self, source, keep_letter_case)
            except bc.NumpyFasta.Unsupported as e:
                raise Engine.Unsupported(str(e))
            Engine.opened.append(self)

        def re_counts_device(self, sites, seg_off=None, seg_len=None):
            off = self.seq_off if seg_off is None else np.asarray(seg_off, np.int64)
            ln = self.seq_len if seg_len is None else np.asarray(seg_len, np.int64)
            Engine.count_calls.append(len(off))
            blob = self._seq.tobytes()
            return np.array([sum(blob[o:o + n].count(s) for s in sites) for o, n in zip(off.tolist(), ln.tolist())], np.int64)

        def fetch(self, off, len):
            if off < 0 or len < 0 or off + len > self._seq.size:
                raise RuntimeError('fetch: bytes [%d, +%d) of %d' % (off, len, self._seq.size))
            Engine.fetched.append((off, len))
            return self._seq[off:off + len].tobytes()

        def sequences(self):
            raise AssertionError('the front of reassign never copies all sequences')

    return Engine


class HostLinkPickle:
    """_lib.LinkPickle's interface over the host reader; HostLinkPickle.open(path) -> a handle or None"""

    opened = []                                  # every handle of this process

    def __init__(self, arrays):
        self._arrays = arrays
        i, _j, _value, is_float, names = arrays
        self.n_keys, self.n_names, self.any_float = len(i), len(names), is_float is not None
        self.key_fetches = 0
        self.closed = False
        HostLinkPickle.opened.append(self)

    @classmethod
    def open(cls, path):
        arrays = lp.host_reader(path)
        return None if arrays is None else cls(arrays)

    def names(self):
        return list(self._arrays[4])

    def arrays(self):
        assert not self.closed
        self.key_fetches += 1
        return self._arrays

    def close(self):
        self.closed = True


class HostReassign(rc.NumpyReassign):
    """NumpyReassign + from_pickle: the refusals by exact integers"""

    REFUSALS = []
    SELF_KEY, FLOAT, NEGATIVE, TOTAL = 1, 2, 4, 8

    @classmethod
    def from_pickle(cls, link_pickle, n_ctg, group, n_groups):
        assert not link_pickle.closed and n_ctg >= link_pickle.n_names
        i, j, value, is_float, _names = link_pickle._arrays               # where they lie: no copy is counted
        why = 0
        if is_float is not None:
            why |= cls.FLOAT
            ints = [int(v) for v, f in zip(value.tolist(), is_float.tolist()) if not f]
        else:
            ints = value.tolist()
        if (i == j).any():
            why |= cls.SELF_KEY
        if any(v < 0 for v in ints):
            why |= cls.NEGATIVE
        if 2 * sum(v for v in ints if v >= 0) >= 2 ** 53:
            why |= cls.TOTAL
        if why:
            cls.REFUSALS.append((why, 'host engine'))
            return None
        return cls(i, j, value, n_ctg, group, n_groups)


# ------------------------------------------------------------------ FASTA cases
def edge_genome(seed=31):
    """(text, names, sequences) of a genome of a few tens of KB for the RE-site counts: contigs of 4095 / 4096 / 4097 bases and one over three
    4096-byte blocks, an empty contig and one shorter than any site, GATC / AAGCTT / GCGC straddling two contigs (no match), runs of GCGCGC for the
    greedy rule, lower-case bases, and a site in the last bytes"""
    rng = np.random.default_rng(seed)

    def rnd(n):
        return bc.bases(rng, n, b'ACGT')
    seqs = [('len4095', rnd(4095)), ('len4096', rnd(4091) + b'GATCG'[:5]), ('len4097', rnd(4097)), ('three_blocks', rnd(4000) + b'GATC' + rnd(5200) + b'AAGCTT'),
            ('empty', b''), ('short', b'GA'), ('left_gatc', rnd(100) + b'GA'), ('right_gatc', b'TC' + rnd(97) + b'AAG'), ('right_aagctt', b'CTT' + rnd(50) + b'GC'),
            ('right_gcgc', b'GC' + rnd(30)), ('greedy', b'GCGCGC' + b'A' + b'GCGCGCGCGC' + b'T' + b'GCGCG' + rnd(40) + b'GCGCGCG'),
            ('lower', b'gatcGATCgaTCaagcttAAGCTTgcgcgcGCGCGAATCgantc' + rnd(300).lower() + rnd(300)),
            ('n_sites', b'GAATCGATTCGACTCGAGTCGANTC' * 7)]
    before = sum(len(s) for _n, s in seqs)
    seqs.append(('block_seam', rnd((-before - 2) % 4096) + b'GATC' + rnd(11)))      # a site across the seam of two 4096-byte blocks of the sequences
    seqs.append(('last', rnd(777) + b'AAGCTTGCGCGATC'))
    text = b''.join(b'>' + n.encode() + b' x\n' + bc.wrap(s, 70 if k % 2 else 61) for k, (n, s) in enumerate(seqs))
    return text, [n for n, _s in seqs], [s for _n, s in seqs]


def fasta_cases():
    """[(name, text bytes, refused by the reader?)]: the text and refusal cases of tests/build_cases.py that concern the reader, and edge_genome()"""
    out = [(c.name, c.fasta, False) for c in bc._text_cases()]
    out += [(c.name, c.fasta, True) for c in bc._refusal_cases() if c.name in ('refuse/high_byte', 'refuse/sequence_first', 'refuse/duplicate_names')]
    out.append(('front/edge_genome', edge_genome()[0], False))
    out.append(('front/no_contig', b'\n \n', False))
    return out


def golden():
    """{(case, keep_letter_case, RE): (names, lengths, RE sites + 1)}, {(case, keep_letter_case): sequences back to back} of the fixture; a case the
    reference raised on maps to the name of its exception"""
    z = np.load(FIXTURE)
    names, name_off = z['names'].tolist(), z['name_off'].tolist()
    ints, int_off = z['ints'], z['int_off'].tolist()
    blob, blob_off = z['blob'].tobytes(), z['blob_off'].tolist()
    tables, seqs = {}, {}
    q = b = 0
    for k, case in enumerate(z['cases'].tolist()):
        for keep in (False, True):
            if z['raises'][k]:
                for RE in RES:
                    tables[(case, keep, RE)] = str(z['raises'][k])
                continue
            n = names[name_off[q]:name_off[q + 1]]
            nums = ints[int_off[q]:int_off[q + 1]].reshape(1 + len(RES), -1)
            for r, RE in enumerate(RES):
                tables[(case, keep, RE)] = (n, nums[0].tolist(), nums[1 + r].tolist())
            if z['has_seq'][k]:
                seqs[(case, keep)] = blob[blob_off[b]:blob_off[b + 1]].decode('ascii')
                b += 1
            q += 1
    return tables, seqs


# ------------------------------------------------------------------ link tables with a grouping
def grouping(names, extra=3, seed=9, n_groups=5):
    """ctg_group_dict over the names of a link table and `extra` contigs no key names: groups dealt by a planted case of tests/reassign_cases.py
    (some 'ungrouped'), in an order that is not the table's"""
    group = rc.build_case(seed, n_groups, 20, 0.3, 0.05, 0.25)[3]
    every = list(names) + ['lonely_%d' % k for k in range(extra)]
    order = np.random.default_rng(seed).permutation(len(every)).tolist()
    return {every[k]: ('ungrouped' if group[k % len(group)] < 0 else 'g%d' % group[k % len(group)]) for k in order}


def round_inputs(ctg_group_dict):
    """fa_dict, RE_site_dict, sorted_ctg_list, group_RE_dict for one round over a grouping, from the contigs' positions alone"""
    ctgs = list(ctg_group_dict)
    fa_dict = {c: [None, 1000 + 37 * (k * k % 101), 2 + k % 29] for k, c in enumerate(ctgs)}
    re_sites = {c: info[2] for c, info in fa_dict.items()}
    sorted_ctg_list = sorted([(c, fa_dict[c][1]) for c in fa_dict], key=lambda x: x[1], reverse=True)
    group_re = {}
    for c, g in ctg_group_dict.items():
        if g != 'ungrouped':
            group_re[g] = group_re.get(g, 1) + re_sites[c] - 1
    return fa_dict, re_sites, sorted_ctg_list, group_re
