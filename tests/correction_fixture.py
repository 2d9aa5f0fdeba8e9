"""tests/golden/correction.npz (made by tests/golden/make_golden_correction.py from the reference's own assembly correction) and what the
tests do with it: rebuild the inputs, drive the mirrors of haphic_amd/correct.py the way correct_assembly :1200-1243 and run() :2835-2873
drive the reference's functions, and compare every stage exactly.  Also a numpy stand-in for the two _lib classes of the correction
(CorrectTable, ContigRemap) on top of tests/oracle_lib.py, for the tests that run without a GPU."""
import hashlib
import json
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'correction.npz')


def load(path=GOLDEN):
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    fx['meta'] = json.loads(str(fx['meta']))
    fx['names'] = [str(n) for n in fx['names']]
    return fx


def write_inputs(fx, d):
    """asm.fa and hic.pairs as the generator wrote them"""
    rng = np.random.default_rng(int(fx['seq_seed']))
    with open(os.path.join(d, 'asm.fa'), 'w') as f:
        for n, l in zip(fx['names'], fx['lens'].tolist()):
            f.write('>%s\n%s\n' % (n, ''.join(rng.choice(list('ACGT'), int(l)))))
    nm = fx['names'] + ['elsewhere']
    with open(os.path.join(d, 'hic.pairs'), 'w') as f:
        f.write('## pairs format v1.0\n')
        f.write(''.join('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, nm[a], p + 1, nm[b], q + 1) for k, (a, p, b, q) in
                        enumerate(zip(fx['id1'].tolist(), fx['pos1'].tolist(), fx['id2'].tolist(), fx['pos2'].tolist()))))


def _args(fx, nrounds):
    r = fx['meta']['ratios']
    return types.SimpleNamespace(alignments='hic.pairs', aln_format='pairs', correct_resolution=int(fx['res']), correct_nrounds=nrounds,
                                 median_cov_ratio=r[0], region_len_ratio=r[1], min_region_cutoff=r[2], RE=fx['meta']['RE'], quick_view=False, gfa=None,
                                 fasta='asm.fa', flank=fx['meta']['flank'], max_read_pairs=200, remove_allelic_links=0, remove_concentrated_links=False,
                                 threads=1)


def _plain(v):
    """JSON round trip of a container value / key, as the generator stored it"""
    if isinstance(v, (set, frozenset)):
        return sorted(list(x) for x in v)
    if hasattr(v, 'tolist'):
        v = v.tolist()
    if isinstance(v, tuple):
        return list(v)
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def _items(d):
    return [[_plain(k), _plain(v)] for k, v in d.items()]


def check_against_mirrors(fx, workdir, files_join=None):
    """the whole correction through haphic_amd.correct / haphic_amd.cluster (whatever `_lib` they are bound to) against the fixture"""
    from haphic_amd import cluster, correct
    cwd = os.getcwd()
    os.chdir(workdir)
    try:
        write_inputs(fx, '.')
        for nrounds in (3, 1):
            want = fx['meta']['runs'][str(nrounds)]
            args = _args(fx, nrounds)
            fa = cluster.parse_fasta('asm.fa', RE=args.RE)
            cov_d, pos_d = correct.parse_pairs_for_correction(fa, args)
            session = cov_d._session
            # ---- pass one: coverage arrays, position lists, their order
            cov_items, pos_items = session.cov_items(), session.pos_items()
            assert [n for n, _v in cov_items] == fx['names']
            for k, (n, v) in enumerate(cov_items):
                assert v.dtype == np.int32 and np.array_equal(v, fx['cov_flat'][fx['cov_ptr'][k]:fx['cov_ptr'][k + 1]]), n
            # (the reference's defaultdict lists its keys by first appearance in the file, the table by contig; nothing reads that order)
            assert sorted(n for n, _v in pos_items) == sorted(fx['meta']['pos_keys']) and len(pos_items) == len(fx['meta']['pos_keys'])
            at = {n: k for k, n in enumerate(fx['meta']['pos_keys'])}
            for n, v in pos_items:                               # every list item for item: the pairs of a contig in file order
                assert v.typecode == 'i' and np.array_equal(np.asarray(v, np.int32), fx['pos_flat'][fx['pos_ptr'][at[n]]:fx['pos_ptr'][at[n] + 1]]), n
            # ---- the rounds, as correct_assembly :1204-1243 runs them
            unbroken, source, fpos, ffrag = set(fa), {}, {}, {}
            n_rounds_run = 0
            for rnd in range(nrounds):
                bp = correct.detect_break_points(cov_d, fa, args)
                got = {c: [[int(p), int(v)] for p, v in pts] for c, pts in bp.items()}
                assert got == want['rounds'][rnd] and list(got) == list(want['rounds'][rnd]), (nrounds, rnd)
                n_rounds_run += 1
                if not bp:
                    break
                if rnd == 0:
                    for c in bp:
                        source[c], fpos[c], ffrag[c] = c, [0], [c]
                last = rnd + 1 == nrounds
                correct.break_and_update_ctgs(bp, pos_d, cov_d, source, fpos, ffrag, fa, {}, unbroken, args, last)
                unbroken -= set(bp)
                state = want['states'][rnd]
                assert (state is None) == last
                if not last:
                    assert cov_d.frozen and pos_d.frozen
                    cov_now = {n: v.tolist() for n, v in session.cov_items()}
                    assert cov_now == state['cov'] and list(cov_now) == list(state['cov']), (nrounds, rnd)
                    pos_now = {n: v.tolist() for n, v in session.pos_items()}
                    assert pos_now == state['pos'], (nrounds, rnd)
            assert n_rounds_run == len(want['rounds'])
            assert fpos == want['final_break_pos_dict'] and ffrag == want['final_break_frag_dict']
            assert list(fpos) == list(want['final_break_pos_dict'])
            assert [[n, v[1], v[2]] for n, v in fa.items()] == want['fa']
            assert ''.join(n + '\n' for n in fa if n not in unbroken) == want['corrected_ctgs']          # :1271-1275
            del cov_d, pos_d, session
            if nrounds != 3:
                continue
            # ---- pass two as run() :2835-2873 calls it, contig and --bin_size variant
            for variant in ('ctg', 'bin'):
                w = want['pass_two_' + variant]
                fd = {n: [None, v[1], v[2]] for n, v in fa.items()}
                nx, split = set(w['Nx_frag_set']), set(w['split_ctg_set'])
                if variant == 'bin':
                    aln = correct.pairs_generator_for_correction('hic.pairs', 'pairs', fpos, ffrag)
                    out = cluster.parse_alignments(aln, fd, args, w['bin_size'], w['frag_len_dict'], nx, split, w['pos_int_type'], w['dist_int_type'])
                else:
                    aln = correct.pairs_generator_for_correction_ctg('hic.pairs', 'pairs', fpos, ffrag)
                    out = cluster.parse_alignments_for_ctgs(aln, fd, args, w['frag_len_dict'], nx, w['pos_int_type'], w['dist_int_type'])
                assert len(out) == len(w['containers'])
                for k, (got_d, want_items) in enumerate(zip(out, w['containers'])):
                    if k == 4:                                   # frag_link_dict: the S5 mirror fills it in fragment order (cluster._s5_containers), the
                        assert sorted(_items(got_d)) == sorted(want_items), (variant, k)      # reference by first appearance; same entries
                    else:
                        assert _items(got_d) == want_items, (variant, k)
                del out
                if files_join is not None:
                    files_join()
                bed = open('alignments.bed', 'rb').read()
                assert len(bed) == w['bed_bytes'] and hashlib.sha256(bed).hexdigest() == w['bed_sha256'], variant
                os.remove('alignments.bed')
    finally:
        os.chdir(cwd)


# ------------------------------------------------------------------ numpy stand-ins for _lib.CorrectTable / _lib.ContigRemap
class CorrectTable:
    """the interface of haphic_amd._lib.CorrectTable over plain numpy / Python (the restatement of tests/test_gpu_correction.py)"""

    def __init__(self, ctg_len, resolution):
        self.lens = [int(x) for x in ctg_len]
        if any(x >= 2 ** 31 - 1 for x in self.lens):
            raise RuntimeError('contigs of 2^31 bp and more are refused')
        self.res = int(resolution)
        self.parts = []

    def push(self, id1, pos1, id2, pos2):
        self.parts.append([np.array(a, np.int64) for a in (id1, pos1, id2, pos2)])

    def push_device(self, n, id1, pos1, id2, pos2):
        self.push(id1[:n], pos1[:n], id2[:n], pos2[:n])

    def finalize(self):
        from tests.test_gpu_correction import ref_pass_one
        a = [np.concatenate([p[c] for p in self.parts]) if self.parts else np.zeros(0, np.int64) for c in range(4)]
        cov, pos = ref_pass_one(self.lens, self.res, *a)
        self.seg = [(c, p, n) for c, p, n in zip(cov, pos, self.lens)]
        return sum(len(p) for p in pos) // 2

    def shape(self):
        return len(self.seg), sum(len(s[0]) for s in self.seg), sum(len(s[1]) for s in self.seg) // 2

    def segments(self):
        nb = np.array([len(s[0]) for s in self.seg], np.int32)
        off = np.concatenate(([0], np.cumsum(nb)[:-1])).astype(np.int64) if len(nb) else np.zeros(0, np.int64)
        po = np.concatenate(([0], np.cumsum([len(s[1]) // 2 for s in self.seg]))).astype(np.int64)
        return off, nb, np.array([s[2] for s in self.seg], np.int32), po

    def coverage(self):
        return np.concatenate([s[0] for s in self.seg]).astype(np.int32) if self.seg else np.zeros(0, np.int32)

    def pairs(self):
        return np.array([x for s in self.seg for x in s[1]], np.int32)

    def detect(self, median_cov_ratio, region_len_ratio, min_region_cutoff):
        from tests.test_gpu_correction import ref_detect
        n_bp, cov, bins = np.zeros(len(self.seg), np.int32), np.zeros(len(self.seg), np.int32), []
        for s, (c, _p, length) in enumerate(self.seg):
            bp = ref_detect(c, length, self.res, median_cov_ratio, region_len_ratio, min_region_cutoff)
            if bp:
                n_bp[s], cov[s] = len(bp), bp[0][1]
                bins.extend(p // self.res for p, _v in bp)
        return n_bp, cov, np.array(bins, np.int32)

    def break_(self, seg, bp_off, bp_pos, zero):
        from tests.test_gpu_correction import ref_break
        new = []
        for b, s in enumerate(seg):
            c, p, length = self.seg[s]
            points = [(int(x), 0 if zero[b] & 1 else 1) for x in bp_pos[bp_off[b]:bp_off[b + 1]]]
            bounds = [0] + [x for x, _v in points] + [length]
            for t, (piece, kid) in enumerate(ref_break(c, p, points, self.res, bool(zero[b] & 2))):
                new.append((piece, kid, bounds[t + 1] - bounds[t]))
        self.seg = new

    def destroy(self):
        pass


class ContigRemap:
    def __init__(self, off, break_pos, new_id):
        self.off, self.pos, self.new = [np.asarray(a, np.int64) for a in (off, break_pos, new_id)]

    def apply(self, n, ids, xs):
        for k in range(int(n)):
            s = int(ids[k])
            if s < 0:
                continue
            nid, shift = -1, 0
            if s < len(self.off) - 1:
                for q in range(self.off[s], self.off[s + 1]):
                    if self.pos[q] <= xs[k]:
                        nid, shift = int(self.new[q]), int(self.pos[q])
            ids[k] = nid
            if nid >= 0:
                xs[k] -= shift

    def destroy(self):
        pass


def stand_in_lib():
    """tests/oracle_lib.py plus the two classes above: what `_lib` is bound to in the tests without a GPU"""
    from tests import oracle_lib
    lib = types.ModuleType('correction_stand_in_lib')
    lib.__dict__.update({k: v for k, v in vars(oracle_lib).items() if not k.startswith('__')})
    lib.CorrectTable, lib.ContigRemap = CorrectTable, ContigRemap
    return lib
