"""Dev container only (needs the reference checkout): tests/golden/correction.npz from the reference's OWN assembly correction.

Runs HapHiC_cluster.parse_pairs_for_correction, correct_assembly (detect_break_points spied per round), stat_fragments, the
*_for_correction(_ctg) generators and parse_alignments(_for_ctgs) on a synthetic chimeric assembly and stores inputs and results as data.
`portion` is not installed here; the stand-in below has the semantics the reference uses: closed atoms, `|` merges atoms that touch,
closed(a, b) - union = the open gaps, len = atom count, .lower / .upper, closed `overlaps` counts touching ends.

    python tests/golden/make_golden_correction.py [reference scripts dir]
"""
import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class Iv:
    """a union of disjoint closed (or, as a difference, open) atoms [(lo, hi), ...] in ascending order"""

    def __init__(self, atoms=()):
        self.atoms = list(atoms)

    def __or__(self, other):
        out = []
        for lo, hi in sorted(self.atoms + other.atoms):
            if out and lo <= out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], hi))
            else:
                out.append((lo, hi))
        return Iv(out)

    def __sub__(self, other):
        assert len(self.atoms) == 1
        at, hi = self.atoms[0]
        gaps = []
        for a, b in other.atoms:
            if a > at:
                gaps.append((at, a))
            at = max(at, b)
        if at < hi:
            gaps.append((at, hi))
        return Iv(gaps)

    def __len__(self):
        return len(self.atoms)

    def __iter__(self):
        return iter(Iv([a]) for a in self.atoms)

    @property
    def lower(self):
        return self.atoms[0][0]

    @property
    def upper(self):
        return self.atoms[-1][1]

    def overlaps(self, other):
        return any(a <= d and c <= b for a, b in self.atoms for c, d in other.atoms)


def load_reference(scripts):
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}),
                        ('portion', {'closed': lambda a, b: Iv([(a, b)]), 'empty': lambda: Iv()})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.path.insert(0, scripts)
    import HapHiC_cluster as H
    H.closed, H.empty = sys.modules['portion'].closed, sys.modules['portion'].empty
    return H


def make_input(seed=20, n_ctg=36, n_pairs=42_000, res=500):
    """contigs of 60-150 kb; a third are chimeras of 2-3 pieces, some joined across a stretch without any read pair, with a few pairs
    leaking over the other joins; 10 % inter-contig pairs; 1 % of the ends name a sequence that is not in the FASTA"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(60_000, 150_000, n_ctg)
    names = ['ctg%02d' % k for k in range(n_ctg)]
    pieces = []
    for c in range(n_ctg):
        n = int(lens[c])
        if c % 3 == 1:
            k = 1 + (c % 2)
            cuts = np.sort(rng.choice(np.arange(20, n // res - 20, 25), k, replace=False)) * res
            gap = (c % 4) * res
            bounds = [0] + cuts.tolist() + [n]
            pieces.append([(bounds[t] + (gap if t else 0), bounds[t + 1]) for t in range(k + 1)])
        else:
            pieces.append([(0, n)])
    ctg = rng.choice(n_ctg, n_pairs, p=lens / lens.sum())
    id1, id2 = ctg.copy(), ctg.copy()
    pos1, pos2 = np.zeros(n_pairs, np.int64), np.zeros(n_pairs, np.int64)
    span = rng.exponential(8 * res, n_pairs).astype(np.int64)
    u = rng.random(n_pairs)
    leak = rng.random(n_pairs) < 0.003
    for c in range(n_ctg):
        idx = np.flatnonzero(ctg == c)
        pc = pieces[c]
        which = rng.integers(0, len(pc), len(idx))
        lo_b, hi_b = np.array([p[0] for p in pc])[which], np.array([p[1] for p in pc])[which]
        lk = leak[idx] & (len(pc) == 2)                      # the three-piece chimeras keep their empty stretches
        lo_b, hi_b = np.where(lk, 0, lo_b), np.where(lk, int(lens[c]), hi_b)
        a = lo_b + (u[idx] * (hi_b - lo_b)).astype(np.int64)
        b = np.minimum(a + span[idx], hi_b - 1)
        swap = rng.random(len(idx)) < 0.5
        pos1[idx], pos2[idx] = np.where(swap, b, a), np.where(swap, a, b)
    other = rng.random(n_pairs)
    inter = other < 0.10
    id2[inter] = rng.integers(0, n_ctg, int(inter.sum()))
    pos2[inter] = (rng.random(int(inter.sum())) * lens[id2[inter]]).astype(np.int64)
    id1[(other >= 0.10) & (other < 0.105)] = n_ctg              # 'elsewhere'
    id2[(other >= 0.105) & (other < 0.11)] = n_ctg
    return names, lens, id1, pos1, id2, pos2


def sequences(names, lens, seed):
    rng = np.random.default_rng(seed)
    return {n: ''.join(rng.choice(list('ACGT'), int(l))) for n, l in zip(names, lens)}


def pairs_text(names, id1, pos1, id2, pos2):
    nm = list(names) + ['elsewhere']
    return '## pairs format v1.0\n' + ''.join('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, nm[a], p + 1, nm[b], q + 1)
                                              for k, (a, p, b, q) in enumerate(zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist())))


def items(d):
    """a dict of the S5 mirrors as JSON-able [[key, value], ...] in insertion order"""
    out = []
    for k, v in d.items():
        if isinstance(v, (set, frozenset)):
            v = sorted(list(x) for x in v)
        elif hasattr(v, 'tolist'):
            v = v.tolist()
        out.append([list(k) if isinstance(k, tuple) else k, v])
    return out


def main():
    scripts = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/scripts'
    H = load_reference(scripts)
    res, seq_seed = 500, 77
    names, lens, id1, pos1, id2, pos2 = make_input(res=res)
    seqs = sequences(names, lens, seq_seed)
    out = {'names': np.array(names), 'lens': lens.astype(np.int64), 'seq_seed': seq_seed, 'res': res,
           'id1': id1.astype(np.int32), 'pos1': pos1.astype(np.int32), 'id2': id2.astype(np.int32), 'pos2': pos2.astype(np.int32)}
    meta = {'ratios': [0.2, 0.1, 5000], 'RE': 'GATC', 'flank': 20, 'bin_size_kb': 20, 'runs': {}}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with open('hic.pairs', 'w') as f:
                f.write(pairs_text(names, id1, pos1, id2, pos2))
            with open('asm.fa', 'w') as f:
                for n in names:
                    f.write('>%s\n%s\n' % (n, seqs[n]))
            for nrounds in (3, 1):
                args = types.SimpleNamespace(alignments='hic.pairs', aln_format='pairs', correct_resolution=res, correct_nrounds=nrounds,
                                             median_cov_ratio=0.2, region_len_ratio=0.1, min_region_cutoff=5000, RE='GATC', quick_view=False, gfa=None,
                                             fasta='asm.fa', flank=20, max_read_pairs=200, remove_allelic_links=0, remove_concentrated_links=False,
                                             threads=1)
                fa_dict = H.parse_fasta('asm.fa', RE='GATC')
                cov_d, pos_d = H.parse_pairs_for_correction(fa_dict, args)
                if nrounds == 3:
                    assert list(cov_d) == names
                    out['cov_flat'] = np.concatenate([cov_d[n] for n in names]).astype(np.int32)
                    out['cov_ptr'] = np.cumsum([0] + [len(cov_d[n]) for n in names]).astype(np.int64)
                    meta['pos_keys'] = list(pos_d)
                    out['pos_flat'] = np.concatenate([np.asarray(pos_d[n], np.int32) for n in pos_d])
                    out['pos_ptr'] = np.cumsum([0] + [len(pos_d[n]) for n in pos_d]).astype(np.int64)
                rounds, states = [], []
                real_detect, real_break = H.detect_break_points, H.break_and_update_ctgs

                def spy(cd, fd, a, real=real_detect, sink=rounds):
                    got = real(cd, fd, a)
                    sink.append({c: [[int(p), int(v)] for p, v in pts] for c, pts in got.items()})
                    return got

                def spy_break(*a, real=real_break, sink=states, **k):
                    real(*a, **k)
                    bp, link_pos, cov = a[0], a[1], a[2]
                    last = a[10] if len(a) > 10 else k.get('last_round', False)
                    if not last:                                 # the table after this round: coverage and position lists of the children
                        sink.append({'cov': {c: v.tolist() for c, v in cov.items()},
                                     'pos': {c: list(link_pos[c]) for c in cov if c in link_pos}})
                    else:
                        sink.append(None)
                H.detect_break_points, H.break_and_update_ctgs = spy, spy_break
                try:
                    nbroken, fpos, ffrag = H.correct_assembly(cov_d, pos_d, fa_dict, {}, args)
                finally:
                    H.detect_break_points, H.break_and_update_ctgs = real_detect, real_break
                run = {'rounds': rounds, 'states': states, 'nbroken': nbroken, 'final_break_pos_dict': fpos, 'final_break_frag_dict': ffrag,
                       'fa': [[n, v[1], v[2]] for n, v in fa_dict.items()], 'corrected_ctgs': open('corrected_ctgs.txt').read()}
                os.remove('corrected_asm.fa')
                if nrounds == 3:
                    # the conditions the fixture must meet
                    r1 = rounds[0]
                    assert any(len(v) >= 2 and v[0][1] == 0 for v in r1.values()), 'no zero-coverage contig with two break points'
                    assert any(v[0][1] != 0 for v in r1.values()), 'no break at non-zero coverage'
                    assert len(rounds) >= 2 and any(':' in c for c in rounds[1]), 'nothing is broken again in round 2'
                    assert any(n in fa_dict for n in names), 'no chimera-free contig'
                    assert (id1 == len(names)).any() and (id2 == len(names)).any(), 'no name outside the FASTA'
                    assert rounds[-1] == {} and len(rounds) <= nrounds, 'the last round is not reached as "no break points"'
                    # an inner child holds one bin fewer than a fresh contig of its length would (:1153)
                    assert any(len(cv) == next(ln for n, ln, _re in run['fa'] if n == c) // res for c, cv in states[-1 if states[-1] else -2]['cov'].items()
                               if any(n == c for n, _l, _r in run['fa'])), 'no inner child with len // res bins'
                    # pass two, both variants
                    for variant, bin_size in (('ctg', 0), ('bin', 20)):
                        fd = {n: list(v) for n, v in fa_dict.items()}
                        _sl, bin_set, bsz, frag_len_dict, nx_set, re_dict, split = H.stat_fragments(fd, 'GATC', {}, set(), nchrs=3, flank=20, Nx=100,
                                                                                                   bin_size=bin_size)
                        pit, dit = H.determine_int_type(fd)
                        if variant == 'bin':
                            assert split, 'no contig is split'
                            aln = H.pairs_generator_for_correction('hic.pairs', 'pairs', fpos, ffrag)
                            res7 = H.parse_alignments(aln, fd, args, bsz, frag_len_dict, nx_set, split, pit, dit)
                        else:
                            assert not split
                            aln = H.pairs_generator_for_correction_ctg('hic.pairs', 'pairs', fpos, ffrag)
                            res7 = H.parse_alignments_for_ctgs(aln, fd, args, frag_len_dict, nx_set, pit, dit)
                        run['pass_two_' + variant] = {'bin_size': bsz, 'frag_len_dict': frag_len_dict, 'Nx_frag_set': sorted(nx_set),
                                                      'split_ctg_set': sorted(split), 'pos_int_type': pit, 'dist_int_type': dit,
                                                      'containers': [items(d) for d in res7]}
                        bed = open('alignments.bed', 'rb').read()
                        run['pass_two_' + variant]['bed_sha256'] = hashlib.sha256(bed).hexdigest()
                        run['pass_two_' + variant]['bed_bytes'] = len(bed)
                else:
                    assert len(rounds) == 1 and states == [None], 'nrounds = 1 must reach its only round as last_round=True'
                meta['runs'][str(nrounds)] = run
        finally:
            os.chdir(cwd)
    out['meta'] = np.array(json.dumps(meta, default=lambda o: o.item() if hasattr(o, 'item') else list(o)))
    path = os.path.join(HERE, 'correction.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: [len(r) for r in v['rounds']] for k, v in meta['runs'].items()})


if __name__ == '__main__':
    main()
