"""Assembly correction on the device (haphic_amd/csrc/hhx_correct.hip) through the C ABI, against a plain numpy / Python
restatement of HapHiC_cluster.py :943-1113 and :1300-1344 that lives in this file and shares no code with haphic_amd/.
Every comparison is exact (integers throughout)."""
import os
from array import array

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the restatement
def ref_pass_one(lens, res, id1, pos1, id2, pos2):
    """:1307-1342 -> coverage arrays and [lo, hi, lo, hi, ...] lists per contig"""
    cov = [np.zeros(n // res + 1, np.int32) for n in lens]
    pos = [[] for _ in lens]
    for a, p, b, q in zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist()):
        if a != b or a < 0:
            continue
        lo, hi = sorted([p, q])
        cov[a][lo // res:hi // res + 1] += 1
        pos[a].extend((lo, hi))
    return cov, pos


def ref_detect(cov, length, res, median_cov_ratio, region_len_ratio, min_region_cutoff):
    """:952-1009 for one contig -> [(position, coverage), ...] or None"""
    if not len(cov):
        return None
    median = np.median(cov)
    if not median:
        return None
    cutoff = median * median_cov_ratio
    region_cutoff = max(min_region_cutoff, length * region_len_ratio)
    high = np.concatenate(([False], cov >= cutoff, [False]))
    edges = np.flatnonzero(high[1:] != high[:-1])
    runs = [(s, e) for s, e in zip(edges[::2].tolist(), edges[1::2].tolist()) if (e - s) * res >= region_cutoff]      # bins [s, e)
    if len(runs) < 2:
        return None
    candidates = []
    for (_s0, e0), (s1, _e1) in zip(runs[:-1], runs[1:]):
        valley = cov[e0:s1]
        zeros = np.flatnonzero(valley == 0)
        if len(zeros):
            candidates.append((int(zeros[0]) + e0, 0))
        else:
            k = int(valley.argmin())
            candidates.append((k + e0, int(valley[k])))
    if any(c == 0 for _b, c in candidates):
        return [(b * res, 0) for b, c in candidates if c == 0]
    b, c = sorted(candidates, key=lambda x: x[1])[0]
    return [(b * res, c)]


def ref_break(cov, pos, points, res, lose_inner=False):
    """:1068-1113 :1153 :1178 for one contig -> [(child coverage, child position list, child length offset)]"""
    zero = points[0][1] == 0
    starts = [0] + [p for p, _c in points]
    kids = [[] for _ in starts]
    for k in range(len(pos) // 2):
        lo, hi = pos[2 * k], pos[2 * k + 1]
        if not zero and lo <= points[0][0] + res and hi >= points[0][0]:
            cov[lo // res:hi // res + 1] -= 1
            continue
        ci = max(t for t, s in enumerate(starts) if s <= lo)
        cj = max(t for t, s in enumerate(starts) if s <= hi)
        if ci == cj and not (lose_inner and ci < len(points)):       # :1050 files them under a name no later round reads
            kids[ci].extend((lo - starts[ci], hi - starts[ci]))
    out = []
    for t, s in enumerate(starts):
        piece = cov[s // res:starts[t + 1] // res] if t + 1 < len(starts) else cov[s // res:]
        out.append((piece, kids[t]))
    return out


# ------------------------------------------------------------------ synthetic chimeric assemblies
def make_case(n_ctg, n_pairs, seed, res, min_len=30_000, max_len=400_000, chimera_share=0.3):
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_len, max_len, n_ctg).astype(np.int64)
    lens[0] = 3 * res - 1                                         # a contig of three bins: too short for two counting runs
    pieces = []                                                   # per contig: list of (start, end) the pairs stay inside
    for c in range(n_ctg):
        n = int(lens[c])
        if c and rng.random() < chimera_share and n > 60 * res:
            k = int(rng.integers(1, 3))
            cuts = np.sort(rng.choice(np.arange(20, n // res - 20), k, replace=False)) * res
            gap = int(rng.integers(0, 4)) * res                   # 0: pairs reach up to the joint; > 0: bins without any coverage
            bounds = [0] + cuts.tolist() + [n]
            pieces.append([(bounds[t] + (gap if t else 0), bounds[t + 1]) for t in range(k + 1)])
        else:
            pieces.append([(0, n)])
    weight = lens / lens.sum()
    ctg = rng.choice(n_ctg, n_pairs, p=weight).astype(np.int32)
    id1, id2 = ctg.copy(), ctg.copy()
    pos1, pos2 = np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int32)
    span = rng.exponential(8 * res, n_pairs).astype(np.int64)
    u = rng.random(n_pairs)
    leak = rng.random(n_pairs) < 0.004                            # a few pairs ignore the joints
    for c in range(n_ctg):
        idx = np.flatnonzero(ctg == c)
        if not len(idx):
            continue
        pc = pieces[c]
        which = rng.integers(0, len(pc), len(idx))
        lo_b = np.array([p[0] for p in pc])[which]
        hi_b = np.array([p[1] for p in pc])[which]
        lk = leak[idx] & (len(pc) > 1)
        lo_b = np.where(lk, 0, lo_b)
        hi_b = np.where(lk, int(lens[c]), hi_b)
        a = lo_b + (u[idx] * (hi_b - lo_b)).astype(np.int64)
        b = np.minimum(a + span[idx], hi_b - 1)
        swap = rng.random(len(idx)) < 0.5
        pos1[idx] = np.where(swap, b, a)
        pos2[idx] = np.where(swap, a, b)
    # inter-contig pairs, names outside the FASTA (-1), filtered BAM records (-2), a position beyond the contig's end
    other = rng.random(n_pairs)
    id2[other < 0.10] = rng.integers(0, n_ctg, int((other < 0.10).sum()))
    id1[(other >= 0.10) & (other < 0.12)] = -1
    both = (other >= 0.12) & (other < 0.13)
    id1[both] = -2
    id2[both] = -2
    far = np.flatnonzero((other >= 0.13) & (other < 0.131) & (id1 == id2) & (id1 >= 0))
    pos2[far] = (lens[id1[far]] + 5 * res).astype(np.int32)
    return lens, id1, pos1, id2, pos2


def table_state(table, names):
    off, nb, length, po = table.segments()
    flat, pairs = table.coverage(), table.pairs()
    cov = {n: flat[o:o + k] for n, o, k in zip(names, off.tolist(), nb.tolist())}
    pos = {n: pairs[2 * a:2 * b].tolist() for n, a, b in zip(names, po[:-1].tolist(), po[1:].tolist())}
    return cov, pos, dict(zip(names, length.tolist()))


def run_rounds(lens, arrays, res, ratios, n_rounds, batches=3, on_device=False):
    """device table and restatement side by side; every round's break points, coverage and position lists must agree"""
    import torch
    from haphic_amd import _lib
    id1, pos1, id2, pos2 = arrays
    table = _lib.CorrectTable(lens, res)
    cuts = np.linspace(0, len(id1), batches + 1).astype(np.int64)
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if on_device:
            dev = [torch.from_numpy(np.ascontiguousarray(x[a:b])).to('cuda:0') for x in arrays]
            torch.cuda.synchronize()
            table.push_device(b - a, *[t.data_ptr() for t in dev])
            _lib.check(_lib.load().hhx_synchronize())
        else:
            table.push(id1[a:b], pos1[a:b], id2[a:b], pos2[a:b])
    kept = table.finalize()
    rcov, rpos = ref_pass_one(lens.tolist(), res, id1, pos1, id2, pos2)
    assert kept == sum(len(p) for p in rpos) // 2 > 0
    names = ['c%d' % k for k in range(len(lens))]
    ref = {n: (rcov[k], rpos[k], int(lens[k]), 0) for k, n in enumerate(names)}      # (coverage, positions, length, start on the original contig)
    stats = []
    for rnd in range(n_rounds):
        cov, pos, length = table_state(table, names)
        assert list(cov) == list(ref)
        for n in names:
            assert np.array_equal(cov[n], ref[n][0]), (rnd, n)
            assert pos[n] == list(ref[n][1]), (rnd, n)
            assert length[n] == ref[n][2], (rnd, n)
        want = {}
        for n in names:
            bp = ref_detect(ref[n][0], ref[n][2], res, *ratios)
            if bp:
                want[n] = bp
        n_bp, bcov, bins = table.detect(*ratios)
        got, at = {}, 0
        for s in np.flatnonzero(n_bp).tolist():
            got[names[s]] = [(int(b) * res, int(bcov[s])) for b in bins[at:at + n_bp[s]]]
            at += int(n_bp[s])
        assert got == want and list(got) == list(want), (rnd, sorted(set(got) ^ set(want))[:5])
        stats.append((len(want), sum(1 for v in want.values() if v[0][1] == 0), sum(1 for v in want.values() if len(v) > 1)))
        if not want:
            break
        seg, bp_off, bp_pos, zero, new_ref = [], [0], [], [], {}
        for n, points in want.items():
            seg.append(names.index(n))
            bp_pos.extend(p for p, _c in points)
            bp_off.append(len(bp_pos))
            lose = ref[n][3] != 0                                 # a piece that does not start its original contig
            zero.append(int(points[0][1] == 0) | (2 if lose else 0))
            bounds = [0] + [p for p, _c in points] + [ref[n][2]]
            for t, (piece, kid) in enumerate(ref_break(ref[n][0], ref[n][1], points, res, lose)):
                new_ref['%s:%d-%d' % (n, bounds[t] + 1, bounds[t + 1])] = (piece, kid, bounds[t + 1] - bounds[t], ref[n][3] + bounds[t])
        table.break_(seg, bp_off, bp_pos, zero)
        ref, names = new_ref, list(new_ref)
    table.destroy()
    return stats


def test_rounds_small_case_host_and_device_push():
    res = 500
    lens, *arrays = make_case(60, 300_000, seed=11, res=res)
    ratios = (0.2, 0.1, 5000)
    stats = run_rounds(lens, arrays, res, ratios, 3)
    assert stats[0][0] > 0 and len(stats) > 1 and stats[1][0] > 0, stats                 # something is broken, and again in round two
    assert run_rounds(lens, arrays, res, ratios, 3, batches=1, on_device=True) == stats


@pytest.mark.parametrize('res,ratios', [(500, (0.2, 0.1, 5000)), (2000, (0.35, 0.05, 12000))])
def test_rounds_randomised_large(res, ratios):
    """beyond the toy regime: 2000 contigs / 2 M read pairs, two resolutions, one non-default ratio set"""
    lens, *arrays = make_case(2000, 2_000_000, seed=5 + res, res=res, chimera_share=0.15)
    stats = run_rounds(lens, arrays, res, ratios, 3, batches=2)
    assert stats[0][0] > stats[0][1] > 0, stats                   # zero and non-zero coverage breaks both occur
    assert stats[0][2] > 0 and stats[1][0] > 0, stats             # contigs with several break points at once; contigs broken again in round two


def test_remap_kernel():
    import torch
    from haphic_amd import _lib
    rng = np.random.default_rng(3)
    n_src = 50
    off, pos, new = [0], [], []
    nid = 0
    for s in range(n_src):
        if s % 7 == 3:                                            # a name without an entry
            off.append(len(pos))
            continue
        k = int(rng.integers(1, 4))
        cuts = [0] + sorted(rng.choice(np.arange(1, 200), k - 1, replace=False) * 500)
        order = rng.permutation(k) + nid                          # corrected ids in no particular order
        nid += k
        pos.extend(int(c) for c in cuts)
        new.extend(int(x) for x in order)
        off.append(len(pos))
    n = 200_000
    ids = rng.integers(-2, n_src, n).astype(np.int32)
    xs = rng.integers(0, 120_000, n).astype(np.int32)
    want_id, want_x = ids.copy(), xs.copy()
    for k in range(n):
        s = int(ids[k])
        if s < 0:
            continue
        ent = [(p, c) for p, c in zip(pos[off[s]:off[s + 1]], new[off[s]:off[s + 1]]) if p <= xs[k]]
        want_id[k] = ent[-1][1] if ent else -1
        if ent:
            want_x[k] = xs[k] - ent[-1][0]
    d_id, d_x = torch.from_numpy(ids).to('cuda:0'), torch.from_numpy(xs).to('cuda:0')
    torch.cuda.synchronize()
    remap = _lib.ContigRemap(off, pos, new)
    remap.apply(n, d_id.data_ptr(), d_x.data_ptr())
    _lib.check(_lib.load().hhx_synchronize())
    assert np.array_equal(d_id.cpu().numpy(), want_id) and np.array_equal(d_x.cpu().numpy(), want_x)
    remap.destroy()


def test_wide_contigs_and_negative_positions_are_refused():
    from haphic_amd import _lib
    with pytest.raises(RuntimeError, match='2\\^31'):
        _lib.CorrectTable([1000, 2 ** 31 + 5], 500)
    t = _lib.CorrectTable([10_000], 500)
    with pytest.raises(RuntimeError, match='negative position'):
        t.push([0], [-1], [0], [40])
    t.destroy()


def test_containers_thaw_into_the_reference_types(tmp_path):
    """pass one from a .pairs file through the mirror; touching a container gives dict{name: int32 array} / defaultdict{name: array('i')}"""
    import types
    from collections import defaultdict
    from haphic_amd import correct
    res = 500
    lens, id1, pos1, id2, pos2 = make_case(12, 20_000, seed=2, res=res)
    names = ['ctg%d' % k for k in range(len(lens))]
    path = tmp_path / 'in.pairs'
    with open(path, 'w') as f:
        f.write('## pairs format v1.0\n')
        for k, (a, p, b, q) in enumerate(zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist())):
            f.write('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, names[a] if a >= 0 else 'elsewhere', p + 1, names[b] if b >= 0 else 'elsewhere', q + 1))
    fa_dict = {n: ['', int(l), 1] for n, l in zip(names, lens)}
    args = types.SimpleNamespace(alignments=str(path), aln_format='pairs', correct_resolution=res, median_cov_ratio=0.2, region_len_ratio=0.1,
                                 min_region_cutoff=5000)
    cov_d, pos_d = correct.parse_pairs_for_correction(fa_dict, args)
    assert cov_d.frozen and pos_d.frozen
    bp = correct.detect_break_points(cov_d, fa_dict, args)       # a mirror: nothing thaws
    assert cov_d.frozen and pos_d.frozen
    rcov, rpos = ref_pass_one(lens.tolist(), res, id1, pos1, id2, pos2)
    want_bp = {n: ref_detect(rcov[k], int(lens[k]), res, 0.2, 0.1, 5000) for k, n in enumerate(names)}
    assert bp == {n: v for n, v in want_bp.items() if v}
    keys = list(cov_d)                                           # anything else: both thaw
    assert keys == names and not cov_d.frozen and not pos_d.frozen
    assert isinstance(cov_d, dict) and isinstance(pos_d, defaultdict)
    for k, n in enumerate(names):
        assert cov_d[n].dtype == np.int32 and np.array_equal(cov_d[n], rcov[k])
    assert list(pos_d) == [n for k, n in enumerate(names) if rpos[k]]
    for k, n in enumerate(names):
        if rpos[k]:
            assert isinstance(pos_d[n], array) and pos_d[n].typecode == 'i' and pos_d[n].tolist() == rpos[k]
    assert pos_d['nobody'] == array('i')                         # the default factory of :1308


def _pass_two_case(tmp_path, n_pairs=40_000, seed=9):
    """an assembly of 20 contigs of which 5 were broken into 2-3 pieces: the .pairs / BAM records name the ORIGINAL contigs"""
    rng = np.random.default_rng(seed)
    orig = ['ctg%02d' % k for k in range(20)]
    lens = rng.integers(60_000, 300_000, len(orig))
    fpos, ffrag, fa = {}, {}, {}
    for k, n in enumerate(orig):
        if k % 4 != 1:
            fa[n] = ['', int(lens[k]), 1]
    for k, n in enumerate(orig):
        if k % 4 == 1:
            cuts = [0] + sorted((rng.choice(np.arange(10, lens[k] // 500 - 10), int(rng.integers(1, 3)), replace=False) * 500).tolist()) + [int(lens[k])]
            names = ['%s:%d-%d' % (n, a + 1, b) for a, b in zip(cuts[:-1], cuts[1:])]
            for name, a, b in zip(names, cuts[:-1], cuts[1:]):
                fa[name] = ['', b - a, 1]
            fpos[n], ffrag[n] = cuts[:-1][::-1], names[::-1]       # descending, as break_and_update_ctgs leaves them
    id1 = rng.integers(-1, len(orig), n_pairs)
    id2 = np.where(rng.random(n_pairs) < 0.4, id1, rng.integers(-1, len(orig), n_pairs))
    pos1 = (rng.random(n_pairs) * lens[np.maximum(id1, 0)]).astype(np.int64)
    pos2 = (rng.random(n_pairs) * lens[np.maximum(id2, 0)]).astype(np.int64)
    cid = {n: i for i, n in enumerate(fa)}

    def convert(i, x):                                            # convert_ctg :1405-1411, then `ref not in fa_dict`
        if i < 0:
            return -1, x
        n = orig[i]
        if n in ffrag:
            for p, f in zip(fpos[n], ffrag[n]):
                if x - p >= 0:
                    return cid[f], x - p
        return cid[n], x
    conv = [convert(i, x) + convert(j, y) for i, x, j, y in zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist())]
    want = [np.array(c, np.int64) for c in zip(*conv)]
    return orig, lens, fa, fpos, ffrag, (id1, pos1, id2, pos2), want


@pytest.mark.parametrize('inter_only', [False, True])
def test_pass_two_remaps_between_front_end_and_ingest(tmp_path, monkeypatch, inter_only):
    """pairs_generator_for_correction(_ctg) / bam_generator_for_correction(_ctg) through the device ingest == the ingest of the same records
    converted on the host; alignments.bed keeps the original names and coordinates (:1429)"""
    from haphic_amd import _lib, cluster, correct
    from tests import bam_fixture
    monkeypatch.chdir(tmp_path)
    orig, lens, fa, fpos, ffrag, (id1, pos1, id2, pos2), want = _pass_two_case(tmp_path)
    name_of = lambda i: orig[i] if i >= 0 else 'elsewhere'        # noqa: E731
    lines = ['r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, name_of(a), p + 1, name_of(b), q + 1)
             for k, (a, p, b, q) in enumerate(zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist()))]
    with open('in.pairs', 'w') as f:
        f.write('## pairs format v1.0\n' + ''.join(lines))
    refs = [(n, int(l)) for n, l in zip(orig, lens)] + [('elsewhere', 1000)]
    recs = [(a if a >= 0 else len(orig), int(p), b if b >= 0 else len(orig), int(q), 0x41) for a, p, b, q in
            zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist())]
    recs += [(0, 5, 0, 900, 0x81)] * 50                           # read2 records: filtered by flag.read1
    with open('in.bam', 'wb') as f:
        f.write(bam_fixture.bam_bytes(refs, recs))
    table = cluster.FragTable.from_reference(fa, {n: v[1] for n, v in fa.items()}, set())
    host = cluster.IdArrays(list(fa), want[0], want[1], want[2], want[3])
    host.inter_only = inter_only
    ref = cluster.ingest_links(host, table, 20_000, False)
    gen_p = correct.pairs_generator_for_correction_ctg if inter_only else correct.pairs_generator_for_correction
    gen_b = correct.bam_generator_for_correction_ctg if inter_only else correct.bam_generator_for_correction
    routes = {'pairs': gen_p('in.pairs', 'pairs', fpos, ffrag), 'bam': gen_b('in.bam', 2, [b'filter=flag.read1'], fpos, ffrag)}
    for route, alignments in routes.items():
        assert alignments.multi_rank() is False
        got = cluster.ingest_links(alignments, table, 20_000, False)
        assert set(got) == set(ref)
        for key in ref:
            assert np.array_equal(got[key], ref[key]), (route, key)
        assert len(ref['full_cnt']) > 50
    _lib.files_join()
    bed = ''.join('%s\t%d\t%d\tr%d/1\t255\t.\n%s\t%d\t%d\tr%d/2\t255\t.\n' % (name_of(a), p, p, k, name_of(b), q, q, k)
                  for k, (a, p, b, q) in enumerate(zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist())))
    assert open('alignments.bed').read() == bed


def test_bam_route_of_pass_one_equals_the_pairs_route(tmp_path, monkeypatch):
    import types
    from haphic_amd import correct
    from tests import bam_fixture
    monkeypatch.chdir(tmp_path)
    res = 500
    lens, id1, pos1, id2, pos2 = make_case(15, 30_000, seed=4, res=res)
    ok = id1 != -2                                                # -2 stands for records the BAM filter drops: written as read2 below
    names = ['ctg%d' % k for k in range(len(lens))]
    name_of = lambda i: names[i] if i >= 0 else 'elsewhere'       # noqa: E731
    with open('in.pairs', 'w') as f:
        for k in np.flatnonzero(ok).tolist():
            f.write('r%d\t%s\t%d\t%s\t%d\t+\t-\n' % (k, name_of(id1[k]), pos1[k] + 1, name_of(id2[k]), pos2[k] + 1))
    refs = [(n, int(l)) for n, l in zip(names, lens)] + [('elsewhere', 1000)]
    far = len(names)
    recs = [((a if a >= 0 else far) if g else 0, int(p), (b if b >= 0 else far) if g else 0, int(q), 0x41 if g else 0x81)
            for a, p, b, q, g in zip(id1.tolist(), pos1.tolist(), id2.tolist(), pos2.tolist(), ok.tolist())]
    with open('in.bam', 'wb') as f:
        f.write(bam_fixture.bam_bytes(refs, recs))
    fa_dict = {n: ['', int(l), 1] for n, l in zip(names, lens)}
    out = {}
    for fmt, path in (('pairs', 'in.pairs'), ('bam', 'in.bam')):
        args = types.SimpleNamespace(alignments=path, aln_format=fmt, threads=2, correct_resolution=res)
        cov_d, pos_d = (correct.parse_bam_for_correction if fmt == 'bam' else correct.parse_pairs_for_correction)(fa_dict, args)
        out[fmt] = ({n: v.tolist() for n, v in cov_d.items()}, {n: v.tolist() for n, v in pos_d.items()})
    assert out['pairs'] == out['bam'] and list(out['pairs'][1]) == list(out['bam'][1])
    rcov, rpos = ref_pass_one(lens.tolist(), res, id1, pos1, id2, pos2)
    assert out['pairs'][0] == {n: rcov[k].tolist() for k, n in enumerate(names)}
    assert out['pairs'][1] == {n: rpos[k] for k, n in enumerate(names) if rpos[k]}
    assert not os.path.exists('alignments.bed')                  # pass one writes no BED (:1319-1342)


def test_reference_fixture(tmp_path):
    """tests/golden/correction.npz — the reference's own parse_pairs_for_correction, correct_assembly (every round), final_break_* dicts, corrected
    contig table, corrected_ctgs.txt, and the pass-two containers and alignments.bed of the contig and --bin_size variants — on the device"""
    from haphic_amd import _lib
    from tests import correction_fixture
    correction_fixture.check_against_mirrors(correction_fixture.load(), str(tmp_path), files_join=_lib.files_join)


def test_wave_merged_atomics_give_the_same_table():
    """the "correct_agg" knob (the adds of a wave merged before they leave it): same coverage, same position lists, on a stream in random
    order and on one grouped by contig, where the lanes of a wave do hit the same words"""
    from haphic_amd import _lib
    res = 500
    lens, id1, pos1, id2, pos2 = make_case(80, 400_000, seed=21, res=res)
    order = np.argsort(id1, kind='stable')
    for arrays in ((id1, pos1, id2, pos2), tuple(a[order] for a in (id1, pos1, id2, pos2))):
        states = []
        for agg in (0, 1):
            _lib.tune('correct_agg', agg)
            try:
                t = _lib.CorrectTable(lens, res)
                t.push(*arrays)
                kept = t.finalize()
                states.append((kept, t.segments()[3].tolist(), t.coverage().tolist(), t.pairs().tolist()))
                t.destroy()
            finally:
                _lib.tune('correct_agg', None)
        assert states[0] == states[1] and states[0][0] > 0
        rcov, rpos = ref_pass_one(lens.tolist(), res, *arrays)
        assert states[1][2] == np.concatenate(rcov).tolist() and states[1][3] == [x for p in rpos for x in p]
