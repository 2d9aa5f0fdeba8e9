"""GPU: the front of `haphic cluster` on the device — _lib.Gfa (csrc/hhx_gfa.hip) on every GFA case of tests/assembly_cases.py, the fragment
statistics and the children of a correction round on the views of a _lib.Fasta — against tests/golden/assembly.npz.  No reference checkout needed;
every comparison is exact."""
import ctypes as C
import gc
import os
import random
import weakref

import numpy as np
import pytest

from haphic_amd import _lib, assembly, cluster
from tests import assembly_cases as ac

pytestmark = pytest.mark.gpu
GOLDEN = ac.golden()
JOBS = ac.gfa_jobs()
COMBOS = ac.fragment_combos()


# ------------------------------------------------------------------ _lib.Gfa
@pytest.fixture(scope='module')
def gfa_files(tmp_path_factory):
    """every file of every job, written once: {(job name, k): path}"""
    root = tmp_path_factory.mktemp('gfa')
    out = {}
    for n, job in enumerate(JOBS):
        d = root / ('job%03d' % n)
        d.mkdir()
        for k, p in enumerate(job.write(str(d))):
            out[(job.name, k)] = str(d / p)
    return out


@pytest.mark.parametrize('grid', (None, 1, 2), ids=['uncapped', 'grid1', 'grid2'])
def test_gfa_tables(grid, gfa_files, monkeypatch):
    """every file from its path and from its bytes: the table the reference's own statements saw, or the refusal — with the grid of every pass
    uncapped and capped at 1 and at 2 workgroups (HHX_GFA_GRID: the grid-stride loops)"""
    if grid is None:
        monkeypatch.delenv('HHX_GFA_GRID', raising=False)
    else:
        monkeypatch.setenv('HHX_GFA_GRID', str(grid))
    served = refused = 0
    for job in JOBS:
        want = GOLDEN['gfa'][job.name]['tables']
        for k, data in enumerate(job.files):
            for source in (gfa_files[(job.name, k)], data):
                where = '%s file %d from %s' % (job.name, k, 'path' if isinstance(source, str) else 'bytes')
                if k in ac.refused_files(job):
                    with pytest.raises(_lib.Gfa.Unsupported, match='hhx_gfa'):
                        _lib.Gfa(source)
                    refused += 1
                    continue
                with _lib.Gfa(source) as g:
                    got = [g.names(), g.lengths.tolist(), g.depths.tolist()]
                assert got == [want[k]['names'], want[k]['lengths'], want[k]['depths']], where
                served += 1
    assert served > 200 and refused > 60


def test_gfa_refusal_leaves_no_handle_and_names_the_line():
    L = _lib.load()
    for text, line, why in ((ac.rec('a', 5, 1) + ac.A_LINE + b'S\tx\t*\tLN:i:5\n' + ac.A_LINE, 3, 'fewer than five fields'),
                            (ac.rec('a', 5, 1) + ac.rec('b', '+5', 1), 2, 'field 3'), (ac.rec('b', 5, '1_0'), 1, 'field 4'),
                            (ac.H_LINE + ac.rec('n' * 256, 5, 1), 2, 'longer than 255'), (ac.rec('a', 5, 1) + b'\x80\n', None, '0x80')):
        buf = np.frombuffer(text, np.uint8)
        h = C.c_void_p(1)
        h.value = None
        assert L.hhx_gfa_open_bytes(_lib.ptr(buf), buf.size, C.byref(h)) == _lib.HHX_UNSUPPORTED and not h.value
        msg = _lib.last_error()
        assert why in msg and (line is None or 'line %d:' % line in msg), msg
    h = C.c_void_p()
    assert L.hhx_gfa_open(os.fsencode(os.path.dirname(os.path.abspath(__file__))), C.byref(h)) == _lib.HHX_UNSUPPORTED and not h.value
    assert L.hhx_gfa_open(b'/no/such/file.gfa', C.byref(h)) == 1 and not h.value
    n = C.c_int64(0)
    assert L.hhx_gfa_counts(None, C.byref(n), C.byref(n)) != 0 and L.hhx_gfa_table(None, None, None, None, None) != 0 and L.hhx_gfa_close(None) == 0


def test_parse_gfa_mirror_on_the_device(tmp_path):
    """the bound seam over _lib.Gfa itself on the jobs of several files and of a mismatch"""
    import logging
    import types
    logger = logging.getLogger('gpu_assembly')
    logger.propagate = False
    parse_gfa = assembly.bind_gfa(types.SimpleNamespace(parse_gfa=lambda *a, **k: 'handed back', logger=logger))
    cwd = os.getcwd()
    for job in JOBS:
        if not job.name.startswith(('files/', 'duplicates/', 'mismatch/', 'sequence/')):
            continue
        d = tmp_path / job.name.replace('/', '_')
        d.mkdir()
        os.chdir(d)
        try:
            want = GOLDEN['gfa'][job.name]
            try:
                got = parse_gfa(job.write('.'), job.fa_dict(), logger=logger)
            except RuntimeError as e:
                assert ['RuntimeError', str(e)] == want['raises'], job.name
                continue
            if ac.refused_files(job):
                assert got == 'handed back', job.name
            else:
                assert [[k, list(v)] for k, v in got.items()] == want['items'], job.name
        finally:
            os.chdir(cwd)


# ------------------------------------------------------------------ the fragment statistics on the views of a _lib.Fasta
def _rows(fa, re_sites):
    return dict(zip(fa.names(), assembly.view_rows(fa, fa.seq_off.tolist(), fa.seq_len.tolist(), re_sites)))


def test_fragment_statistics_on_the_device():
    """the cross product of bin sizes, flanks, Nx, whitelist, read depths and RE strings through stat_fragments on views of one resident genome:
    the seven return values, fa_dict, read_depth_dict, the log and the random module's next number are the reference's; the handle goes with
    the last row"""
    import logging
    text, names, lengths = ac.genome()
    fa = _lib.Fasta(text)
    assert fa.names() == names and fa.seq_len.tolist() == lengths
    sites = {RE: (fa.re_counts_device(cluster._sites_of(RE)) + 1).tolist() for RE in ac.RES}
    for RE in ac.RES:
        assert [[n, l, s] for n, l, s in zip(names, lengths, sites[RE])] == GOLDEN['fragments']['__fa__'][RE]
    logger = logging.getLogger('gpu_assembly_stat')
    logger.propagate = False
    logger.setLevel(logging.DEBUG)
    records = []
    handler = logging.Handler()
    handler.emit = lambda r: records.append([r.levelname, r.getMessage()])
    logger.handlers[:] = [handler]
    fa_dict = None
    for key, RE, bin_size, flank, Nx, whitelist, with_depth in COMBOS:
        fa_dict = _rows(fa, sites[RE])
        depth = ac.depth_dict(names) if with_depth else {}
        del records[:]
        random.seed(99)
        result = cluster.stat_fragments(fa_dict, RE, depth, whitelist, nchrs=ac.NCHRS, flank=flank, Nx=Nx, bin_size=bin_size, logger=logger)
        got = ac.plain_stat(result, fa_dict, depth)
        got['log'], got['random'] = list(records), random.random()
        assert got == GOLDEN['fragments'][key], key
        assert all(row.view is None for row in fa_dict.values())
    gone = weakref.ref(fa)
    del fa, fa_dict, result
    gc.collect()
    assert gone() is None                                            # nothing but the rows held the handle: its finaliser has closed it


def test_children_of_a_round_are_counted_in_one_call(monkeypatch):
    """the children of every broken contig as views of their parents' views: one hhx_fasta_re_counts call for all of them, equal to str.count on
    the slices fetched from the device"""
    import types
    from haphic_amd import correct
    text, names, lengths = ac.genome()
    fa = _lib.Fasta(text)
    calls = []
    real = _lib.Fasta.re_counts_device
    monkeypatch.setattr(_lib.Fasta, 're_counts_device', lambda self, *a, **k: (calls.append(len(a[1])), real(self, *a, **k))[1])
    fa_dict = _rows(fa, [0] * len(names))
    points = {'c00': [(4096, 3), (100000, 3), (249999, 3)], 'c02': [(1, 3)], 'c04': [(15, 0), (16, 0), (17, 0)], 'c11': [(2000, 2)]}
    src, fpos, ffrag = {c: c for c in points}, {c: [0] for c in points}, {c: [c] for c in points}
    args = types.SimpleNamespace(RE='GATC,AAGCTT,GANTC')
    kids = correct.update_bookkeeping(points, src, fpos, ffrag, fa_dict, {}, set(names), args)
    n_kids = sum(len(v) for v in kids.values())
    assert calls == [n_kids] and n_kids == 4 + 2 + 4 + 2
    whole = fa.sequences().tobytes().decode()
    off = dict(zip(names, fa.seq_off.tolist()))
    sites = [s.decode() for s in cluster._sites_of(args.RE)]
    for parent, children in kids.items():
        assert parent not in fa_dict
        for child in children:
            s, e = (int(x) for x in child.rsplit(':', 1)[1].split('-'))
            row = fa_dict[child]
            piece = whole[off[parent] + s - 1:off[parent] + e]
            assert row.view == (fa, off[parent] + s - 1, e - s + 1) and row[1] == len(piece) and row[2] == sum(piece.count(x) for x in sites), child
            assert row[0] == piece and row.view is not None, child
    # a second round on a child
    kids2 = correct.update_bookkeeping({'c00:4097-100000': [(50000, 3)]}, src, fpos, ffrag, fa_dict, {}, set(names) - set(points), args)
    assert calls[1:] == [2] and kids2 == {'c00:4097-100000': ['c00:4097-54096', 'c00:54097-100000']}
    row = fa_dict['c00:54097-100000']
    assert row[0] == whole[54096:100000] and row[2] == sum(row[0].count(x) for x in sites)
