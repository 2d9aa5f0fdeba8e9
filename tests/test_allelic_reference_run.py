"""HapHiC_cluster.run(args) with --remove_allelic_links N, twice on the same inputs with the seams re-bound: once as patch_reference(H) binds them
(remove_allelic_HiC_links stays the reference's and thaws the containers) and once with patch_reference(H, allelic=True) — every file
compared, and no container thawed on the second run.  Needs the reference checkout (dev container only); tests/allelic_cases.library()
stands in for the HIP library, as tests/oracle_lib.py does in tests/test_reference_run_integration.py, whose input writers are used here."""
import logging
import os
import pickle

import pytest

from tests import allelic_cases
from tests.test_reference_run_integration import REF, _load_reference, _run, _tree, _write_inputs


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference checkout not present')
@pytest.mark.parametrize('split,poly,extra', [(False, False, ['--remove_allelic_links', '2', '--max_read_pairs', '60']),
                                              (False, True, ['--remove_allelic_links', '4', '--max_read_pairs', '40']),
                                              (False, True, ['--remove_allelic_links', '4', '--max_read_pairs', '40', '--normalize_by_nlinks']),
                                              (True, False, ['--bin_size', '40', '--remove_allelic_links', '2', '--max_read_pairs', '40'])])
def test_run_with_the_allelic_seam_writes_the_same_files(tmp_path, monkeypatch, split, poly, extra):
    pytest.importorskip('networkx')
    import haphic_amd
    from haphic_amd import cluster, containers, patch
    H = _load_reference()
    _write_inputs(str(tmp_path), split, poly=poly)
    monkeypatch.setattr(H, 'dot_product_mkl', lambda a, b, **k: (a @ b).tocsc(), raising=False)
    monkeypatch.setattr(H, 'INTEL_MKL', True, raising=False)
    lib = allelic_cases.library()
    monkeypatch.setattr(haphic_amd, '_lib', lib)
    monkeypatch.setattr(cluster, '_lib', lib)
    monkeypatch.setattr(patch, '_lib', lib, raising=False)
    nchrs = 4 if poly else 3
    thawed = []
    real_thaw = containers._Frozen._thaw
    monkeypatch.setattr(containers._Frozen, '_thaw', lambda self: (thawed.append(self._kind), real_thaw(self))[1])
    logs = {}
    for tag, allelic in (('keep', False), ('device', True)):
        msgs = logs[tag] = []
        handler = logging.Handler(logging.INFO)
        handler.emit = lambda rec, sink=msgs: sink.append(rec.getMessage())
        saved = patch.patch_reference(H, allelic=allelic)
        H.logger.addHandler(handler)
        del thawed[:]
        try:
            _run(H, str(tmp_path / tag), extra, nchrs=nchrs)
        finally:
            H.logger.removeHandler(handler)
            patch.unpatch_reference(H, saved)
        assert set(thawed) == ({'full', 'flank', 'crd'} if not allelic else set()), (tag, thawed)
    stable = lambda msgs: [m for m in msgs if 'alleic' in m or 'isolated' in m or 'fragments removed' in m or m.startswith('[')]     # noqa: E731
    assert stable(logs['keep']) == stable(logs['device']) and any('fragments kept' in m for m in logs['device'])
    want, got = _tree(str(tmp_path / 'keep')), _tree(str(tmp_path / 'device'))
    assert sorted(want) == sorted(got) and 'full_links.pkl' in want and any(k.endswith('.clusters.txt') for k in want)
    for k in want:
        if k.endswith('.pkl'):
            a, b = pickle.loads(want[k]), pickle.loads(got[k])
            assert type(a) is type(b) and list(a.items()) == list(b.items()), 'pickle differs: ' + k
            assert [type(v) for v in a.values()] == [type(v) for v in b.values()], 'value types differ: ' + k
        else:
            assert want[k] == got[k], 'file differs: ' + k
