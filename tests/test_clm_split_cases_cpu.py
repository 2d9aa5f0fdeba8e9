"""CPU: the CLM-split corpus (tests/clm_split_cases.py) against the golden fixture the reference's split_clm_file wrote, the host mirror of
the device's state machine against the contract, the wrapper haphic_amd.reassign.split_clm_file over a stand-in splitter, and the
`reassign` command of python -m haphic_amd.  No GPU; the reference checkout is used where it exists."""
import os
import sys
import types

import numpy as np
import pytest

from tests import clm_split_cases as cc
from tests.conftest import load_golden

REF = '/root/reference/scripts'


@pytest.fixture(scope='module')
def golden():
    return load_golden('clm_split.npz')


def test_corpus_is_deterministic_and_in_domain():
    first = [(c.section, c.name, c.text, tuple(c.names), tuple(c.group_of_name), c.n_groups, c.kind) for c in cc.cases()]
    cc.section.cache_clear()
    again = [(c.section, c.name, c.text, tuple(c.names), tuple(c.group_of_name), c.n_groups, c.kind) for c in cc.cases()]
    assert first == again and len({(s, n) for s, n, *_ in first}) == len(first)
    assert {c.section for c in cc.cases()} == {name for name, _ in cc.SECTIONS}
    for c in cc.cases():                                              # (the domain check itself runs when a case is built)
        assert (c.want is IndexError) == (c.kind == 'error'), c
    assert sum(c.small for c in cc.cases(cc.SMALL_SECTIONS)) >= 40
    assert cc.file_text() == cc.file_text() and cc.long_line_text(True) == cc.long_line_text(True)


def test_split_spec_reproduces_the_golden_fixture(golden):
    cases = cc.golden_cases(golden)
    ours = {'%s/%s' % (c.section, c.name): c for c in cc.cases()}
    assert len(cases) > 50 and sum(w is IndexError for *_, w in cases) >= 12
    for name, text, names, group, G, want in cases:
        assert ours[name].text == text and ours[name].names == names, name      # the fixture was made from this corpus
        try:
            got = cc.split_spec(text, names, group, G)
        except IndexError as e:
            assert str(e) == 'list index out of range'
            got = IndexError
        assert got == want, name


@pytest.mark.parametrize('size', [None, 1, 2, 3, 7, 64])
def test_host_mirror_of_the_state_machine_equals_the_contract(size):
    """simulate() — the held '\\r', the carried head, continuation segments — gives split_spec's bytes for every way of cutting the text"""
    for c in cc.cases(cc.SMALL_SECTIONS) + [cc.size_case(L, 3, 'src') for L in cc.SIZE_LENGTHS if size in (None, 64)]:
        try:
            got, stat = cc.simulate([c.text] if size is None else cc.pushes(c.text, size), *c.args())
        except IndexError:
            got = IndexError
        assert got == c.want, (c, size)


def test_host_mirror_reaches_every_counter():
    seen = dict.fromkeys(cc.STATS, 0)
    for c in cc.cases(cc.SMALL_SECTIONS, 'ok'):
        for size in (None, 1, 7):
            for k, v in cc.simulate([c.text] if size is None else cc.pushes(c.text, size), *c.args())[1].items():
                seen[k] += v
    for c in (cc.size_case(cc.GATHER_TILE + 1, 0, 'dst'),):
        for k, v in cc.simulate([c.text], *c.args())[1].items():
            seen[k] += v
    assert all(seen.values()), seen


def test_head_bound_is_a_refusal():
    for size in (None, 4096, 65536, 1000):                            # wherever the cuts fall
        with pytest.raises(RuntimeError, match='first two tokens'):
            cc.simulate([cc.head_bound_text()] if size is None else cc.pushes(cc.head_bound_text(), size), cc.NAMES3, cc.GROUP3, 3)
    ok = b'ctgA+' + b' ' * (cc.HEAD_MAX - 12) + b'ctgB- 1 5\n'          # the second token ends on byte HEAD_MAX - 1: inside the bound
    assert cc.simulate(cc.pushes(ok, 4096), ['ctgA', 'ctgB'], [0, 0], 1)[0] == [ok]


@pytest.fixture(scope='module')
def reference():
    if not os.path.isdir(REF):
        pytest.skip('reference checkout not present')
    from tests.golden import make_golden_clm_split as mk
    return mk, mk.load_reference_reassign(REF)


def test_live_reference_agrees_on_every_case(reference):
    mk, R = reference
    for c in cc.cases(cc.SMALL_SECTIONS) + [cc.size_case(cc.TX_BLOCK - 1, 9, 'dst')]:
        tree = mk.run_reference(R, c.text, *mk.case_dicts(c))
        if c.want is IndexError:
            assert tree is IndexError, c
        else:
            assert [tree['split_clms/g%d.clm' % g][1] for g in range(c.n_groups)] == c.want, c


@pytest.mark.parametrize('line', [b'\n', b' \t\x0b\n', b'ctgA+\n', b'\r'])
def test_live_reference_raises_on_the_four_blank_shapes(reference, line):
    mk, R = reference
    text = b'ctgA+ ctgB- 1 5\n' + line + b'ctgA+ ctgB- 1 6\n'
    assert mk.run_reference(R, text, {'g0': [set(), 0]}, {'ctgA': 'g0', 'ctgB': 'g0'}) is IndexError
    with pytest.raises(IndexError):
        cc.split_spec(text, ['ctgA', 'ctgB'], [0, 0], 1)


# ------------------------------------------------------------------ the wrapper
def spec_splitter(calls):
    def split(clm_file, names, group_of_name, paths):
        calls.append((clm_file, list(names), list(group_of_name), list(paths)))
        with open(clm_file, 'rb') as f:
            outs = cc.split_spec(f.read(), names, group_of_name, len(paths))
        for p, data in zip(paths, outs):
            with open(p, 'wb') as f:
                f.write(data)
    return split


def test_wrapper_over_a_stand_in_splitter_leaves_the_reference_tree(golden, tmp_path, monkeypatch, caplog):
    from haphic_amd import reassign
    calls = []
    monkeypatch.setattr(reassign, '_device_split', spec_splitter(calls))
    text, group_ctg_dict, ctg_group_dict, subdir = cc.seam_inputs()
    clm = tmp_path / 'paired_links.clm'
    clm.write_bytes(text)
    run = tmp_path / 'run'
    run.mkdir()
    monkeypatch.chdir(run)
    with caplog.at_level('INFO', logger='HapHiC_reassign'):
        assert reassign.split_clm_file(str(clm), group_ctg_dict, ctg_group_dict, subdir) is None
    assert 'Splitting clm file into subfiles by group...' in caplog.text
    assert cc.read_tree(str(run)) == cc.golden_tree(golden)
    assert len(calls) == 1 and calls[0][3] == ['split_clms/%s.clm' % g for g in group_ctg_dict]
    # 'hc_groups' gives the other prefix; anything else is the reference's AssertionError, after final_groups/ was made
    run2 = tmp_path / 'run2'
    run2.mkdir()
    monkeypatch.chdir(run2)
    reassign.split_clm_file(str(clm), group_ctg_dict, ctg_group_dict, 'hc_groups')
    assert os.readlink('final_groups/group1.txt') == '../hc_groups/hc_group1.txt' and os.readlink('final_groups/final_clusters.txt') == '../hc_groups/hc_clusters.txt'
    run3 = tmp_path / 'run3'
    run3.mkdir()
    monkeypatch.chdir(run3)
    with pytest.raises(AssertionError):
        reassign.split_clm_file(str(clm), group_ctg_dict, ctg_group_dict, 'elsewhere')
    assert os.listdir('.') == ['final_groups']


@pytest.mark.parametrize('what', ['group_without_entry', 'empty_name', 'name_not_str'])
def test_wrapper_hands_the_reference_its_own_error_paths(what, tmp_path, monkeypatch):
    from haphic_amd import reassign
    monkeypatch.setattr(reassign, '_device_split', lambda *a: pytest.fail('the device splitter was called'))
    group_ctg_dict = {'g1': [{'a', 'b'}, 2]}
    ctg_group_dict = {'a': 'g1', 'b': 'g1'}
    if what == 'group_without_entry':
        ctg_group_dict['c'] = 'g2'
    elif what == 'empty_name':
        ctg_group_dict[''] = 'g1'
    else:
        ctg_group_dict[7] = 'g1'
    monkeypatch.chdir(tmp_path)
    seen = []
    assert reassign.split_clm_file('x.clm', group_ctg_dict, ctg_group_dict, 'hc_groups', _original=lambda *a: seen.append(a) or 'theirs') == 'theirs'
    assert seen == [('x.clm', group_ctg_dict, ctg_group_dict, 'hc_groups')] and os.listdir('.') == []      # handed over before anything was created
    with pytest.raises(ValueError):
        reassign.split_clm_file('x.clm', group_ctg_dict, ctg_group_dict, 'hc_groups')
    assert os.listdir('.') == []


def test_patch_reassign_rebinds_both_seams():
    from haphic_amd import build, cluster, patch, reassign
    build.build()
    R = types.ModuleType('HapHiC_reassign_stub')
    R.parse_link_dict = lambda link_dict, ctg_group_dict, normalize_by_nlinks=False: 'theirs'
    R.split_clm_file = lambda clm_file, group_ctg_dict, ctg_group_dict, subdir: ('theirs', clm_file, subdir)
    originals = (R.parse_link_dict, R.split_clm_file)
    saved = patch.patch_reassign(R)
    assert saved == {'parse_link_dict': originals[0], 'split_clm_file': originals[1]}
    assert R.parse_link_dict.__wrapped__ is cluster.parse_link_dict and R.split_clm_file.__wrapped__ is reassign.split_clm_file
    import inspect
    assert [p for p in inspect.signature(reassign.split_clm_file).parameters if not p.startswith('_')] == ['clm_file', 'group_ctg_dict', 'ctg_group_dict', 'subdir']
    assert R.split_clm_file('f.clm', {}, {'a': 'nowhere'}, 'hc_groups') == ('theirs', 'f.clm', 'hc_groups')       # the KeyError path is the reference's


# ------------------------------------------------------------------ the command line
def run_main(argv):
    from haphic_amd import __main__ as cli
    with pytest.raises(SystemExit) as e:
        cli.main(list(argv))
    return str(e.value)


def test_reassign_is_a_command_now(monkeypatch):
    monkeypatch.delenv('HAPHIC_REFERENCE', raising=False)
    assert 'HapHiC checkout not found' in run_main(['reassign', '--reference', '/nonexistent'])
    assert '--gpus is a flag of the "cluster" step only' in run_main(['reassign', '--gpus', '2', '--reference', '/nonexistent'])
    from haphic_amd import __main__ as cli
    assert 'python -m haphic_amd reassign' in cli.__doc__


def test_plot_and_cluster_behave_as_before(monkeypatch):
    monkeypatch.delenv('HAPHIC_REFERENCE', raising=False)
    assert 'HapHiC checkout not found' in run_main(['plot', '--reference', '/nonexistent'])
    assert 'HapHiC checkout not found' in run_main(['cluster', '--reference', '/nonexistent'])
    assert '--gpus is a flag of the "cluster" step only' in run_main(['plot', '--gpus', '2'])
    msg = run_main(['sort'])
    assert 'steps only' in msg and "'sort'" in msg and 'HapHiC checkout' not in msg
