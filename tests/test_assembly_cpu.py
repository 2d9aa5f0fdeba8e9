"""CPU: the front of `haphic cluster` — parse_fasta, parse_gfa, stat_fragments and the bookkeeping of --correct_nrounds on rows whose sequences
stay with the engine — through the host stand-ins of tests/assembly_cases.py, against tests/golden/assembly.npz (the reference's own functions
wrote it) and, where the checkout is present, against those functions themselves."""
import gc
import hashlib
import importlib.util
import logging
import os
import random
import sys
import types

import numpy as np
import pytest

from haphic_amd import assembly, cluster, containers, correct, patch
from tests import assembly_cases as ac
from tests import correction_fixture
from tests import oracle_lib

REF = '/root/reference/scripts'
HAVE_REF = os.path.isdir(REF)
needs_reference = pytest.mark.skipif(not HAVE_REF, reason='reference checkout not present')
GOLDEN = ac.golden()
JOBS = ac.gfa_jobs()
COMBOS = ac.fragment_combos()


# ------------------------------------------------------------------ helpers
class _Records(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.items = []

    def emit(self, record):
        self.items.append([record.levelname, record.getMessage()])


def _logger(name='assembly_cpu'):
    logger = logging.getLogger(name)
    logger.handlers[:] = []
    logger.propagate = False
    logger.setLevel(logging.DEBUG)
    handler = _Records()
    logger.addHandler(handler)
    return logger, handler.items


_PRIVATE = []


def _reference():
    """HapHiC_cluster.py under a private module name, with the interval stand-in of tests/golden/make_golden_correction.py where `portion` is absent"""
    if _PRIVATE:
        return _PRIVATE[0]
    spec = importlib.util.spec_from_file_location('_make_golden_correction_for_assembly', os.path.join(ac.HERE, 'golden', 'make_golden_correction.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    added = []
    for name, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}),
                        ('portion', {'closed': lambda a, b: gen.Iv([(a, b)]), 'empty': lambda: gen.Iv()})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
            added.append(name)
    shared = {k: sys.modules.pop(k) for k in list(sys.modules) if k.startswith('HapHiC_') or k == '_version'}
    spec = importlib.util.spec_from_file_location('_haphic_cluster_assembly_private', os.path.join(REF, 'HapHiC_cluster.py'))
    H = importlib.util.module_from_spec(spec)
    sys.path.insert(0, REF)
    try:
        spec.loader.exec_module(H)
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k.startswith('HapHiC_') or k == '_version'] + added:
            del sys.modules[k]
        sys.modules.update(shared)
    H.closed, H.empty = (lambda a, b: gen.Iv([(a, b)])), (lambda: gen.Iv())
    H.logger.setLevel(logging.CRITICAL)
    _PRIVATE.append(H)
    return H


class _Original:
    """an original function that must be reached exactly once, before any log record"""

    def __init__(self, records):
        self.records, self.calls = records, []

    def __call__(self, *args, **kwargs):
        assert self.records == [], 'logged before the call was handed back'
        self.calls.append((args, kwargs))
        return 'handed back'


def _run_gfa(parse_gfa, job, directory, logger):
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        paths = job.write('.')
        try:
            got = parse_gfa(paths, job.fa_dict(), logger=logger)
        except Exception as e:      # noqa: BLE001 — compared with the reference's
            return {'raises': [type(e).__name__, str(e)]}
        return {'items': [[k, list(v)] for k, v in got.items()]} if isinstance(got, dict) else got
    finally:
        os.chdir(cwd)


# ------------------------------------------------------------------ 1. the GFA reader's stand-in and the mirror of parse_gfa
def test_cases_are_the_fixture_s():
    assert sorted(GOLDEN['gfa']) == sorted(j.name for j in JOBS)
    for job in JOBS:
        assert GOLDEN['gfa'][job.name]['digest'] == job.digest(), job.name
    assert GOLDEN['fragments']['__digest__'] == hashlib.sha256(ac.genome()[0]).hexdigest()
    assert sorted(k for k in GOLDEN['fragments'] if not k.startswith('__')) == sorted(c[0] for c in COMBOS)


@pytest.mark.parametrize('job', JOBS, ids=repr)
def test_host_reader_gives_the_reference_s_tables(job, tmp_path):
    """HostGfa from a path and from bytes: the names and integers the reference's own statements saw, refusals where the header says so, and
    never an answer where Python raises"""
    want = GOLDEN['gfa'][job.name]['tables']
    paths = job.write(str(tmp_path))
    for k, data in enumerate(job.files):
        for source in (os.path.join(str(tmp_path), paths[k]), data):
            try:
                g = ac.HostGfa(source)
            except ac.HostGfa.Unsupported:
                assert k in ac.refused_files(job), 'refused: file %d' % k
                continue
            assert k not in ac.refused_files(job) and 'raises' not in want[k]
            assert [g.names(), g.lengths.tolist(), g.depths.tolist()] == [want[k]['names'], want[k]['lengths'], want[k]['depths']]


@pytest.mark.parametrize('job', JOBS, ids=repr)
def test_parse_gfa_mirror_against_the_fixture(job, tmp_path):
    """the bound seam: dict values and order, log records and exception texts are the reference's; a job with a refused file reaches the original
    function exactly once, before anything is logged, and returns what it returns"""
    logger, records = _logger()
    original = _Original(records)
    M = types.SimpleNamespace(parse_gfa=original, logger=logger)
    got = _run_gfa(assembly.bind_gfa(M, ac.HostGfa), job, str(tmp_path), logger)
    want = GOLDEN['gfa'][job.name]
    if ac.refused_files(job):
        assert got == 'handed back' and len(original.calls) == 1 and records == []
        args, kwargs = original.calls[0]
        assert args[0] == ['f%d.gfa' % k for k in range(len(job.files))] and list(args[1]) == list(job.fa) and (args[2:] + (kwargs.get('logger'),))[0] is logger
    else:
        assert original.calls == []
        assert got == {k: want[k] for k in ('items', 'raises') if k in want}
        assert records == want['log']


def test_parse_gfa_hands_back_what_is_no_file(tmp_path):
    logger, records = _logger()
    original = _Original(records)
    parse_gfa = assembly.bind_gfa(types.SimpleNamespace(parse_gfa=original, logger=logger), ac.HostGfa)
    good = tmp_path / 'a.gfa'
    good.write_bytes(ac.rec('utg1', 5, 1))
    for bad in (str(tmp_path / 'missing.gfa'), str(tmp_path), 7):
        assert parse_gfa([str(good), bad], {}, logger) == 'handed back'
    assert len(original.calls) == 3 and records == []


@needs_reference
@pytest.mark.parametrize('job', JOBS, ids=repr)
def test_parse_gfa_live(job, tmp_path):
    """the reference's own parse_gfa on the same files, and the mirror bound around it: results, exceptions and log records equal — for the refused
    files too, where they are Python's own"""
    H = _reference()
    want = GOLDEN['gfa'][job.name]
    logger, records = _logger()
    ref = _run_gfa(H.parse_gfa, job, str(tmp_path), logger)
    assert ref == {k: want[k] for k in ('items', 'raises') if k in want} and records == want['log']      # the fixture is the reference's
    del records[:]
    got = _run_gfa(assembly.bind_gfa(H, ac.HostGfa), job, str(tmp_path), logger)
    assert got == ref and records == want['log']


# ------------------------------------------------------------------ 2. rows with a view
def _source(seq=b'ACGTNacgt'):
    Engine = ac.fasta_engine()
    fa = Engine(b'>x\nAC\n>c\n' + seq + b'\n', keep_letter_case=True)
    return Engine, assembly.Resident(fa), fa


@pytest.mark.parametrize('bulk', (False, True))
def test_view_survives_a_load_and_dies_with_element_0(bulk, monkeypatch):
    monkeypatch.setattr(assembly, 'BULK_FETCH', bulk)
    Engine, source, fa = _source()
    row = assembly.ViewRow(source, 2, 9, 3)
    assert row.view == (fa, 2, 9) and row[1] == 9 and row[2] == 3 and len(row) == 3 and Engine.fetched == [] and Engine.bulk == []
    assert row[0] == 'ACGTNacgt' and list(row) == ['ACGTNacgt', 9, 3] and row.view == (fa, 2, 9)
    assert (Engine.fetched, Engine.bulk) == (([], [11]) if bulk else ([(2, 9)], []))
    row[2] = 5
    assert row.view == (fa, 2, 9)
    row[0] = None
    assert row.view is None and list(row) == [None, 9, 5]
    other = assembly.ViewRow(source, 0, 2, 1)
    other[0] = 'TT'                                                  # replaced unseen
    assert other.view is None and list(other) == ['TT', 2, 1] and len(Engine.fetched) + len(Engine.bulk) == 1
    for name, op in (('sort', lambda r: r.sort(key=str)), ('pop', lambda r: r.pop(0)), ('slice', lambda r: r.__setitem__(slice(0, 1), ['x'])),
                     ('del', lambda r: r.__delitem__(0)), ('clear', lambda r: r.clear()), ('iadd', lambda r: r.__iadd__([1]))):
        r, plain = assembly.ViewRow(source, 2, 9, 3), ['ACGTNacgt', 9, 3]
        op(r), op(plain)
        assert r.view is None and list(r) == plain, name
    assert type(row.copy()) is list and isinstance(row, containers.FastaRow)


def test_rows_let_go_of_the_engine():
    Engine, source, fa = _source()
    rows = [assembly.ViewRow(source, 0, 2, 1), assembly.ViewRow(source, 2, 9, 3)]
    del source, fa
    gc.collect()
    assert Engine.live == 1
    rows[0][0] = None
    assert rows[1][0] == 'ACGTNacgt'
    gc.collect()
    assert Engine.live == 1                                          # the loaded row keeps its view
    rows[1][0] = None
    gc.collect()
    assert Engine.live == 0


# ------------------------------------------------------------------ 3. parse_fasta for cluster
def _fasta_module(records, logger):
    original = _Original(records)

    def parse_fasta(fasta, RE='GATC', keep_letter_case=False, logger=logger):
        return original(fasta, RE, keep_letter_case, logger)
    return types.SimpleNamespace(parse_fasta=parse_fasta, logger=logger), original


@pytest.mark.parametrize('RE', ac.RES)
def test_parse_fasta_rows_have_views(RE, tmp_path):
    text, names, lengths = ac.genome()
    path = tmp_path / 'asm.fa'
    path.write_bytes(text)
    logger, records = _logger()
    M, original = _fasta_module(records, logger)
    Engine = ac.fasta_engine()
    fa_dict = assembly.bind_fasta(M, Engine)(str(path), RE=RE)
    assert type(fa_dict) is dict and original.calls == [] and records == [['INFO', 'Parsing input FASTA file...']]
    assert [[n, v[1], v[2]] for n, v in fa_dict.items()] == GOLDEN['fragments']['__fa__'][RE]
    at = 0
    for row, length in zip(fa_dict.values(), lengths):
        assert type(row) is assembly.ViewRow and row.view[1:] == (at, length) and isinstance(row.view[0], Engine)
        at += length
    assert Engine.count_calls == [len(names)] and Engine.fetched == [] and Engine.bulk == [] and Engine.live == 1
    del fa_dict, row
    gc.collect()
    assert Engine.live == 0


def test_parse_fasta_hands_back(tmp_path):
    logger, records = _logger()
    M, original = _fasta_module(records, logger)
    parse_fasta = assembly.bind_fasta(M, ac.fasta_engine())
    for k, text in enumerate(('>a café\nACGT\n'.encode('utf-8'), b'\nACGT\n>a\nAC\n', b'>a\nAC\n>b\nGG\n>a\nTT\n')):
        path = tmp_path / ('bad%d.fa' % k)
        path.write_bytes(text)
        assert parse_fasta(str(path), RE='GATC') == 'handed back'
    assert parse_fasta(str(tmp_path / 'missing.fa')) == 'handed back' and parse_fasta(str(tmp_path)) == 'handed back'
    assert len(original.calls) == 5 and records == []


# ------------------------------------------------------------------ 4. stat_fragments on resident rows
@pytest.fixture(scope='module')
def parsed():
    """the genome in one engine per test module: (Engine, handle, names, {RE: RE sites + 1})"""
    text, names, _lengths = ac.genome()
    Engine = ac.fasta_engine()
    fa = Engine(text)
    sites = {RE: (fa.re_counts_device(cluster._sites_of(RE)) + 1).tolist() for RE in ac.RES}
    return Engine, fa, names, sites


def _rows(parsed, RE):
    _Engine, fa, names, sites = parsed
    return dict(zip(names, assembly.view_rows(fa, fa.seq_off.tolist(), fa.seq_len.tolist(), sites[RE])))


def _want_segments(g, flank_kb):
    """the segments of one call by the rule :192-199, :230-264: every bin, and every unsplit contig longer than both flanks; two for what is longer"""
    f, bins, n = 1000 * flank_kb, set(g['bin_set']), 0
    for frag, length in g['frag_len_dict']:
        if f and length > 2 * f:
            n += 2
        elif frag in bins:
            n += 1
    return n


def _stat(fa_dict, combo, names):
    key, RE, bin_size, flank, Nx, whitelist, with_depth = combo
    depth = ac.depth_dict(names) if with_depth else {}
    logger, records = _logger()
    random.seed(99)
    result = cluster.stat_fragments(fa_dict, RE, depth, whitelist, nchrs=ac.NCHRS, flank=flank, Nx=Nx, bin_size=bin_size, logger=logger)
    got = ac.plain_stat(result, fa_dict, depth)
    got['log'], got['random'] = records, random.random()
    return got


@pytest.mark.parametrize('combo', COMBOS, ids=[c[0] for c in COMBOS])
def test_stat_fragments_on_views(combo, parsed):
    """all seven return values, fa_dict and read_depth_dict afterwards, the log and the state of the random module are the reference's; the
    segments are counted in one call, no row fetches, every row ends with element 0 None and no view"""
    Engine, _fa, names, _sites = parsed
    del Engine.count_calls[:], Engine.fetched[:], Engine.bulk[:]
    fa_dict = _rows(parsed, combo[1])
    got = _stat(fa_dict, combo, names)
    assert got == GOLDEN['fragments'][combo[0]]
    want_segments = _want_segments(GOLDEN['fragments'][combo[0]], combo[3])
    assert Engine.count_calls == ([want_segments] if want_segments else []) and Engine.fetched == [] and Engine.bulk == []
    assert all(row.view is None and list.__getitem__(row, 0) is None for row in fa_dict.values())


def test_stat_fragments_frees_the_engine(tmp_path):
    text, names, _lengths = ac.genome()
    Engine = ac.fasta_engine()
    logger, records = _logger()
    M, _original = _fasta_module(records, logger)
    (tmp_path / 'asm.fa').write_bytes(text)
    fa_dict = assembly.bind_fasta(M, Engine)(str(tmp_path / 'asm.fa'))
    assert Engine.live == 1
    cluster.stat_fragments(fa_dict, 'GATC', {}, set(), nchrs=2, flank=1, Nx=100, bin_size=5, logger=logger)
    gc.collect()
    assert Engine.live == 0 and len(fa_dict) == len(names)


@pytest.mark.parametrize('combo', [c for c in COMBOS if c[0].endswith('Nx80|wl1|depth1')], ids=lambda c: c[0])
def test_stat_fragments_falls_back_to_strings(combo, parsed, monkeypatch):
    """one row that was assigned a string: the whole call takes the string path (no segment call), the rows with a view fetch, same result"""
    monkeypatch.setattr(cluster, '_lib', oracle_lib)
    Engine, fa, names, _sites = parsed
    del Engine.count_calls[:], Engine.fetched[:], Engine.bulk[:]
    fa_dict = _rows(parsed, combo[1])
    victim = names[4]
    fa_dict[victim][0] = str(fa_dict[victim][0])
    assert fa_dict[victim].view is None
    got = _stat(fa_dict, combo, names)
    assert got == GOLDEN['fragments'][combo[0]] and Engine.count_calls == []
    assert len(Engine.fetched) + len(Engine.bulk) >= 1


@needs_reference
@pytest.mark.parametrize('combo', COMBOS[::7], ids=lambda c: c[0])
def test_stat_fragments_live(combo, parsed):
    """the reference's own stat_fragments on strings beside the mirror on views: results, logs and the random module's state"""
    H = _reference()
    Engine, fa, names, sites = parsed
    key, RE, bin_size, flank, Nx, whitelist, with_depth = combo
    seq = fa._seq.tobytes().decode()
    ref_fa = {n: [seq[o:o + l], l, s] for n, o, l, s in zip(names, fa.seq_off.tolist(), fa.seq_len.tolist(), sites[RE])}
    depth = ac.depth_dict(names) if with_depth else {}
    logger, records = _logger()
    random.seed(99)
    want = ac.plain_stat(H.stat_fragments(ref_fa, RE, depth, whitelist, nchrs=ac.NCHRS, flank=flank, Nx=Nx, bin_size=bin_size, logger=logger), ref_fa, depth)
    want['log'], want['random'] = list(records), random.random()
    assert _stat(_rows(parsed, RE), combo, names) == want == GOLDEN['fragments'][key]


# ------------------------------------------------------------------ 5. --correct_nrounds on views
def _bind_stand_in(monkeypatch):
    import haphic_amd
    lib = correction_fixture.stand_in_lib()
    monkeypatch.setattr(haphic_amd, '_lib', lib)
    for mod in (cluster, correct):
        monkeypatch.setattr(mod, '_lib', lib)
    monkeypatch.setattr(patch, '_lib', lib, raising=False)
    return lib


def _correct_assembly(fa_dict, args):
    """correct_assembly :1200-1275 restated for where the reference is absent: the round loop over the bound mirrors and both writers"""
    cov_d, pos_d = correct.parse_pairs_for_correction(fa_dict, args)
    unbroken, source, fpos, ffrag = set(fa_dict), {}, {}, {}
    for rnd in range(args.correct_nrounds):
        bp = correct.detect_break_points(cov_d, fa_dict, args)
        if not bp:
            break
        if rnd == 0:
            for c in bp:
                source[c], fpos[c], ffrag[c] = c, [0], [c]
        correct.break_and_update_ctgs(bp, pos_d, cov_d, source, fpos, ffrag, fa_dict, {}, unbroken, args, rnd + 1 == args.correct_nrounds)
        unbroken -= set(bp)
    with open('corrected_asm.fa', 'w') as f:
        for ctg, ctg_info in fa_dict.items():
            f.write('>{}\n{}\n'.format(ctg, ctg_info[0]))
    with open('corrected_ctgs.txt', 'w') as f:
        for ctg in fa_dict:
            if ctg not in unbroken:
                f.write(ctg + '\n')


@pytest.mark.parametrize('live', [False, pytest.param(True, marks=needs_reference)], ids=['restated', 'live'])
@pytest.mark.parametrize('bulk', (False, True), ids=['per_row', 'bulk'])
def test_correction_job_on_views(bulk, live, tmp_path, monkeypatch):
    """one --correct_nrounds 2 job: the children are views, counted once per round; corrected_asm.fa and corrected_ctgs.txt are the reference's bytes;
    the views outlive the writer's reads, so stat_fragments afterwards makes exactly one segment-count call and no fetch"""
    _bind_stand_in(monkeypatch)
    monkeypatch.setattr(assembly, 'BULK_FETCH', bulk)
    want = GOLDEN['correction']
    fx = correction_fixture.load()
    monkeypatch.chdir(tmp_path)
    correction_fixture.write_inputs(fx, '.')
    args = correction_fixture._args(fx, 2)
    Engine = ac.fasta_engine()
    logger, records = _logger()
    if live:
        H = _reference()
        saved = patch.patch_reference(H, front=True, front_engine=Engine, gfa_engine=ac.HostGfa)
        try:
            fa_dict = H.parse_fasta('asm.fa', RE=args.RE)
            cov_d, pos_d = H.parse_pairs_for_correction(fa_dict, args)
            H.correct_assembly(cov_d, pos_d, fa_dict, {}, args)
            del cov_d, pos_d
        finally:
            patch.unpatch_reference(H, saved)
    else:
        M, _original = _fasta_module(records, logger)
        fa_dict = assembly.bind_fasta(M, Engine)('asm.fa', RE=args.RE)
        _correct_assembly(fa_dict, args)
    asm = open('corrected_asm.fa', 'rb').read()
    assert (hashlib.sha256(asm).hexdigest(), len(asm)) == (want['asm_sha256'], want['asm_bytes'])
    assert open('corrected_ctgs.txt').read() == want['corrected_ctgs']
    assert [[n, v[1], v[2]] for n, v in fa_dict.items()] == want['fa']
    n_children = [n for n in Engine.count_calls[1:]]
    assert Engine.count_calls[0] == len(fx['names']) and len(n_children) == 2 and sum(n_children) >= len([n for n in fa_dict if ':' in n])
    assert all(type(row) is assembly.ViewRow and row.view is not None for row in fa_dict.values())
    if bulk:
        assert Engine.bulk == [int(fx['lens'].sum())] and Engine.fetched == []
    else:
        assert Engine.bulk == [] and len(Engine.fetched) == len(fa_dict)
    del Engine.count_calls[:], Engine.fetched[:], Engine.bulk[:]
    result = cluster.stat_fragments(fa_dict, args.RE, {}, set(), nchrs=3, flank=args.flank, Nx=100, bin_size=20, logger=logger)
    assert ac.plain_stat(result, fa_dict, {}) == want['stat']
    assert len(Engine.count_calls) == 1 and Engine.fetched == [] and Engine.bulk == []
    del result
    gc.collect()
    assert Engine.live == 0


def test_bookkeeping_mixes_views_and_strings(monkeypatch):
    """a parent with a view gets view children counted in one call, a parent that is a plain list keeps the string code"""
    Engine = ac.fasta_engine()
    seq = bytes(np.frombuffer(b'ACGT', np.uint8)[np.random.default_rng(3).integers(0, 4, 300)]) + b'GATC' * 5
    fa = Engine(b'>v\n' + seq + b'\n')
    source = assembly.Resident(fa)
    text = seq.decode()
    fa_dict = {'v': assembly.ViewRow(source, 0, len(seq), text.count('GATC') + 1), 'p': [text, len(seq), text.count('GATC') + 1]}
    args = types.SimpleNamespace(RE='GATC')
    src, fpos, ffrag = {'v': 'v', 'p': 'p'}, {'v': [0], 'p': [0]}, {'v': ['v'], 'p': ['p']}
    del Engine.count_calls[:]
    kids = correct.update_bookkeeping({'v': [(100, 3), (250, 3)], 'p': [(100, 3)]}, src, fpos, ffrag, fa_dict, {}, {'v', 'p'}, args,
                                      count_re=lambda s, RE: s.count(RE))
    assert kids == {'v': ['v:1-100', 'v:101-250', 'v:251-320'], 'p': ['p:1-100', 'p:101-320']}
    assert Engine.count_calls == [3] and Engine.fetched == [] and Engine.bulk == []
    for name, (s, e) in (('v:1-100', (0, 100)), ('v:101-250', (100, 250)), ('v:251-320', (250, 320))):
        row = fa_dict[name]
        assert type(row) is assembly.ViewRow and row.view == (fa, s, e - s) and row[1:] == [e - s, text[s:e].count('GATC')]
        assert row[0] == text[s:e]
    assert fa_dict['p:101-320'] == [text[100:], 220, text[100:].count('GATC')] and type(fa_dict['p:1-100']) is list


# ------------------------------------------------------------------ 6. binding
def _fake_reference():
    H = types.ModuleType('HapHiC_cluster_stand_in')
    for table in (patch.SEAMS, patch.CONTAINER_SEAMS, patch.OPTIONAL, patch.CORRECTION_SEAMS, patch.FRONT_SEAMS):
        for name in table:
            setattr(H, name, (lambda n: lambda *a, **k: ('original', n))(name))
    H.logger = logging.getLogger('stand_in')
    return H


def test_patch_reference_front_is_opt_in():
    H = _fake_reference()
    originals = {n: getattr(H, n) for n in patch.FRONT_SEAMS}
    saved = patch.patch_reference(H)
    try:
        assert H.parse_gfa is originals['parse_gfa'] and H.parse_fasta is cluster.parse_fasta        # what patch_reference(H) binds today
    finally:
        patch.unpatch_reference(H, saved)
    saved = patch.patch_reference(H, front=True, front_engine=ac.fasta_engine(), gfa_engine=ac.HostGfa)
    try:
        assert H.parse_gfa is not originals['parse_gfa'] and H.parse_fasta is not cluster.parse_fasta
        assert H.parse_gfa(['no such file'], {}) == ('original', 'parse_gfa') and H.parse_fasta('no such file') == ('original', 'parse_fasta')
        assert H.stat_fragments is cluster.stat_fragments
    finally:
        patch.unpatch_reference(H, saved)
    assert all(getattr(H, n) is originals[n] for n in patch.FRONT_SEAMS)
    saved = patch.patch_reference(H, ingest=False, front=True, front_engine=ac.fasta_engine(), gfa_engine=ac.HostGfa)
    try:
        assert H.parse_gfa is originals['parse_gfa']                # the front travels with `ingest`
    finally:
        patch.unpatch_reference(H, saved)


def test_patch_reassign_gfa(tmp_path):
    R = types.SimpleNamespace(parse_link_dict=lambda *a, **k: None, split_clm_file=lambda *a, **k: None, parse_gfa=lambda *a, **k: ('original', 'parse_gfa'),
                              logger=logging.getLogger('stand_in'))
    saved = patch.patch_reassign(R, gfa=True, gfa_engine=ac.HostGfa)
    path = tmp_path / 'a.gfa'
    path.write_bytes(ac.rec('utg1', 5, 9))
    assert R.parse_gfa([str(path)], {'utg1': [None, 5, 1]}) == {'utg1': (0, 9)} and R.parse_gfa([str(tmp_path)], {}) == ('original', 'parse_gfa')
    assert saved['parse_gfa'](1) == ('original', 'parse_gfa')


# ------------------------------------------------------------------ 7. _lib.Gfa owns nothing
class _FakeLib:
    """records (symbol, handle) of every hhx_gfa_* call; hhx_gfa_open* leave handle 0x77; rc: {symbol: return code}"""

    def __init__(self, rc=None):
        self.calls, self.rc = [], rc or {}

    def __getattr__(self, name):
        if not name.startswith('hhx_'):
            raise AttributeError(name)

        def fn(*args):
            if name in ('hhx_gfa_open', 'hhx_gfa_open_bytes') and not self.rc.get(name):
                args[-1]._obj.value = 0x77
            self.calls.append(name)
            return b'boom' if name == 'hhx_last_error' else self.rc.get(name, 0)
        return fn


@pytest.mark.parametrize('source', ['reads.gfa', b'S\ta\t*\t1\t2\n'], ids=['path', 'bytes'])
def test_gfa_releases_its_handle_in_the_constructor(source, monkeypatch):
    """the table is copied and the library's handle released before the constructor returns — once, also when reading the table fails; a refused file
    made no handle, so nothing is released"""
    from haphic_amd import _lib
    opener = 'hhx_gfa_open' if isinstance(source, str) else 'hhx_gfa_open_bytes'
    fake = _FakeLib()
    monkeypatch.setattr(_lib, '_lib', fake)
    with _lib.Gfa(source) as g:
        assert fake.calls == [opener, 'hhx_gfa_counts', 'hhx_gfa_table', 'hhx_gfa_close'] and g.n_rec == 0 and g.names() == []
    g.close()
    assert fake.calls.count('hhx_gfa_close') == 1 and not issubclass(_lib.Gfa, _lib.Handle)
    for failing in ('hhx_gfa_counts', 'hhx_gfa_table'):
        fake = _FakeLib({failing: 1})
        monkeypatch.setattr(_lib, '_lib', fake)
        with pytest.raises(RuntimeError, match='libhaphic_hip: boom'):
            _lib.Gfa(source)
        assert fake.calls.count('hhx_gfa_close') == 1 and fake.calls[-1] == 'hhx_gfa_close'
    fake = _FakeLib({opener: 2})
    monkeypatch.setattr(_lib, '_lib', fake)
    with pytest.raises(_lib.Gfa.Unsupported, match='^boom$'):
        _lib.Gfa(source)
    assert 'hhx_gfa_close' not in fake.calls
