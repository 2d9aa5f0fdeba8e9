"""The handle lifecycle and the error path of haphic_amd/_lib.py against a recording stand-in for the library (no GPU, nothing is dlopened)."""
import ctypes as C

import numpy as np
import pytest

from haphic_amd import _lib

RELEASE = {
    'DeviceCSR': 'hhx_csr_free', 'DenseMatrix': 'hhx_dmat_free', 'DenseRows': 'hhx_dense_free', 'LinkPickle': 'hhx_pickle_free',
    'ByteSink': 'hhx_byte_sink_close', 'TextReader': 'hhx_text_reader_close', 'ClmSplit': 'hhx_clm_split_destroy',
    'SortGraph': 'hhx_sort_graph_destroy', 'Reassign': 'hhx_reassign_destroy', 'Fasta': 'hhx_fasta_close', 'BamReader': 'hhx_bam_close',
    'ContactMap': 'hhx_contact_map_destroy', 'PlotNorm': 'hhx_plotnorm_destroy', 'PairsParser': 'hhx_pairs_parser_destroy',
    'Ingest': 'hhx_ingest_destroy', 'CorrectTable': 'hhx_correct_destroy', 'ContigRemap': 'hhx_remap_destroy', 'ShardBuild': 'hhx_shard_destroy',
}
CLASSES = [getattr(_lib, name) for name in sorted(RELEASE)]
HANDLE = 0x1000


class FakeLib:
    """every hhx_* attribute records (symbol, args) and returns rc[symbol] (default 0), or raises it when it is an exception; effect[symbol]
    runs on the arguments first (to write through an out-parameter)"""

    def __init__(self):
        self.calls, self.rc, self.effect, self.error = [], {}, {}, b'boom'

    def __getattr__(self, name):
        if not name.startswith('hhx_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == 'hhx_last_error':
                return self.error
            if name in self.effect:
                self.effect[name](*args)
            rc = self.rc.get(name, 0)
            if isinstance(rc, Exception):
                raise rc
            return rc
        return fn

    def names(self):
        return [name for name, _ in self.calls]


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, '_lib', lib)
    return lib


def bare(cls, h=HANDLE):
    obj = object.__new__(cls)
    if h is not Ellipsis:
        obj.h = C.c_void_p(h) if isinstance(h, int) else h
    return obj


def assert_one_release(fake, cls):
    assert fake.names() == [cls._release]
    assert fake.calls[0][1][0].value == HANDLE


def test_the_handle_classes():
    assert {c.__name__ for c in _lib.Handle.__subclasses__()} == set(RELEASE)
    for cls in CLASSES:
        assert cls._release == RELEASE[cls.__name__]
        assert cls._release in _lib.SIGNATURES
        assert _lib.SIGNATURES[cls._release][1][0] is C.c_void_p
        if cls is not _lib.ByteSink:
            assert not {'close', 'free', 'destroy', '__del__', '__enter__', '__exit__'} & set(vars(cls)), cls
    assert sum('__del__' in vars(c) for c in [_lib.Handle] + CLASSES) == 1


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
@pytest.mark.parametrize('method', ['close', 'free', 'destroy'])
def test_release_once(fake, cls, method):
    obj = bare(cls)
    getattr(obj, method)()
    assert_one_release(fake, cls)
    assert obj.h is None
    for again in ('close', 'free', 'destroy'):
        getattr(obj, again)()
    assert len(fake.calls) == 1


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
@pytest.mark.parametrize('h', [None, C.c_void_p()], ids=['none', 'null'])
def test_no_call_without_a_handle(fake, cls, h):
    obj = bare(cls, h)
    obj.close(), obj.free(), obj.destroy()
    assert fake.calls == [] and obj.h is None


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
def test_with_releases(fake, cls):
    with bare(cls) as obj:
        assert fake.calls == []
    assert_one_release(fake, cls)
    assert obj.h is None
    del fake.calls[:]
    with pytest.raises(KeyError):
        with bare(cls) as obj:
            raise KeyError('body')
    assert_one_release(fake, cls)


@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: c.__name__)
def test_finaliser_never_raises(fake, cls):
    bare(cls, Ellipsis).__del__()                      # __init__ raised before self.h existed
    assert fake.calls == []
    fake.rc[cls._release] = OSError('release failed')
    bare(cls).__del__()
    if cls is _lib.ByteSink:
        assert fake.calls == []                        # no finaliser: see the class
    else:
        assert_one_release(fake, cls)


def test_aliases_honour_an_override(fake):
    class Counting(_lib.DeviceCSR):
        closed = 0

        def close(self):
            self.closed += 1
            super().close()
    obj = Counting(HANDLE)                              # (an int, as DeviceCSR always took)
    obj.free()
    obj.destroy()
    assert obj.closed == 2
    assert_one_release(fake, Counting)


def test_byte_sink_close_is_an_action(fake):
    assert '__del__' not in vars(_lib.ByteSink)
    fake.effect['hhx_byte_sink_close'] = lambda h, n: setattr(n._obj, 'value', 1234)
    sink = bare(_lib.ByteSink)
    assert sink.close() == 1234
    assert_one_release(fake, _lib.ByteSink)
    assert sink.h is None and sink.close() == 0 and len(fake.calls) == 1
    fake.rc['hhx_byte_sink_close'] = 1
    with pytest.raises(RuntimeError, match='libhaphic_hip: boom'):
        bare(_lib.ByteSink).close()
    with pytest.raises(RuntimeError, match='libhaphic_hip: boom'):
        with bare(_lib.ByteSink):
            pass


def test_bam_reader_releases_after_a_failed_header(fake):
    fake.effect['hhx_bam_open'] = lambda path, threads, out: setattr(out._obj, 'value', 0x2000)
    fake.rc['hhx_bam_header'] = 1
    with pytest.raises(RuntimeError, match='libhaphic_hip: boom'):
        _lib.BamReader('reads.bam')
    assert fake.names() == ['hhx_bam_open', 'hhx_bam_header', 'hhx_last_error', 'hhx_bam_close']
    assert fake.calls[-1][1][0].value == 0x2000


def test_link_pickle_open_releases_once_after_failed_sizes(fake):
    import gc
    fake.effect['hhx_pickle_open'] = lambda path, out: setattr(out._obj, 'value', 0x3000)
    fake.rc['hhx_pickle_sizes'] = 1
    with pytest.raises(RuntimeError):
        _lib.LinkPickle.open('full_links.pkl')
    gc.collect()
    assert fake.names().count('hhx_pickle_free') == 1
    fake.rc = {'hhx_pickle_open': 2}
    fake.error = b'not a protocol-4 pickle'
    assert _lib.LinkPickle.open('full_links.pkl') is None
    assert _lib.PICKLE_REFUSALS.pop() == 'not a protocol-4 pickle'


PY_ERRORS = [(b'IndexError: list index out of range', IndexError, 'list index out of range'),
             (b'ValueError: invalid literal for int() with base 10: \'x\'', ValueError, 'invalid literal for int() with base 10: \'x\''),
             (b'boom', RuntimeError, 'libhaphic_hip: boom')]


@pytest.mark.parametrize('error, kind, text', PY_ERRORS, ids=['index', 'value', 'other'])
def test_pairs_parser_raises_the_reference_s_exception(fake, error, kind, text):
    ps = _lib.PairsParser(['ctg1', 'ctg2'])
    assert fake.names() == ['hhx_pairs_parser_create'] and fake.calls[0][1][0] == 2
    fake.rc['hhx_pairs_parse'], fake.error = 1, error
    for kwargs in (dict(text=b'r\tctg1\n'), dict(text=None, device_ptr=64, n_bytes=7), dict(text=None, host_ptr=64, n_bytes=7)):
        with pytest.raises(kind) as e:
            ps.parse(**kwargs)
        assert type(e.value) is kind and e.value.args == (text,)


@pytest.mark.parametrize('error, kind, text', [PY_ERRORS[0], PY_ERRORS[2]], ids=['index', 'other'])
def test_clm_split_raises_the_reference_s_exception(fake, error, kind, text):
    """(the table is shared with PairsParser: hhx_clm_split_* has no message that begins with 'ValueError: ')"""
    split = _lib.ClmSplit(['a', 'b'], [0, -1], ['g0.clm'])
    assert split.n_groups == 1
    fake.error = error
    for symbol, call in (('hhx_clm_split_push', lambda: split.push(b'a+ b-\t1\t5\n')), ('hhx_clm_split_push', lambda: split.push(device_ptr=64, n_bytes=4)),
                         ('hhx_clm_split_file', lambda: split.push_file('x.clm')), ('hhx_clm_split_finish', split.finish)):
        fake.rc = {symbol: 1}
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and e.value.args == (text,)


def test_unsupported_has_one_value():
    assert _lib.HHX_UNSUPPORTED == 2
    assert _lib.GROUP_STATS_UNSUPPORTED is _lib.HHX_UNSUPPORTED and _lib.PICKLE_NOT_OURS is _lib.HHX_UNSUPPORTED
    assert _lib.Ingest.UNSUPPORTED is _lib.HHX_UNSUPPORTED


def test_unsupported_raises_the_caller_s_class(fake):
    fake.error = b'not served'
    fake.rc = {'hhx_reassign_create': 2, 'hhx_fasta_open_bytes': 2, 'hhx_fasta_open': 2, 'hhx_sort_verdict_sums': 2}
    with pytest.raises(_lib.Reassign.Unsupported, match='^not served$'):
        _lib.Reassign([0], [1], [5], 2, [0, 1], 2)
    with pytest.raises(_lib.Fasta.Unsupported, match='^not served$'):
        _lib.Fasta(b'>a\nACGT\n')
    with pytest.raises(_lib.Fasta.Unsupported, match='^not served$'):
        _lib.Fasta('contigs.fa')
    with pytest.raises(_lib.SortVerdictUnsupported, match='^not served$'):
        _lib.sort_verdict_sums([1, -2, 3], [10, 20, 30])
    fake.rc = {'hhx_reassign_round': 2}
    r = _lib.Reassign([0], [1], [5], 2, [0, 1], 2)
    with pytest.raises(_lib.Reassign.Unsupported):
        r.round(np.zeros(2, np.int32), np.zeros(2, np.int64), [1, 1], [0, 1], [0, 0], None, 1, 0, 0, 0, False, False, 0)
    fake.rc = {'hhx_reassign_create': 1}
    with pytest.raises(RuntimeError, match='libhaphic_hip: not served') as e:
        _lib.Reassign([0], [1], [5], 2, [0, 1], 2)
    assert type(e.value) is RuntimeError


def test_unsupported_yields_none(fake):
    ing = bare(_lib.Ingest)
    ing.n_full, ing.n_flank, ing.n_frag = 3, 2, 4
    fake.rc = {'hhx_ingest_concordance': 2, 'hhx_ingest_drop_links': 2, 'hhx_ingest_group_stats': 2, 'hhx_group_stats': 2, 'hhx_allelic_nonmax': 2}
    assert ing.concordance_counts(10, 4) is None
    assert ing.drop_links(np.zeros(3, np.uint8), np.ones(4, np.uint8)) is None
    group = np.zeros((1, 2), np.int32)
    assert ing.group_stats(group, [1], [7], [3, 4]) is None
    assert _lib.group_stats([0], [1], [5], group, [1], [7], [3, 4]) is None
    assert _lib.allelic_nonmax([0], [1], [5], 2, [0, 2], [0, 1]) is NotImplemented
    assert 'hhx_last_error' not in fake.names()
    fake.rc = {'hhx_ingest_concordance': 0}
    m, diag, anti = ing.concordance_counts(10, 4)
    assert m.shape == diag.shape == anti.shape == (3,)
    fake.rc = {'hhx_ingest_concordance': 1}
    with pytest.raises(RuntimeError, match='libhaphic_hip: boom'):
        ing.concordance_counts(10, 4)
    ing.h = None
