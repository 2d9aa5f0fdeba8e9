"""What the S5 mirrors hand back to the reference's run() (:2869-2935): dict-shaped containers that stay ARRAYS.

The reference's loops return `defaultdict`s keyed by name tuples (:1605-1620) and its run() then walks them through
output_pickle :710, output_clm :376, normalize_by_nlinks :718, filter_fragments :741, dict_to_matrix :310.  At 100k contigs /
500 M pairs those dicts hold 1.6e8 + 1.2e8 + ~3e8 keys: building them as Python objects costs minutes around a link-matrix
build that takes 40 ms on the device.  So the mirrors return

    LinkTable  (full_link_dict, flank_link_dict, HT_link_dict)   — a defaultdict subclass backed by an IngestSession
    PairLists  (clm_dict, ctg_coord_dict)                        — the same for the per-contig-pair arrays

whose entries exist only as the device tables of the ingest handle (and, once someone asks, as numpy arrays in dict order).
The seams that run() calls next (cluster.filter_fragments / normalize_by_nlinks / dict_to_matrix / output_pickle / output_clm)
recognise a table that is still `frozen` and work on the arrays with no per-key Python.  ANY other access — item lookup,
iteration, assignment, deletion, as remove_allelic_HiC_links :474-689 or the --remove_concentrated_links loop :2888-2891 do —
thaws the container first: the real dict is filled with C-speed constructors (`dict.update(zip(...))`), the object turns into a
plain defaultdict subclass, and from then on every mirror takes its generic dict path.  Pickling never needs the subclass:
`__reduce_ex__` describes a plain `collections.defaultdict`, which is what HapHiC sort / reassign unpickle.
"""
from array import array
from collections import defaultdict
from itertools import repeat

import numpy as np


THAW_LOG = []          # (kind, keys, seconds) of every thaw of this process: what the reference's own Python costs when it touches a table


class Thawed(defaultdict):
    """A LinkTable / PairLists after its entries became real dict entries: a defaultdict in all but the class name."""

    def __reduce_ex__(self, protocol):
        return defaultdict, (self.default_factory,), None, None, iter(dict.items(self))

    __reduce__ = lambda self: self.__reduce_ex__(2)             # noqa: E731

    @property
    def frozen(self):
        return False


def _thawing(name):
    def method(self, *args, **kwargs):
        self._thaw()
        return getattr(self, name)(*args, **kwargs)
    method.__name__ = name
    return method


class _Frozen(defaultdict):
    """Base of the array-backed containers.  `_source_items()` yields the (key, value) pairs in dict insertion order."""

    frozen = True

    def __init__(self, factory, session, kind):
        defaultdict.__init__(self, factory)
        self._session = session
        self._kind = kind

    def _n(self):
        raise NotImplementedError

    def _source_items(self):
        raise NotImplementedError

    def _thaw(self):
        if type(self) is Thawed:
            return
        import gc
        import time
        t0 = time.perf_counter()
        session = self._session
        kind = self._kind
        collect = gc.isenabled()
        gc.disable()                      # millions of fresh tuples: the generational collector would walk them again and again
        try:
            dict.update(self, self._source_items())
        except BaseException:             # a MemoryError half-way: stay frozen (and retryable), never a truncated plain dict
            dict.clear(self)
            raise
        finally:
            if collect:
                gc.enable()
        self.__dict__.clear()
        self.__class__ = Thawed
        session.note_thawed()
        THAW_LOG.append((kind, dict.__len__(self), time.perf_counter() - t0))

    # answered from the arrays
    def __len__(self):
        return self._n()

    def __bool__(self):
        return self._n() > 0

    def __reduce_ex__(self, protocol):
        return defaultdict, (self.default_factory,), None, None, iter(self._source_items())

    __reduce__ = lambda self: self.__reduce_ex__(2)             # noqa: E731

    def __copy__(self):
        out = defaultdict(self.default_factory)
        out.update(self._source_items())
        return out

    copy = __copy__


for _name in ('__getitem__', '__setitem__', '__delitem__', '__contains__', '__iter__', '__reversed__', '__missing__', 'keys', 'values',
              'items', 'get', 'pop', 'popitem', 'setdefault', 'update', 'clear', '__eq__', '__ne__', '__repr__', '__or__', '__ror__',
              '__ior__'):
    setattr(_Frozen, _name, _thawing(_name))


class LinkTable(_Frozen):
    """full_link_dict / flank_link_dict / HT_link_dict (:1605-1616): {(name, name): links}.  kind = 'full' | 'flank' | 'HT'."""

    def __init__(self, session, kind):
        _Frozen.__init__(self, int, session, kind)

    def _n(self):
        return self._session.n_keys(self._kind)

    def arrays(self):
        """(i, j, value, names): ids into `names` and the values (int64 counts, or float64 after a weighting step) in dict order"""
        return self._session.link_arrays(self._kind)

    def _source_items(self):
        i, j, v, names = self.arrays()
        table = np.empty(len(names), object)                  # the names gathered by numpy's take on an object array: 1.5 x the rate
        table[:] = names                                       # of map(names.__getitem__, ids) (measured; the dict insert itself is ~half the time)
        return zip(zip(table[i].tolist(), table[j].tolist()), v.tolist())


class PairLists(_Frozen):
    """clm_dict (update_clm_dict :395-401) / ctg_coord_dict (record_coord_pairs :454-471): {(ctg, ctg): array}.
    kind = 'clm' | 'crd'."""

    def __init__(self, session, kind, code):
        _Frozen.__init__(self, lambda: array(code), session, kind)

    def _n(self):
        return self._session.n_keys('full')

    def _source_items(self):
        return self._session.pair_items(self._kind)


def slices_as_arrays(code, flat, ptr, width):
    """array(code) objects over flat[width * ptr[k] : width * ptr[k + 1]] for every k, built by C-level iterators only
    (slice objects -> memoryview slices -> array(code, bytes) = array.frombytes)."""
    view = memoryview(np.ascontiguousarray(flat)).cast('B')
    step = width * flat.dtype.itemsize
    bounds = (np.asarray(ptr, np.int64) * step).tolist()
    return map(array, repeat(code), map(bytes, map(view.__getitem__, map(slice, bounds[:-1], bounds[1:]))))


# ------------------------------------------------------------------ fa_dict of `haphic build` (haphic_amd/scaffolds.py)
class ThawedFasta(dict):
    """A FastaTable after its entries became real dict entries: the reference's fa_dict in all but the class name."""

    @property
    def frozen(self):
        return False


class FastaTable(dict):
    """fa_dict (parse_fasta, HapHiC_cluster.py:87-113): {ctg: [seq, len, RE sites + 1]} whose sequences exist only in the memory of the device
    (engine: _lib.Fasta or a stand-in with its interface).  len(), `in` and iteration over the names in file order are answered from the arrays —
    what parse_tours :29-57 needs — and the build_final_scaffolds mirror works on `engine`, `names`, `lengths` and index_of().  ANY other access
    ([], .items(), .values(), assignment, deletion, ...) thaws it first: the sequences come to the host (engine.sequences()), the RE sites are
    counted (engine.re_counts(sites)), the object turns into a plain dict subclass and `frozen` is False for good."""

    frozen = True

    def __init__(self, engine, sites):
        dict.__init__(self)
        self.engine = engine
        self.sites = list(sites)
        self.names = engine.names()
        self.lengths = np.asarray(engine.seq_len, np.int64)
        self._index = None

    def index_of(self, name):
        """position of the contig in the file, -1 when it has none"""
        if self._index is None:
            self._index = dict(zip(self.names, range(len(self.names))))
        return self._index.get(name, -1)

    def _thaw(self):
        if type(self) is ThawedFasta:
            return
        import time
        t0 = time.perf_counter()
        engine, names = self.engine, self.names
        blob = engine.sequences().tobytes().decode('ascii')
        counts = engine.re_counts(self.sites) if names else []
        off, ln = np.asarray(engine.seq_off, np.int64).tolist(), self.lengths.tolist()
        try:
            dict.update(self, ((names[k], [blob[off[k]:off[k] + ln[k]], ln[k], int(counts[k]) + 1]) for k in range(len(names))))    # pseudo-count of 1 (:110)
        except BaseException:
            dict.clear(self)
            raise
        self.__dict__.clear()
        self.__class__ = ThawedFasta
        THAW_LOG.append(('fasta', dict.__len__(self), time.perf_counter() - t0))

    # answered from the arrays
    def __len__(self):
        return len(self.names)

    def __bool__(self):
        return len(self.names) > 0

    def __contains__(self, name):
        return self.index_of(name) >= 0

    def __iter__(self):
        return iter(self.names)

    def __copy__(self):
        self._thaw()
        return dict(self)

    copy = __copy__

    def __reduce_ex__(self, protocol):
        self._thaw()
        return dict, (), None, None, iter(dict.items(self))

    __reduce__ = lambda self: self.__reduce_ex__(2)             # noqa: E731


for _name in ('__getitem__', '__setitem__', '__delitem__', '__reversed__', 'keys', 'values', 'items', 'get', 'pop', 'popitem', 'setdefault', 'update',
              'clear', '__eq__', '__ne__', '__repr__', '__or__', '__ror__', '__ior__'):
    setattr(FastaTable, _name, _thawing(_name))


# ------------------------------------------------------------------ fa_dict rows of `haphic reassign` (haphic_amd/reassign.py bind_fasta)
class FastaRow(list):
    """One value of fa_dict (parse_fasta, HapHiC_cluster.py:87-113): [sequence, length, RE sites + 1] whose sequence stays in the memory of the
    device until somebody looks at it.  row[1], row[2], len(row) and assignments to single elements (row[0] = None included) never fetch; whatever
    observes element 0 — index 0 or -3, a slice that covers it, iteration and unpacking, comparison, repr, copy, pickling, sort, reverse,
    concatenation — and every change of the list's shape fetches it first (fetch(key) -> str), after which the row is the reference's list.  A copy or
    an unpickled row is a plain list."""

    __slots__ = ('_fetch', '_key')

    def __init__(self, fetch, key, length, re_sites):
        list.__init__(self, (None, length, re_sites))
        self._fetch, self._key = fetch, key

    def _load(self):
        fetch = self._fetch
        if fetch is not None:
            list.__setitem__(self, 0, fetch(self._key))
            self._fetch = self._key = None

    def __getitem__(self, index):
        if self._fetch is not None and (0 in range(3)[index] if isinstance(index, slice) else index in (0, -3)):
            self._load()
        return list.__getitem__(self, index)

    def __setitem__(self, index, value):
        if self._fetch is not None:
            if isinstance(index, slice):
                self._load()
            elif index in (0, -3):
                self._fetch = self._key = None                  # replaced unseen
        list.__setitem__(self, index, value)

    def __copy__(self):
        self._load()
        return list(self)

    copy = __copy__

    def __reduce_ex__(self, protocol):
        self._load()
        return list, (), None, list.__iter__(self)

    __reduce__ = lambda self: self.__reduce_ex__(2)             # noqa: E731


def _loading(name):
    def method(self, *args, **kwargs):
        self._load()
        for other in args:                                       # list's own methods read the other operand's slots in C
            if type(other) is FastaRow:
                other._load()
        return getattr(list, name)(self, *args, **kwargs)
    method.__name__ = name
    return method


for _name in ('__iter__', '__reversed__', '__contains__', '__eq__', '__ne__', '__lt__', '__le__', '__gt__', '__ge__', '__repr__', '__add__', '__mul__',
              '__rmul__', '__iadd__', '__imul__', '__delitem__', 'index', 'count', 'sort', 'reverse', 'append', 'extend', 'insert', 'pop', 'remove',
              'clear'):
    setattr(FastaRow, _name, _loading(_name))
FastaRow.__radd__ = lambda self, other: other + list(self)      # plain list + row reads the row's slots in C otherwise
