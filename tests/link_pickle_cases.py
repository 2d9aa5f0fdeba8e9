"""Link pickles (full_links.pkl / HT_links.pkl) for the reader of csrc/hhx_pickleread.hip: the accepted cases in both dialects — Python's pickler on a
dict whose keys hold fresh or shared str objects, and the library's own writer (hhx_write_link_pickle, host code) — the files the reader must hand
back, the oracle (pickle.load + cluster._dict_arrays) and a host restatement of the reader over pickletools.genops, which stands in for the device
in the CPU tests."""
import io
import pickle
import pickletools
import struct
from collections import defaultdict

import numpy as np

from haphic_amd import _lib, cluster

HEAD = (b'\x8c\x0bcollections\x94\x8c\x0bdefaultdict\x94\x93\x94\x8c\x08builtins\x94\x8c\x03int\x94\x93\x94\x85\x94R\x94')
LETTERS = 'hjusKMJGXR(.'
VALUES = [0, 140, 148, 255, 256, 0x9486, 65535, 65536, -1, 2 ** 31, -2 ** 31, 2 ** 31 - 1, -2 ** 31 - 1, 2 ** 40, -2 ** 40, 2 ** 63 - 1, -2 ** 63]
SLOTS = [0x8c94, 0x9486, 0x8695, 0x9528, 0x2875, 0x7528, 0x948c, 0x10000, 0x1288c, 0x8c]       # memo slots whose bytes are opcodes


def _fresh(fmt, k):
    return fmt % k                                                    # a new str object per call, as the reference's keys hold


def counted(n, fmt='ctg%d'):
    """n keys over ~sqrt(n) names, every key with str objects of its own: Python writes every name as a literal again"""
    d = defaultdict(int)
    w = max(2, int(n ** 0.5) + 1)
    for k in range(n):
        d[(_fresh(fmt, k // w), _fresh(fmt, w + k % w))] = 1 + k % 300
    assert len(d) == n
    return d


def shared(n_names, keys):
    names = ['s%d' % k for k in range(n_names)]
    d = defaultdict(int)
    for k, (a, b) in enumerate(keys):
        d[(names[a], names[b])] = 1 + k % 70001
    return d


def many_slots():
    """80 000 names introduced two per key (one object each: memo references in both dialects), then keys over the names whose slots spell opcodes"""
    n = 80000
    keys = [(2 * k, 2 * k + 1) for k in range(n // 2)]
    for s in SLOTS:
        keys += [(s - 8, 3), (5, s - 8), (s - 8, s - 7)]
    return shared(n, keys)


def straddle():
    """names of opcode letters, lengths 1 .. 255 stepped against each other, so that opcodes of every kind meet the 512-byte seams everywhere"""
    d = defaultdict(int)
    for k in range(640):
        a = ''.join(LETTERS[(k + q) % len(LETTERS)] for q in range(1 + k * 7 % 255))
        b = ''.join(LETTERS[(3 * k + 5 * q) % len(LETTERS)] for q in range(1 + k * 13 % 254))
        d[(a, b + '.')] = VALUES[k % len(VALUES)]
    return d


def accepted():
    """{name: defaultdict(int)}"""
    cases = {'n%d' % n: counted(n) for n in (0, 1, 2, 999, 1000, 1001, 2001)}
    cases['frames'] = counted(16000, 'contig_%07d')                   # ~ 400 KB: several 64 KiB frames, their borders inside batches
    cases['many_slots'] = many_slots()
    mixed = shared(40, [(a, b) for a in range(40) for b in range(a + 1, 40)])
    for k in range(300):
        mixed[(_fresh('s%d', k % 40), _fresh('f%d', k))] = k
    cases['shared_and_fresh'] = mixed
    cases['straddle'] = straddle()
    values = defaultdict(int)
    for k, v in enumerate(VALUES * 3):
        values[('K%d' % (k % 7), 'M\x8cJ%d' % k)] = v
    cases['values'] = values
    floats = defaultdict(int)
    for k in range(1200):
        floats[('a%d' % (k % 30), 'b%d' % k)] = k / 7.0 - 3.0
    floats[('a0', 'nan')] = float('inf')
    cases['floats'] = floats
    both = defaultdict(int)
    for k in range(1500):
        both[('a%d' % (k % 30), 'b%d' % k)] = k if k % 3 else k * 0.5
    both[('a1', 'big')] = 2 ** 53
    cases['int_and_float'] = both
    utf8 = defaultdict(int)
    for k in range(700):
        utf8[('ČŒ%d' % (k % 9), 'ctg鱼\U0001f600%d\u0094' % k)] = k
    cases['utf8'] = utf8
    ht = defaultdict(int)
    for k in range(1100):
        ht[('ctg%d_%s' % (k // 40, 'HT'[k % 2]), 'ctg%d_%s' % (30 + k % 40, 'TH'[k % 3 % 2]))] = 1 + k
    cases['HT_links'] = ht
    return cases


def library_can_write(d):
    return all(type(v) is int and -2 ** 63 <= v < 2 ** 63 for v in d.values()) and all(len(n.encode()) < 256 for key in d for n in key)


def write_python(d, path, protocol=4):
    with open(path, 'wb') as f:
        pickle.dump(d, f, protocol)


def write_library(d, path):
    names = {}
    i, j, v = cluster._dict_arrays(d, names)
    _lib.write_link_pickle(path, i, j, np.fromiter(d.values(), np.int64, len(d)), list(names))


def golden():
    """{'full_links' | 'HT_links': bytes} of tests/golden/link_pickles.npz: the files the reference's own code wrote (make_golden_link_pickles.py)"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'link_pickles.npz'))
    return {k: z[k].tobytes() for k in z.files}


def _body(items):
    return b'\x80\x04' + HEAD + items + b'.'


def handed_back():
    """{name: bytes} of files the reader must refuse; pickle.load answers every one (with a dict or with its own exception)"""
    one = defaultdict(int, {('a', 'b'): 1, ('a', 'c'): 2})
    out = {'plain_dict': pickle.dumps(dict(one), 4), 'defaultdict_list': pickle.dumps(defaultdict(list, one), 4), 'protocol3': pickle.dumps(one, 3),
           'tuple3': pickle.dumps(defaultdict(int, {('a', 'b', 'c'): 1}), 4), 'true': pickle.dumps(defaultdict(int, {('a', 'b'): True}), 4),
           'none': pickle.dumps(defaultdict(int, {('a', 'b'): None}), 4), 'two_to_63': pickle.dumps(defaultdict(int, {('a', 'b'): 2 ** 63}), 4),
           'name256': pickle.dumps(defaultdict(int, {('a' * 256, 'b'): 1}), 4),
           'after_stop': pickle.dumps(one, 4) + b'.', 'after_stop_library': _body(b'(\x8c\x01a\x94\x8c\x01b\x94\x86K\x01u') + b'K\x01',
           'big_int_beside_float': pickle.dumps(defaultdict(int, {('a', 'b'): 2 ** 53 + 1, ('a', 'c'): 0.5}), 4),
           'key_twice': _body(b'(\x8c\x01a\x94\x8c\x01b\x94\x86K\x01h\x08h\x09\x86K\x02u'),
           'memo_of_a_tuple': _body(b'(\x8c\x01a\x94\x8c\x01b\x94\x86\x94K\x01h\x0ah\x08\x86K\x02u'),
           'memo_of_the_header': _body(b'(\x8c\x01a\x94h\x00\x86K\x01u'),
           'setitems_without_mark': _body(b'\x8c\x01a\x94\x8c\x01b\x94\x86K\x01u'),
           'frame_too_long': b'\x80\x04\x95' + struct.pack('<Q', 1000) + HEAD + b'(\x8c\x01a\x94\x8c\x01b\x94\x86K\x01u.'}
    whole = pickle.dumps(counted(40), 4)
    for cut in (1, 2, 11, 40, len(HEAD) + 11, len(HEAD) + 13, len(whole) // 2, len(whole) - 3, len(whole) - 1):
        out['cut_at_%d' % cut] = whole[:cut]
    lib = _body(b'(' + b''.join(b'\x8c\x04n%03d\x94\x8c\x04m%03d\x94\x86M\x8c\x94' % (k, k) for k in range(50)) + b'u')
    for cut in (len(lib) // 2, len(lib) // 2 + 1, len(lib) - 1):
        out['library_cut_at_%d' % cut] = lib[:cut]
    return out


def load_or_error(data):
    """what pickle.load says about the bytes: ('ok', object) or ('error', exception type)"""
    try:
        return 'ok', pickle.load(io.BytesIO(data))
    except Exception as e:                                            # noqa: BLE001 — whatever Python raises is the oracle
        return 'error', type(e)


def expected(d):
    """(i, j, values as Python objects, names) of a loaded dict: the numbering cluster._dict_arrays gives the real dict"""
    names = {}
    i, j, _v = cluster._dict_arrays(d, names)
    return i, j, list(d.values()), list(names)


def check_arrays(got, d):
    """the result of a reader (the shape of _lib.read_link_pickle) against the dict pickle.load gave"""
    assert got is not None, 'handed back'
    i, j, value, is_float, names = got
    ei, ej, ev, enames = expected(d)
    assert names == enames
    assert i.dtype == np.int32 and j.dtype == np.int32 and np.array_equal(i, ei) and np.array_equal(j, ej)
    kinds = [type(v) is float for v in ev]
    if is_float is None:
        assert value.dtype == np.int64 and not any(kinds) and value.tolist() == ev
    else:
        assert value.dtype == np.float64 and any(kinds) and is_float.tolist() == kinds
        assert value.tolist() == [float(v) for v in ev] and all(int(g) == v for g, v, f in zip(value.tolist(), ev, kinds) if not f)


# ------------------------------------------------------------------ the reader restated on the host
def host_reader(path):
    """_lib.read_link_pickle's contract, opcode by opcode over pickletools.genops: the same grammar, the same refusals, the same numbering"""
    data = open(path, 'rb').read()
    if len(data) < 2 + len(HEAD) + 1 or data[0] != 0x80 or data[1] not in (4, 5):
        return None
    at, frames = 2, []
    if data[2] == 0x95:
        if len(data) < 11 + len(HEAD):
            return None
        frames.append((2, struct.unpack('<Q', data[3:11])[0]))
        at = 11
    if data[at:at + len(HEAD)] != HEAD:
        return None
    body0 = at + len(HEAD)
    try:
        ops = [(op.name, arg, pos) for op, arg, pos in pickletools.genops(data) if pos >= body0]
    except Exception:                                                 # noqa: BLE001 — a truncated or unknown opcode
        return None
    if not ops or ops[-1][0] != 'STOP' or ops[-1][2] != len(data) - 1:
        return None
    memo, names, ids, key, values, kinds = [], {}, [], [], [], []
    batch, since, prev = False, 0, None
    for name, arg, pos in ops:
        role = len(key)
        if name == 'FRAME':
            frames.append((pos, arg))
            continue
        if name in ('SHORT_BINUNICODE', 'BINGET', 'LONG_BINGET'):
            if role > 1 or (role == 0 and not batch and since):
                return None
            if name != 'SHORT_BINUNICODE':
                if not 8 <= arg < 8 + len(memo) or memo[arg - 8] is None:
                    return None
                arg = memo[arg - 8]
            key.append(names.setdefault(arg, len(names)))
            since += 1
        elif name == 'TUPLE2':
            if role != 2:
                return None
            key.append(None)
            since += 1
        elif name in ('BININT1', 'BININT2', 'BININT', 'LONG1', 'BINFLOAT'):
            if role != 3 or (name == 'LONG1' and not -2 ** 63 <= arg < 2 ** 63):
                return None
            ids.append(key[:2])
            values.append(arg)
            kinds.append(name == 'BINFLOAT')
            key = []
            since += 1
        elif name == 'MEMOIZE':
            if prev is None or prev[0] not in ('SHORT_BINUNICODE', 'TUPLE2'):
                return None
            memo.append(prev[1] if prev[0] == 'SHORT_BINUNICODE' else None)
        elif name == 'MARK':
            if role or batch or since:
                return None
            batch, since = True, 0
        elif name == 'SETITEMS':
            if role or not batch:
                return None
            batch, since = False, 0
        elif name == 'SETITEM':
            if role or batch or since != 4:
                return None
            since = 0
        elif name == 'STOP':
            if role or batch or since:
                return None
        else:
            return None
        prev = (name, arg, pos)
    for k, (pos, size) in enumerate(frames):
        if (k == 0 and pos != 2) or pos + 9 + size != (frames[k + 1][0] if k + 1 < len(frames) else len(data)):
            return None
    if len(set(map(tuple, ids))) != len(ids):
        return None
    ids = np.array(ids, np.int32).reshape(len(ids), 2)
    i, j = np.ascontiguousarray(ids[:, 0]), np.ascontiguousarray(ids[:, 1])
    if not any(kinds):
        return i, j, np.array(values, np.int64).reshape(len(values)), None, list(names)
    if any(abs(v) > 2 ** 53 for v, f in zip(values, kinds) if not f):
        return None
    return i, j, np.array([float(v) for v in values], np.float64), np.array(kinds, bool), list(names)
