"""haphic_amd.ranks without a GPU: the byte-range rule of a multi-rank .pairs ingest against the brute-force owner of every line, the
--gpus / --host-transport command line, and world 1 leaving every mirror on its one-rank path."""
import os
import random
import sys

import pytest

from haphic_amd import ranks


def _line_starts(data):
    """every line's first byte: 0 and after every '\\n' (a trailing '\\n' starts no line)"""
    return [0] + [k + 1 for k, b in enumerate(data) if b == 0x0A and k + 1 < len(data)] if data else []


def _brute(data, world):
    """rank -> the bytes of the lines whose first byte lies in its raw range, in order"""
    bounds = ranks.byte_ranges(len(data), world)
    starts = _line_starts(data)
    ends = starts[1:] + [len(data)]
    out = [b''] * world
    for s, e in zip(starts, ends):
        owner = [r for r, (b0, b1) in enumerate(bounds) if b0 <= s < b1]
        assert len(owner) == 1
        out[owner[0]] += data[s:e]
    return out


def _files():
    rng = random.Random(7)
    body = ''.join('r{}\tctg{}\t{}\tctg{}\t{}\t+\t-\n'.format(k, rng.randrange(9), rng.randrange(1, 10 ** 6), rng.randrange(9),
                                                            rng.randrange(1, 10 ** 6)) for k in range(40))
    yield 'plain', body.encode()
    yield 'crlf', body.replace('\n', '\r\n').encode()
    yield 'no trailing newline', body.rstrip('\n').encode()
    yield 'header', ('## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n' + body).encode()
    yield 'long line', (body[:200] + 'x' * 5000 + '\n' + body[200:]).encode()
    yield 'few lines', b'a\tb\t1\tc\t2\n#\n'
    yield 'one byte', b'\n'
    yield 'blank lines', b'\n\n\nr\tb\t1\tc\t2\n\n'
    yield 'empty', b''


@pytest.mark.parametrize('name,data', list(_files()), ids=[n for n, _ in _files()])
def test_owned_ranges_match_the_owner_of_each_line(name, data):
    for world in range(1, 17):
        bounds = ranks.byte_ranges(len(data), world)
        assert bounds[0][0] == 0 and bounds[-1][1] == len(data)
        assert all(bounds[r][1] == bounds[r + 1][0] for r in range(world - 1))
        got = [ranks.owned_range(data, b, e) for b, e in bounds]
        want = _brute(data, world)
        assert [data[lo:hi] for lo, hi in got] == want, (name, world)
        assert b''.join(data[lo:hi] for lo, hi in got) == data                     # every line once, in order
        assert all(got[r][1] == got[r + 1][0] for r in range(world - 1))


def test_a_line_longer_than_a_range_leaves_ranks_empty():
    data = b'x' * 1000 + b'\nab\n'
    got = [ranks.owned_range(data, b, e) for b, e in ranks.byte_ranges(len(data), 8)]
    assert got[0] == (0, 1001)
    assert sum(hi > lo for lo, hi in got) == 2                                  # the long line on rank 0, 'ab' on the rank holding byte 1001
    assert got[1][0] == got[1][1]                                               # [125, 250) lies inside the long line


def test_more_ranks_than_lines():
    data = b'a\nb\n'
    got = [ranks.owned_range(data, b, e) for b, e in ranks.byte_ranges(len(data), 16)]
    assert sum(hi > lo for lo, hi in got) == 2
    assert b''.join(data[lo:hi] for lo, hi in got) == data


def test_take_args():
    argv = ['--gpus', '4', '--host-transport', 'asm.fa', 'x.pairs', '10']
    assert ranks.take_args(argv) == (4, True)
    assert argv == ['asm.fa', 'x.pairs', '10']
    argv = ['asm.fa', 'x.pairs', '10', '--gpus', '1']
    assert ranks.take_args(argv) == (1, False) and argv == ['asm.fa', 'x.pairs', '10']
    argv = ['asm.fa']
    assert ranks.take_args(argv) == (None, False) and argv == ['asm.fa']
    for bad in (['--gpus'], ['--gpus', 'two'], ['--gpus', '0']):
        with pytest.raises(SystemExit):
            ranks.take_args(list(bad))


def test_child_env():
    env = ranks.child_env({'PATH': '/bin'}, 2, 4, 29500, True)
    assert (env['RANK'], env['WORLD_SIZE'], env['LOCAL_RANK'], env['MASTER_PORT']) == ('2', '4', '2', '29500')
    assert env['MASTER_ADDR'] == '127.0.0.1' and env['HAPHIC_HOST_TRANSPORT'] == '1' and env['PATH'] == '/bin'
    assert 'HAPHIC_HOST_TRANSPORT' not in ranks.child_env({}, 0, 2, 1, False)


def test_main_gpus_spawns_children_without_exec(monkeypatch):
    from haphic_amd import __main__ as M
    seen = []
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(ranks, 'launch', lambda cmd, world, host: seen.append((cmd, world, host)) or 7)
    assert M.main(['cluster', 'asm.fa', 'x.pairs', '12', '--gpus', '3', '--host-transport', '--reference', '/nowhere']) == 7
    cmd, world, host = seen[0]
    assert cmd[:4] == [sys.executable, '-m', 'haphic_amd', 'cluster'] and world == 3 and host is True
    assert '--gpus' not in cmd and '--host-transport' not in cmd and cmd[4:] == ['asm.fa', 'x.pairs', '12', '--reference', '/nowhere']
    with pytest.raises(SystemExit):
        M.main(['plot', 'a', '--gpus', '2'])


def test_launch_returns_the_first_failure_and_stops_the_rest(tmp_path):
    # two tiny children (no GPU): rank 1 fails at once, rank 0 would sleep for a minute — it is terminated
    script = tmp_path / 'child.py'
    script.write_text('import os, sys, time\nif os.environ["RANK"] == "1": sys.exit(5)\ntime.sleep(60)\n')
    import time
    t = time.perf_counter()
    assert ranks.launch([sys.executable, str(script)], 2, env=dict(os.environ, MASTER_PORT='1')) == 5
    assert time.perf_counter() - t < 30


def test_world_one_keeps_the_one_rank_paths(monkeypatch, tmp_path):
    from haphic_amd import cluster
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert ranks.init() is None and ranks.current() is None and not ranks.active()
    monkeypatch.setenv('WORLD_SIZE', '1')
    assert ranks.init() is None and not ranks.active()
    p = tmp_path / 'x.pairs'
    p.write_bytes(b'r\ta\t1\tb\t2\n')
    assert not cluster.PairsText(str(p), 'pairs', False).multi_rank()
    # run_rank without a context is the plain call
    calls = []
    assert ranks.run_rank(lambda: calls.append(1)) == 0 and calls == [1]
