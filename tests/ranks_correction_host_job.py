"""One rank of the host-side twin of tests/ranks_correction_job.py, for tests/test_ranks_correction_host.py: no GPU.  The process group is
gloo, the context has no device, and `_lib` is the numpy stand-in of tests/correction_fixture.py with what a multi-rank job needs on top
(a ranged text reader over ranks.owned_range, export / absorb on the table).  What runs unchanged: ranks.announce / serve and their phases
`correct_pass1` and `ingest`, correct.parse_pairs_for_correction with its rank-order merge, ranks.ingest_spec carrying the remap tables,
ranks._ingest_worker building its remap from them, ranks.gather_into.  What is stood in for: the device (ranks._take hands over host tensors).

    python tests/ranks_correction_host_job.py PAIRS OUT.json        (RANK / WORLD_SIZE / MASTER_* from ranks.launch)"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stand_in_lib():
    from haphic_amd import ranks
    from tests import correction_fixture
    lib = correction_fixture.stand_in_lib()

    class Table(correction_fixture.CorrectTable):
        """+ hhx_correct_export / hhx_correct_absorb: the kept records in push order and the difference array, as the library keeps them"""

        def __init__(self, ctg_len, resolution):
            super().__init__(ctg_len, resolution)
            self.got_diff = self.want_diff = 0                    # difference arrays absorbed / those of the absorbed records

        def _bins(self):
            return [n // self.res + 1 for n in self.lens]

        def _kept(self):
            rows = [np.stack(p, 1) for p in self.parts] or [np.zeros((0, 4), np.int64)]
            a = np.concatenate(rows)
            return a[(a[:, 0] == a[:, 2]) & (a[:, 0] >= 0) & (a[:, 0] < len(self.lens))]

        def export_shape(self):
            return self.res, sum(self._bins()), len(self._kept())

        def export_diff(self):
            k = self._kept()
            off = np.concatenate(([0], np.cumsum(self._bins())))
            diff = np.zeros(off[-1], np.int32)
            lo, hi = np.minimum(k[:, 1], k[:, 3]), np.maximum(k[:, 1], k[:, 3])
            for c, a, b in zip(k[:, 0].tolist(), (lo // self.res).tolist(), (hi // self.res).tolist()):
                nb = off[c + 1] - off[c]
                if a < nb:
                    diff[off[c] + a] += 1
                if b + 1 < nb:
                    diff[off[c] + b + 1] -= 1
            return diff

        def export_pairs(self, first, count):
            k = self._kept()[first:first + count]
            lo, hi = np.minimum(k[:, 1], k[:, 3]), np.maximum(k[:, 1], k[:, 3])
            return k[:, 0].astype(np.int32), np.stack([lo, hi], 1).reshape(-1).astype(np.int32)

        def absorb(self, resolution, cov_diff, pair_ctg, pair_lo_hi):
            if int(resolution) != self.res or (cov_diff is not None and len(cov_diff) != sum(self._bins())):
                raise RuntimeError('absorb: shape mismatch')
            if cov_diff is not None:
                self.got_diff = self.got_diff + np.asarray(cov_diff, np.int64)
            ctg, lh = np.asarray(pair_ctg, np.int64), np.asarray(pair_lo_hi, np.int64).reshape(-1, 2)
            if len(ctg):
                piece = Table(self.lens, self.res)
                piece.parts = [[ctg, lh[:, 0], ctg, lh[:, 1]]]
                self.want_diff = self.want_diff + piece.export_diff().astype(np.int64)
                self.parts.append([ctg, lh[:, 0], ctg, lh[:, 1]])

        def finalize(self):
            assert np.array_equal(self.got_diff, self.want_diff), 'the difference arrays absorbed are not those of the records absorbed'
            return super().finalize()

    class TextReader:
        """hhx_text_reader_open_range over a plain file: the lines whose first byte lies in the byte range, in chunks of whole lines"""

        def __init__(self, path, chunk_bytes, threads=1, bgzf=False, byte_range=None):
            assert not bgzf and byte_range is not None
            with open(path, 'rb') as f:
                data = f.read()
            lo, hi = ranks.owned_range(data, *byte_range)
            self.chunks, at = [], lo
            while at < hi:
                end = min(at + max(int(chunk_bytes), 1), hi)
                cut = hi if end == hi else data.rfind(b'\n', at, end) + 1
                if cut <= at:
                    k = data.find(b'\n', end, hi)
                    cut = hi if k < 0 else k + 1
                self.chunks.append(data[at:cut])
                at = cut

        def __iter__(self):
            return iter((c, len(c)) for c in self.chunks)

        def close(self):
            pass

    class PairsParser(lib.PairsParser):
        def parse(self, text, want_bed=False, device_ptr=None, n_bytes=None, host_ptr=None):
            n = super().parse(host_ptr if text is None else text, want_bed=want_bed)
            self.arr = [np.array(a) for a in self.arr]            # the remap works in place
            return n

    lib.CorrectTable, lib.TextReader, lib.PairsParser = Table, TextReader, PairsParser
    return lib


class Collector:
    """what cluster._ingest_handle's _lib.Ingest is to ranks.gather_into: it takes pushes of host pointers"""

    def __init__(self):
        self.rows = []

    def push_device(self, n, id1, pos1, id2, pos2, wide=False):
        cols = [np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), (n,)).copy() for p in (id1, pos1, id2, pos2)]
        self.rows.append(np.stack(cols, 1))

    def push(self, cols):
        self.rows.append(np.stack([np.asarray(c, np.int32) for c in cols], 1))

    def stream(self):
        return np.concatenate(self.rows).tolist() if self.rows else []


def _take(parser, k, wide):
    import torch
    a = [np.asarray(x[:k], np.int32) for x in parser.device_arrays()[:4]]
    keep = (a[0] >= 0) & (a[2] >= 0)
    return torch.from_numpy(np.stack([x[keep] for x in a]))


def drive(pairs, out_path):
    import types
    from haphic_amd import cluster, correct, ranks
    from tests import correction_fixture
    fx = correction_fixture.load()
    names = fx['names']
    fa = {n: [None, int(l), 1] for n, l in zip(names, fx['lens'].tolist())}
    args = types.SimpleNamespace(alignments=pairs, aln_format='pairs', correct_resolution=int(fx['res']))
    # ---- pass one: the phase `correct_pass1`, the tables absorbed in rank order
    cov_d, pos_d = correct.parse_pairs_for_correction(fa, args)
    session = cov_d._session
    out = {'cov': [[n, v.tolist()] for n, v in session.cov_items()], 'pos': [[n, v.tolist()] for n, v in session.pos_items()]}
    # ---- pass two: the first half of every third contig becomes a piece of its own; the remap tables go out with the ingest spec
    fpos, ffrag, corrected = {}, {}, []
    for k, n in enumerate(names):
        if k % 3 == 0:
            cut = (fa[n][1] // 2) // 500 * 500
            kids = ['%s:1-%d' % (n, cut), '%s:%d-%d' % (n, cut + 1, fa[n][1])]
            fpos[n], ffrag[n] = [cut, 0], kids[::-1]
    corrected = [n for n in names if n not in fpos] + [kid for n in fpos for kid in ffrag[n][::-1]]
    text = correct.pairs_generator_for_correction_ctg(pairs, 'pairs', fpos, ffrag)
    text.bed_path = None
    text.chunk_bytes = 100_000                                    # several chunks per rank
    assert text.multi_rank() and text.inter_only
    src_names, remap = text.remap_for(corrected)
    ranks.announce('ingest', ranks.ingest_spec(text, src_names, False))
    ing, lines = Collector(), 0
    for parser, k in text.batches(src_names):
        lines += k
        if k:
            p = parser.device_arrays()
            remap.apply(k, p[0], p[1])
            remap.apply(k, p[2], p[3])
            keep = (p[0][:k] >= 0) & (p[2][:k] >= 0)
            ing.push([x[:k][keep] for x in p[:4]])
    ranks.gather_into(ing, False)
    ranks.record('ingest', lines, None, 0.0)                     # as cluster._ingest_handle does for rank 0
    out['pass_two'] = ing.stream()
    out['src_names'], out['corrected'] = list(src_names), corrected
    out['fpos'], out['ffrag'] = fpos, ffrag
    out['record'] = ranks.RECORD
    with open(out_path, 'w') as f:
        json.dump(out, f)


def main():
    pairs, out_path = sys.argv[1:3]
    import datetime
    import torch.distributed as dist
    import haphic_amd
    from haphic_amd import cluster, correct, ranks
    from haphic_amd.host_transport import HostStagedCollectives
    lib = stand_in_lib()
    haphic_amd._lib = lib
    cluster._lib = correct._lib = lib
    ranks._take = _take
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    ranks._CTX = ranks.Context(rank, world, None, HostStagedCollectives(dist), dist, True)
    status = ranks.run_rank(lambda: drive(pairs, out_path))
    if rank > 0:
        with open('%s.rank%d' % (out_path, rank), 'w') as f:
            json.dump(ranks.RECORD, f)
    return status


if __name__ == '__main__':
    sys.exit(main())
