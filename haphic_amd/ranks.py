"""One `haphic cluster` job as N ranks, one process per rank (`python -m haphic_amd cluster --gpus N ...`).

Rank 0 drives: it runs the reference's run() with the seams patched, exactly as a one-rank job does, and writes every file and log line.
Ranks > 0 serve: serve() joins the collective phases rank 0 announces with a small broadcast —

  correct_pass1  (from correct.parse_pairs_for_correction, --correct_nrounds): every rank tokenises the lines of its own byte range into a
          correction table of its own (_lib.CorrectTable: coverage difference array + kept intra-contig pairs in file order, no BED output);
          ranks > 0 export theirs and send it, rank 0 absorbs them IN RANK ORDER (hhx_correct_absorb) and finalizes: the table of one pass over
          the whole file, bit for bit.  Detection, breaking and the bookkeeping stay on rank 0 (O(contigs), on its device).
  ingest  (from the .pairs mirrors, cluster._ingest_handle): every rank reads the lines of its own byte range of the file (owned_range) and
          tokenises them on its device; rank 0 pushes its own chunks into its ingest handle as it parses them, then the other ranks' id /
          position arrays IN RANK ORDER.  The handle so sees the file's pairs in file order, as the one-rank run does: HT order, CLM lists,
          coordinates and ctg_pair_to_frag come out the same, and the writers run unchanged on rank 0.  Every rank writes its own BED records
          into alignments.bed at the offset of the ranks before it (a deferred byte sink, placed once the BED sizes are all-gathered).
          After a correction (correct.CorrectedPairsText) the spec carries the contig remap tables as well: every rank tokenises the ORIGINAL
          names, builds its own _lib.ContigRemap and converts both ends of every batch on its device (convert_ctg :1405-1411) before it sends;
          the intra-contig drop after the conversion (:1437) is the one of rank 0's ingest handle, applied once to the whole stream.
  sweep   (from run_mcl_clustering): rank 0 broadcasts the link matrix and the sweep parameters, every rank runs sharded.sweep_sharded, rank 0
          writes inflation_*/.
  done / abort

BAM and plain-gzip input have no byte ranges to share out: rank 0 reads them alone in every phase.  HAPHIC_RANKS_RECORD=DIR makes every rank
write DIR/rank<r>.json when it ends: per phase the lines it parsed, the pairs it kept, its seconds and the bytes it sent to rank 0.

The transport is RCCL (device to device) with one device per rank, or gloo with HostStagedCollectives (host_transport.py) when ranks share a
device (--host-transport; the default when there are more ranks than devices)."""
import datetime
import json
import os
import subprocess
import time

_CTX = None
TIMEOUT_S = int(os.environ.get('HAPHIC_RANKS_TIMEOUT_S', '1800'))       # a collective that waits longer than this fails the rank


class Context:
    """rank, world, device (LOCAL_RANK % device count) and the collectives of this job"""

    def __init__(self, rank, world, device, dist, raw, host_transport):
        self.rank, self.world, self.device = rank, world, device
        self.dist, self.raw, self.host_transport = dist, raw, host_transport


def current():
    return _CTX


# ------------------------------------------------------------------ the per-rank record
RECORD = []                              # this rank's share of every phase it took part in, in order


def record(phase, lines, pairs, seconds, bytes_sent=0):
    RECORD.append({'phase': phase, 'lines': int(lines), 'pairs': None if pairs is None else int(pairs), 'seconds': float(seconds),
                   'bytes_sent': int(bytes_sent)})


def write_record(rank):
    where = os.environ.get('HAPHIC_RANKS_RECORD')
    if where:
        with open(os.path.join(where, 'rank{}.json'.format(rank)), 'w') as f:
            json.dump({'rank': rank, 'world': _CTX.world if _CTX is not None else 1, 'phases': RECORD}, f)


def _dev():
    """the torch device of this rank's tensors (a context without a device, as the host-side tests make one, keeps them in host memory)"""
    return 'cpu' if _CTX.device is None else 'cuda:%d' % _CTX.device


def _torch_sync():
    if _CTX.device is not None:
        import torch
        torch.cuda.synchronize()


def active():
    """True when this process is one rank of a job of several: the mirrors then take their multi-rank paths"""
    return _CTX is not None and _CTX.world > 1


# ------------------------------------------------------------------ the byte-range rule
def byte_ranges(size, world):
    """the raw boundaries: rank r gets [r * size // world, (r + 1) * size // world)"""
    return [(r * size // world, (r + 1) * size // world) for r in range(world)]


def line_start(data, x):
    """the first line start at or after byte x: a line starts at 0 and after every b'\\n'; a boundary inside a line moves past its end"""
    if x <= 0 or x >= len(data) or data[x - 1] == 0x0A:
        return min(max(x, 0), len(data))
    k = data.find(b'\n', x)
    return len(data) if k < 0 else k + 1


def owned_range(data, begin, end):
    """[lo, hi): the bytes of the lines whose first byte lies in [begin, end) — what hhx_text_reader_open_range hands out (may be empty)"""
    lo = line_start(data, begin)
    return lo, max(lo, line_start(data, end))


# ------------------------------------------------------------------ command line
def take_args(argv):
    """--gpus N and --host-transport out of argv (in place); returns (gpus or None, host_transport)"""
    gpus, host = None, False
    if '--gpus' in argv:
        k = argv.index('--gpus')
        if k + 1 >= len(argv):
            raise SystemExit('--gpus needs a value')
        try:
            gpus = int(argv[k + 1])
        except ValueError:
            raise SystemExit('--gpus needs a number of ranks, got {!r}'.format(argv[k + 1]))
        if gpus < 1:
            raise SystemExit('--gpus needs at least 1 rank, got {}'.format(gpus))
        del argv[k:k + 2]
    if '--host-transport' in argv:
        argv.remove('--host-transport')
        host = True
    return gpus, host


def in_torchrun():
    return 'RANK' in os.environ and 'WORLD_SIZE' in os.environ


def child_env(base, rank, world, port, host_transport):
    env = dict(base)
    env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR=env.get('MASTER_ADDR', '127.0.0.1'),
               MASTER_PORT=str(port))
    if host_transport:
        env['HAPHIC_HOST_TRANSPORT'] = '1'
    return env


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def launch(cmd, world, host_transport=False, env=None, poll_s=0.2):
    """run `cmd` (a list) as `world` fresh child processes, one per rank; if one fails the others are terminated.  Returns the exit status
    (0, or the first failure's)"""
    env = os.environ if env is None else env
    port = int(env.get('MASTER_PORT') or free_port())
    procs = [subprocess.Popen(cmd, env=child_env(env, r, world, port, host_transport)) for r in range(world)]
    status = 0
    try:
        live = list(procs)
        while live:
            for p in list(live):
                rc = p.poll()
                if rc is None:
                    continue
                live.remove(p)
                if rc != 0 and status == 0:
                    status = rc if rc > 0 else 128 - rc
                    for q in live:
                        q.terminate()
            time.sleep(poll_s)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return status


# ------------------------------------------------------------------ the job context
def init(host_transport=None):
    """the context of this rank from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT (torchrun's or launch()'s); None for a
    one-rank job.  Sets the device of the library and of torch."""
    global _CTX
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1:
        _CTX = None
        return None
    import torch
    import torch.distributed as dist
    from . import _lib
    from .host_transport import HostStagedCollectives
    rank, local = int(os.environ['RANK']), int(os.environ.get('LOCAL_RANK', os.environ['RANK']))
    n_dev = _lib.device_count()
    if n_dev < 1:
        raise RuntimeError('haphic_amd: no GPU visible to rank {}'.format(rank))
    device = local % n_dev
    if host_transport is None:
        host_transport = os.environ.get('HAPHIC_HOST_TRANSPORT', '') == '1' or world > n_dev
    _lib.set_device(device)
    torch.cuda.set_device(device)
    timeout = datetime.timedelta(seconds=TIMEOUT_S)
    if host_transport:
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=timeout)
        coll = HostStagedCollectives(dist)
    else:
        dist.init_process_group('nccl', rank=rank, world_size=world, timeout=timeout, device_id=torch.device('cuda', device))
        coll = dist
    _CTX = Context(rank, world, device, coll, dist, host_transport)
    return _CTX


def shutdown():
    global _CTX
    if _CTX is not None:
        try:
            _CTX.raw.destroy_process_group()
        finally:
            _CTX = None


# ------------------------------------------------------------------ the phase protocol
def _broadcast(obj):
    box = [obj]
    _CTX.raw.broadcast_object_list(box, src=0)
    return box[0]


def announce(phase, payload=None):
    """rank 0: the other ranks enter `phase` with `payload`"""
    assert _CTX.rank == 0
    _broadcast((phase, payload))


def finish(ok):
    """rank 0 at the end of the job: `done`, or `abort` (every worker then exits non-zero)"""
    if active() and _CTX.rank == 0:
        announce('done' if ok else 'abort')


def serve():
    """ranks > 0: join the phases rank 0 announces until `done` (returns 0) or `abort` (returns 1)"""
    from . import _lib
    while True:
        phase, payload = _broadcast(None)
        if phase == 'ingest':
            _ingest_worker(payload)
        elif phase == 'correct_pass1':
            _correct_pass1_worker(payload)
        elif phase == 'sweep':
            _sweep_worker(payload)
        elif phase == 'done':
            _lib.files_join()                    # this rank's share of alignments.bed is on disk before the process ends
            return 0
        elif phase == 'abort':
            try:
                _lib.files_join()
            except RuntimeError:
                pass
            return 1
        else:
            raise RuntimeError('haphic_amd.ranks: unknown phase {!r}'.format(phase))


# ---- correct_pass1
def correct_spec(text, names, lens, resolution):
    """what rank 0 broadcasts for pass one of the assembly correction over a PairsText"""
    return {'path': os.path.abspath(text.path), 'format': text.aln_format, 'names': list(names), 'lens': [int(x) for x in lens],
            'resolution': int(resolution), 'chunk_bytes': int(text.chunk_bytes)}


def fill_table(table, text, names):
    """this rank's lines of `text` pushed into `table`; returns the number of lines"""
    lines = 0
    for parser, k in text.batches(names):
        lines += k
        if k:
            table.push_device(k, *parser.device_arrays()[:4])
    return lines


TABLE_PIECE = int(os.environ.get('HAPHIC_TABLE_PIECE', str(1 << 26)))     # kept pairs per message of a correction table (12 bytes each)


def _pieces(n):
    return [(lo, min(TABLE_PIECE, n - lo)) for lo in range(0, n, max(TABLE_PIECE, 1))]


def _send_table(table):
    """ranks > 0: the shapes all-gathered, then this rank's table in int32 messages — the difference array, then the kept pairs TABLE_PIECE at a
    time as [contig ids | lo, hi interleaved], so that neither a message nor rank 0's staging grows with the table; returns (kept pairs, bytes sent)"""
    import numpy as np
    import torch
    res, n_bins, n = table.export_shape()
    shapes = [None] * _CTX.world
    _CTX.dist.all_gather_object(shapes, (res, n_bins, n))
    host = _CTX.host_transport               # the wire is host memory anyway: host copies straight from the library
    if n_bins:
        if host:
            _CTX.raw.send(torch.from_numpy(table.export_diff()), 0)
        else:
            blob = torch.empty(n_bins, dtype=torch.int32, device=_dev())
            table.export_device(blob.data_ptr(), 0, 0, 0, 0)
            _CTX.dist.send(blob, 0)
    for first, m in _pieces(n):
        if host:
            _CTX.raw.send(torch.from_numpy(np.concatenate(table.export_pairs(first, m))), 0)
        else:
            blob = torch.empty(3 * m, dtype=torch.int32, device=_dev())
            table.export_device(0, first, m, blob.data_ptr(), blob.data_ptr() + 4 * m)
            _CTX.dist.send(blob, 0)
    return n, 4 * (n_bins + 3 * n)


def gather_tables(table):
    """rank 0, after its own lines: the other ranks' tables absorbed in rank order, which is file order, piece by piece as _send_table sends them"""
    import torch
    res, n_bins, _n = table.export_shape()
    shapes = [None] * _CTX.world
    _CTX.dist.all_gather_object(shapes, (res, n_bins, 0))
    host = _CTX.host_transport

    def receive(count, r):
        blob = torch.empty(count, dtype=torch.int32, device='cpu' if host else _dev())
        (_CTX.raw if host else _CTX.dist).recv(blob, r)
        if not host:
            _torch_sync()
        return blob

    for r in range(1, _CTX.world):
        res_r, nb_r, n_r = shapes[r]
        if nb_r:
            blob = receive(nb_r, r)
            if host:
                table.absorb(res_r, blob.numpy(), [], [])
            else:
                table.absorb_device(res_r, nb_r, blob.data_ptr(), 0, 0, 0)          # returns once it has read the tensor
        elif (res_r, nb_r) != (res, n_bins):
            raise RuntimeError('haphic_amd.ranks: rank {} built a correction table of another shape'.format(r))
        for _first, m in _pieces(n_r):
            blob = receive(3 * m, r)
            if host:
                a = blob.numpy()
                table.absorb(res_r, None, a[:m], a[m:])
            else:
                table.absorb_device(res_r, nb_r, 0, m, blob.data_ptr(), blob.data_ptr() + 4 * m)


def _correct_pass1_worker(spec):
    from . import _lib, cluster
    t0 = time.perf_counter()
    table = _lib.CorrectTable(spec['lens'], spec['resolution'])
    try:
        text = cluster.PairsText(spec['path'], spec['format'], False, chunk_bytes=spec['chunk_bytes'], bed_path=None)
        lines = fill_table(table, text, spec['names'])
        kept, sent = _send_table(table)
    finally:
        table.destroy()
    record('correct_pass1', lines, kept, time.perf_counter() - t0, sent)


# ---- ingest
def ingest_spec(text, names, wide):
    """what rank 0 broadcasts for the ingest phase of a PairsText: `names` are the names to tokenise — after a correction the ORIGINAL contigs
    (the sources of correct._remap_tables), with the remap tables (off, break_pos, new_id) every rank builds its _lib.ContigRemap from"""
    remap = getattr(text, 'remap_tables', None)
    return {'path': os.path.abspath(text.path), 'format': text.aln_format, 'inter_only': bool(text.inter_only), 'names': list(names),
            'wide': bool(wide), 'bed_path': os.path.abspath(text.bed_path) if text.bed_path else None, 'chunk_bytes': int(text.chunk_bytes),
            'remap': None if remap is None else tuple(a.tolist() for a in remap)}


def bed_bases(my_bytes):
    """all-gather of every rank's alignments.bed size: this rank's offset in the file"""
    sizes = [None] * _CTX.world
    _CTX.dist.all_gather_object(sizes, int(my_bytes))
    return sum(sizes[:_CTX.rank])


def _take(parser, k, wide):
    """the parsed chunk's pairs (lines with an unknown name or no pair dropped, as hhx_ingest_push would) as one device tensor [4, n] of the
    position type, copied before the parser's next chunk overwrites its arrays"""
    import torch
    from . import _lib
    from .sharded import HipEngine
    _lib.synchronize()
    eng = HipEngine('cuda:%d' % _CTX.device)
    p = parser.device_arrays()
    pt, pd = ('<i8', torch.int64) if wide else ('<i4', torch.int32)
    id1, id2 = eng.view(p[0], k, '<i4', torch.int32), eng.view(p[2], k, '<i4', torch.int32)
    keep = (id1 >= 0) & (id2 >= 0)
    out = torch.stack([id1[keep].to(pd), eng.view(p[1], k, pt, pd)[keep], id2[keep].to(pd), eng.view(p[3], k, pt, pd)[keep]])
    torch.cuda.synchronize()
    return out


def _ingest_worker(spec):
    import torch
    from . import _lib, cluster
    t0 = time.perf_counter()
    text = cluster.PairsText(spec['path'], spec['format'], spec['inter_only'], chunk_bytes=spec['chunk_bytes'], bed_path=spec['bed_path'])
    remap = _lib.ContigRemap(*spec['remap']) if spec.get('remap') else None
    parts, lines = [], 0
    try:
        for parser, k in text.batches(spec['names'], wide=spec['wide']):
            lines += k
            if k:
                if remap is not None:        # convert_ctg :1405-1411 on both ends, on this rank's device; the BED bytes were formatted before
                    ptrs = parser.device_arrays()
                    remap.apply(k, ptrs[0], ptrs[1])
                    remap.apply(k, ptrs[2], ptrs[3])
                parts.append(_take(parser, k, spec['wide']))
    finally:
        if remap is not None:
            remap.destroy()
    mine = torch.cat(parts, 1) if parts else torch.empty((4, 0), dtype=torch.int64 if spec['wide'] else torch.int32, device=_dev())
    del parts
    counts = [None] * _CTX.world
    _CTX.dist.all_gather_object(counts, int(mine.shape[1]))
    if counts[_CTX.rank]:
        _CTX.dist.send(mine.contiguous(), 0)
    record('ingest', lines, mine.shape[1], time.perf_counter() - t0, mine.numel() * mine.element_size())


def gather_into(ing, wide):
    """rank 0, after its own chunks: the other ranks' pairs pushed into `ing` in rank order"""
    import torch
    counts = [None] * _CTX.world
    _CTX.dist.all_gather_object(counts, 0)
    for r in range(1, _CTX.world):
        if not counts[r]:
            continue
        buf = torch.empty((4, counts[r]), dtype=torch.int64 if wide else torch.int32, device=_dev())
        _CTX.dist.recv(buf, r)
        id1, id2 = buf[0].to(torch.int32).contiguous(), buf[2].to(torch.int32).contiguous()
        p1, p2 = buf[1].contiguous(), buf[3].contiguous()
        _torch_sync()
        ing.push_device(counts[r], id1.data_ptr(), p1.data_ptr(), id2.data_ptr(), p2.data_ptr(), wide=wide)
        from . import _lib
        _lib.check(_lib.load().hhx_synchronize())            # the push has read the tensors before they go
        del buf, id1, id2, p1, p2


# ---- sweep
def share_sweep(m, payload):
    """rank 0 in run_mcl_clustering: the others join the sweep over the same link matrix; returns the collectives for dist="""
    indptr, indices, data = m.to_arrays()
    announce('sweep', dict(payload, csr=(indptr, indices, data, int(m.shape3[1]))))
    return _CTX.dist


def _sweep_worker(payload):
    from . import _lib, cluster
    indptr, indices, data, n_cols = payload.pop('csr')
    m = _lib.DeviceCSR.from_arrays(indptr, indices, data, n_cols)
    cluster.run_mcl_clustering(m, dist=_CTX.dist, **payload)


# ------------------------------------------------------------------ a rank's process
def run_rank(drive):
    """the body of one rank's process: rank 0 calls drive() and announces done / abort; the other ranks serve().  Returns the exit status."""
    ctx = current()
    if ctx is None or ctx.rank == 0:
        ok = False
        try:
            drive()
            ok = True
        finally:
            try:
                if ok:
                    write_record(0)
            finally:
                if ctx is not None:
                    try:
                        finish(ok)
                    finally:
                        shutdown()
        return 0
    try:
        status = serve()
        if status == 0:
            write_record(ctx.rank)
        return status
    finally:
        shutdown()
