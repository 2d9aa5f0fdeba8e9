"""The handle classes that gained a finaliser (PlotNorm, ContactMap) or moved into _lib (ShardBuild), and the aliases of the release, on the
device at the smallest valid shapes."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _scaled(pn):
    """apply() wants a balancing that converged: one block over the whole matrix"""
    pn.set_blocks([0], [pn.n])
    assert not pn.balance()[2].any()
    return pn.apply()


def test_plot_norm_with_block_and_finaliser():
    from haphic_amd import _lib
    counts = np.eye(4, dtype=np.int64)
    with _lib.PlotNorm(counts) as pn:
        assert pn.h and pn.n == 4
        got = _scaled(pn)
    assert pn.h is None
    pn.destroy()                                        # a no-op after the block
    assert pn.h is None
    second = _lib.PlotNorm(counts)
    assert got.shape == (4, 4) and np.array_equal(got, _scaled(second))
    second.destroy()
    third = _lib.PlotNorm(counts)
    del third                                           # nobody released it: the finaliser does
    gc.collect()
    with _lib.PlotNorm(counts) as fourth:
        assert np.array_equal(_scaled(fourth), got)


def test_contact_map_with_block():
    from haphic_amd.plot import ContactTable
    from oracle import plot_oracle as po
    from tests.test_plot import _flat_inputs
    bin_size = 5000
    agp = 'group1\t1\t9000\t1\tW\tctg0\t1\t9000\t+\n'  # one contig over two bins
    cd, cad, sizes, frags, gfd = po.parse_agp(agp, bin_size)
    mat, to_total, group_list, ctg_set = po.generate_contact_matrix(sizes, frags, gfd, bin_size, 0, None)
    assert mat.shape == (2, 2)
    table = ContactTable(cd, cad, bin_size, to_total, group_list, ctg_set, mat.shape[0])
    records = [('ctg0', 10, 'ctg0', 7000), ('ctg0', 6000, 'ctg0', 8999)]
    inputs = _flat_inputs(table, records)
    want, bad = po.bin_flat(*table.arrays, bin_size, mat.shape[0], *inputs)
    assert bad == -1 and want.sum() > 0
    with table.device() as cm:
        assert cm.push(*inputs) == -1
        got = cm.fetch()
    assert cm.h is None and np.array_equal(got, want)
    cm.destroy()
    del cm
    gc.collect()


def test_shard_build_is_the_engine_s_round_trip():
    import torch
    from haphic_amd import _lib, sharded
    from haphic_amd.cluster import FragTable
    torch.cuda.set_device(0)
    _lib.set_device(0)
    table = FragTable.for_contigs(np.arange(3, dtype=np.int32), np.full(3, 1_000_000, np.int64), np.ones(3, np.uint8))
    ing = _lib.Ingest(table, 500_000, bins=False, skip_intra=True)
    ing.push(np.array([0, 1, 0, 0], np.int32), np.array([10, 20, 999_000, 30], np.int32),
             np.array([1, 2, 2, 1], np.int32), np.array([999_990, 40, 50, 60], np.int32))
    ing.finalize()
    in_set = np.ones(3, np.uint8)
    eng = sharded.HipEngine('cuda:0')
    # through the engine, as build_link_matrix_sharded drives it
    st = eng.shard_open(ing, in_set)
    assert isinstance(st, _lib.ShardBuild)
    first_e = eng.shard_first(st).clone()
    fidx_e, n_linked_e = eng.rank_first(first_e)
    w0, w1, counts_e = eng.shard_emit(st, fidx_e, [0, 3])
    eng.sync()
    w0_e, w1_e = w0.cpu().numpy(), w1.cpu().numpy()
    block = eng.rows_from_entries(w0, w1, 0, 3, 3, recv_counts=counts_e)
    eng.shard_close(st)
    assert st.h is None
    eng.shard_close(st)
    # the handle itself
    with _lib.ShardBuild(ing, in_set) as sb:
        assert sb.n_frag == 3
        first = eng.view(sb.first(), 3, '<i8', torch.int64).clone()
        fidx = torch.empty(3, dtype=torch.int32, device='cuda:0')
        torch.cuda.synchronize()
        n_linked = _lib.rank_first(3, first.data_ptr(), fidx.data_ptr())
        p0, p1, counts = sb.emit(fidx.data_ptr(), [0, 3])
        n = int(counts.sum())
        eng.sync()
        got0, got1 = (eng.view(p, n, '<i8', torch.int64).cpu().numpy() for p in (p0, p1))
    assert sb.h is None
    assert np.array_equal(first.cpu().numpy(), first_e.cpu().numpy()) and np.array_equal(fidx.cpu().numpy(), fidx_e.cpu().numpy())
    assert n_linked == n_linked_e == 3 and counts.tolist() == counts_e and n > 0
    assert np.array_equal(got0, w0_e) and np.array_equal(got1, w1_e)
    # one rank's block is the whole link matrix of the one-GPU path
    m, fi, nl = ing.link_matrix(in_set)
    assert nl == 3 and np.array_equal(fi, fidx.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(block.to_arrays(), m.to_arrays()))
    for h in (block, m, ing):
        h.close()


def test_device_csr_aliases_and_copy():
    from haphic_amd import _lib
    m = _lib.DeviceCSR.from_arrays([0, 1, 3], [0, 0, 1], [1.0, 2.0, 3.0])
    c = m.copy()
    m.free()
    m.free()
    assert m.h is None
    assert c.nnz == 3 and c.shape3 == (2, 2, 3)
    assert np.array_equal(c.to_arrays()[2], np.array([1, 2, 3], np.float32))
    c.destroy()
    assert c.h is None
