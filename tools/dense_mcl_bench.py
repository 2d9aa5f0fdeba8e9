#!/usr/bin/env python3
"""The --dense_matrix mode on one MI355X (csrc/hhx_densemcl.hip): profiles/dense_mcl_bench.json and profiles/dense_mcl_parity.json.

    python tools/dense_mcl_bench.py [--out DIR] [--gemm 4096,8192,16384,32768] [--mcl 2048,4096,8192,32768] [--sparse 2048,4096,8192] [--cpu 8192]
                                    [--cpu-first-product 32768]

gemm     k_dmcl_gemm alone on column-stochastic float32 operands: HIP-event time of the kernel (hhx_profile, "dmcl_gemm") over `reps` launches after a
         warm-up, 2 n^3 flop over it, beside the 122 TF of the kernel guide's untuned LDS-tiled kernel at 4096^3 and the 157 TF float32 peak
mcl      a whole mcl() at inflation 2.0 on a planted link matrix (4 chromosomes' worth of clusters, density 0.3 / 0.01, counts 1..39): wall seconds
         (host clock around the call, which ends in a device synchronise), rounds, and the HIP-event seconds of the product, the epilogue and the
         convergence test per round
cpu      the yardstick for time: the same recurrence in numpy float32 on this box's CPUs (the host model of tests/dense_mcl_cases.py: the reference's
         numpy calls — matmul, power, column sums, prune, allclose — without sklearn; the reference itself is not on the GPU box), in full at
         --cpu orders and the first product alone at --cpu-first-product orders
sparse   the sparse mode (hhx_mcl_links: the project's own mcl() on CSR, its own convergence rule) on the SAME planted matrices, wall seconds and rounds:
         where a dense run stops being the faster of the two
parity   per golden case the device's worst |device - float64| over the rounds, each from the device's own state, beside the reference's ref_step_err
No tile skipping is built, so no share of skipped K-blocks is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haphic_amd import _lib, build  # noqa: E402

PEAK_TF = 157.0
GUIDE_TF_4096 = 122.0


def stochastic(n, seed):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    m = torch.rand((n, n), device='cuda', generator=g)
    m /= m.sum(dim=0, keepdim=True)
    return m.cpu().numpy()


def planted_links(n, seed, k=4):
    """the planted matrix of the tests at a user's size, drawn on the device (numpy would take a minute at n = 32768)"""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    label = torch.sort(torch.randint(0, k, (n,), device='cuda', generator=g)).values
    same = label[:, None] == label[None, :]
    keep = torch.rand((n, n), device='cuda', generator=g) < torch.where(same, 0.3, 0.01)
    cnt = torch.randint(1, 40, (n, n), device='cuda', generator=g).float() * keep
    del keep, same
    cnt = torch.triu(cnt, 1)
    cnt = cnt + cnt.T
    cnt.fill_diagonal_(1.0)
    return cnt.cpu().numpy()


def event_ms(name):
    return _lib.profile_get(name)


def bench_gemm(n, reps):
    m = stochastic(n, n)
    a = _lib.DenseMatrix.from_numpy(m)
    del m
    _lib.dmat_gemm(a, a).free()                                      # warm-up: code object, pool blocks
    _lib.load().hhx_synchronize()
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(reps):
        _lib.dmat_gemm(a, a).free()
    _lib.load().hhx_synchronize()
    ms, launches = event_ms('dmcl_gemm')
    _lib.profile_enable(False)
    a.free()
    per = ms / launches / 1e3
    tf = 2.0 * n ** 3 / per / 1e12
    return dict(n=n, launches=launches, seconds_per_product=per, tflops=tf, share_of_f32_peak=tf / PEAK_TF, guide_untuned_tflops_4096=GUIDE_TF_4096,
                f32_peak_tflops=PEAK_TF)


def bench_mcl(n, inflation=2.0, expansion=2, max_iter=200, pruning=1e-4):
    links = _lib.DenseMatrix.from_numpy(planted_links(n, n + 1))
    _lib.dmat_normalize_l1(links)
    t0 = time.perf_counter()
    pre = _lib.dmat_power(links, expansion)
    _lib.load().hhx_synchronize()
    t_pre = time.perf_counter() - t0
    links.free()
    res, _, _ = _lib.dmat_mcl(pre, expansion, inflation, 3, pruning)          # warm-up of every kernel and pool block of the loop
    res.free()
    _lib.profile_enable(True)
    _lib.profile_reset()
    t0 = time.perf_counter()
    res, rounds, converged = _lib.dmat_mcl(pre, expansion, inflation, max_iter, pruning)
    wall = time.perf_counter() - t0
    parts = {k: event_ms('dmcl_' + k) for k in ('gemm', 'epilogue', 'allclose')}
    _lib.profile_enable(False)
    csr = res.to_csr()
    nnz = csr.nnz
    csr.free(), res.free(), pre.free()
    out = dict(n=n, inflation=inflation, expansion=expansion, rounds=rounds, converged=converged, wall_seconds=wall, seconds_per_round=wall / rounds,
               pre_expansion_seconds=t_pre, final_nnz=nnz)
    for k, (ms, launches) in parts.items():
        out[k + '_seconds_total'], out[k + '_launches'] = ms / 1e3, launches
        out[k + '_seconds_per_launch'] = ms / 1e3 / max(launches, 1)
    out['product_share_of_wall'] = out['gemm_seconds_total'] / wall
    return out


def bench_sparse(n, inflation=2.0, expansion=2, max_iter=200, pruning=1e-4):
    import scipy.sparse as sp
    links = _lib.DeviceCSR.from_scipy_csc(sp.csc_matrix(planted_links(n, n + 1)))
    nnz = links.nnz
    res, _, _ = _lib.mcl(links, expansion, inflation, 3, pruning, links=True)           # warm-up
    res.free()
    _lib.load().hhx_synchronize()
    t0 = time.perf_counter()
    res, rounds, converged = _lib.mcl(links, expansion, inflation, max_iter, pruning, links=True)
    _lib.load().hhx_synchronize()
    wall = time.perf_counter() - t0
    res.free(), links.free()
    return dict(n=n, link_nnz=nnz, inflation=inflation, expansion=expansion, rounds=rounds, converged=bool(converged), wall_seconds=wall,
                seconds_per_round=wall / rounds)


def bench_cpu(n, full, inflation=2.0, expansion=2, max_iter=200, pruning=1e-4):
    from tests import dense_mcl_cases as dc
    links = planted_links(n, n + 1)
    m = dc.normalize_l1(links)
    del links
    t0 = time.perf_counter()
    pre = m @ m
    t_first = time.perf_counter() - t0
    out = dict(n=n, cpus=len(os.sched_getaffinity(0)), omp_num_threads=os.environ.get('OMP_NUM_THREADS'), first_product_seconds=t_first,
               first_product_tflops=2.0 * n ** 3 / t_first / 1e12)
    if full:
        t0 = time.perf_counter()
        _, rounds, converged, _ = dc.mcl(pre, expansion, inflation, max_iter, pruning)
        wall = time.perf_counter() - t0
        out.update(rounds=rounds, converged=converged, wall_seconds=wall, seconds_per_round=wall / rounds)
    return out


def parity():
    from tests import dense_mcl_cases as dc
    from tests.conftest import load_golden
    from tests.test_dense_mcl_cpu import source_of
    from tests.test_gpu_dense_mcl import device_pre, f64_round_with_band
    golden = load_golden('dense_mcl.npz')
    rows = []
    for case in dc.cases():
        err = float(golden[case.name + '_ref_step_err'])
        cur = device_pre(_lib, golden, case)
        worst = 0.0
        for k in range(int(golden[case.name + '_rounds'])):
            state = cur.to_numpy()
            nxt, _, _ = _lib.dmat_mcl(cur, case.expansion, case.inflation, k + 1, case.pruning, done=k)
            cur.free()
            cur = nxt
            got = cur.to_numpy()
            want, _ = f64_round_with_band(state.astype(np.float64), k, case, got, 4 * err)
            worst = max(worst, float(np.abs(got - want).max()))
        cur.free()
        rows.append(dict(case=case.name, n=int(source_of(golden, case)[0]) if not case.public else 8, device_worst_abs_err=worst, ref_step_err=err,
                         ratio=(worst / err if err else None)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--gemm', default='4096,8192,16384,32768')
    ap.add_argument('--mcl', default='2048,4096,8192,32768')
    ap.add_argument('--sparse', default='2048,4096,8192')
    ap.add_argument('--cpu', default='8192')
    ap.add_argument('--cpu-first-product', default='32768')
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(',') if x]            # noqa: E731
    _lib.load()
    assert _lib.device_count() >= 1, 'needs a GPU'
    os.makedirs(args.out, exist_ok=True)
    res = dict(source_hash=build.source_hash(), gemm=[], mcl=[], sparse=[], cpu=[])

    def save():
        with open(os.path.join(args.out, 'dense_mcl_bench.json'), 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
    for n in ints(args.gemm):
        res['gemm'].append(bench_gemm(n, args.reps))
        print(json.dumps(res['gemm'][-1]), flush=True)
        save()
    for n in ints(args.mcl):
        res['mcl'].append(bench_mcl(n))
        print(json.dumps(res['mcl'][-1]), flush=True)
        save()
    for n in ints(args.sparse):
        res['sparse'].append(bench_sparse(n))
        print(json.dumps(res['sparse'][-1]), flush=True)
        save()
    for g, c in ((g, c) for g in res['mcl'] for c in res['sparse'] if c['n'] == g['n']):
        g['sparse_mode_wall_seconds'] = c['wall_seconds']
    with open(os.path.join(args.out, 'dense_mcl_parity.json'), 'w') as fh:
        json.dump(dict(source_hash=res['source_hash'], cases=parity()), fh, indent=1)
        fh.write('\n')
    for n in ints(args.cpu):
        res['cpu'].append(bench_cpu(n, True))
        print(json.dumps(res['cpu'][-1]), flush=True)
        save()
    for n in ints(args.cpu_first_product):
        res['cpu'].append(bench_cpu(n, False))
        print(json.dumps(res['cpu'][-1]), flush=True)
        save()
    for g, c in ((g, c) for g in res['mcl'] for c in res['cpu'] if c['n'] == g['n'] and 'wall_seconds' in c):
        g['cpu_wall_seconds'], g['speedup_over_numpy'] = c['wall_seconds'], c['wall_seconds'] / g['wall_seconds']
    save()


if __name__ == '__main__':
    main()
