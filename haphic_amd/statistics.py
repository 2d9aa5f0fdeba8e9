"""output_statistics :2279-2478, the last step of `haphic cluster`, on the device tables.

The reference's function builds, per inflation, ctg_group_link_dict = parse_link_dict(full_link_dict, ctg_group_dict) :2252-2268 — one Python dict entry
per (contig, group) cell — sorts every contig's cells (:2365), keeps three numbers per contig (links to the best group, their density, the ratio of
that density to the average density of the other groups, :2366-2384), sorts each of the three lists, accumulates them into the axes of generate_axes
:2281-2301 and writes four text files and statistics.pdf.  Here the cells are never built: one call of hhx_ingest_group_stats
(haphic_amd/csrc/hhx_groupstats.hip) on the contig-pair table of the ingest handle returns, for every inflation at once, the number of cells, the
first cell and the ordered sum of the other cells' densities per contig; the remaining divisions, the stable sorts and the cumulative axes are numpy
on arrays of len(fa_dict), in the same IEEE operations as the reference's Python.

What the mirror has to carry besides the numbers is the TYPE of each value: the reference's lists mix int (0 for a contig without cells, 1000000 for a
ratio without other groups, the link counts) and float, generate_axes keys its dicts by them (0 == 0.0, 1000000 == 1000000.0 are ONE key), and the
text printed for a merged key is that of whichever was inserted first — the initial int 0, or the first in stable sorted order.

Served: a still-frozen full_link_dict (cluster._frozen(link_dict, 'full')) with integer counts on a one-rank session, contigs with at least one RE
site.  Everything else — a thawed or plain dict, float values after reduce_inter_hap_HiC_links or the concentrated-links loop, a rank of a multi-rank
job, HHX_UNSUPPORTED, names the table does not know — goes to the reference's own function (`_original`, bound by
patch.patch_reference(H, statistics=True)), under which cluster.group_link_dict stays bound as before."""
import sys
import time

import numpy as np

from . import _lib
from .cluster import _frozen, logger

SENTINEL_RATIO = 1000000            # :2383
SUM_MODE = 1 if sys.version_info >= (3, 12) else 0      # sum() of floats: plain up to CPython 3.11, Neumaier-compensated from 3.12
STATS = {}                          # the last call's timing split (tools/statistics_bench.py); device_s = everything before the first file, prepare_s = its host part


def generate_axes(values, is_int, lengths, total_n, total_len):
    """generate_axes :2281-2301 for one list: values (int64, or float64 with is_int marking the entries that are Python ints in the reference) in
    fa_dict order, all >= 0.  Returns (x, y1, y2): x as Python ints / floats the way the reference would print them, y1 / y2 float64 arrays."""
    as_float = values.astype(np.float64, copy=False)
    order = np.argsort(as_float, kind='stable')                    # list.sort(key=value): stable, ties in fa_dict order
    v = as_float[order]
    # the dict starts as {0: 0}: zeros join that key, every other run of equal values is a key of its own
    start = np.flatnonzero(np.concatenate(([True], v[1:] != v[:-1]))) if len(v) else np.zeros(0, np.int64)
    has_zero = len(v) > 0 and v[0] == 0
    cum_n = np.concatenate((start[1:], [len(v)])).astype(np.int64) if len(v) else np.zeros(0, np.int64)
    cum_len = np.cumsum(lengths[order])[cum_n - 1] if len(v) else np.zeros(0, np.int64)
    first = order[start]
    if values.dtype.kind in 'iu':
        x = values[first].tolist()
    else:
        x = as_float[first].tolist()
        if is_int is not None:
            for k in np.flatnonzero(is_int[first]).tolist():
                x[k] = int(x[k])
    if has_zero:
        x[0] = 0                                                   # the initial key, an int, whatever joined it
    else:
        x = [0] + x
        cum_n = np.concatenate(([0], cum_n))
        cum_len = np.concatenate(([0], cum_len))
    y1 = cum_n / total_n * 100
    y2 = (total_len - cum_len) / total_len * 100
    return x, y1, y2


def write_result(x, y1, y2, title, inflation):
    """write_result :2303-2307"""
    with open('inflation_{}/{}_statistics.txt'.format(inflation, title), 'w') as fout:
        fout.write('{}\tFiltered_ctg_n\tRest_ctg_len\n'.format(title))
        fout.write(''.join(map('>{}\t{}\t{}\n'.format, x, y1.tolist(), y2.tolist())))


def contig_values(n_cells, max_links, max_group, other_sum, own_group, group_re, ctg_re):
    """:2361-2391 for one inflation from the device's per-contig outputs: ((links, None), (density, is_int), (ratio, is_int))"""
    has = n_cells > 0
    g = np.where(has, max_group, 0)
    gre = group_re[g] if len(group_re) else np.ones(len(g), np.int64)
    den = np.where(g == own_group, gre, gre + ctg_re - 1)          # cal_link_density :2271-2276
    with np.errstate(all='ignore'):
        density = np.where(has, max_links / np.where(has, den, 1), 0.0)
        if len(group_re) > 1:
            avg = other_sum / (len(group_re) - 1)                  # :2377
        else:
            avg = np.zeros(len(g), np.float64)                     # :2379
        real = has & (avg != 0)
        ratio = np.where(real, density / np.where(real, avg, 1.0), np.where(has, float(SENTINEL_RATIO), 0.0))
    links = np.where(has, max_links, 0).astype(np.int64)
    return (links, None), (density, ~has), (ratio, ~real)


def _draw(plt, curves, inflation):
    """:2412-2478, from the same arrays"""
    fig = plt.figure(figsize=(8, 7))
    panels = ((221, 'RE site threshold', 'Number of RE sites', [0, 500]), (222, 'Hi-C link threshold', 'Number of links to the best group', [0, 500]),
              (223, 'Link density threshold', 'Link density to the best group', [0, 0.001]),
              (224, 'Link density ratio threshold', 'Link density ratio (best/average)', [0, 20]))
    for (where, title, xlabel, xlim), (x, y1, y2) in zip(panels, curves):
        ax1 = fig.add_subplot(where)
        ax1.plot(x, y1, 'b')
        ax1.tick_params(axis='y', colors='b')
        ax1.set_xlim(xlim)
        ax1.set_ylim([0, 50])
        ax1.set_ylabel('Number of contigs filtered out (%)', color='b')
        ax1.set_title(title)
        ax1.set_xlabel(xlabel)
        ax2 = ax1.twinx()
        ax2.plot(x, y2, 'r')
        ax2.tick_params(axis='y', colors='r')
        ax2.set_ylim([90, 100])
        ax2.set_ylabel('Length of remaining contigs (%)', color='r')
    fig.tight_layout(w_pad=1, h_pad=1)
    plt.savefig('inflation_{}/statistics.pdf'.format(inflation))
    plt.close()


def _device_inputs(fa_dict, link_dict, result_clusters_list):
    """the arrays of one engine call, or None when the call is the reference function's"""
    from . import ranks
    if not _frozen(link_dict, 'full') or ranks.active():
        return None
    session = link_dict._session
    names = session.table.ctg_names
    where = {name: k for k, name in enumerate(fa_dict)}
    try:
        to_fa = np.fromiter(map(where.__getitem__, names), np.int64, len(names))       # contig id of the table -> position in fa_dict
    except KeyError:
        return None                                                # the reference's loop raises on such a key: let it
    info = list(fa_dict.values())
    if not info:
        return None
    lengths = np.fromiter((v[1] for v in info), np.int64, len(info))
    re_sites = np.fromiter((v[2] for v in info), np.int64, len(info))
    if len(re_sites) and int(re_sites.min()) < 1:
        return None                                                # a denominator of :2271-2276 may be zero or negative: the reference's to raise
    n_sets = len(result_clusters_list)
    own = np.full((n_sets, len(info)), -1, np.int32)
    group_re = []
    for s, (_inflation, result_clusters) in enumerate(result_clusters_list):
        gre = np.ones(len(result_clusters), np.int64)
        for n, (ctgs, _) in enumerate(result_clusters):            # :2347-2351
            idx = np.fromiter(map(where.__getitem__, ctgs), np.int64, len(ctgs))
            own[s, idx] = n
            gre[n] += int((re_sites[idx] - 1).sum())
        group_re.append(gre)
    return session, to_fa, lengths, re_sites, own, group_re


def _engine_call(session, link_dict, group, n_groups, group_re, ctg_re):
    """the handle's table where there is one; an array-backed container without a handle gives its arrays in dict order"""
    ing = getattr(session, 'ing', None)
    if ing is not None and hasattr(ing, 'group_stats'):
        return ing.group_stats(group, n_groups, group_re, ctg_re, SUM_MODE)
    fi, fj, v, _names = link_dict.arrays()
    if np.asarray(v).dtype.kind not in 'iu':
        return None                                                # float links: the summation order of the reference's dict loop matters
    return _lib.group_stats(fi, fj, v, group, n_groups, group_re, ctg_re, SUM_MODE)


def output_statistics(fa_dict, link_dict, result_clusters_list, _original=None):
    """output_statistics() :2279-2478 (see the module docstring)"""
    def original():
        if _original is None:
            raise ValueError('output_statistics: this call is the reference function\'s (see haphic_amd/statistics.py) and none was bound')
        return _original(fa_dict, link_dict, result_clusters_list)

    t0 = time.perf_counter()
    try:
        inputs = _device_inputs(fa_dict, link_dict, result_clusters_list)
    except KeyError:
        inputs = None                                              # a cluster names a contig fa_dict does not have: the reference's KeyError
    if inputs is None:
        return original()
    session, to_fa, lengths, re_sites, own, group_re = inputs
    t_prepared = time.perf_counter()
    n_groups = np.array([len(g) for g in group_re], np.int32)
    out = None
    if len(result_clusters_list):
        out = _engine_call(session, link_dict, np.ascontiguousarray(own[:, to_fa]), n_groups,
                           np.concatenate(group_re) if group_re else np.zeros(0, np.int64), re_sites[to_fa])
        if out is None:
            return original()
    t_device = time.perf_counter()
    logger.info('Making some statistics for the next HapHiC reassignment step...')
    total_n, total_len = len(fa_dict), int(lengths.sum())
    curve_re = generate_axes(re_sites, None, lengths, total_n, total_len)              # :2312-2322, once
    try:                                                           # :2325-2336
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        import warnings
        warnings.filterwarnings('ignore', category=UserWarning)
    except Exception:
        plt = None
        logger.warning('Module matplotlib is not correctly installed, HapHiC will NOT draw statistical plots')
    t_axes = t_text = t_pdf = 0.0
    for s, (inflation, _clusters) in enumerate(result_clusters_list):
        t1 = time.perf_counter()
        write_result(*curve_re, 'RE_site_threshold', inflation)
        t2 = time.perf_counter()
        per_fa = []
        for a, fill in zip(out, (0, 0, -1, 0.0)):                  # table ids -> fa_dict order; a contig without a table row has no cells
            full = np.full(len(fa_dict), fill, a.dtype)
            full[to_fa] = a[s]
            per_fa.append(full)
        lists = contig_values(*per_fa, own[s], group_re[s], re_sites)
        curves = [generate_axes(v, k, lengths, total_n, total_len) for v, k in lists]
        t3 = time.perf_counter()
        for curve, title in zip(curves, ('Link_threshold', 'Link_density_threshold', 'Link_density_ratio_threshold')):
            write_result(*curve, title, inflation)
        t4 = time.perf_counter()
        if plt is not None:
            _draw(plt, [curve_re] + curves, inflation)
        t_axes += t3 - t2
        t_text += (t2 - t1) + (t4 - t3)
        t_pdf += time.perf_counter() - t4
    STATS.clear()
    STATS.update(device_s=t_device - t0, prepare_s=t_prepared - t0, axes_s=t_axes, text_s=t_text, pdf_s=t_pdf, total_s=time.perf_counter() - t0, sets=len(result_clusters_list),
                 engine='device')
