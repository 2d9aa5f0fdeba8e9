"""`haphic reassign` (scripts/HapHiC_reassign.py) on the MI355X library: the last step of run(), split_clm_file :581-622, which
routes every line of paired_links.clm (26 GB at 100k contigs / 500 M pairs) to split_clms/<group>.clm.  The reference reads the file
through `for line in f` with a split(), two dict lookups and a write per line; here the text goes through the device in raw chunks
(haphic_amd/csrc/hhx_clmsplit.hip) and leaves through the library's writer lanes.

The middle of the step — the rescue and reassignment rounds (run_reassignment :266-427) and the group-pair sums of the agglomerative step
(:489-560) — runs on the device too when patch.patch_reassign(R, rounds=True) binds the three mirrors of bind_rounds() below
(haphic_amd/csrc/hhx_reassign.hip).  parse_link_dict then leaves the per-(contig, group) cells in HBM and returns two RoundTable containers that
share the handle; run_reassignment computes what is elementwise on the host (the RE filter and the length rule as flag bytes, the dismissal as a
group mask, by the reference's own expressions), runs the round on the device and writes only the changed values back into ctg_group_dict and
group_RE_dict, which stay real dicts.  Whatever the device does not answer exactly as the reference goes to the original function: containers
that are not ours, a whitelist, min_links below 1, the per-contig DEBUG lines, totals that reach 2^53, float or normalised links.

The step's first line — parse_pickle :38-50, pickle.load of full_links.pkl — is bound by patch_reassign(R, pickle=True) to bind_pickle() below:
the file is read into arrays on the device (haphic_amd/csrc/hhx_pickleread.hip) and full_link_dict is a frozen containers.LinkTable, which the
mirrors above consume without a Python object per key.  With resident=True the table stays open on the device (ResidentSession) and the
parse_link_dict mirror builds the handle of the rounds from it there (hhx_reassign_create_from_pickle): no key comes to the host unless something
turns full_link_dict into a dict.

run()'s very first line — parse_fasta, HapHiC_cluster.py:87-113 — is bound by patch_reassign(R, fasta=True) to bind_fasta() below: the file is
parsed and its RE sites are counted on the device, fa_dict is a plain dict of containers.FastaRow whose sequences stay there (run() never reads one)."""
import logging
import os
from collections import defaultdict

import numpy as np

from . import _lib, cluster, containers, statistics

logger = logging.getLogger('HapHiC_reassign')   # the reference module's own logger name; handlers come from the caller

CHUNK_BYTES = 64 << 20                          # raw chunk of the read-ahead reader: two pinned buffers of it, a work and an output buffer in HBM


def _device_split(clm_file, names, group_of_name, paths):
    """every line of clm_file whose two contigs (names[k] in group group_of_name[k]) share a group -> paths[group]; complete on return"""
    s = _lib.ClmSplit(names, group_of_name, paths)
    try:
        s.push_file(clm_file, CHUNK_BYTES)
        s.finish()
    finally:
        s.close()


def _ours(group_ctg_dict, ctg_group_dict):
    """False: a case the reference answers with its own exception or that lies outside the name table (handed to the original function)"""
    for ctg, group in ctg_group_dict.items():
        if not isinstance(ctg, str) or not ctg or group not in group_ctg_dict:
            return False
        try:
            ctg.encode()
        except UnicodeEncodeError:
            return False
    return True


def split_clm_file(clm_file, group_ctg_dict, ctg_group_dict, subdir, _original=None):
    """split_clm_file :581-622: final_groups/ with its links, split_clms/<group>.clm for every group (possibly empty), lines in file
    order; an IndexError for the first line with fewer than two columns, as :617 raises.  The files are complete when it returns
    (`haphic sort` reads them next)."""
    if not _ours(group_ctg_dict, ctg_group_dict):
        if _original is None:
            raise ValueError('split_clm_file: contig names must be non-empty str and every group of ctg_group_dict a key of group_ctg_dict')
        return _original(clm_file, group_ctg_dict, ctg_group_dict, subdir)

    logger.info('Splitting clm file into subfiles by group...')

    final_dir = 'final_groups'
    os.mkdir(final_dir)
    if subdir == 'reassigned_groups':
        prefix = 'reassigned'
    else:
        assert subdir == 'hc_groups'
        prefix = 'hc'
    for group in group_ctg_dict:
        os.symlink('../{0}/{1}_{2}.txt'.format(subdir, prefix, group), '{0}/{1}.txt'.format(final_dir, group))
    os.symlink('../{0}/{1}_clusters.txt'.format(subdir, prefix), '{0}/final_clusters.txt'.format(final_dir))

    subdir = 'split_clms'
    os.mkdir(subdir)
    groups = list(group_ctg_dict)
    index = {group: g for g, group in enumerate(groups)}
    names = list(ctg_group_dict)
    _device_split(clm_file, names, [index[ctg_group_dict[ctg]] for ctg in names], ['{}/{}.clm'.format(subdir, group) for group in groups])


# ------------------------------------------------------------------ parse_pickle :38-50 (patch_reassign(R, pickle=True))
class PickleSession:
    """what a containers.LinkTable needs of its session, over the arrays of one link pickle (_lib.read_link_pickle): ids into `names` and the values
    in dict order.  value: int64 when every value of the file is an integer; float64 when all are floats; an object array of Python int / float per
    key when the file mixes them (a thaw then gives every key the type pickle.load gives it)."""

    def __init__(self, i, j, value, is_float, names):
        if is_float is not None and not is_float.all():
            mixed = np.empty(len(value), object)
            mixed[:] = value.tolist()
            at = np.flatnonzero(~is_float)
            mixed[at] = value[at].astype(np.int64).tolist()                      # exact: read_link_pickle hands back integers beyond 2^53 beside floats
            value = mixed
        self.i, self.j, self.value, self.names = i, j, value, names
        self.thawed = False

    def n_keys(self, _kind):
        return len(self.i)

    def link_arrays(self, _kind):
        return self.i, self.j, self.value, self.names

    def note_thawed(self):
        self.thawed = True
        self.i = self.j = self.value = self.names = None                         # the dict holds them now


class ResidentSession:
    """PickleSession over a link pickle that stays open on the device (_lib.LinkPickle or a stand-in with its interface): n_keys, any_float and the
    names are the handle's own, known without a key; (i, j, value) come to the host when link_arrays is asked for the first time — a thaw, the host
    passes of parse_link_dict, the thaw of linked_ctg_dict — and `fetches` counts those copies.  Only tables without a float value are kept
    resident (bind_pickle), so value is int64."""

    resident = True

    def __init__(self, handle, names):
        self.handle, self.names = handle, names
        self.any_float = bool(handle.any_float)
        self.keys = handle.n_keys
        self.fetches = 0
        self.thawed = False
        self._arrays = None

    def n_keys(self, _kind):
        return self.keys

    def link_arrays(self, _kind):
        if self._arrays is None:
            i, j, value, _is_float, _names = self.handle.arrays()
            self.fetches += 1
            self._arrays = (i, j, value)
        return self._arrays + (self.names,)

    def note_thawed(self):
        self.thawed = True
        self._arrays = self.names = None                                         # the dict holds them now
        self.handle.close()
        self.handle = None


def bind_pickle(R, engine=None, resident=False):
    """-> the mirror of parse_pickle :38-50 for the imported HapHiC_reassign module R: the same log line, sorted_ctg_list and RE_site_dict by the
    reference's own expressions, full_link_dict as a frozen containers.LinkTable over the arrays the device read from the file — no dict of every
    key (tens of GB of Python objects at 100k contigs) that parse_link_dict would flatten again.  A file the reader hands back (include/haphic_hip.h
    lists them: another header or protocol, other opcodes, names of 256 bytes and more, integers beyond 64 bits, a truncated file, bytes after
    STOP ...) goes through pickle.load, so that Python's own result or error is what the caller sees.  engine: a stand-in for _lib.read_link_pickle
    (the tests' host reader).
    resident=True: the table stays open on the device behind a ResidentSession and no key comes to the host until somebody asks for the arrays;
    the parse_link_dict of bind_rounds builds its handle from it there.  engine is then a stand-in for _lib.LinkPickle.open.  A table with a float
    value is read as without `resident`: whether it can be served at all is decided on its values."""
    import pickle
    read = engine if engine is not None else _lib.LinkPickle.open if resident else _lib.read_link_pickle

    def read_table(pickle_file):
        """-> a session, or None for a file that goes through pickle.load"""
        if not resident:
            arrays = read(pickle_file)
            return None if arrays is None else PickleSession(*arrays)
        handle = read(pickle_file)
        if handle is None:
            return None
        if handle.any_float:
            try:
                arrays = handle.arrays()
            finally:
                handle.close()
            return None if arrays is None else PickleSession(*arrays)
        try:
            return ResidentSession(handle, handle.names())
        except UnicodeDecodeError:                                               # pickle.load raises its own error for such a name
            handle.close()
            return None

    def parse_pickle(fa_dict, pickle_file):
        R.logger.info('Parsing input pickle file...')
        session = read_table(pickle_file)
        if session is None:
            with open(pickle_file, 'rb') as f:
                full_link_dict = pickle.load(f)
        else:
            full_link_dict = containers.LinkTable(session, 'full')
        # sort by contig length
        sorted_ctg_list = sorted([(ctg, fa_dict[ctg][1]) for ctg in fa_dict], key=lambda x: x[1], reverse=True)
        RE_site_dict = {ctg: ctg_info[2] for ctg, ctg_info in fa_dict.items()}
        return full_link_dict, sorted_ctg_list, RE_site_dict

    return parse_pickle


# ------------------------------------------------------------------ parse_fasta (patch_reassign(R, fasta=True))
def bind_fasta(R, engine=None, original=None, rows=None):
    """-> the mirror of parse_fasta (HapHiC_cluster.py:87-113, as HapHiC_reassign imports it :23) for the module R.  run() :782-916 never reads a
    sequence: it asks fa_dict for lengths, RE sites, iteration and `in`.  So the file is parsed on the device (_lib.Fasta), the RE sites of all
    contigs are counted there in one call on the sequences where they lie (re_counts_device), and fa_dict is a plain dict {name: containers.FastaRow}
    in file order whose rows fetch their sequence only if somebody looks at it.  The log line is the reference's, through the logger given.  The
    original function takes the call for a file the reader refuses (a byte >= 0x80, a sequence line before the first header, a text beyond half of
    the device's memory), for repeated contig names, and for a path that is no file (its own exception is raised).  engine: a stand-in for _lib.Fasta
    (the tests' numpy engine).  original: the function that takes those calls (by default what R binds now).  rows(fa, off, lengths, re_sites) -> the
    rows of fa_dict in file order, for a caller whose rows carry more than a fetch (haphic_amd/assembly.py: the views of `haphic cluster`)."""
    Engine = engine if engine is not None else _lib.Fasta
    if original is None:
        original = R.parse_fasta
    try:
        import inspect
        default_logger = inspect.signature(original).parameters['logger'].default
    except (KeyError, TypeError, ValueError):
        default_logger = R.logger

    def parse_fasta(fasta, RE='GATC', keep_letter_case=False, logger=default_logger):
        if isinstance(fasta, (str, os.PathLike)) and not os.path.isfile(fasta):
            return original(fasta, RE, keep_letter_case, logger)
        try:
            fa = Engine(fasta, keep_letter_case=keep_letter_case)
        except Engine.Unsupported:
            return original(fasta, RE, keep_letter_case, logger)
        names = fa.names()
        if len(set(names)) != len(names):                                         # fa_dict[ctg] = list() :99 on a name seen before
            fa.close()
            return original(fasta, RE, keep_letter_case, logger)
        logger.info('Parsing input FASTA file...')
        counts = fa.re_counts_device(cluster._sites_of(RE)) if names else np.zeros(0, np.int64)
        off, lengths = np.asarray(fa.seq_off, np.int64).tolist(), np.asarray(fa.seq_len, np.int64).tolist()
        if rows is not None:
            return dict(zip(names, rows(fa, off, lengths, (counts + 1).tolist())))

        def fetch(k):
            return fa.fetch(off[k], lengths[k]).decode('ascii')
        return dict(zip(names, map(containers.FastaRow, [fetch] * len(names), range(len(names)), lengths, (counts + 1).tolist())))    # :110

    return parse_fasta


# ------------------------------------------------------------------ the rounds and the agglomerative step (patch_reassign(R, rounds=True))
class _Job:
    """what one parse_link_dict call leaves behind: the handle, the numbering of contigs and groups, and the dict it was built from"""

    def __init__(self, engine, link_dict, id_names, group_names):
        self.engine = engine
        self.link_dict, self.n_keys = link_dict, len(link_dict)
        self.id_names, self.ids = id_names, {c: k for k, c in enumerate(id_names)}
        self.group_names, self.gids = group_names, {g: k for k, g in enumerate(group_names)}
        self.gids['ungrouped'] = -1
        self.device_rounds = 0

    def matches(self, link_dict):
        return self.link_dict is link_dict and len(link_dict) == self.n_keys


class RoundTable(defaultdict):
    """ctg_group_link_dict / linked_ctg_dict of parse_link_dict :217-263 while their content lives in the handle of a _Job (the style of
    containers.LinkTable).  The mirrors of bind_rounds() recognise the pair and never look inside.  Any other access thaws the container into
    exactly the defaultdict cluster.parse_link_dict returns — as long as no round has run on the device; after one, the cells in HBM have moved
    on and only the device knows them, so a thaw raises."""

    frozen = True

    def __init__(self, factory, job, kind):
        defaultdict.__init__(self, factory)
        self._job = job
        self._kind = kind

    def _thaw(self):
        if type(self) is containers.Thawed:
            return
        job = self._job
        if job.device_rounds:
            raise RuntimeError('{}: {} round(s) of run_reassignment have run on the device; the table exists in device memory only and cannot be '
                               'read as a dict any more (bind the reference rounds with patch_reassign(R) / --keep-reference-rounds)'
                               .format(self._kind, job.device_rounds))
        if self._kind == 'ctg_group_link_dict':
            sums, first = job.engine.cells()
            dict.update(self, cluster.nested_group_links(sums, first, job.id_names, job.group_names))
        else:
            fi, fj, _val = cluster._dict_arrays(job.link_dict, {})                 # the same numbering: the dict's names come first in id_names
            dict.update(self, cluster.linked_contigs(fi, fj, job.id_names))
        self.__dict__.clear()
        self.__class__ = containers.Thawed


for _name in ('__getitem__', '__setitem__', '__delitem__', '__contains__', '__iter__', '__reversed__', '__missing__', '__len__', '__bool__', 'keys',
              'values', 'items', 'get', 'pop', 'popitem', 'setdefault', 'update', 'clear', 'copy', '__copy__', '__eq__', '__ne__', '__repr__',
              '__or__', '__ror__', '__ior__', '__reduce_ex__', '__reduce__'):
    setattr(RoundTable, _name, containers._thawing(_name))


def _our_pair(ctg_group_link_dict, linked_ctg_dict):
    """the _Job of two RoundTables from one parse_link_dict call, else None"""
    if type(ctg_group_link_dict) is RoundTable and type(linked_ctg_dict) is RoundTable and ctg_group_link_dict._job is linked_ctg_dict._job:
        return ctg_group_link_dict._job
    return None


def bind_rounds(R, engine=None):
    """-> {name: mirror} of parse_link_dict :217-263, run_reassignment :266-427 and agglomerative_hierarchical_clustering :489-560 for the
    imported HapHiC_reassign module R (its logger, dict_to_matrix and AgglomerativeClustering are resolved through R at call time, as the
    reference's functions resolve them).  engine: a stand-in for _lib.Reassign (the tests' numpy engine)."""
    Engine = engine if engine is not None else _lib.Reassign
    unsupported = getattr(Engine, 'Unsupported', ())
    original_parse = R.parse_link_dict
    original_round = R.run_reassignment
    original_hc = R.agglomerative_hierarchical_clustering
    jobs = []                                                                       # the last parse_link_dict's, for the agglomerative step

    def todays_parse(link_dict, ctg_group_dict, normalize_by_nlinks):
        return cluster.parse_link_dict(link_dict, ctg_group_dict, normalize_by_nlinks, _original=original_parse)

    def resident_parse(link_dict, session, ctg_group_dict):
        """the tables from a link pickle that is still open on the device, without a key on the host: the numbering below is the one _dict_arrays
        gives (the reader numbers the names in order of first appearance, i before j, key by key).  None: a case of the code below"""
        names = session.names
        if any(c not in ctg_group_dict for c in names):
            return None
        named = set(names)
        id_names = list(names) + [c for c in ctg_group_dict if c not in named]    # contigs no key names are visited too
        groups = {}
        grp = np.fromiter((-1 if ctg_group_dict[c] == 'ungrouped' else groups.setdefault(ctg_group_dict[c], len(groups)) for c in id_names),
                          np.int32, len(id_names))
        group_names = list(groups)
        if not group_names:
            return None
        try:
            handle = Engine.from_pickle(session.handle, len(id_names), grp, len(group_names))
        except unsupported as e:                                                   # the cells do not fit: what the code below would meet after its host passes
            logger.info('parse_link_dict: %s; the reference function takes the call', e)
            return original_parse(link_dict, ctg_group_dict, False)
        if handle is None:                                                         # a key naming one contig twice, a negative value, totals beyond 2^52
            return None
        job = _Job(handle, link_dict, id_names, group_names)
        jobs[:] = [job]
        return RoundTable(dict, job, 'ctg_group_link_dict'), RoundTable(set, job, 'linked_ctg_dict')

    def parse_link_dict(link_dict, ctg_group_dict, normalize_by_nlinks=False):
        session = getattr(link_dict, '_session', None) if cluster._frozen(link_dict, 'full') else None
        if (not normalize_by_nlinks and getattr(session, 'resident', False) and session.handle is not None and not session.any_float
                and hasattr(Engine, 'from_pickle')):
            tables = resident_parse(link_dict, session, ctg_group_dict)           # ahead of integral_links, which asks for the arrays
            if tables is not None:
                return tables
        if normalize_by_nlinks or not cluster.integral_links(link_dict):
            return original_parse(link_dict, ctg_group_dict, normalize_by_nlinks)
        names = {}
        fi, fj, val = cluster._dict_arrays(link_dict, names)
        # a key that names one contig twice, or totals that leave the exact range of float64: not the device's case
        if (fi == fj).any() or 2 * float(val.sum()) >= 2.0 ** 53 or any(c not in ctg_group_dict for c in names):
            return todays_parse(link_dict, ctg_group_dict, normalize_by_nlinks)
        for c in ctg_group_dict:                                                   # contigs no key names are visited too
            names.setdefault(c, len(names))
        id_names = list(names)
        groups = {}
        grp = np.fromiter((-1 if ctg_group_dict[c] == 'ungrouped' else groups.setdefault(ctg_group_dict[c], len(groups)) for c in id_names),
                          np.int32, len(id_names))
        group_names = list(groups)
        if not group_names:
            return todays_parse(link_dict, ctg_group_dict, normalize_by_nlinks)
        try:
            handle = Engine(fi, fj, val.astype(np.int64), len(id_names), grp, len(group_names))
        except unsupported as e:
            logger.info('parse_link_dict: %s; the reference function takes the call', e)
            return original_parse(link_dict, ctg_group_dict, normalize_by_nlinks)
        job = _Job(handle, link_dict, id_names, group_names)
        jobs[:] = [job]
        return RoundTable(dict, job, 'ctg_group_link_dict'), RoundTable(set, job, 'linked_ctg_dict')

    def run_reassignment(sorted_ctg_list, ctg_group_link_dict, ctg_group_dict, full_link_dict, linked_ctg_dict, fa_dict, RE_site_dict, gfa,
                         group_RE_dict, max_ctg_len, min_RE_sites, min_links, min_link_density, min_density_ratio, ambiguous_cutoff, min_group_len,
                         whitelist, nround):
        args = (sorted_ctg_list, ctg_group_link_dict, ctg_group_dict, full_link_dict, linked_ctg_dict, fa_dict, RE_site_dict, gfa, group_RE_dict,
                max_ctg_len, min_RE_sites, min_links, min_link_density, min_density_ratio, ambiguous_cutoff, min_group_len, whitelist, nround)
        job = _our_pair(ctg_group_link_dict, linked_ctg_dict)

        def hand_back():
            for table in (ctg_group_link_dict, linked_ctg_dict):
                if type(table) is RoundTable:
                    table._thaw()                                                  # raises once a device round has run
            return original_round(*args)
        if job is None or not job.matches(full_link_dict) or whitelist or not min_links >= 1 or R.logger.isEnabledFor(logging.DEBUG):
            return hand_back()
        ids, gids, id_names, group_names = job.ids, job.gids, job.id_names, job.group_names
        try:
            order = np.fromiter((ids[ctg] for ctg, _len in sorted_ctg_list), np.int32, len(sorted_ctg_list))
            ctg_len = np.fromiter((ctg_len for _ctg, ctg_len in sorted_ctg_list), np.float64, len(sorted_ctg_list))
            visited_re = [RE_site_dict[ctg] for ctg, _len in sorted_ctg_list]
            group = np.fromiter((gids[ctg_group_dict[c]] for c in id_names), np.int32, len(id_names))
            group_re = np.fromiter((group_RE_dict[g] for g in group_names), np.int64, len(group_names))
        except (KeyError, TypeError, ValueError, OverflowError):                    # a name or a value the numbering does not hold
            return hand_back()
        if len(group_RE_dict) != len(group_names) or not all(isinstance(v, (int, np.integer)) for v in visited_re):
            return hand_back()
        ctg_re = np.ones(len(id_names), np.int64)
        ctg_re[order] = visited_re
        if float(np.abs(ctg_re).sum()) + float(np.abs(group_re).sum()) >= 2.0 ** 53:
            return hand_back()
        flags = np.zeros(len(id_names), np.uint8)
        flags[order] = (~(ctg_re[order] - 1 < min_RE_sites)).astype(np.uint8)       # :335
        flags[order] |= (ctg_len <= max_ctg_len * 1000).astype(np.uint8) << 1        # :415
        dismissed = None
        if min_group_len and nround > 1:                                           # :304-316, the reference's own expressions
            group_len_dict = defaultdict(int)
            for ctg, g in ctg_group_dict.items():
                if g != 'ungrouped':
                    group_len_dict[g] += fa_dict[ctg][1]
            dismissed = np.zeros(len(group_names), np.uint8)
            for g, group_len in group_len_dict.items():
                if group_len / 1000000 < min_group_len:
                    dismissed[gids[g]] = 1
        if nround:
            R.logger.info('Performing reassignment...')
            round_name = 'round{}'.format(nround)
        else:
            R.logger.info('Performing additional round of rescue...')
            round_name = 'additional_rescue'
        before, re_before = group.copy(), group_re.copy()
        counts = job.engine.round(group, group_re, ctg_re, order, flags, dismissed, min_links, min_link_density, min_density_ratio, ambiguous_cutoff,
                                  not nround, bool(gfa), statistics.SUM_MODE)
        job.device_rounds += 1
        for k in np.flatnonzero(group != before).tolist():
            ctg_group_dict[id_names[k]] = group_names[group[k]] if group[k] >= 0 else 'ungrouped'
        for k in np.flatnonzero(group_re != re_before).tolist():
            group_RE_dict[group_names[k]] = int(group_re[k])
        R.logger.info('[result::{}] Total: {}, consistent: {}, rescued: {}, reassigned: {}, not rescued: {}'.format(
            round_name, len(sorted_ctg_list), int(counts[0]), int(counts[1]), int(counts[2]), int(counts[3])))

    def agglomerative_hierarchical_clustering(full_link_dict, grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict, nclusters,
                                              normalize_by_nlinks=False):
        job = jobs[0] if jobs and jobs[0].matches(full_link_dict) else None
        if job is None or normalize_by_nlinks:
            return original_hc(full_link_dict, grouped_ctgs, new_ctg_group_dict, group_hiconf_RE_dict, new_old_group_dict, nclusters,
                               normalize_by_nlinks)
        R.logger.info('Performing additional agglomerative hierarchical clustering...')
        # :494-508 on the device: the links between high-confidence contigs of different groups, per group pair, in first-contribution order
        gnames = list(dict.fromkeys(new_ctg_group_dict.values()))
        gid = {g: k for k, g in enumerate(gnames)}
        member = np.fromiter((c in grouped_ctgs for c in job.id_names), np.uint8, len(job.id_names))
        group_of = np.fromiter((gid[new_ctg_group_dict[c]] if c in new_ctg_group_dict else -1 for c in job.id_names), np.int32, len(job.id_names))
        sums, first = job.engine.pair_sums(member, group_of, len(gnames))
        lo, hi = np.nonzero(first >= 0)
        by_first = np.argsort(first[lo, hi], kind='stable')
        group_link_dict = defaultdict(int)
        for a, b in zip(lo[by_first].tolist(), hi[by_first].tolist()):
            group_link_dict[tuple(sorted([gnames[a], gnames[b]]))] = int(sums[a, b])
        # :510-560 as the reference has them
        with open('hc_groups/group_group_links.txt', 'w') as f:
            f.write('group1\tgroup2\tlinks\tlink_density\n')
            max_link_density = 0
            for group_name_pair, links in group_link_dict.items():
                group_i, group_j = group_name_pair
                group_RE_sites_i = group_hiconf_RE_dict[new_old_group_dict[group_i]]
                group_RE_sites_j = group_hiconf_RE_dict[new_old_group_dict[group_j]]
                link_density = links / (group_RE_sites_i * group_RE_sites_j)
                max_link_density = max(max_link_density, link_density)
                group_link_dict[group_name_pair] = link_density
                f.write('{}\t{}\t{}\t{}\n'.format(group_i, group_j, links, link_density))
        group_link_matrix, group_index_dict = R.dict_to_matrix(group_link_dict, set(new_old_group_dict.keys()))
        index_group_dict = {i: g for g, i in group_index_dict.items()}
        group_link_matrix = max_link_density - group_link_matrix
        AgglomerativeClustering = R.AgglomerativeClustering
        if 'affinity' in AgglomerativeClustering._get_param_names():
            clust = AgglomerativeClustering(n_clusters=nclusters, affinity="precomputed", linkage="average", distance_threshold=None)
        else:
            R.logger.info('The parameter "affinity" is not found in AgglomerativeClustering, use "metric" instead')
            assert 'metric' in AgglomerativeClustering._get_param_names()
            clust = AgglomerativeClustering(n_clusters=nclusters, metric="precomputed", linkage="average", distance_threshold=None)
        clusters = clust.fit_predict(group_link_matrix)
        hc_cluster_dict = defaultdict(list)
        for index, new_cluster in enumerate(clusters):
            hc_cluster_dict[new_cluster].append(index_group_dict[index])
        return hc_cluster_dict

    return {'parse_link_dict': parse_link_dict, 'run_reassignment': run_reassignment,
            'agglomerative_hierarchical_clustering': agglomerative_hierarchical_clustering}
