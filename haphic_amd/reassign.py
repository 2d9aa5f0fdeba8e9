"""`haphic reassign` (scripts/HapHiC_reassign.py) on the MI355X library: the last step of run(), split_clm_file :581-622, which
routes every line of paired_links.clm (26 GB at 100k contigs / 500 M pairs) to split_clms/<group>.clm.  The reference reads the file
through `for line in f` with a split(), two dict lookups and a write per line; here the text goes through the device in raw chunks
(haphic_amd/csrc/hhx_clmsplit.hip) and leaves through the library's writer lanes.  The rescue rounds (run_reassignment) are a
sequential greedy walk and stay the reference's code; parse_link_dict is re-bound by patch.patch_reassign as before."""
import logging
import os

from . import _lib

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
