"""Writes tests/golden/clm_split.npz from the reference's own split_clm_file (scripts/HapHiC_reassign.py:581-622).

    python tests/golden/make_golden_clm_split.py [path/to/HapHiC/scripts]

For every small case of tests/clm_split_cases.py (and one of the size cases) the function runs in a temporary directory on a file
holding the case's bytes; the fixture keeps the inputs and what it wrote per group, or that it raised IndexError.  'seam_*' holds
the whole tree of one run (directories, link targets, file bytes) for the test of haphic_amd.reassign.split_clm_file.  Data only."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import clm_split_cases as cc      # noqa: E402


def load_reference_reassign(scripts, name='_haphic_reassign_reference_private'):
    """HapHiC_reassign.py under a private module name (a cached `HapHiC_reassign` may carry the product's seams); pysam / portion stubbed when absent"""
    for mod, attrs in (('pysam', {'set_verbosity': lambda *a, **k: None, 'AlignmentFile': None}), ('portion', {'closed': None, 'empty': None})):
        try:
            __import__(mod)
        except ImportError:
            m = types.ModuleType(mod)
            m.__dict__.update(attrs)
            sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, 'HapHiC_reassign.py'))
    module = importlib.util.module_from_spec(spec)
    sys.path.insert(0, scripts)
    try:
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(scripts)
    return module


def run_reference(R, text, group_ctg_dict, ctg_group_dict, subdir='reassigned_groups'):
    """-> the tree split_clm_file left in a fresh directory (clm_split_cases.read_tree), or IndexError"""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        clm = os.path.join(tmp, 'paired_links.clm')
        with open(clm, 'wb') as f:
            f.write(text)
        work = os.path.join(tmp, 'run')
        os.mkdir(work)
        os.chdir(work)
        try:
            R.split_clm_file(clm, group_ctg_dict, ctg_group_dict, subdir)
        except IndexError as e:
            assert str(e) == 'list index out of range', e
            return IndexError
        finally:
            os.chdir(cwd)
            import gc
            gc.collect()                      # the reference leaves its files open when it raises: closed (and flushed) here
        return cc.read_tree(work)


def case_dicts(case):
    """group g of the case is called 'g<g>' in the reference's dicts"""
    group_ctg_dict = {'g%d' % g: [set(), 0] for g in range(case.n_groups)}
    ctg_group_dict = {n: 'g%d' % g for n, g in zip(case.names, case.group_of_name) if g >= 0}
    return group_ctg_dict, ctg_group_dict


def golden_cases():
    return cc.cases(cc.SMALL_SECTIONS) + [cc.size_case(cc.TX_BLOCK + 1, 5, 'src')]


def main():
    scripts = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/scripts'
    R = load_reference_reassign(scripts)
    cases = golden_cases()
    texts, names, groups, raises, outs, out_len = [], [], [], [], [], []
    for c in cases:
        tree = run_reference(R, c.text, *case_dicts(c))
        texts.append(c.text)
        names.append(c.names)
        groups.append(c.group_of_name)
        raises.append(tree is IndexError)
        if tree is not IndexError:
            files = [tree['split_clms/g%d.clm' % g][1] for g in range(c.n_groups)]
            assert sum(1 for p in tree if p.startswith('split_clms/')) == c.n_groups
            outs += files
            out_len += [len(f) for f in files]
    # few arrays (every member of an .npz costs a few hundred bytes): case k owns text[text_off[k]:text_off[k + 1]], the names / groups
    # name_off[k]:name_off[k + 1] and, unless it raises, the next n_groups[k] entries of out_len
    out = {'case_names': np.array(['%s/%s' % (c.section, c.name) for c in cases]),
           'text': np.frombuffer(b''.join(texts), np.uint8), 'text_off': np.cumsum([0] + [len(t) for t in texts]).astype(np.int64),
           'names': np.array([n for ns in names for n in ns], dtype=str), 'name_off': np.cumsum([0] + [len(ns) for ns in names]).astype(np.int64),
           'group': np.array([g for gs in groups for g in gs], np.int32), 'n_groups': np.array([c.n_groups for c in cases], np.int32),
           'raises': np.array(raises, np.bool_), 'out': np.frombuffer(b''.join(outs), np.uint8), 'out_len': np.array(out_len, np.int64)}
    text, group_ctg_dict, ctg_group_dict, subdir = cc.seam_inputs()
    tree = run_reference(R, text, group_ctg_dict, ctg_group_dict, subdir)
    paths = sorted(tree)
    out['seam_paths'] = np.array(paths)
    out['seam_kinds'] = np.array([tree[p][0] for p in paths])
    out['seam_payload'] = np.frombuffer(b''.join(tree[p][1] if tree[p][0] == 'file' else tree[p][1].encode() if tree[p][0] == 'link' else b'' for p in paths), np.uint8)
    out['seam_payload_len'] = np.array([len(tree[p][1]) if tree[p][0] == 'file' else len(tree[p][1].encode()) if tree[p][0] == 'link' else 0 for p in paths], np.int64)
    path = os.path.join(ROOT, 'tests', 'golden', 'clm_split.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(cases), 'cases')


if __name__ == '__main__':
    main()
