"""CPU: the feature typing's definition (restated in tests/feature_reference.py from DESIGN.md 2.9 "Features") on the named molecules
with hand-written answers, the make-up of the random family and its rejection rule, the kernel's rules compiled for the host under
ASan / UBSan (tools/feature_host_check.cpp) against the restatement, the SDF item, the binding and its argument errors.

The kernel itself is held against the restatement in tests/test_gpu_molfeat.py."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import feature_reference as FR
import kekule_reference as K
import mol_reference as R
from mol_support import arg_count, build_host_check, header_macro, header_text
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_tables():
    assert M.FEATURE_TYPES == ('HD', 'AR', 'PO', 'HA', 'HY', 'NE', 'XB')
    assert (M.FEAT_NO_KEKULE, M.FEAT_UNMATCHED, M.FEAT_HAS_UNTYPED, M.FEAT_NONFINITE) == (1, 2, 4, 8)
    assert M.FEAT_FAIL_MASK == 1 | 2 | 8 and sorted(M.FEAT_NAMES) == [1, 2, 4, 8]
    assert M.FEATURE_COUNTS[:4] == ('typed_points', 'matched', 'unmatched', 'untyped_points') and len(M.FEATURE_COUNTS) == 25
    assert M.FEATURE_COUNTS[4:11] == tuple('atoms_' + t for t in M.FEATURE_TYPES)
    assert M.FEATURE_COUNTS[11:18] == tuple('points_' + t for t in M.FEATURE_TYPES)
    assert M.FEATURE_COUNTS[18:] == tuple('matched_' + t for t in M.FEATURE_TYPES)
    from phoregen_amd.data import PHORETYPES1
    x = torch.eye(len(PHORETYPES1))
    assert M.point_kinds_of(x, PHORETYPES1).tolist() == [-1, 0, 1, 2, 3, 4, 5, -1, -1, -1, -1, 6, -2]
    assert M.point_kinds_of(x[:0], PHORETYPES1).shape == (0,)


def test_feature_limits():
    lim = M.FeatureLimits()
    assert lim.feat_cut == 2.0 == M.GeomLimits().feat_cut and lim.max_unmatched == 2 ** 31 - 1
    with pytest.raises(Exception):                                     # frozen
        lim.max_unmatched = 0
    assert M.FeatureLimits(max_unmatched=0).max_unmatched == 0 and M.FeatureLimits(feat_cut=1).feat_cut == 1
    for bad in (dict(max_unmatched=-1), dict(max_unmatched=2 ** 31), dict(max_unmatched=1.0), dict(max_unmatched=True),
                dict(feat_cut=float('nan')), dict(feat_cut=float('inf')), dict(feat_cut=-1.0), dict(feat_cut='2'), dict(feat_cut=True)):
        with pytest.raises(ValueError, match='FeatureLimits'):
            M.FeatureLimits(**bad)
    with pytest.raises(ValueError, match='features='):
        M.sample_valid(None, None, 1, features=(None, None))
    with pytest.raises(ValueError, match='features='):
        M.sample_valid(None, None, 1, features=(None, None, {'max_unmatched': 0}))


@pytest.mark.parametrize('name', list(FR.NAMED))
def test_named_molecule_by_hand(name):
    classes, bonds, _ = FR.NAMED[name]
    inputs = FR.cpu_inputs(classes, bonds)
    got = FR.type_atoms(*inputs[:5], inputs[6], inputs[5])
    assert got == FR.named_answer(name), (name, got)
    r = FR.features_of_rows(*inputs, np.zeros((len(classes), 3)), np.zeros((0, 3)), [])
    assert r['atom_fp'].dtype == np.uint8 and r['atom_fp'].tolist() == [sum(1 << M.FEATURE_TYPES.index(t) for t in s) for s in got]
    assert r['status'] == (M.FEAT_NO_KEKULE if name == 'indene-like' else 0) and r['ok'] == (name != 'indene-like')


def test_named_details_by_hand():
    # the charged pass is what types N-methylpyridinium; without a Kekulé structure nothing is typed and every typed point is unmatched
    assert K.kekule_of_rows(*K.rows_of(*FR.NAMED['N-methylpyridinium'][:2]))['status'] & M.KEKULE_CHARGED
    inputs = FR.cpu_inputs(*FR.NAMED['indene-like'][:2])
    assert not inputs[5]
    pos = np.arange(27, dtype=np.float32).reshape(9, 3)
    r = FR.features_of_rows(*inputs, pos, pos[[0, 3, 4]], [1, 4, -1])
    c = dict(zip(M.FEATURE_COUNTS, r['counts'].tolist()))
    assert r['status'] == M.FEAT_NO_KEKULE | M.FEAT_HAS_UNTYPED and not r['ok'] and not r['atom_fp'].any()
    assert (c['typed_points'], c['matched'], c['unmatched'], c['untyped_points']) == (2, 0, 2, 1)
    assert np.isinf(r['point_dist']).all() and r['point_atom'].tolist() == [-1, -1, -1]
    # ethanol with a donor point on the O, an aromatic point on the O and a donor point just outside the cutoff of the O
    inputs = FR.cpu_inputs(*FR.NAMED['ethanol'][:2])
    pos = np.array([[0, 0, 0], [1.5, 0, 0], [2.2, 1.2, 0]], dtype=np.float32)
    pts = np.array([[2.2, 1.2, 0.5], [2.2, 1.2, 0], [2.2, 1.2, 2.5], [0, 0, 0], [9, 9, 9]], dtype=np.float32)
    r = FR.features_of_rows(*inputs, pos, pts, [0, 1, 0, 4, -2])
    c = dict(zip(M.FEATURE_COUNTS, r['counts'].tolist()))
    assert r['point_atom'].tolist() == [2, -1, 2, 0, -1] and r['point_dist'][:3].tolist() == [0.5, np.inf, 2.5]
    assert (c['typed_points'], c['matched'], c['unmatched'], c['untyped_points']) == (4, 2, 2, 0)
    assert (c['points_HD'], c['matched_HD'], c['points_AR'], c['matched_AR'], c['matched_HY'], c['atoms_HD'], c['atoms_HY']) == (2, 1, 1, 0, 1, 1, 1)
    assert r['status'] == 0 and FR.features_of_rows(*inputs, pos, pts, [0, 1, 0, 4, -2], M.FeatureLimits(max_unmatched=1))['status'] == M.FEAT_UNMATCHED
    # the cutoff is strict; a dropped atom carries nothing and is not in the compact numbering; a NaN sets NONFINITE
    assert FR.features_of_rows(*inputs, pos, pos[2:] + np.float32([0, 0, 2]), [0])['counts'][1] == 0
    inputs = FR.cpu_inputs([11, FR.C_, FR.O_], {(1, 2): 1, (0, 1): 1})
    r = FR.features_of_rows(*inputs, pos, pos[[2]], [0])
    assert r['atom_fp'].tolist() == [0, 0, 1 | 8] and r['point_atom'].tolist() == [1]
    bad = pos.copy()
    bad[1, 1] = np.nan
    assert FR.features_of_rows(*inputs, bad, pos[[2]], [0])['status'] == M.FEAT_NONFINITE
    assert FR.features_of_rows(*inputs, pos, bad[[1]], [-1])['status'] == M.FEAT_NONFINITE
    assert FR.features_of_rows(*inputs, pos, bad[[1]], [-2])['status'] == 0


@pytest.fixture(scope='module')
def family():
    stats = [0, 0]
    cases = FR.random_family(stats=stats)
    inputs = [FR.cpu_inputs(c['classes'], c['bonds']) for c in cases]
    return cases, inputs, [FR.restate_case(c, i) for c, i in zip(cases, inputs)], stats


def test_random_family_make_up(family):
    cases, inputs, want, stats = family
    assert stats[1] == len(cases) and stats[1] / stats[0] >= 0.90, stats      # the rejection rule leaves at least 90 % of the draws
    assert {1, 2, 3, 63, 64, 65, 127, 128} <= {len(c['classes']) for c in cases}
    assert {len(c['kinds']) for c in cases} == set(FR.FAMILY_POINTS)
    total = sum(w['counts'].astype(np.int64) for w in want)
    c = dict(zip(M.FEATURE_COUNTS, total.tolist()))
    assert all(c['atoms_' + t] > 0 for t in M.FEATURE_TYPES), c
    assert c['matched'] >= 40 and c['unmatched'] >= 200 and c['untyped_points'] >= 40
    assert sum(c['matched_' + t] > 0 for t in M.FEATURE_TYPES) >= 5, c
    assert any(11 in case['classes'] for case in cases) and any(not i[5] for i in inputs) and sum(i[5] for i in inputs) >= 50
    for case in cases:                                                 # the rule itself, restated: nothing within GAP of the cutoff
        if len(case['points']) and len(case['pos']):
            d = np.sqrt(((case['pos'].astype(np.float64)[None] - case['points'].astype(np.float64)[:, None]) ** 2).sum(-1))
            assert (np.abs(d - 2.0) > FR.GAP).all()


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')
def test_rules_on_the_host_under_sanitizers(family, tmp_path):
    """The text the kernel compiles (csrc/feature_core.h), built as a stand-alone host program with ASan + UBSan, on the named
    molecules, the random family and six hundred further random graphs."""
    cases, inputs, want, _ = family
    exe = build_host_check('feature_host_check', tmp_path)
    named = [k for k in FR.NAMED if k != 'indene-like']
    todo = [(FR.cpu_inputs(*FR.NAMED[k][:2]), FR.fp_of(FR.named_answer(k))) for k in named]
    todo += [(i, w['atom_fp']) for i, w in zip(inputs, want) if i[5]]
    rng = np.random.default_rng(31)
    for _ in range(600):
        i = FR.cpu_inputs(*FR.decorate(rng, *K.random_graph(rng, int(rng.integers(1, 41)))))
        if i[5]:
            todo.append((i, FR.fp_of(FR.type_atoms(*i[:5], i[6], i[5]))))
    got = FR.run_host_check(exe, [i for i, _ in todo], tmp_path)
    assert len(got) == len(todo) >= 400
    for k, (g, (_, w)) in enumerate(zip(got, todo)):
        assert np.array_equal(g, w), (k, g.tolist(), w.tolist())
    # a star of 128 atoms: every mask word full
    i = FR.cpu_inputs(*FR.star_graph(128))
    (g,) = FR.run_host_check(exe, [i], tmp_path)
    assert np.array_equal(g, FR.fp_of(FR.type_atoms(*i[:5], i[6], i[5])))


def _features_dict():
    counts = dict.fromkeys(M.FEATURE_COUNTS, 0)
    counts.update(typed_points=3, matched=2, unmatched=1, untyped_points=1, atoms_HD=1, points_HD=2, matched_HD=1, points_AR=1, matched_AR=1)
    return dict(counts, status=M.FEAT_HAS_UNTYPED, features_ok=True, atom_fp=np.array([0, 2, 9], dtype=np.uint8),
                atom_types=[(), ('AR',), ('HD', 'HA')], point_kind=np.array([0, -1, 1, -2, 0], dtype=np.int8),
                point_dist=np.array([0.5, np.inf, 1.25, np.inf, 2.5], dtype=np.float32), point_atom=np.array([2, -1, 1, -1, 2], dtype=np.int16),
                point_matched=np.array([True, False, True, False, False]))


def test_sdf_item(tmp_path):
    mol = {'element': [6, 6, 8], 'atom_pos': torch.zeros(3, 3), 'bond_index': torch.tensor([[0, 1], [1, 2]]), 'bond_type': torch.tensor([1, 1]),
           'status': 0, 'valid': True}
    path = tmp_path / 'f.sdf'
    M.write_sdf(str(path), [dict(mol, features=_features_dict()), mol], names=['a', 'b'])
    text = path.read_text()
    item = ('> <PHOREGEN_FEATURES>\nstatus 0x04\n' + ''.join('%s %d\n' % (k, _features_dict()[k]) for k in M.FEATURE_COUNTS)
            + 'HD 3 0.5000\nAR 2 1.2500\nHD - 2.5000\n\n')
    assert text == M.mol_block(mol, 'a') + item + '$$$$\n' + M.mol_block(mol, 'b') + '$$$$\n'
    assert 'typed_points 3\nmatched 2\nunmatched 1\nuntyped_points 1\natoms_HD 1\n' in item
    ft = _features_dict()
    ft.update(point_dist=np.array([np.inf], dtype=np.float32), point_atom=np.array([-1], dtype=np.int16), point_kind=np.array([6], dtype=np.int8),
              point_matched=np.array([False]))
    assert M._features_item(ft).endswith('matched_XB 0\nXB - inf\n\n')


def test_features_needs_the_device():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    res = {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.features(res, torch.zeros(1, 3), torch.zeros(1, dtype=torch.int8))


def test_binding_declares_the_feature_kernel():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_feat\s*\(', header)
    assert 'pg_mol_feat' in hip.EXPORTS and hasattr(lib, 'pg_mol_feat')
    assert len(hip._PROTOS['pg_mol_feat'][1]) == 31 == arg_count('pg_mol_feat')
    csrc = os.path.join(ROOT, 'phoregen_amd', 'csrc')
    assert 'mol_feat.hip' in open(os.path.join(csrc, 'Makefile')).read() and os.path.exists(os.path.join(csrc, 'feature_core.h'))
    for bit, name in M.FEAT_NAMES.items():
        assert header_macro('PG_FEAT_' + name) == str(bit), name
    assert header_macro('PG_FEAT_N_COUNTS') == str(len(M.FEATURE_COUNTS))
    # argument errors are refused before any launch, without a GPU: oversize, negative sizes, null arrays
    buf = hip.C.cast((hip.C.c_uint8 * 64)(), hip.C.c_void_p)

    def args(B, n_lig, n_bond, max_n, F=1, n_point=0, n_out=0, max_unmatched=0, ptr=None):
        return (ptr, 0, *([ptr] * 10), B, F, n_lig, n_bond, max_n, ptr, ptr, n_point, ptr, ptr, n_out, 2.0, max_unmatched, *([ptr] * 5), None)
    assert lib.pg_mol_feat(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1, ptr=buf)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_feat' in lib.pg_last_error()
    for bad in (args(1, 4, 12, -1), args(-1, 4, 12, 4), args(1, -4, 12, 4), args(1, 4, -12, 4), args(1, 4, 12, 4, F=-1), args(1, 4, 11, 4),
                args(1, 4, 12, 4, n_point=-1), args(1, 4, 12, 4, n_out=-1), args(1, 4, 12, 4, max_unmatched=-1)):
        assert lib.pg_mol_feat(*bad) != 0 and b'pg_mol_feat' in lib.pg_last_error()
    assert lib.pg_mol_feat(*args(1, 4, 12, 4)) != 0                    # every array null
    assert b'pg_mol_feat' in lib.pg_last_error() and b'null' in lib.pg_last_error()
    assert lib.pg_mol_feat(*args(0, 0, 0, 0)) == 0 and lib.pg_mol_feat(*args(3, 4, 12, 4, F=0)) == 0
