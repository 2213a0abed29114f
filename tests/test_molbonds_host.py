"""CPU: the distance bond screen's table, options, restatement and plumbing (phoregen_amd/molecule.py screen(bonds='distance'),
csrc/mol_screen_dist.hip).  The table and the restatement of tests/bonds_reference.py are held against what the reference's own
utils/predict_bonds.py answered, recorded in tests/golden/distance_bonds_v1.npz (tools/make_distance_bond_golden.py)."""
import os
import re

import numpy as np
import pytest
import torch

import bonds_reference as BR
import mol_reference as R
from mol_support import arg_count, header_macro, header_text, listed_pairs
import molkey_reference as K
from phoregen_amd import hip, molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_, C_, N_, O_, SI, P_, S_, CL, I_ = (ATOM_TYPES.index(z) for z in (5, 6, 7, 8, 14, 15, 16, 17, 53))


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'distance_bonds_v1.npz')))


def golden_molecules(g):
    """(classes, fp32 pos [n, 3], recorded bond_index [2, nb], bond_type [nb]) per molecule of the fixture."""
    n0 = 0
    for m, n in enumerate(g['sizes'].tolist()):
        b0, b1 = g['bond_off'][m], g['bond_off'][m + 1]
        yield ([ATOM_TYPES.index(z) for z in g['elements'][n0:n0 + n].tolist()], g['pos'][n0:n0 + n], g['bond_index'][:, b0:b1],
               g['bond_type'][b0:b1])
        n0 += n


def test_table_equals_the_reference_lookup(golden):
    lengths = np.asarray(M.BOND_LENGTHS_PM)
    assert lengths.shape == (3, 11, 11) and lengths.dtype.kind == 'i' and (lengths >= 0).all()
    assert golden['table_pairs'].shape == (66, 2) and len({tuple(p) for p in golden['table_pairs'].tolist()}) == 66
    for (z1, z2), want in zip(golden['table_pairs'].tolist(), golden['table_lengths'].tolist()):
        i, j = ATOM_TYPES.index(z1), ATOM_TYPES.index(z2)
        assert lengths[:, i, j].tolist() == want == lengths[:, j, i].tolist(), (z1, z2)
    for m in lengths:
        assert np.array_equal(m, m.T)
    assert lengths[1, C_, S_] == 160 == lengths[1, S_, C_]                       # listed from carbon's side only: still a double bond
    none = {(M.ELEMENT_SYMBOL[ATOM_TYPES[i]], M.ELEMENT_SYMBOL[ATOM_TYPES[j]]) for i in range(11) for j in range(i, 11) if lengths[0, i, j] == 0}
    assert none == {('B', x) for x in ('B', 'C', 'N', 'O', 'F', 'Si', 'P', 'S', 'Br', 'I')} | {('N', 'Si'), ('Si', 'P'), ('P', 'I'), ('Cl', 'I'),
                                                                                             ('Br', 'I')}
    assert ((lengths[1] > 0) <= (lengths[0] > 0)).all() and ((lengths[2] > 0) <= (lengths[1] > 0)).all()


def test_margins_and_thresholds():
    m = M.BondMargins()
    assert (m.single, m.double, m.triple) == (10, 5, 3)
    with pytest.raises(Exception):                                               # frozen
        m.single = 4
    for bad in (dict(single=-1), dict(double=float('nan')), dict(triple='3'), dict(single=True), dict(double=None), dict(triple=float('inf'))):
        with pytest.raises(ValueError, match='BondMargins'):
            M.BondMargins(**bad)
    t = M.bond_thresholds()
    assert t.shape == (11, 11, 3) and t.dtype == np.float32 and np.array_equal(t, t.transpose(1, 0, 2))
    assert t[C_, C_].tolist() == [164.0, 139.0, 123.0] and t[C_, S_].tolist() == [192.0, 165.0, 0.0] and t[P_, I_].tolist() == [0.0, 0.0, 0.0]
    t2 = M.bond_thresholds(M.BondMargins(single=0, double=2.5, triple=0))
    assert t2[C_, C_].tolist() == [154.0, 136.5, 120.0] and t2[O_, O_].tolist() == [148.0, 123.5, 0.0]     # an absent entry stays 0
    assert M.STATUS_DIST_UNMAPPED_ELEMENT == 64 and M.STATUS_DIST_UNMAPPED_ELEMENT not in M.STATUS_NAMES
    assert not M.FAIL_MASK & M.STATUS_DIST_UNMAPPED_ELEMENT and M.STATUS_HAD_ABSORBING_BOND not in M.DISTANCE_STATUS_NAMES
    assert M.DISTANCE_STATUS_NAMES[64] == 'DIST_UNMAPPED_ELEMENT' and sorted(M.DISTANCE_STATUS_NAMES) == [1, 2, 4, 8, 16, 64]
    assert M.BOND_AGREE_COUNTS == ('both_same', 'both_aromatic', 'both_differ', 'predicted_only', 'distance_only', 'neither')


def test_fixture_meets_its_conditions(golden):
    t = M.bond_thresholds()
    sizes = golden['sizes'].tolist()
    assert 60 <= len(sizes) <= 70 and min(sizes) == 1 and max(sizes) == 60 and golden['pos'].dtype == np.float32
    assert set(golden['elements'].tolist()) <= set(ATOM_TYPES) - {5, 14}
    assert float(golden['margin_pm']) == BR.MARGIN_PM == 1e-3
    for cls, pos, _, _ in golden_molecules(golden):
        assert BR.min_margin_pm(cls, pos, t) >= BR.MARGIN_PM
    census = np.bincount(golden['bond_type'], minlength=4) // 2                   # (both directions are recorded)
    assert census.size == 4 and (census[1:] >= 50).all(), census
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'distance_bonds_v1.npz')) < 256 * 1024


def test_restatement_reproduces_the_reference(golden):
    t = M.bond_thresholds()
    for cls, pos, bi, bt in golden_molecules(golden):
        order = BR.distance_orders(cls, pos, t)
        nz, a, b = listed_pairs(len(cls), order)
        # the reference appends (i, j) then (j, i) for every bonded pair i < j in row-major order
        want_index = np.stack([np.stack([a, b]), np.stack([b, a])], axis=2).reshape(2, -1)
        assert np.array_equal(bi, want_index) and np.array_equal(bt, np.repeat(order[nz], 2))


def _graph(classes, pos):
    node = torch.zeros(len(classes), 12)
    node[torch.arange(len(classes)), torch.tensor(classes)] = 1.0
    return BR.screen_graph(node, torch.tensor(pos, dtype=torch.float32))


def _pair(ca, cb, d):
    return _graph([ca, cb], [[0.0, 0.0, 0.0], [d, 0.0, 0.0]])


def test_hand_cases():
    assert [int(_pair(C_, C_, d)['order'][0]) for d in (1.54, 1.34, 1.20)] == [1, 2, 3]
    assert _pair(C_, S_, 1.60)['order'][0] == 2 == _pair(S_, C_, 1.60)['order'][0]
    assert _pair(O_, O_, 1.00)['order'][0] == 2                                   # no triple entry
    assert _pair(N_, N_, 1.05)['order'][0] == 3
    r = _pair(P_, I_, 1.0)
    assert r['order'][0] == 0 and r['status'] == M.STATUS_DISCONNECTED
    r = _pair(B_, C_, 1.5)
    assert r['order'][0] == 0 and r['status'] == M.STATUS_DISCONNECTED | M.STATUS_DIST_UNMAPPED_ELEMENT
    r = _pair(SI, C_, 1.85)
    assert r['order'][0] == 1 and r['status'] == M.STATUS_DIST_UNMAPPED_ELEMENT and r['valid']
    assert _pair(B_, CL, 1.80)['order'][0] == 1                                    # boron's one entry
    # strict compares: exactly on a threshold is the weaker order (distances whose hundredfold is exact in fp32); the triple test
    # lies inside the double test, so a pair without a double threshold is single however short
    t = np.zeros((11, 11, 3), dtype=np.float32)
    t[C_, C_], t[C_, N_] = (150.0, 125.0, 100.0), (150.0, 0.0, 100.0)
    two = lambda d: np.array([[0, 0, 0], [d, 0, 0]], dtype=np.float32)           # noqa: E731
    assert [int(BR.distance_orders([C_, C_], two(d), t)[0]) for d in (1.5, 1.25, 1.0, 0.75)] == [0, 1, 2, 3]
    assert [int(BR.distance_orders([C_, N_], two(d), t)[0]) for d in (1.5, 1.25, 0.75)] == [0, 1, 1]
    # ethanol-like chain C-C-O, a masked atom and a NaN coordinate: orders, valence, components
    r = _graph([C_, C_, O_, 11, C_], [[0, 0, 0], [1.5, 0, 0], [2.2, 1.2, 0], [0.5, 0.5, 0], [0, float('nan'), 0]])
    assert r['order'].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0, 0] and r['valence2'].tolist() == [2, 4, 2, 0, 0]
    assert r['status'] == M.STATUS_DISCONNECTED | M.STATUS_NONFINITE | M.STATUS_HAD_MASKED_ATOM and r['counts'].tolist() == [4, 2, 2, 3]


def test_agreement_counts_by_hand():
    pred = np.array([1, 2, 4, 4, 4, 3, 1, 0, 5, 5, 0, 2])
    order = np.array([1, 2, 1, 2, 3, 1, 0, 2, 1, 0, 0, 2], dtype=np.int8)
    both = np.array([True] * 11 + [False])
    assert BR.agreement(pred, order, both).tolist() == [2, 2, 2, 1, 2, 2]


def test_binding_declares_the_distance_screen():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_screen_dist\s*\(', header)
    assert 'pg_mol_screen_dist' in hip.EXPORTS and hasattr(lib, 'pg_mol_screen_dist')
    assert len(hip._PROTOS['pg_mol_screen_dist'][1]) == 24 == arg_count('pg_mol_screen_dist')
    assert len(hip._PROTOS['pg_mol_screen'][1]) == 22 == arg_count('pg_mol_screen')
    assert hip.ABI_VERSION == 11 == lib.pg_abi_version()
    makefile = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert 'mol_screen_dist.hip' in makefile and re.search(r'mol_screen_dist\.o[^\n]*: mol_common\.h', makefile)
    assert header_macro('PG_MOL_DIST_UNMAPPED_ELEMENT') == str(M.STATUS_DIST_UNMAPPED_ELEMENT)
    # argument errors are refused before any launch, without a GPU: oversize, negative sizes, missing tables, scores without agree
    val, thr, cnt = (hip.C.c_ubyte * 16)(), (hip.C.c_float * 363)(), (hip.C.c_int * 8)()
    scores, misaligned = 64, 68                                                  # (addresses that are never read)

    def args(B, n_lig, n_bond, max_n, F=1, val=val, thr=thr, edge=None, agree=None, node=None, node_fs=0, edge_fs=0):
        return (node, node_fs, None, 0, edge, edge_fs, None, None, B, F, n_lig, n_bond, max_n, val, thr, None, None, None, None, None, None,
                None, agree, None)
    assert lib.pg_mol_screen_dist(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_screen_dist' in lib.pg_last_error()
    for bad in (args(1, 4, 12, -1), args(-1, 4, 12, 4), args(1, -4, 12, 4), args(1, 4, -12, 4), args(1, 4, 12, 4, F=-1), args(1, 4, 11, 4),
                args(1, 4, 12, 4, val=None), args(1, 4, 12, 4, thr=None), args(1, 4, 12, 4, edge=scores),
                args(1, 4, 12, 4, node=misaligned), args(2, 4, 12, 4, F=2, node_fs=50),
                args(1, 4, 12, 4, edge=misaligned, agree=cnt),
                args(1, 4, 12, 4, F=2, edge=scores, agree=cnt, edge_fs=73)):
        assert lib.pg_mol_screen_dist(*bad) != 0 and b'pg_mol_screen_dist' in lib.pg_last_error()
    assert lib.pg_mol_screen_dist(*args(0, 0, 0, 0)) == 0 and lib.pg_mol_screen_dist(*args(3, 4, 12, 4, F=0)) == 0


def _cpu_result():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    return {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}


def test_screen_arguments_and_no_cpu_fallback():
    res = _cpu_result()
    for bad in ('x', 'openbabel', None, 1):
        with pytest.raises(ValueError, match='bonds must be one of'):
            M.screen(res, bonds=bad)
    with pytest.raises(ValueError, match='BondMargins'):
        M.screen(res, bonds='distance', margins=(10, 5, 3))
    for call in (lambda: M.screen(res, bonds='distance'), lambda: M.bond_agreement(res), lambda: M.screen(res)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(ValueError, match='add_edge'):
        M.sample_valid(None, None, 1, add_edge='openbabel')
    with pytest.raises(ValueError, match='BondMargins'):
        M.sample_valid(None, None, 1, add_edge='distance', bond_margins=(10, 5, 3))


def _screen_of(n_atoms, bonds, agree=False):
    z = lambda *shape, dt=torch.int32: torch.zeros(*shape, dtype=dt)             # noqa: E731
    h = n_atoms * (n_atoms - 1) // 2
    return M.Screen(status=z(1, 1), counts=z(1, 1, 4), valid=z(1, 1, dt=torch.bool), cls=z(1, n_atoms, dt=torch.int8),
                    compact=torch.arange(n_atoms, dtype=torch.int16).reshape(1, -1), valence2=z(1, n_atoms, dt=torch.uint8),
                    comp=z(1, n_atoms, dt=torch.int16), order=z(1, h, dt=torch.int8), lig_off=torch.tensor([0, n_atoms], dtype=torch.int32),
                    bond_off=torch.tensor([0, 2 * h], dtype=torch.int32), num_atoms=[n_atoms], bonds=bonds,
                    agree=torch.arange(6, dtype=torch.int32).reshape(1, 1, 6) + 1 if agree else None)


def test_screen_dataclass_and_same_screen():
    by_keyword = M.Screen(status=None, counts=None, valid=None, cls=None, compact=None, valence2=None, comp=None, order=None, lig_off=None,
                          bond_off=None, num_atoms=[])
    assert by_keyword.bonds == 'predicted' and by_keyword.agree is None          # the new fields have defaults
    p, d = _screen_of(3, 'predicted'), _screen_of(3, 'distance')
    assert M._same_screen(p, _screen_of(3, 'predicted')) and M._same_screen(d, _screen_of(3, 'distance')) and M._same_screen(d, d)
    assert not M._same_screen(p, d) and not M._same_screen(d, _screen_of(4, 'distance'))


def test_assemble_takes_a_screen_and_refuses_a_mixed_bond_source():
    res = {'pred': [torch.zeros(3, 12), torch.arange(9, dtype=torch.float32).reshape(3, 3), torch.zeros(6, 6)]}
    d = _screen_of(3, 'distance', agree=True)
    d.order[0, 1] = 2                                                            # the pair (0, 2)
    mols = M.assemble(res, screen=d)                                             # (CPU tensors: nothing is launched with a screen handed in)
    assert len(mols) == 1 and mols[0]['bonds'] == 'distance' and mols[0]['bond_index'].tolist() == [[0], [2]]
    assert mols[0]['bond_type'].tolist() == [2] and mols[0]['element'] == [5, 5, 5]
    assert mols[0]['bond_agreement'] == dict(zip(M.BOND_AGREE_COUNTS, range(1, 7)))
    assert 'bond_agreement' not in M.assemble(res, screen=_screen_of(3, 'distance'))[0]
    rings_of_predicted = M.Rings(status=torch.zeros(1, 1, dtype=torch.int32), counts=torch.zeros(1, 1, 10, dtype=torch.int32),
                                 ok=torch.ones(1, 1, dtype=torch.bool), ring_size=torch.zeros(1, 3, dtype=torch.uint8),
                                 atom_ring=torch.zeros(1, 3, dtype=torch.uint8), ring_sys=torch.zeros(1, 3, dtype=torch.int16),
                                 limits=M.RingLimits(), screen=_screen_of(3, 'predicted'))
    with pytest.raises(ValueError, match='bond sources'):
        M.assemble(res, rings=rings_of_predicted, screen=d)
    rings_of_predicted.screen = _screen_of(3, 'distance')
    assert M.assemble(res, rings=rings_of_predicted, screen=d)[0]['rings']['rings_ok']
    with pytest.raises(ValueError, match='screen= must be a Screen'):
        M.assemble(res, screen=_screen_of(4, 'distance'))


class _Model:
    def sample(self, data, n, device, **kw):
        return [dict(K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 1})) for _ in range(n)]


def test_sample_valid_hands_the_mode_to_every_analysis(monkeypatch):
    seen, screens = [], []

    def assemble(res, keys=False, **kw):
        seen.append(dict(kw))
        return [dict(m, rings={'rings_ok': True}, kekule={'kekule_ok': True}, smiles={'smiles_ok': True}) for m in res]

    def screen(res, frames, bonds='predicted', margins=None):
        screens.append((frames, bonds, margins))
        return 'screen-%s' % bonds
    monkeypatch.setattr(M, 'assemble', assemble)
    monkeypatch.setattr(M, '_screen', screen)
    monkeypatch.setattr(M, '_rings', lambda res, screen, limits: ('rings', screen))
    monkeypatch.setattr(M, '_kekulize', lambda res, screen, options: ('kekule', screen))
    monkeypatch.setattr(M, '_smiles', lambda res, screen, kekule, stereo: ('smiles', screen, kekule))
    monkeypatch.setattr(M, '_fingerprints', lambda sc, radius: ('fps', sc))
    monkeypatch.setattr(M, 'molecule_keys', lambda sc: ('keys', sc))
    margins = M.BondMargins(single=8)
    out = M.sample_valid(_Model(), None, num_samples=2, rings=True, kekule=True, smiles=True, fingerprints=True, add_edge='distance',
                         bond_margins=margins)
    sc = 'screen-distance'
    assert len(out['finished']) == 2 and screens == [('final', 'distance', margins)]         # one screen per draw
    assert seen == [{'rings': ('rings', sc), 'kekule': ('kekule', sc), 'smiles': ('smiles', sc, ('kekule', sc)), 'fingerprints': ('fps', sc),
                     'screen': sc}]
    del seen[:], screens[:]
    M.sample_valid(_Model(), None, num_samples=1, rings=True, add_edge='distance')
    assert screens == [('final', 'distance', M.BondMargins())] and seen == [{'rings': ('rings', sc), 'screen': sc}]
    del seen[:], screens[:]
    monkeypatch.setattr(M, 'bond_agreement', lambda res, frames, margins: ('agreement', frames, margins))
    M.sample_valid(_Model(), None, num_samples=1, rings=True, add_edge='distance', bond_agreement=True)
    ag = ('agreement', 'final', M.BondMargins())
    assert screens == [] and seen == [{'rings': ('rings', ag), 'screen': ag}]    # the agreement screen IS the draw's distance screen
    del seen[:], screens[:]
    M.sample_valid(_Model(), None, num_samples=1, rings=True)                   # the default: as it always was, no screen= keyword
    assert screens == [('final', 'predicted', None)] and seen == [{'rings': ('rings', 'screen-predicted')}]


def test_write_sdf_bonds_item(tmp_path):
    mol = {'element': [6, 6, 8], 'atom_pos': torch.tensor([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.2, 1.2, 0.0]]),
           'bond_index': torch.tensor([[0, 1], [1, 2]]), 'bond_type': torch.tensor([1, 1]), 'status': 0, 'valid': True}
    agree = dict(zip(M.BOND_AGREE_COUNTS, [2, 0, 0, 1, 0, 0]))
    path = tmp_path / 'b.sdf'
    M.write_sdf(str(path), [dict(mol, bonds='distance', bond_agreement=agree, key=0x1F), dict(mol, bonds='distance'), mol], names=['x', 'y', 'z'])
    item = '> <PHOREGEN_BONDS>\nmode distance\nboth_same 2\nboth_aromatic 0\nboth_differ 0\npredicted_only 1\ndistance_only 0\nneither 0\n\n'
    assert path.read_text() == (M.mol_block(mol, 'x') + item + '> <PHOREGEN_KEY>\n000000000000001f\n\n' + '$$$$\n'
                                + M.mol_block(mol, 'y') + '> <PHOREGEN_BONDS>\nmode distance\n\n$$$$\n' + M.mol_block(mol, 'z') + '$$$$\n')
    M.write_sdf(str(path), [mol, dict(mol, key=3)], names=['x', 'y'])           # without the new keys: the text is as it always was
    assert path.read_text() == M.mol_block(mol, 'x') + '$$$$\n' + M.mol_block(mol, 'y') + '> <PHOREGEN_KEY>\n0000000000000003\n\n$$$$\n'
    assert M.mol_block(dict(mol, bonds='distance', bond_agreement=agree), 'x') == M.mol_block(mol, 'x')


def test_generated_batch_keeps_its_margin():
    node, pos, edge, sizes = BR.generate_batch()
    t, n0 = M.bond_thresholds(), 0
    for n in sizes:
        cls = node[n0:n0 + n].argmax(-1).numpy()
        assert BR.min_margin_pm(cls, pos[n0:n0 + n].numpy(), t) >= BR.MARGIN_PM
        n0 += n
    for n in (1, 2, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
