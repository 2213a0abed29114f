"""CPU: the restatement of the molecule screen (tests/mol_reference.py) on hand-built molecules, the V2000 writer, the binding.

The kernel itself is held against the restatement in tests/test_gpu_molecule.py; here the restatement's own rule is pinned on cases
small enough to check by eye, so that "kernel == restatement" means something."""
import os
import re

import numpy as np
import pytest
import torch

import mol_reference as R
from mol_support import header_text
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_, C_, N_, O_, F_ = 0, 1, 2, 3, 4          # atom classes (ATOM_TYPES order)


def _screen(atom_cls, bonds, **kw):
    node, pos, edge, ei = R.scores_from_classes(atom_cls, bonds, **kw)
    return R.screen_graph(node, pos, edge, ei)


def test_constants_and_table():
    from phoregen_amd.utils.sample_utils import ATOM_TYPES
    assert M.FAIL_MASK == M.STATUS_NO_ATOMS | M.STATUS_DISCONNECTED | M.STATUS_VALENCE | M.STATUS_NONFINITE == 15
    assert (M.STATUS_HAD_MASKED_ATOM | M.STATUS_HAD_ABSORBING_BOND) & M.FAIL_MASK == 0
    assert list(M.MAX_VALENCE) == ATOM_TYPES == list(M.ELEMENT_SYMBOL)
    assert [M.MAX_VALENCE[z] for z in ATOM_TYPES] == [3, 4, 4, 2, 1, 4, 7, 6, 1, 1, 5]
    # the header's constants and the Python mirrors
    header = header_text()
    defs = dict(re.findall(r'#define (PG_MOL_[A-Z_]+) (\d+)', header))
    assert int(defs['PG_MOL_MAX_ATOMS']) == M.MAX_ATOMS == hip.PG_MOL_MAX_ATOMS >= 128
    for bit, name in M.STATUS_NAMES.items():
        assert int(defs['PG_MOL_' + name]) == bit


def test_benzene_is_valid():
    r = _screen([C_] * 6, {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 4): 4, (4, 5): 4, (0, 5): 4})
    assert r['status'] == 0 and r['valid']
    assert r['counts'].tolist() == [6, 6, 1, 6]
    assert r['valence2'].tolist() == [6] * 6 and r['degree'].tolist() == [2] * 6 and r['comp'].tolist() == [0] * 6
    assert r['order'][R.pair_row(0, 5, 6)] == 4 and int((r['order'] > 0).sum()) == 6


def test_ethanol_plus_water_is_disconnected():
    r = _screen([C_, C_, O_, O_], {(0, 1): 1, (1, 2): 1})
    assert r['status'] == M.STATUS_DISCONNECTED and not r['valid']
    assert r['counts'].tolist() == [4, 2, 2, 3]
    assert r['comp'].tolist() == [0, 0, 0, 3]


def test_valence_rule():
    five = _screen([C_] * 6, {(0, b): 1 for b in range(1, 6)})
    assert five['status'] == M.STATUS_VALENCE and five['valence2'][0] == 10
    n4 = _screen([N_] + [C_] * 4, {(0, b): 1 for b in range(1, 5)})
    assert n4['status'] == 0 and n4['valid'] and n4['valence2'][0] == 8
    f2 = _screen([F_, C_], {(0, 1): 2})
    assert f2['status'] == M.STATUS_VALENCE
    # an aromatic atom may carry half a bond more: C with three aromatic bonds (4.5) passes, with a single on top (5.5) not
    fused = _screen([C_] * 4, {(0, 1): 4, (0, 2): 4, (0, 3): 4})
    assert fused['valence2'][0] == 9 and not fused['status'] & M.STATUS_VALENCE
    over = _screen([C_] * 5, {(0, 1): 4, (0, 2): 4, (0, 3): 4, (0, 4): 1})
    assert over['valence2'][0] == 11 and over['status'] & M.STATUS_VALENCE


def test_masked_atom_and_its_bond_are_dropped():
    r = _screen([C_, 11, C_, O_], {(0, 1): 1, (0, 2): 1, (2, 3): 2})
    assert r['status'] == M.STATUS_HAD_MASKED_ATOM and r['valid']
    assert r['cls'].tolist() == [1, -1, 1, 3] and r['compact'].tolist() == [0, -1, 1, 2] and r['comp'].tolist() == [0, -1, 0, 0]
    assert r['counts'].tolist() == [3, 2, 1, 3]
    assert r['order'][R.pair_row(0, 1, 4)] == 0
    assert r['decoded']['element'] == [6, 6, 8]
    assert r['decoded']['bond_index'].tolist() == [[0, 1], [1, 2]] and r['decoded']['bond_type'].tolist() == [1, 2]


def test_absorbing_bond_row_is_no_bond():
    r = _screen([C_, C_, C_], {(0, 1): 1, (1, 2): 1, (0, 2): 5})
    assert r['status'] == M.STATUS_HAD_ABSORBING_BOND and r['valid']
    assert r['counts'].tolist() == [3, 2, 1, 3] and r['order'].tolist() == [1, 0, 1]


def test_reversed_half_is_ignored():
    r = _screen([C_, C_, C_], {(0, 1): 1}, reversed_only={(1, 2): 1, (0, 2): 5})
    assert r['status'] == M.STATUS_DISCONNECTED                 # no bond 1-2, no absorbing bit
    assert r['counts'].tolist() == [3, 1, 2, 2] and r['order'].tolist() == [1, 0, 0]


def test_all_masked_and_nan():
    r = _screen([11, 11, 11], {(0, 1): 1})
    assert r['status'] == M.STATUS_NO_ATOMS | M.STATUS_HAD_MASKED_ATOM and not r['valid']
    assert r['counts'].tolist() == [0, 0, 0, 0]
    pos = torch.zeros(3, 3)
    pos[1, 2] = float('nan')
    r = _screen([C_, C_, C_], {(0, 1): 1, (1, 2): 1}, pos=pos)
    assert r['status'] == M.STATUS_NONFINITE and not r['valid']
    pos[1, 2] = float('inf')
    assert _screen([C_, C_, C_], {(0, 1): 1, (1, 2): 1}, pos=pos)['status'] == M.STATUS_NONFINITE
    # a non-finite coordinate of a DROPPED atom does not count
    assert _screen([C_, 11, C_], {(0, 2): 1}, pos=pos)['status'] == M.STATUS_HAD_MASKED_ATOM


def test_one_and_two_atoms():
    assert _screen([C_], {})['counts'].tolist() == [1, 0, 1, 1]
    assert _screen([C_, O_], {(0, 1): 2})['counts'].tolist() == [2, 1, 1, 2]
    assert _screen([C_, O_], {})['status'] == M.STATUS_DISCONNECTED


def test_first_maximum_wins():
    node, pos, edge, ei = R.scores_from_classes([C_, C_], {(0, 1): 1})
    node[0] = 0.0                     # all equal: class 0 (B)
    edge[0, :] = 1.0                  # all equal: class 0, no bond
    r = R.screen_graph(node, pos, edge, ei)
    assert r['cls'].tolist() == [0, 1] and r['order'].tolist() == [0]


def test_generated_batch_is_not_empty_of_any_kind():
    """The frozen generator of the GPU comparison, judged by the restatement alone."""
    node, pos, edge, sizes = R.generate_batch()
    for n in (1, 2, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
    c = R.census(R.screen_batch(node, pos, edge, sizes))
    assert c['valid'] >= 10 and c['DISCONNECTED'] >= 10 and c['VALENCE'] >= 10, c
    assert min(c.values()) >= 1, c


ETHANOL = {'element': [6, 6, 8], 'atom_pos': torch.tensor([[-0.8883, 0.1670, -0.0273], [0.4658, -0.5116, -0.0368], [1.4311, 0.3229, 0.5867]]),
           'bond_index': torch.tensor([[0, 1], [1, 2]]), 'bond_type': torch.tensor([1, 1])}
ETHANOL_BLOCK = (
    'ethanol\n'
    '  PhoreGen          3D\n'
    '\n'
    '  3  2  0  0  0  0  0  0  0  0999 V2000\n'
    '   -0.8883    0.1670   -0.0273 C   0  0  0  0  0  0  0  0  0  0  0  0\n'
    '    0.4658   -0.5116   -0.0368 C   0  0  0  0  0  0  0  0  0  0  0  0\n'
    '    1.4311    0.3229    0.5867 O   0  0  0  0  0  0  0  0  0  0  0  0\n'
    '  1  2  1  0\n'
    '  2  3  1  0\n'
    'M  END\n')


def test_mol_block_of_ethanol():
    """The literal was written by hand from the CTfile V2000 layout (name / program line with the dimension code in columns 21-22 /
    comment; counts line aaabbblllfffcccsssxxxrrrpppiiimmmvvvvvv; atom line xxxxx.xxxxyyyyy.yyyyzzzzz.zzzz aaaddcccssshhhbbbvvvHHHrrriiimmmnnneee;
    bond line 111222tttsss).  There is no RDKit in this project to read it back with."""
    assert M.mol_block(ETHANOL, 'ethanol') == ETHANOL_BLOCK
    for line in ETHANOL_BLOCK.split('\n')[4:7]:
        assert len(line) == 69 and line[31:34] in ('C  ', 'O  ')
    with pytest.raises(ValueError):
        M.mol_block(dict(ETHANOL, atom_pos=torch.full((3, 3), float('nan'))))


def _parse_sdf(text):
    """Minimal V2000 reader by columns: [(name, atoms [(x, y, z, symbol)], bonds [(a, b, type)])]."""
    recs = text.split('$$$$\n')
    assert recs[-1] == ''
    out = []
    for rec in recs[:-1]:
        lines = rec.split('\n')
        na, nb = int(lines[3][0:3]), int(lines[3][3:6])
        assert lines[3].endswith('V2000') and lines[4 + na + nb] == 'M  END' and lines[5 + na + nb:] == ['']
        atoms = [(float(l[0:10]), float(l[10:20]), float(l[20:30]), l[31:34].strip()) for l in lines[4:4 + na]]
        bonds = [(int(l[0:3]), int(l[3:6]), int(l[6:9])) for l in lines[4 + na:4 + na + nb]]
        out.append((lines[0], atoms, bonds))
    return out


def test_sdf_round_trip(tmp_path):
    node, pos, edge, ei = R.scores_from_classes([C_] * 6 + [8], {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 4): 4, (4, 5): 4, (0, 5): 4, (5, 6): 1},
                                                pos=torch.randn(7, 3, generator=torch.Generator().manual_seed(3)) * 4)
    chlorobenzene = R.screen_graph(node, pos, edge, ei)['decoded']
    path = tmp_path / 'two.sdf'
    M.write_sdf(str(path), [ETHANOL, chlorobenzene], names=['a', 'b'])
    text = path.read_text()
    assert text.count('$$$$') == 2
    recs = _parse_sdf(text)
    assert [r[0] for r in recs] == ['a', 'b']
    for (name, atoms, bonds), mol in zip(recs, (ETHANOL, chlorobenzene)):
        assert [a[3] for a in atoms] == [M.ELEMENT_SYMBOL[z] for z in mol['element']]
        xyz = np.array([a[:3] for a in atoms])
        assert np.array_equal(xyz, np.round(mol['atom_pos'].double().numpy(), 4))
        assert [(a - 1, b - 1) for a, b, _ in bonds] == [tuple(p) for p in mol['bond_index'].T.tolist()]
        assert [t for _, _, t in bonds] == mol['bond_type'].tolist()
    assert [t for _, _, t in recs[1][2]].count(4) == 6 and recs[1][1][6][3] == 'Cl'
    with pytest.raises(ValueError):
        M.write_sdf(str(path), [ETHANOL], names=['a', 'b'])


def test_screen_argument_errors_need_no_gpu():
    res = {'pred': [torch.zeros(2, 12), torch.zeros(2, 3), torch.zeros(2, 6)], 'traj': [None, None, None],
           'lig_info': [torch.tensor([2])]}
    with pytest.raises(ValueError, match='return_traj'):
        M.screen(res, frames='traj')
    with pytest.raises(ValueError, match='frames'):
        M.screen(res, frames='last')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.screen(res)


def test_binding_declares_the_screen():
    lib = hip.load_library()
    assert 'pg_mol_screen' in hip.EXPORTS and hasattr(lib, 'pg_mol_screen')
    assert len(hip._PROTOS['pg_mol_screen'][1]) == 22
    assert 'mol_screen.hip' in open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
