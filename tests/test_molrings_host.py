"""CPU: the ring screen's definition (restated in tests/ring_reference.py from DESIGN.md 2.9 "Rings") on the named molecules with
hand-written answers and against networkx, the limits, the SDF data item, the binding and its argument errors.

The kernel itself is held against the restatement in tests/test_gpu_molrings.py."""
import os
import re

import numpy as np
import pytest
import torch

import mol_reference as R
import ring_reference as G
from mol_support import arg_count, header_macro, header_text
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', list(G.NAMED))
def test_named_molecule_by_hand(name):
    classes, bonds, counts, status, status_filter = G.NAMED[name]
    cls, order = G.rows_of(classes, bonds)
    r = G.rings_of_rows(cls, order)
    assert dict(zip(M.RING_COUNTS, r['counts'].tolist())) == dict(zip(M.RING_COUNTS, counts))
    assert r['status'] == status and r['ok'] == (status & M.RING_FAIL_MASK == 0)
    assert G.rings_of_rows(cls, order, M.RingLimits(**G.FILTER))['status'] == status_filter
    # ring_size is 0 exactly off the ring bonds, atom_ring / ring_sys are set exactly on the atoms of a ring bond
    n = len(classes)
    on = np.zeros(n, dtype=bool)
    for (a, b), t in bonds.items():
        rs = int(r['ring_size'][R.pair_row(a, b, n)])
        if rs:
            on[[a, b]] = True
            assert min(r['atom_ring'][a], r['atom_ring'][b]) <= rs and r['ring_sys'][a] == r['ring_sys'][b]
    assert np.count_nonzero(r['ring_size']) == counts[1] and ((r['atom_ring'] > 0) == on).all() and ((r['ring_sys'] >= 0) == on).all()


def test_named_details_by_hand():
    size = lambda name: G.rings_of_rows(*G.rows_of(*G.NAMED[name][:2]))   # noqa: E731
    r = size('norbornane')
    assert sorted(r['ring_size'][r['ring_size'] > 0].tolist()) == [5] * 8 and r['atom_ring'].tolist() == [5] * 7
    r = size('cubane')
    assert sorted(r['ring_size'][r['ring_size'] > 0].tolist()) == [4] * 12
    r = size('spiro[4.5]decane')
    assert r['atom_ring'].tolist() == [5] * 5 + [6] * 5 and r['ring_sys'].tolist() == [0] * 10   # the spiro atom joins the two rings
    assert r['ring_size'][R.pair_row(0, 4, 10)] == 5 and r['ring_size'][R.pair_row(0, 9, 10)] == 6
    r = size('biphenyl')
    assert r['ring_sys'].tolist() == [0] * 6 + [6] * 6 and r['ring_size'][R.pair_row(0, 6, 12)] == 0
    r = size('toluene_aromatic_methyl')
    assert r['atom_ring'].tolist() == [6] * 6 + [0] and r['ring_sys'].tolist() == [0] * 6 + [-1]
    # a dropped atom takes its bonds with it: the ring through it opens, the rest keeps its local indices
    cls, order = G.rows_of([1, 1, 11, 1, 1, 1, 1], {**G.cycle(4), **G.cycle(3, off=4), (3, 4): 1})
    r = G.rings_of_rows(cls, order)
    assert r['counts'].tolist() == [1, 3, 3, 1, 3, 3, 3, 2, 0, 0] and r['ring_sys'].tolist() == [-1] * 4 + [4] * 3
    assert r['ring_size'][R.pair_row(0, 1, 7)] == 0 and r['ring_size'][R.pair_row(1, 2, 7)] == 0
    # nothing at all, one atom, one bond
    assert G.rings_of_rows(*G.rows_of([], {}))['counts'].tolist() == [0] * 10
    assert G.rings_of_rows(*G.rows_of([1], {}))['counts'].tolist() == [0] * 10
    assert G.rings_of_rows(*G.rows_of([1, 1], {(0, 1): 4}))['counts'].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 2]


def _random_rows(rng, n, p_bond):
    cls = rng.choice([1, 1, 1, 2, 3, 11], n)
    bonds = {(a, b): int(rng.integers(1, 6)) for a in range(n) for b in range(a + 1, n) if rng.random() < p_bond}
    return G.rows_of(cls.tolist(), bonds)


def test_restatement_against_networkx():
    nx = pytest.importorskip('networkx')
    rng = np.random.default_rng(11)
    cases = [G.rows_of(*G.NAMED[k][:2]) for k in G.NAMED]
    cases += [_random_rows(rng, int(rng.integers(3, 30)), p) for p in (0.05, 0.1, 0.2, 0.5) for _ in range(6)]
    for cls, order in cases:
        r = G.rings_of_rows(cls, order)
        g = G.nx_graph(cls, order)
        c = dict(zip(M.RING_COUNTS, r['counts'].tolist()))
        assert c['ring_bonds'] == g.number_of_edges() - len(list(nx.bridges(g)))
        assert c['rings'] == len(nx.cycle_basis(g))
        if g.number_of_nodes() <= 14:                                  # (the small cases: the minimum cycle basis is slow)
            assert c['ring_min'] == min((len(x) for x in nx.minimum_cycle_basis(g)), default=0)
        # ring systems: the connected components of the graph of ring bonds that have more than one atom
        ring_only = g.copy()
        ring_only.remove_edges_from(list(nx.bridges(g)))
        want = sorted(sorted(x) for x in nx.connected_components(ring_only) if len(x) > 1)
        got = {}
        for i, s in enumerate(r['ring_sys'].tolist()):
            if s >= 0:
                got.setdefault(s, []).append(i)
        assert sorted(got.values()) == want and all(k == v[0] for k, v in got.items())
        assert c['ring_systems'] == len(want) and c['largest_system'] == max((len(x) for x in want), default=0)


def test_ring_limits():
    lim = M.RingLimits()
    assert (lim.ring_min, lim.ring_max, lim.system_max, lim.rotatable_max) == (3, M.MAX_ATOMS, M.MAX_ATOMS, M.MAX_ATOMS * (M.MAX_ATOMS - 1) // 2)
    with pytest.raises(Exception):                                     # frozen
        lim.ring_min = 4
    for bad in (dict(ring_min=-1), dict(ring_max=2.5), dict(system_max='9'), dict(rotatable_max=2 ** 31), dict(ring_min=True), dict(ring_max=None)):
        with pytest.raises(ValueError, match='RingLimits'):
            M.RingLimits(**bad)
    assert M.RingLimits(ring_min=np.int64(5), ring_max=8).ring_min == 5
    assert M.RING_FAIL_MASK == 1 | 2 | 4 | 8 | 16 and sorted(M.RING_NAMES) == [1, 2, 4, 8, 16, 32] and len(M.RING_COUNTS) == 10
    assert M.RING_COUNTS == ('rings', 'ring_bonds', 'ring_atoms', 'ring_systems', 'ring_min', 'ring_max', 'largest_system', 'rotatable',
                             'aromatic_outside_ring', 'aromatic_lone')


def test_write_sdf_rings_item(tmp_path):
    mol = {'element': [6, 6, 8], 'atom_pos': torch.tensor([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.2, 1.2, 0.0]]),
           'bond_index': torch.tensor([[0, 1], [1, 2]]), 'bond_type': torch.tensor([1, 1]), 'status': 0, 'valid': True}
    ring = dict(zip(M.RING_COUNTS, [2, 11, 10, 1, 5, 6, 10, 3, 1, 2]), status=M.RING_AROMATIC_OUTSIDE | M.RING_AROMATIC_LONE | M.RING_ROTATABLE,
                rings_ok=False, bond_ring_size=np.zeros(2, dtype=np.uint8), atom_ring=np.zeros(3, dtype=np.uint8),
                ring_sys=np.full(3, -1, dtype=np.int16))
    assert M.mol_block(dict(mol, rings=ring), 'x') == M.mol_block(mol, 'x')            # the block itself does not change
    path = tmp_path / 'r.sdf'
    M.write_sdf(str(path), [dict(mol, rings=ring, key=0x1F), mol], names=['x', 'y'])
    item = ('> <PHOREGEN_RINGS>\nstatus 0x31\nrings 2\nring_bonds 11\nring_atoms 10\nring_systems 1\nring_min 5\nring_max 6\n'
            'largest_system 10\nrotatable 3\naromatic_outside_ring 1\naromatic_lone 2\n\n')
    assert path.read_text() == M.mol_block(mol, 'x') + '> <PHOREGEN_KEY>\n000000000000001f\n\n' + item + '$$$$\n' + M.mol_block(mol, 'y') + '$$$$\n'


def test_rings_needs_the_device():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    res = {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.rings(res)
    with pytest.raises(ValueError, match='RingLimits'):
        M.sample_valid(None, None, 1, rings=(5, 8))


def test_binding_declares_the_ring_screen():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_rings\s*\(', header)
    assert 'pg_mol_rings' in hip.EXPORTS and hasattr(lib, 'pg_mol_rings')
    assert len(hip._PROTOS['pg_mol_rings'][1]) == 16 == arg_count('pg_mol_rings')
    assert hip.ABI_VERSION == 11 == lib.pg_abi_version()
    assert 'mol_rings.hip' in open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    for bit, name in M.RING_NAMES.items():
        assert header_macro('PG_RING_' + name) == str(bit), name
    assert header_macro('PG_RING_N_COUNTS') == str(len(M.RING_COUNTS))
    # argument errors are refused before any launch, without a GPU: oversize, negative sizes, no limits
    lim = (hip.C.c_int * 4)(3, 128, 128, 8128)
    args = lambda B, n_lig, n_bond, max_n, F=1, limits=lim: (None, None, None, None, B, F, n_lig, n_bond, max_n, limits, None, None, None,   # noqa: E731
                                                             None, None, None)
    assert lib.pg_mol_rings(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_rings' in lib.pg_last_error()
    for bad in (args(1, 4, 12, -1), args(-1, 4, 12, 4), args(1, -4, 12, 4), args(1, 4, -12, 4), args(1, 4, 12, 4, F=-1), args(1, 4, 11, 4)):
        assert lib.pg_mol_rings(*bad) != 0 and b'pg_mol_rings' in lib.pg_last_error()
    assert lib.pg_mol_rings(*args(1, 4, 12, 4, limits=None)) != 0
    assert b'pg_mol_rings' in lib.pg_last_error() and b'limits' in lib.pg_last_error()
    assert lib.pg_mol_rings(*args(0, 0, 0, 0)) == 0 and lib.pg_mol_rings(*args(3, 4, 12, 4, F=0)) == 0
