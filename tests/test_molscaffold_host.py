"""CPU: the scaffold's definition (restated in tests/scaffold_reference.py from DESIGN.md 2.9 "Scaffolds") against the ring screen's
restatement and on the named molecules with hand-written answers; the selection logic the kernel compiles (csrc/scaffold_core.h,
csrc/ring_search.h) as a stand-alone program under the host sanitizers against the restatement; `batch_of`, `scaffold_groups`,
`pick_per_scaffold` and the options on CPU tensors; the binding and its argument errors.

The kernel itself is held against the restatement in tests/test_gpu_molscaffold.py."""
import os
import re

import numpy as np
import pytest
import torch

import mol_reference as R
import ring_reference as G
import scaffold_reference as S
from mol_support import C_, arg_count, build_host_check, cycle, header_macro, header_text, mol_dict, mol_result, rows_of, run_program
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import scaffold as SC
from phoregen_amd.plan import make_edge_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY, WANTS = S.family()


# ---- the restatement against the ring screen's restatement ---------------------------------------------------------------------------------
def test_ring_and_linker_split_agrees_with_the_ring_restatement_on_the_family():
    seen = {role: 0 for role in S.ROLES}
    for (classes, bonds), want in zip(FAMILY, WANTS):
        cls, order = rows_of(classes, bonds)
        n = len(classes)
        r, rr = S.scaffold_of_rows(cls, order), G.rings_of_rows(cls, order)
        ring_rows = sorted(R.pair_row(a, b, n) for a, b in r['ring_bonds'])
        assert ring_rows == np.nonzero(rr['ring_size'])[0].tolist()
        assert ((r['part'] == SC.PART_RING) == (rr['atom_ring'] > 0)).all()
        assert r['counts'][2] == rr['counts'][2] and r['counts'][6] == rr['counts'][3]       # ring atoms, ring systems
        # a linker bond is a bridge between two atoms of the core; every ring atom is in the core
        assert all(rr['ring_size'][R.pair_row(a, b, n)] == 0 and a in r['core'] and b in r['core'] for a, b in r['linker_bonds'])
        assert {int(i) for i in np.nonzero(rr['atom_ring'])[0]} <= r['core']
        # the numbering of the family puts the chosen parts at the word and lane boundaries
        for i, role in want.items():
            assert r['part'][i] == role, (n, i, role)
            seen[role] += 1
    assert min(seen.values()) >= 5, seen
    assert {len(g[0]) for g in FAMILY} >= set(S.FAMILY_SIZES)


# ---- the named molecules, by hand: part, scaffold bonds, the eight counts (exocyclic=True, generic=False) -----------------------------
RING6 = cycle(6, 1)
AROM6, AROM6B = cycle(6, 4), cycle(6, 4, off=6)
FUSED = {**AROM6, (0, 6): 4, (6, 7): 4, (7, 8): 4, (8, 9): 4, (1, 9): 4}
SPIRO = {**cycle(5, 1), (0, 5): 1, (5, 6): 1, (6, 7): 1, (7, 8): 1, (8, 9): 1, (0, 9): 1}
BY_HAND = {
    'none': ([], {}, [0, 0, 0, 0, 0, 0, 0, 0]),
    'one_atom': ([1], {}, [0, 0, 0, 0, 0, 1, 0, 0]),
    'two_atoms': ([1, 1], {}, [0, 0, 0, 0, 0, 2, 0, 0]),
    'three_atoms': ([1, 1, 1], {}, [0, 0, 0, 0, 0, 3, 0, 0]),
    'chain128': ([1] * 128, {}, [0, 0, 0, 0, 0, 128, 0, 0]),
    'ring3_tail125': ([3, 3, 3] + [1] * 125, {(0, 1): 1, (1, 2): 1, (0, 2): 1}, [3, 3, 3, 0, 0, 125, 1, 0]),
    'benzene': ([3] * 6, AROM6, [6, 6, 6, 0, 0, 0, 1, 0]),
    'toluene': ([3] * 6 + [1], AROM6, [6, 6, 6, 0, 0, 1, 1, 0]),
    'biphenyl': ([3] * 12, {**AROM6, **AROM6B, (0, 6): 1}, [12, 13, 12, 0, 0, 0, 2, 1]),
    'diphenylmethane_methyl': ([3] * 12 + [2, 1], {**AROM6, **AROM6B, (0, 12): 1, (6, 12): 1}, [13, 14, 12, 1, 0, 1, 2, 2]),
    'spiro': ([3] * 10, SPIRO, [10, 11, 10, 0, 0, 0, 1, 0]),
    'fused': ([3] * 10, FUSED, [10, 11, 10, 0, 0, 0, 1, 0]),
    'bridged': ([3] * 7, {**RING6, (0, 6): 1, (3, 6): 1}, [7, 8, 7, 0, 0, 0, 1, 0]),
    'ring_carbonyl': ([3] * 6 + [4], {**RING6, (0, 6): 2}, [7, 7, 6, 0, 1, 0, 1, 0]),
    'linker_carbonyl': ([3] * 12 + [2, 4], {**AROM6, **AROM6B, (0, 12): 1, (6, 12): 1, (12, 13): 2}, [14, 15, 12, 1, 1, 0, 2, 2]),
    'ring_exocyclic_carbon': ([3] * 6 + [4, 1, 1], {**RING6, (0, 6): 2}, [7, 7, 6, 0, 1, 2, 1, 0]),
    'ring_triple': ([3] * 6 + [1, 1], RING6, [6, 6, 6, 0, 0, 2, 1, 0]),
    'two_ring_systems': ([3] * 11 + [1], {**AROM6, **cycle(5, 1, off=6)}, [11, 11, 11, 0, 0, 1, 2, 0]),
    'dropped_in_ring': ([1, 1, 1, 0, 1, 1, 1], {}, [0, 0, 0, 0, 0, 6, 0, 0]),
    'absorbing_on_ring': ([1] * 7, {}, [0, 0, 0, 0, 0, 7, 0, 0]),
}
# the same under exocyclic=False where that differs: the `=X` atoms are side chains
BY_HAND_PLAIN = {
    'ring_carbonyl': ([3] * 6 + [1], RING6, [6, 6, 6, 0, 0, 1, 1, 0]),
    'linker_carbonyl': ([3] * 12 + [2, 1], {**AROM6, **AROM6B, (0, 12): 1, (6, 12): 1}, [13, 14, 12, 1, 0, 1, 2, 2]),
    'ring_exocyclic_carbon': ([3] * 6 + [1, 1, 1], RING6, [6, 6, 6, 0, 0, 3, 1, 0]),
}


def _bonds_of(r, n):
    a, b = np.triu_indices(n, 1)
    return {(int(a[p]), int(b[p])): int(r['order'][p]) for p in np.nonzero(r['order'])[0]}


def test_every_named_molecule_has_an_answer():
    assert set(BY_HAND) == set(S.NAMED) and set(BY_HAND_PLAIN) <= set(BY_HAND)


@pytest.mark.parametrize('name', list(S.NAMED))
def test_named_molecule_by_hand(name):
    classes, bonds = S.NAMED[name]
    cls, order = rows_of(classes, bonds)
    n = len(classes)
    for exocyclic in (True, False):
        part, s_bonds, counts = (BY_HAND if exocyclic else {**BY_HAND, **BY_HAND_PLAIN})[name]
        r = S.scaffold_of_rows(cls, order, exocyclic=exocyclic)
        assert r['part'].tolist() == part
        assert _bonds_of(r, n) == s_bonds
        assert dict(zip(SC.SCAFFOLD_COUNTS, r['counts'].tolist())) == dict(zip(SC.SCAFFOLD_COUNTS, counts))
        # the scaffold as a screen
        in_s = np.array([p >= 2 for p in part], dtype=bool)
        assert ((r['cls'] >= 0) == in_s).all() and (r['cls'][in_s] == cls[in_s]).all()
        assert r['compact'][in_s].tolist() == list(range(int(in_s.sum()))) and (r['compact'][~in_s] == -1).all()
        assert r['s_counts'][:2].tolist() == counts[:2]
        g = S.scaffold_of_rows(cls, order, exocyclic=exocyclic, generic=True)
        assert g['part'].tolist() == part and (g['cls'][in_s] == C_).all() and _bonds_of(g, n) == {ab: 1 for ab in s_bonds}
        assert g['counts'].tolist() == counts


def test_named_status_components_and_valence_by_hand():
    one = lambda name, **kw: S.scaffold_of_rows(*rows_of(*S.NAMED[name]), **kw)
    for name in ('none', 'one_atom', 'chain128', 'dropped_in_ring', 'absorbing_on_ring'):
        r = one(name)
        assert r['status'] == M.STATUS_NO_ATOMS and not r['valid'] and r['s_counts'].tolist() == [0, 0, 0, 0]
    r = one('two_ring_systems')
    assert r['status'] == M.STATUS_DISCONNECTED and r['s_counts'].tolist() == [11, 11, 2, 6]
    assert r['comp'].tolist() == [0] * 6 + [6] * 5 + [-1]
    r = one('linker_carbonyl')
    assert r['status'] == 0 and r['valid'] and r['s_counts'].tolist() == [14, 15, 1, 14]
    # benzophenone: the ipso carbons 3 + 3 + 2, the other aromatic carbons 3 + 3, the carbonyl carbon 2 + 2 + 4, the oxygen 4
    assert r['valence2'].tolist() == [8, 6, 6, 6, 6, 6, 8, 6, 6, 6, 6, 6, 8, 4]
    g = one('linker_carbonyl', generic=True)
    assert g['valence2'].tolist() == [6, 4, 4, 4, 4, 4, 6, 4, 4, 4, 4, 4, 6, 2]
    # the documented case that does not reproduce itself: generic + exocyclic, a second pass drops the former `=O`
    again = S.scaffold_of_rows(g['cls'], g['order'], generic=True)
    assert again['part'].tolist() == [3] * 12 + [2, 1] and again['counts'][0] == 13
    # every other combination reproduces itself
    for exo, gen in ((True, False), (False, False), (False, True)):
        for name in S.NAMED:
            r = one(name, exocyclic=exo, generic=gen)
            again = S.scaffold_of_rows(r['cls'], r['order'], exocyclic=exo, generic=gen)
            assert all(np.array_equal(again[k], r[k]) for k in ('cls', 'compact', 'valence2', 'comp', 'order', 's_counts')), name
            assert set(again['part'].tolist()) <= {0, 2, 3, 4}


# ---- the kernel's selection logic on the host, under the sanitizers ----------------------------------------------------------------------
def test_scaffold_core_on_the_host_matches_the_restatement(tmp_path):
    exe = build_host_check('scaffold_host_check', tmp_path)
    graphs = list(S.NAMED.values()) + FAMILY
    cases = tmp_path / 'cases.txt'
    S.write_cases(str(cases), graphs)
    got = run_program(exe, cases)
    want = S.expected_lines(graphs)
    assert len(got) == len(want) + 1 and got[-1] == ''
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k // 3 // len(S.OPTIONS), S.OPTIONS[k // 3 % len(S.OPTIONS)], k % 3)


# ---- batch_of, groups, picks, options: CPU tensors ----------------------------------------------------------------------------------------
def test_batch_of_reproduces_the_molecules():
    mols = [mol_dict([6, 6, 8], [(0, 1), (2, 1)], [1, 2]), mol_dict([7], [], []), mol_dict([], [], []),
            mol_dict([6] * 6 + [17], [(i, (i + 1) % 6) for i in range(6)] + [(6, 0)], [4] * 6 + [1])]
    res = SC.batch_of(mols, 'cpu')
    node, pos, edge = res['pred']
    sizes = res['lig_info'][0].tolist()
    assert sizes == [3, 1, 0, 7] and res['traj'] == [None, None, None]
    assert node.shape == (11, 12) and edge.shape == (6 + 42, 6) and (node.sum(1) == 1).all() and (edge.sum(1) == 1).all()
    ei, eb = make_edge_data(torch.tensor(sizes))
    assert torch.equal(res['lig_info'][2], ei) and torch.equal(res['lig_info'][3], eb)
    assert res['lig_info'][1].tolist() == [0] * 3 + [1] + [3] * 7
    h = edge.size(0)
    for g, (m, ref) in enumerate(zip(mols, R.screen_batch(node, pos, edge, sizes))):
        d = ref['decoded']
        assert d['element'] == m['element'] and torch.equal(d['atom_pos'], m['atom_pos'])
        want = sorted((min(a, b), max(a, b), t) for (a, b), t in zip(m['bond_index'].T.tolist(), m['bond_type'].tolist()))
        assert sorted((a, b, t) for (a, b), t in zip(d['bond_index'].T.tolist(), d['bond_type'].tolist())) == want
    # both halves of the edge rows carry the bond
    e0 = 0
    for n in sizes:
        hh = n * (n - 1) // 2
        assert torch.equal(edge[e0:e0 + hh], edge[e0 + hh:e0 + 2 * hh])
        e0 += 2 * hh
    assert e0 == h
    for bad, word in ((mol_dict([6, 1], [(0, 1)], [1]), 'element 1'), (mol_dict([6, 6], [(0, 1)], [5]), 'outside 1..4'),
                      (mol_dict([6, 6], [(0, 1)], [0]), 'outside 1..4'), (mol_dict([6, 6], [(0, 2)], [1]), 'outside its 2 atoms'),
                      (mol_dict([6, 6], [(1, 1)], [1]), 'to itself'), (mol_dict([6, 6], [(0, 1), (1, 0)], [1, 1]), 'twice')):
        with pytest.raises(ValueError, match=word):
            SC.batch_of([bad], 'cpu')


def test_scaffold_groups_and_picks():
    keys = torch.tensor([7, -3, 7, 5, -3, 7, 9], dtype=torch.int64)
    group, sizes = SC.scaffold_groups(keys)
    assert group.tolist() == [0, 1, 0, 3, 1, 0, 6] and sizes.tolist() == [3, 2, 3, 1, 2, 3, 1]
    assert SC.pick_per_scaffold(group, 1).tolist() == [0, 1, 3, 6]
    assert SC.pick_per_scaffold(group, 2).tolist() == [0, 1, 2, 3, 4, 6]
    assert SC.pick_per_scaffold(group, 3).tolist() == list(range(7)) == SC.pick_per_scaffold(group, 10).tolist()
    assert SC.pick_per_scaffold(group, 0).tolist() == []
    empty = SC.scaffold_groups(torch.zeros(0, dtype=torch.int64))
    assert empty[0].tolist() == [] and empty[1].tolist() == [] and SC.pick_per_scaffold(empty[0], 2).tolist() == []
    # with molecules, equal keys are confirmed: rows 0 and 2 share a key and differ, rows 0 and 5 are one molecule renumbered
    ring = mol_dict([6] * 5 + [7], [(i, (i + 1) % 6) for i in range(6)], [1] * 6)
    ring2 = mol_dict([7] + [6] * 5, [(i, (i + 1) % 6) for i in range(6)], [1] * 6)
    other = mol_dict([6] * 6, [(i, (i + 1) % 6) for i in range(6)], [1] * 6)
    none = mol_dict([], [], [])
    mols = [ring, none, other, other, none, ring2, ring]
    group, sizes = SC.scaffold_groups(keys, mols)
    assert group.tolist() == [0, 1, 2, 3, 1, 0, 6] and sizes.tolist() == [2, 2, 1, 1, 2, 2, 1]
    with pytest.raises(ValueError, match='7 keys and 2 molecules'):
        SC.scaffold_groups(keys, mols[:2])
    for bad in (keys.int(), keys.reshape(1, -1), [1, 2]):
        with pytest.raises(ValueError, match='int64 tensor'):
            SC.scaffold_groups(bad)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match='k must be'):
            SC.pick_per_scaffold(group, bad)
    with pytest.raises(ValueError, match='int64 tensor'):
        SC.pick_per_scaffold(group.int(), 1)


def test_options_are_validated():
    o = SC.ScaffoldOptions()
    assert (o.exocyclic, o.generic, o.flags) == (True, False, 1)
    assert [SC.ScaffoldOptions(e, g).flags for e, g in S.OPTIONS] == [1, 0, 3, 2]
    for kw in (dict(exocyclic=1), dict(generic='no'), dict(exocyclic=None)):
        with pytest.raises(ValueError, match='must be a bool'):
            SC.ScaffoldOptions(**kw)
    assert SC.SCAFFOLD_COUNTS == ('scaffold_atoms', 'scaffold_bonds', 'ring_atoms', 'linker_atoms', 'exocyclic_atoms', 'side_chain_atoms',
                                  'ring_systems', 'linker_bonds')
    assert (SC.PART_NONE, SC.PART_SIDE_CHAIN, SC.PART_LINKER, SC.PART_RING, SC.PART_EXOCYCLIC) == (0, 1, 2, 3, 4)


# ---- the binding and the argument errors ---------------------------------------------------------------------------------------------------
def test_binding_exports_the_entry_point_and_the_header_documents_it():
    header = header_text()
    assert 'pg_mol_scaffold' in hip.EXPORTS and hip.ABI_VERSION == 11
    res, args = hip._PROTOS['pg_mol_scaffold']
    assert len(args) == arg_count('pg_mol_scaffold') == 20
    doc = header[header.index('Murcko scaffold of the molecules'):header.index('int pg_mol_scaffold(')]
    for word in ('DESIGN.md 2.9 "Scaffolds"', 'part', 's_cls', 's_compact', 's_valence2', 's_comp', 's_order', 's_counts', 's_status',
                 'no valence rule', 'error before anything is launched', 'Every element of every output is written',
                 'do not depend on its batch'):
        assert word in doc, word
    for name, value in (('PG_SCAF_EXOCYCLIC', hip.PG_SCAF_EXOCYCLIC), ('PG_SCAF_GENERIC', hip.PG_SCAF_GENERIC),
                        ('PG_SCAF_N_COUNTS', len(SC.SCAFFOLD_COUNTS)), ('PG_SCAF_CARBON', C_), ('PG_SCAF_PART_NONE', SC.PART_NONE),
                        ('PG_SCAF_PART_SIDE_CHAIN', SC.PART_SIDE_CHAIN), ('PG_SCAF_PART_LINKER', SC.PART_LINKER),
                        ('PG_SCAF_PART_RING', SC.PART_RING), ('PG_SCAF_PART_EXOCYCLIC', SC.PART_EXOCYCLIC)):
        assert int(header_macro(name)) == value, name
    lib = hip.load_library()
    assert lib.pg_abi_version() == 11 and lib.pg_mol_scaffold.argtypes == args
    csrc = os.path.join(ROOT, 'phoregen_amd', 'csrc')
    makefile = open(os.path.join(csrc, 'Makefile')).read()
    assert ' mol_scaffold.hip' in makefile and re.search(r'mol_rings\.o \$\(OUT\)/mol_scaffold\.o: ring_search\.h', makefile)
    assert '$(OUT)/mol_scaffold.o: mol_common.h scaffold_core.h' in makefile
    # one copy of the ring search: the header has it, neither kernel file does
    assert 'int ring_through(' in open(os.path.join(csrc, 'ring_search.h')).read()
    for f in ('mol_rings.hip', 'mol_scaffold.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "ring_search.h"' in text and 'int ring_through(' not in text and 'ring_through(s_adj, a, b)' in text


def test_argument_errors_without_a_device():
    node, pos, edge, sizes = G.batch_from([S.NAMED['toluene'], S.NAMED['biphenyl']])
    res = mol_result(node, pos, edge, sizes, dev='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.screen(res)
    refs = R.screen_batch(node, pos, edge, sizes)
    cat = lambda k, dt: torch.from_numpy(np.concatenate([r[k] for r in refs])).to(dt).reshape(1, -1)
    na = torch.tensor(sizes)
    off = lambda v: torch.cat([torch.zeros(1, dtype=torch.long), v.cumsum(0)]).int()
    sc = M.Screen(status=torch.zeros(1, 2, dtype=torch.int32), counts=torch.zeros(1, 2, 4, dtype=torch.int32),
                  valid=torch.ones(1, 2, dtype=torch.bool), cls=cat('cls', torch.int8), compact=cat('compact', torch.int16),
                  valence2=cat('valence2', torch.uint8), comp=cat('comp', torch.int16), order=cat('order', torch.int8),
                  lig_off=off(na), bond_off=off(na * (na - 1)), num_atoms=sizes)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        SC.scaffolds(sc)
    with pytest.raises(ValueError, match='options must be a ScaffoldOptions'):
        SC.scaffolds(sc, options=dict(generic=True))
    with pytest.raises(ValueError, match='needs a Screen'):
        SC.scaffolds(res)
    with pytest.raises(ValueError, match='needs a Scaffolds'):
        SC.scaffold_keys(sc)
    # the library itself refuses bad sizes and flags before it looks at a pointer or a device
    lib = hip.load_library()
    ok = dict(B=1, F=1, n_lig=2, n_bond=2, max_n=2, flags=1)

    def call(**kw):
        a = {**ok, **kw}
        return lib.pg_mol_scaffold(None, None, None, None, a['B'], a['F'], a['n_lig'], a['n_bond'], a['max_n'], a['flags'], *([None] * 10))
    for kw, word in ((dict(max_n=129), 'PG_MOL_MAX_ATOMS'), (dict(n_lig=-1), 'n_lig -1'), (dict(n_bond=3), 'both directions'),
                     (dict(flags=4), 'flags 4'), (dict(flags=-1), 'flags -1')):
        assert call(**kw) != 0, kw
        message = lib.pg_last_error().decode()
        assert message.startswith('pg_mol_scaffold') and word in message, (kw, message)
    assert call(B=0) == 0 and call(F=0) == 0                           # nothing to launch
