"""CPU: the hydrogen placement without a device -- the constants and options of phoregen_amd/hydrogens.py, the float64 restatement of
tests/hydrogen_reference.py against facts that do not come from it (lengths, ideal angles, staggered and planar torsions, hydrogen
counts), the conditions on the generated family, the core of csrc/hydrogen_core.h compiled for the host under ASan / UBSan against
the restatement (integers `==`, positions within the derived bound), the all-atom mol block, the binding and the argument errors."""
import math
import os
import re

import numpy as np
import pytest
import torch

import hydrogen_reference as H
from mol_support import build_host_check, header_macro as macro, header_text, mol_result, read_mol_block as _read_block
from phoregen_amd import hip, hydrogens as HY, molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TET_ANGLE = math.degrees(math.acos(-1.0 / 3.0))


@pytest.fixture(scope='module')
def family():
    """(graphs, drawn): built once, read by several tests, changed by none."""
    return H.family()


@pytest.fixture(scope='module')
def host_check(tmp_path_factory):
    return build_host_check('hydrogen_host_check', tmp_path_factory.mktemp('hydrogen_host_check'))


def _exact(name, options=None):
    """The restatement on an example's float64 coordinates as they are: (result, heavy positions, neighbours)."""
    c, b, p, _ = H.EXAMPLES[name]
    r = H.hydrogens_of(c, b, p, options, exact=True)
    rows = H.all_rows(c, b, p)
    return r, np.asarray(p, dtype=np.float64), H.graph_of_rows(rows.cls, rows.kekule_order, rows.order)[1]


def test_constants_options_and_header_agree():
    for bit, name in HY.HYD_NAMES.items():
        assert int(macro('PG_HYD_' + name)) == bit
    assert HY.HYD_FAIL_MASK == 1 | 2 | 4 | 8 and len(HY.HYD_COUNTS) == int(macro('PG_HYD_N_COUNTS')) == hip.PG_HYD_N_COUNTS == 8
    assert HY.MAX_PER_ATOM == int(macro('PG_HYD_MAX_PER_ATOM')) == 4 and float(macro('PG_HYD_DEG_EPS').rstrip('f')) == HY.DEG_EPS == 1e-3
    assert [int(macro('PG_HYD_SHAPE_' + n.upper())) for n in HY.SHAPE_NAMES[1:]] == [1, 2, 3, 4]
    assert [HY.XH_LENGTH[z] for z in ATOM_TYPES] == [1.19, 1.09, 1.01, 0.96, 0.92, 1.48, 1.42, 1.34, 1.27, 1.41, 1.61]
    opt = HY.HydrogenOptions()
    assert opt.xh_length == tuple(HY.XH_LENGTH[z] for z in ATOM_TYPES) and opt.clash_min == 1.5 and opt.max_contacts == 2 ** 31 - 1
    assert HY.HydrogenOptions(xh_length=[1] * 11).xh_length == (1.0,) * 11            # a list is taken, and frozen as a tuple
    with pytest.raises(Exception):
        opt.clash_min = 2.0
    for bad in (dict(xh_length=(1.0,) * 10), dict(xh_length='1.09'), dict(xh_length=(float('nan'),) + (1.0,) * 10),
                dict(xh_length=(-1.0,) + (1.0,) * 10), dict(clash_min=-0.1), dict(clash_min=float('inf')), dict(clash_min=True),
                dict(max_contacts=-1), dict(max_contacts=1.5), dict(max_contacts=2 ** 31)):
        with pytest.raises(ValueError, match='HydrogenOptions'):
            HY.HydrogenOptions(**bad)
    assert HY.status_names(HY.HYD_GENERIC | HY.HYD_HAS_HYDROGEN) == ('GENERIC', 'HAS_HYDROGEN') and HY.status_names(0) == ()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read().split('* **Hydrogens**')[1].split('\n* **')[0]
    for text in (HY.__doc__, design):                                  # both say what the numbers are
        assert 'design choices' in text and 'RDKit' in text and 'from memory' in text


def test_restatement_lengths_counts_and_shapes_on_the_hand_examples():
    for name, (c, b, p, sites) in H.EXAMPLES.items():
        r, pos, nbrs = _exact(name)
        rows = H.all_rows(c, b, p)
        assert {i: (int(r['h_placed'][i]), int(r['site_shape'][i])) for i in range(len(c)) if r['h_placed'][i]} == sites, name
        assert r['counts'][0] == sum(int(x) for x in rows.hcount) == sum(h for h, _ in sites.values()), name   # every counted hydrogen is placed
        assert r['counts'][1] == len(sites) and r['counts'][2:6].sum() == len(sites) and r['counts'][7] == len(c), name
        assert r['ok'] and r['status'] & HY.HYD_HAS_HYDROGEN and bool(r['status'] & HY.HYD_GENERIC) == any(s == H.GEN for _, s in sites.values())
        for i, (h, _) in sites.items():
            for k in range(4):
                d = np.linalg.norm(r['h_pos'][i, k] - pos[i])
                assert abs(d - HY.XH_LENGTH[ATOM_TYPES[c[i]]]) < 1e-12 if k < h else not r['h_pos'][i, k].any(), (name, i, k)
    # the kekulisation's own census agrees: PHOREGEN_KEKULE's hydrogens are the ones placed
    c, b, p, _ = H.EXAMPLES['acetamide']
    import kekule_reference as K
    assert K.kekule_of_rows(*K.rows_of(c, b))['counts'][5] == 5


def test_restatement_ideal_angles_on_ideal_skeletons():
    ideal = {H.TET: TET_ANGLE, H.TRIG: 120.0, H.LIN: 180.0}
    checked = 0
    for name in H.IDEAL_SKELETONS:
        r, pos, nbrs = _exact(name)
        for i in range(len(pos)):
            h, want = int(r['h_placed'][i]), ideal[int(r['site_shape'][i])] if r['h_placed'][i] else None
            want = 126.0 if name == 'pyrrole' else want                # a regular pentagon: the bisector of 360 - 108 degrees
            for k in range(h):
                for j in nbrs[i]:
                    assert abs(H.angle(r['h_pos'][i, k], pos[i], pos[j]) - want) < 1e-9, (name, i, k, j)
                    checked += 1
                for k2 in range(k + 1, h):
                    assert abs(H.angle(r['h_pos'][i, k], pos[i], r['h_pos'][i, k2]) - want) < 1e-9, (name, i, k, k2)
                    checked += 1
    assert checked >= 150
    # the generic example: the four carbons lean away from +z, the hydrogen stands there
    r, pos, _ = _exact('tetramethylphosphorane')
    assert np.allclose(r['h_pos'][0, 0], [0.0, 0.0, HY.XH_LENGTH[15]], atol=1e-12)
    # the collinear example: the first fixed vertex, for the amine and (after the hydrogen opposite the bond) for the methyls
    r, pos, _ = _exact('collinear dimethylamine')
    assert np.allclose(r['h_pos'][1, 0], HY.XH_LENGTH[7] * H.VERTICES[0], atol=1e-12)
    assert np.allclose(r['h_pos'][0, 0] - pos[0], [-HY.XH_LENGTH[6], 0.0, 0.0], atol=1e-12)


def test_restatement_torsions_staggered_ethane_planar_amide_and_pyrrole():
    r, pos, _ = _exact('ethane')
    ts = sorted(round(abs(H.torsion(r['h_pos'][0, a], pos[0], pos[1], r['h_pos'][1, b])), 9) for a in range(3) for b in range(3))
    assert ts == [60.0] * 6 + [180.0] * 3
    r, pos, _ = _exact('methanol')                                     # the hydroxyl hydrogen is anti to nothing: the axis rule; staggered all the same
    assert sorted(round(abs(H.torsion(r['h_pos'][0, a], pos[0], pos[1], r['h_pos'][1, 0])), 9) for a in range(3)) == [60.0, 60.0, 180.0]
    r, pos, _ = _exact('acetamide')                                    # N-H in the plane of C, C(=O), N: anti and syn to the methyl carbon
    assert abs(abs(H.torsion(r['h_pos'][3, 0], pos[3], pos[1], pos[0])) - 180.0) < 1e-9 and abs(H.torsion(r['h_pos'][3, 1], pos[3], pos[1], pos[0])) < 1e-9
    assert abs(r['h_pos'][3, 0][2]) < 1e-12 and abs(r['h_pos'][3, 1][2]) < 1e-12
    for name in ('pyrrole', 'benzene', 'pyridine', 'ethene', 'formaldehyde'):
        r, pos, _ = _exact(name)                                       # flat skeletons in z = 0 keep their hydrogens there
        assert np.abs(r['h_pos'][..., 2]).max() < 1e-12, name
    r, pos, _ = _exact('pyrrole')                                      # and the N-H points out of the ring
    assert np.linalg.norm(r['h_pos'][0, 0]) > np.linalg.norm(pos[0]) + 0.99 * HY.XH_LENGTH[7]


def test_family_conditions(family):
    graphs, drawn = family
    assert len(graphs) == H.FAMILY_GRAPHS + 2 and drawn - H.FAMILY_GRAPHS <= 0.05 * drawn        # at most 5 % redrawn
    opt = HY.HydrogenOptions(clash_min=H.FAMILY_CLASH)
    census = H.census(graphs, opt)
    assert all(row in census for row in H.TABLE_ROWS), [row for row in H.TABLE_ROWS if row not in census]
    assert sum(v for (s, _, _), v in census.items() if s == H.GEN) >= 20                       # and the generic rule
    assert {len(c) for c, _, _ in graphs} >= {1, 2, 64, 65, 128}
    assert all(H.is_safe(H.hydrogens_of(*g, options=opt), opt) for g in graphs)
    for clash in H.EXAMPLE_CLASH:
        o = HY.HydrogenOptions(clash_min=clash)
        for g in H.example_graphs():
            assert H.is_safe(H.hydrogens_of(*g, options=o), o) and H.is_safe(H.hydrogens_of(g[0], g[1], H.mirrored(g[2]), options=o), o)
    # the default clash_min lies within a factor 2 of the 1-3 distances of every molecule: contacts are not compared with `==` at it
    assert not H.is_safe(H.hydrogens_of(*H.example_graphs()[1]))


def test_host_core_against_the_restatement(host_check, family, tmp_path):
    graphs = H.example_graphs()
    graphs += [(c, b, H.mirrored(p)) for c, b, p in graphs]
    worst = 0.0
    for clash in H.EXAMPLE_CLASH:
        opt = HY.HydrogenOptions(clash_min=clash, max_contacts=10)
        cases = [H.all_rows(*g) for g in graphs]
        got = H.run_host_check(host_check, cases, tmp_path, opt)
        for g, (x, rows) in enumerate(zip(got, cases)):
            worst = max(worst, H.compare(x, H.restate(rows, opt), rows.pos, opt, where='example %d clash %g' % (g, clash)))
        contacts = [int(x['counts'][6]) for x in got]
        assert (max(contacts) == 0) if clash < 1 else (min(c for c, g in zip(contacts, graphs) if len(g[0]) > 1) > 0)
        assert any(x['status'] & HY.HYD_CONTACTS for x in got) == (clash > 1)
    opt = HY.HydrogenOptions(clash_min=H.FAMILY_CLASH)
    cases = [H.all_rows(*g) for g in family[0]]
    got = H.run_host_check(host_check, cases, tmp_path, opt)
    ratios = [H.compare(x, H.restate(rows, opt), rows.pos, opt, where='family %d' % g) for g, (x, rows) in enumerate(zip(got, cases))]
    worst = max(worst, max(ratios))
    print('host core, worst error / bound: %.4f' % worst)
    assert 0.0 < worst <= 1.0
    assert [x['status'] for x in got[-2:]] == [HY.HYD_NO_KEKULE] * 2 and not any(x['h_pos'].any() or x['counts'].any() for x in got[-2:])
    # the cases without a geometry of their own: a NaN coordinate, a dropped atom between kept ones, five hydrogens on one atom
    c, b, p, _ = H.EXAMPLES['propane']
    nan = np.array(p, dtype=np.float32)
    nan[0, 1] = np.nan
    dropped = ([c[0], 11, c[1], c[2]], {(0, 2): 1, (2, 3): 1, (0, 1): 1}, [p[0], [9.0, 9.0, 9.0], p[1], p[2]])
    cases = [H.all_rows(c, b, nan), H.all_rows(*dropped), H.all_rows(c, b, p)._replace(hcount=[3, 5, 3])]
    got = H.run_host_check(host_check, cases, tmp_path)
    for g, (x, rows) in enumerate(zip(got, cases)):
        H.compare({**x, 'min_contact': H.restate(rows)['min_contact']}, H.restate(rows), rows.pos, where='special %d' % g)
    # (nothing at the atom or next to it; the far methyl's torsion reference is the NaN atom, so it takes the generic rule)
    assert got[0]['status'] == HY.HYD_NONFINITE | HY.HYD_GENERIC | HY.HYD_HAS_HYDROGEN
    assert got[0]['h_placed'].tolist() == [0, 0, 3] and got[0]['site_shape'].tolist() == [0, 0, H.GEN]
    assert got[1]['h_placed'].tolist() == [3, 0, 2, 3] and got[1]['counts'][7] == 3 and got[1]['status'] == HY.HYD_HAS_HYDROGEN
    assert got[2]['status'] == HY.HYD_TOO_MANY and got[2]['counts'].tolist() == [0] * 7 + [3] and not got[2]['h_pos'].any()


# ---- the mol block ---------------------------------------------------------------------------------------------------------------------------
def _assembled(name, options=None):
    """What `assemble(kekule=, hydrogens=)` returns for an example without dropped atoms, by the restatements alone."""
    import kekule_reference as K
    c, b, p, _ = H.EXAMPLES[name]
    rows = H.all_rows(c, b, p)
    r = H.restate(rows, options)
    pairs = sorted(b)
    at = [a * len(c) - a * (a + 1) // 2 + (x - a - 1) for a, x in pairs]
    m = {'element': [ATOM_TYPES[k] for k in c], 'atom_pos': torch.as_tensor(np.asarray(p, dtype=np.float32)),
         'bond_index': torch.tensor(pairs, dtype=torch.long).reshape(-1, 2).T, 'bond_type': torch.tensor([b[k] for k in pairs], dtype=torch.long),
         'status': 0, 'valid': True}
    formula, weight = M.formula_of(m['element'], rows.hcount, int(sum(rows.charge)))
    m['kekule'] = dict({'status': rows.kekule_status, 'kekule_ok': not rows.kekule_status & M.KEKULE_FAILED,
                        'bond_type': torch.tensor([int(rows.kekule_order[k]) for k in at]),
                        'hcount': np.asarray(rows.hcount, dtype=np.uint8), 'charge': np.asarray(rows.charge, dtype=np.int8), 'formula': formula,
                        'mol_weight': weight},
                       **{M._KEKULE_KEYS[k]: int(x) for k, x in zip(M.KEKULE_COUNTS, K.kekule_of_rows(rows.cls, rows.order)['counts'])})
    m['hydrogens'] = HY.molecule_entry(r['status'], r['counts'], r['min_contact'], r['h_pos'], r['h_placed'], r['site_shape'])
    return m


def test_mol_block_is_unchanged_without_hydrogens_and_all_atom_with_them(tmp_path):
    m = _assembled('acetamide')
    plain = {k: v for k, v in m.items() if k != 'hydrogens'}
    heavy = M.mol_block(plain, 'x')
    assert heavy == ('x\n  PhoreGen          3D\n\n  4  3  0  0  0  0  0  0  0  0999 V2000\n'
                     '    1.5200    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0\n'
                     '    0.0000    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0\n'
                     '   -0.6150    1.0652    0.0000 O   0  0  0  0  0  0  0  0  0  0  0  0\n'
                     '   -0.6700   -1.1605    0.0000 N   0  0  0  0  0  0  0  0  0  0  0  0\n'
                     '  1  2  1  0\n  2  3  2  0\n  2  4  1  0\nM  END\n')
    # 'hydrogens' that is not ok, or without an ok Kekulé form, changes no byte
    assert M.mol_block({**m, 'hydrogens': {**m['hydrogens'], 'hydrogens_ok': False}}, 'x') == heavy
    assert M.mol_block({k: v for k, v in m.items() if k != 'kekule'}, 'x') == M.mol_block({k: v for k, v in plain.items() if k != 'kekule'}, 'x')
    assert M.mol_block({**m, 'kekule': {**m['kekule'], 'kekule_ok': False}}, 'x') == M.mol_block({**plain, 'kekule': {**m['kekule'], 'kekule_ok': False}}, 'x')
    # the all-atom block: heavy lines first and unchanged, then the hydrogens and their bonds
    full = M.mol_block(m, 'x')
    atoms, bonds = _read_block(full)
    h_atoms, h_bonds = _read_block(heavy)
    assert len(atoms) == 4 + 5 and len(bonds) == 3 + 5 and atoms[:4] == h_atoms and bonds[:3] == h_bonds
    assert [a[0] for a in atoms[4:]] == ['H'] * 5 and [(a, b, t) for a, b, t in bonds[3:]] == [(0, 4, 1), (0, 5, 1), (0, 6, 1), (3, 7, 1), (3, 8, 1)]
    assert m['hydrogens']['h_parent'].tolist() == [0, 0, 0, 3, 3]
    for (a, hh, _), k in zip(bonds[3:], range(5)):
        d = math.dist(atoms[a][1:], atoms[hh][1:])
        assert abs(d - HY.XH_LENGTH[m['element'][a]]) < 2e-4 and np.allclose(atoms[hh][1:], m['hydrogens']['h_pos'][k], atol=5.1e-5)
    elements, pos = HY.all_atoms(m)
    assert elements == [6, 6, 8, 7] + [1] * 5 and pos.shape == (9, 3) and np.allclose(pos[4:], m['hydrogens']['h_pos'])
    assert HY.all_atoms(plain)[0] == [6, 6, 8, 7]
    # a charged atom keeps its charge lines; the data item carries status, counts and min_contact
    n4 = _assembled('tetramethylammonium')
    text = M.mol_block(n4)
    assert 'M  CHG  1   1   1\nM  END\n' in text and len(_read_block(text)[0]) == 5 + 12
    path = tmp_path / 'h.sdf'
    M.write_sdf(str(path), [m, plain])
    out = path.read_text()
    assert out.count('> <PHOREGEN_HYDROGENS>') == 1 and out.startswith(M.mol_block(m))
    assert '> <PHOREGEN_HYDROGENS>\nstatus 0x20\nhydrogens 5\nsites 2\nsites_tetrahedral 1\nsites_trigonal 1\nsites_linear 0\nsites_generic 0\n' in out
    assert 'contacts 0\nkept_atoms 4\nmin_contact %.4f\n\n$$$$\n' % m['hydrogens']['min_contact'] in out
    with pytest.raises(ValueError, match='mol_block'):
        M.mol_block({**m, 'hydrogens': {**m['hydrogens'], 'h_parent': np.array([0, 0, 0, 3, 9])}})


# ---- the binding and the argument errors -------------------------------------------------------------------------------------------------------
def test_binding_exports_the_entry_point_and_the_header_documents_it():
    header = header_text()
    assert 'pg_mol_hydrogens' in hip.EXPORTS and hip.ABI_VERSION == 11
    res, args = hip._PROTOS['pg_mol_hydrogens']
    proto = re.search(r'int pg_mol_hydrogens\((.*?)\);', header, re.S).group(1)
    assert len(args) == len(proto.split(',')) == 25
    doc = header[header.index('3D positions for the hydrogens'):header.index('int pg_mol_hydrogens(')]
    for word in ('DESIGN.md 2.9 "Hydrogens"', 'h_pos', 'h_placed', 'site_shape', 'min_contact', 'counts', 'status', 'error before anything is launched',
                 'Every element of every output is written', 'do not depend on its batch'):
        assert word in doc, word
    lib = hip.load_library()
    assert lib.pg_abi_version() == 11 and lib.pg_mol_hydrogens.argtypes == args
    makefile = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert ' mol_hydrogens.hip' in makefile and '$(OUT)/mol_hydrogens.o: mol_common.h hydrogen_core.h' in makefile


def test_argument_errors_without_a_device():
    node, pos, edge, sizes = H.batch_from(H.example_graphs()[:2])
    res = mol_result(node, pos, edge, sizes, dev='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HY.hydrogens(res)
    with pytest.raises(ValueError, match="frames must be 'final' or 'traj'"):
        HY.hydrogens(res, frames='all')
    with pytest.raises(ValueError, match='hydrogens='):
        M.sample_valid(None, None, 1, hydrogens='yes')
    with pytest.raises(ValueError, match='hydrogens='):
        M.sample_valid(None, None, 1, hydrogens=M.StereoLimits())
    with pytest.raises(ValueError, match='hydrogens= must be a Hydrogens'):
        M.assemble(res, hydrogens=HY.HydrogenOptions())
    # the library itself refuses bad sizes and options before it looks at a pointer or a device
    lib = hip.load_library()
    ok = dict(B=1, F=1, n_lig=2, n_bond=2, max_n=2, table=1, clash=1.5, contacts=0)

    def call(**kw):
        a = {**ok, **kw}
        return lib.pg_mol_hydrogens(None, 0, None, None, None, None, None, None, None, None, a['B'], a['F'], a['n_lig'], a['n_bond'], a['max_n'],
                                    a['table'], a['clash'], a['contacts'], None, None, None, None, None, None, None)
    for kw, word in ((dict(max_n=129), 'PG_MOL_MAX_ATOMS'), (dict(n_lig=-1), 'n_lig -1'), (dict(n_bond=3), 'both directions'),
                     (dict(clash=float('nan')), 'clash_min'), (dict(clash=-1.0), 'clash_min'), (dict(clash=float('inf')), 'clash_min'),
                     (dict(contacts=-1), 'max_contacts'), (dict(table=None), 'X-H lengths'), ({}, 'an array is null')):
        assert call(**kw) != 0, kw
        message = lib.pg_last_error().decode()
        assert message.startswith('pg_mol_hydrogens') and word in message, (kw, message)
    assert call(B=0) == 0 and call(F=0) == 0                           # nothing to launch
