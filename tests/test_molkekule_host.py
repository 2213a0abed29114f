"""CPU: the Kekulé form's definition (restated in tests/kekule_reference.py from DESIGN.md 2.9 "Kekulé form") on the named molecules
with hand-written answers, the make-up of the random family, the kernel's matching core compiled for the host under ASan / UBSan
(tools/kekule_host_check.cpp) against the restatement, the mol block and SDF item, the binding and its argument errors.

The kernel itself is held against the restatement in tests/test_gpu_molkekule.py."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import kekule_reference as K
import mol_reference as R
from mol_support import arg_count, build_host_check, header_macro, header_text, mol_dict as _mol
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables_and_constants():
    from phoregen_amd.utils.sample_utils import ATOM_TYPES
    assert ATOM_TYPES == [5, 6, 7, 8, 9, 14, 15, 16, 17, 35, 53]
    assert [M.KEKULE_DBL_NEUTRAL[z] for z in ATOM_TYPES] == [0, 4, 3, 0, 0, 4, 3, 0, 0, 0, 0]
    assert [M.KEKULE_DBL_CHARGED[z] for z in ATOM_TYPES] == [0, 0, 4, 0, 0, 0, 4, 3, 0, 0, 0]
    assert [M.KEKULE_MUST[z] for z in ATOM_TYPES] == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert [M.H_VALENCES[z] for z in ATOM_TYPES] == [(3,), (4,), (3,), (2,), (1,), (4,), (3, 5), (2, 4, 6), (1,), (1,), (1, 3, 5)]
    assert (M.KEKULE_FAILED, M.KEKULE_CHARGED, M.KEKULE_HAS_AROMATIC, M.KEKULE_CATION) == (1, 2, 4, 8) and M.KEKULE_FAIL_MASK == 1
    assert sorted(M.KEKULE_NAMES) == [1, 2, 4, 8]
    assert M.KEKULE_COUNTS == ('aromatic_atoms', 'aromatic_bonds', 'doubled', 'must_atoms', 'may_matched', 'hydrogens', 'charge', 'hbd',
                               'hba', 'heavy_atoms')
    assert M.KekuleOptions().allow_charged is True
    with pytest.raises(Exception):                                     # frozen
        M.KekuleOptions().allow_charged = False
    with pytest.raises(ValueError, match='KekuleOptions'):
        M.KekuleOptions(allow_charged=1)
    with pytest.raises(ValueError, match='KekuleOptions'):
        M.sample_valid(None, None, 1, kekule=(True,))


@pytest.mark.parametrize('name', list(K.NAMED))
def test_named_molecule_by_hand(name):
    classes, bonds, allow, status, doubled, hydrogens, charge, atoms = K.NAMED[name]
    cls, order = K.rows_of(classes, bonds)
    r = K.kekule_of_rows(cls, order, allow)
    c = dict(zip(M.KEKULE_COUNTS, r['counts'].tolist()))
    assert r['status'] == status and r['ok'] == (status & M.KEKULE_FAILED == 0)
    assert (c['doubled'], c['hydrogens'], c['charge']) == (doubled, hydrogens, charge)
    assert {i: (int(r['hcount'][i]), int(r['charge'][i])) for i in atoms} == atoms
    assert c['heavy_atoms'] == len(classes) and c['aromatic_bonds'] == sum(t == 4 for t in bonds.values())
    if r['ok']:
        assert sorted(set(r['kekule_order'].tolist())) in ([0, 1, 2], [1, 2], [2]) and int((r['kekule_order'] == 2).sum()) >= doubled
    else:
        assert np.array_equal(r['kekule_order'], order)
    K.check_assignment(cls, order, r, allow, where=name)               # the restatement's own matching passes its own property check


def test_named_details_by_hand():
    kinds = lambda name, pas: K.classify(K.graph_of_rows(*K.rows_of(*K.NAMED[name][:2])), pas)   # noqa: E731
    assert kinds('2-pyridone', 0) == [K.MAY, K.NOT] + [K.MUST] * 4 + [K.NONE]                   # the C=O carbon cannot take the ring double bond
    assert kinds('pyrrole', 0) == [K.MAY] + [K.MUST] * 4 and kinds('furan', 1) == [K.NOT] + [K.MUST] * 4
    assert kinds('N-methylpyridinium', 0)[0] == K.NOT and kinds('N-methylpyridinium', 1)[0] == K.MAY
    assert kinds('thiopyrylium', 0)[0] == K.NOT and kinds('thiopyrylium', 1)[0] == K.MAY
    sol = lambda name: K.kekule_of_rows(*K.rows_of(*K.NAMED[name][:2]), K.NAMED[name][2])        # noqa: E731
    r = sol('pyridine')
    assert r['solution']['matching'] & {(0, 1), (0, 5)} and dict(zip(M.KEKULE_COUNTS, r['counts']))['may_matched'] == 1
    r = sol('pyrrole')
    assert r['solution']['matching'] == {(1, 2), (3, 4)} and dict(zip(M.KEKULE_COUNTS, r['counts']))['hbd'] == 1
    r = sol('imidazole')
    assert sorted(r['hcount'][[0, 2]].tolist()) == [0, 1]              # one NH, whichever
    r = sol('pyridazine')
    assert r['solution']['size'] == 3                                  # N=N or two C=N: three double bonds either way
    r = sol('indole')
    assert not any(0 in e for e in r['solution']['matching'])
    r = sol('thiopyrylium')
    assert r['solution']['pass'] == 1 and int(r['kekule_order'].max()) == 2
    # a four-valent N is N+ without any aromatic bond; a dropped atom takes its bonds with it; nothing at all
    r = K.kekule_of_rows(*K.rows_of([K.N_] + [K.C_] * 4, {(0, i): 1 for i in range(1, 5)}))
    assert r['status'] == M.KEKULE_CATION and r['charge'].tolist() == [1, 0, 0, 0, 0] and r['hcount'].tolist() == [0, 3, 3, 3, 3]
    r = K.kekule_of_rows(*K.rows_of([K.C_, K.C_, 11, K.C_, K.C_, K.C_], K.cycle(6)))
    assert r['status'] == M.KEKULE_HAS_AROMATIC | M.KEKULE_FAILED and r['counts'].tolist()[:4] == [5, 4, 0, 5]   # a path of five MUST atoms
    assert K.kekule_of_rows(*K.rows_of([], {}))['counts'].tolist() == [0] * 10
    r = K.kekule_of_rows(*K.rows_of([K.S_], {}))
    assert r['counts'].tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0, 1] and r['status'] == 0
    for name, (classes, bonds) in K.BLOSSOM.items():
        r = K.kekule_of_rows(*K.rows_of(classes, bonds))
        assert r['ok'] and 2 * r['solution']['size'] == len(classes), name


def test_formula_and_weight():
    assert M.formula_of([6] * 6, [1] * 6) == ('C6H6', pytest.approx(78.114))
    assert M.formula_of([7, 6, 6, 6, 6, 6, 6], [0, 1, 1, 1, 1, 1, 3], 1) == ('C6H8N+', pytest.approx(94.137))
    assert M.formula_of([8, 16, 8, 8, 8], [1, 0, 0, 0, 1])[0] == 'H2O4S' and M.formula_of([17, 6, 35], [0, 2, 0])[0] == 'CH2BrCl'
    assert M.formula_of([7, 7], [0, 0], 2)[0] == 'N22+' and M.formula_of([], [])[0] == ''


def _documented_block(mol, name, types=None, charge=None):
    """The V2000 block as the format documents it, written here independently of mol_block."""
    n = len(mol['element'])
    charge = charge or [0] * n
    types = types if types is not None else mol['bond_type'].tolist()
    out = [name, '  PhoreGen' + ' ' * 10 + '3D', '', '%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (n, len(types))]
    for z, p, q in zip(mol['element'], mol['atom_pos'].tolist(), charge):
        out.append('%10.4f%10.4f%10.4f %-3s%2d%3d' % (p[0], p[1], p[2], M.ELEMENT_SYMBOL[z], 0, {0: 0, 1: 3}[q]) + '  0' * 10)
    for (a, b), t in zip(mol['bond_index'].T.tolist(), types):
        out.append('%3d%3d%3d  0' % (a + 1, b + 1, t))
    ch = [(i + 1, q) for i, q in enumerate(charge) if q]
    for k in range(0, len(ch), 8):
        out.append('M  CHG%3d' % len(ch[k:k + 8]) + ''.join(' %3d %3d' % e for e in ch[k:k + 8]))
    return '\n'.join(out + ['M  END']) + '\n'


def _kek(mol, types, h, q, status=M.KEKULE_HAS_AROMATIC, ok=True):
    formula, weight = M.formula_of(mol['element'], h, sum(q))
    counts = dict(zip(M.KEKULE_COUNTS, [6, 6, 3, 5, 1, sum(h), sum(q), 0, 1, len(h)]))
    counts['net_charge'] = counts.pop('charge')                        # ('charge' is the per-atom array of a molecule's dict)
    return dict(counts, status=status, kekule_ok=ok, bond_type=torch.tensor(types), hcount=np.array(h, dtype=np.uint8),
                charge=np.array(q, dtype=np.int8), formula=formula, mol_weight=weight)


def test_mol_block_and_sdf(tmp_path):
    ring = [(0, 1), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]
    pyr = _mol([7, 6, 6, 6, 6, 6, 6], ring + [(0, 6)], [4] * 6 + [1])
    # without 'kekule', or with a failed one, the block is byte for byte the documented one with type 4 and no charges
    plain = _documented_block(pyr, 'p')
    assert M.mol_block(pyr, 'p') == plain and '  1  2  4  0\n' in plain and 'CHG' not in plain
    assert plain.split('\n')[4] == '   -1.0000   -0.5000    0.0000 N   0  0  0  0  0  0  0  0  0  0  0  0'
    failed = _kek(pyr, [4] * 6 + [1], [1, 2, 2, 2, 2, 2, 3], [0] * 7, M.KEKULE_HAS_AROMATIC | M.KEKULE_FAILED, ok=False)
    assert M.mol_block(dict(pyr, kekule=failed), 'p') == plain
    # the Kekulé block of N-methylpyridinium: types 1 / 2 only, ccc = 3 on the N, one M  CHG line
    types = [2, 1, 1, 2, 1, 2, 1]
    good = _kek(pyr, types, [0, 1, 1, 1, 1, 1, 3], [1, 0, 0, 0, 0, 0, 0], M.KEKULE_HAS_AROMATIC | M.KEKULE_CHARGED | M.KEKULE_CATION)
    block = M.mol_block(dict(pyr, kekule=good), 'p')
    assert block == _documented_block(pyr, 'p', types, [1, 0, 0, 0, 0, 0, 0])
    lines = block.split('\n')
    assert {ln[6:9] for ln in lines[11:18]} == {'  1', '  2'} and lines[4][34:39] == ' 0  3' and all(ln[36:39] == '  0' for ln in lines[5:11])
    assert [ln for ln in lines if ln.startswith('M  ')] == ['M  CHG  1   1   1', 'M  END']
    # nine charged atoms: two M  CHG lines, eight and one
    n9 = _mol([7] * 9 + [6], [(i, 9) for i in range(9)], [1] * 9)
    nine = _kek(n9, [1] * 9, [0] * 10, [1] * 9 + [0], M.KEKULE_CATION)
    chg = [ln for ln in M.mol_block(dict(n9, kekule=nine)).split('\n') if ln.startswith('M  CHG')]
    assert chg == ['M  CHG  8' + ''.join(' %3d   1' % i for i in range(1, 9)), 'M  CHG  1   9   1']
    assert nine['formula'] == 'CN99+'
    with pytest.raises(ValueError, match='kekule'):
        M.mol_block(dict(pyr, kekule=dict(good, bond_type=torch.tensor([1, 2]))))
    # the SDF item, after the other items; a molecule without 'kekule' is written as before
    path = tmp_path / 'k.sdf'
    M.write_sdf(str(path), [dict(pyr, kekule=good, key=0x2A), pyr, dict(pyr, kekule=failed)], names=['a', 'b', 'c'])
    item = ('> <PHOREGEN_KEKULE>\nstatus 0x0e\nformula C6H8N+\nmol_weight 94.137\naromatic_atoms 6\naromatic_bonds 6\ndoubled 3\nmust_atoms 5\n'
            'may_matched 1\nhydrogens 8\ncharge 1\nhbd 0\nhba 1\nheavy_atoms 7\n\n')
    text = path.read_text()
    assert text.startswith(_documented_block(pyr, 'a', types, [1, 0, 0, 0, 0, 0, 0]) + '> <PHOREGEN_KEY>\n000000000000002a\n\n' + item + '$$$$\n'
                           + _documented_block(pyr, 'b') + '$$$$\n' + _documented_block(pyr, 'c') + '> <PHOREGEN_KEKULE>\nstatus 0x05\nformula C6H14N\n')


@pytest.fixture(scope='module')
def family():
    graphs = K.random_family()
    rows = [K.rows_of(c, b) for c, b in graphs]
    return graphs, rows, [K.kekule_of_rows(cls, order) for cls, order in rows]


def test_random_family_make_up(family):
    graphs, rows, want = family
    assert sorted({len(c) for c, _ in graphs}) == sorted(K.FAMILY_SIZES)
    kinds = [K.outcome(w['solution']) for w in want]
    share = {k: kinds.count(k) / len(kinds) for k in ('neutral', 'charged', 'failed')}
    assert min(share.values()) >= 0.15, share
    odd = [K.has_odd_cycle(w['graph']['n'], K.allowed_edges(w['graph'], w['solution']['kinds'])) for w in want]
    assert sum(odd) / len(odd) >= 0.30, sum(odd) / len(odd)
    assert max(int(w['counts'][0]) for w in want) <= K.MAX_AROMATIC
    deg = [max(w['graph']['a'], default=0) for w in want]
    assert max(deg) == 3
    assert any(-1 in cls.tolist() for cls, _ in rows) and any(w['counts'][4] > 0 for w in want) and any(w['status'] & M.KEKULE_CATION for w in want)


def test_hydrogens_minus_charge_is_the_same_for_every_maximum_matching(family):
    """Restated exhaustively on the small aromatic parts: every maximum matching that covers the MUST atoms gives one value."""
    _, _, want = family
    seen = 0
    for w in want:
        g, sol = w['graph'], w['solution']
        edges = K.allowed_edges(g, sol['kinds'])
        if not sol['feasible'] or not 1 <= len(edges) <= 12:
            continue
        values = set()
        for pick in range(1 << len(edges)):
            m = {e for k, e in enumerate(edges) if pick >> k & 1}
            ends = [x for e in m for x in e]
            if len(m) != sol['size'] or len(set(ends)) != len(ends) or any(sol['kinds'][i] == K.MUST and i not in ends for i in range(g['n'])):
                continue
            r = K.results_for(g, sol, m)
            values.add(int(r['hcount'].sum()) - int(r['charge'].sum()))
        assert values == {w['h_minus_q']}, values
        seen += 1
    assert seen >= 20


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')
def test_matching_core_on_the_host_under_sanitizers(family, tmp_path):
    """The text the kernel compiles (csrc/kekule_core.h), built as a stand-alone host program with ASan + UBSan, on the named
    molecules, the blossom cases, the random family (both options) and two thousand further random graphs."""
    graphs, rows, want = family
    exe = build_host_check('kekule_host_check', tmp_path)
    cases = [(*K.rows_of(c, b), allow) for c, b, allow, *_ in K.NAMED.values()] + [(*K.rows_of(c, b), True) for c, b in K.BLOSSOM.values()]
    cases += [(cls, order, True) for cls, order in rows] + [(cls, order, False) for cls, order in rows]
    rng = np.random.default_rng(77)
    cases += [(*K.rows_of(*K.random_graph(rng, int(rng.integers(1, 41)))), bool(rng.random() < 0.8)) for _ in range(2000)]
    got = K.run_host_check(exe, cases, tmp_path)
    assert len(got) == len(cases)
    for k, ((cls, order, allow), r) in enumerate(zip(cases, got)):
        sol = K.check_assignment(cls, order, r, allow, where='case %d' % k)
        ref = K.kekule_of_rows(cls, order, allow)
        assert int(r['hcount'].sum()) - int(r['charge'].sum()) == ref['h_minus_q'], k
        ci = M.KEKULE_COUNTS.index
        assert all(int(r['counts'][ci(c)]) == int(ref['counts'][ci(c)]) for c in K.INDEPENDENT), k
        assert sol['size'] == ref['solution']['size']
    # the ladder of 128 aromatic carbons, and the one with an O that leaves an odd path
    lad = K.rows_of([K.C_] * 128, K.ladder(64))
    broken = K.rows_of([K.C_] * 64 + [K.O_] + [K.C_] * 63, K.ladder(64))
    g_lad, g_broken = K.run_host_check(exe, [(*lad, True), (*broken, True)], tmp_path)
    K.check_assignment(*lad, g_lad, expect=(True, 0, 64), where='ladder')
    K.check_assignment(*broken, g_broken, expect=(False, 1, 0), where='broken ladder')


def test_kekulize_needs_the_device():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    res = {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.kekulize(res)


def test_binding_declares_the_kekule_kernel():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_kekule\s*\(', header)
    assert 'pg_mol_kekule' in hip.EXPORTS and hasattr(lib, 'pg_mol_kekule')
    assert len(hip._PROTOS['pg_mol_kekule'][1]) == 20 == arg_count('pg_mol_kekule')
    assert hip.ABI_VERSION == 11 == lib.pg_abi_version()
    assert 'mol_kekule.hip' in open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    for bit, name in M.KEKULE_NAMES.items():
        assert header_macro('PG_KEKULE_' + name) == str(bit), name
    assert header_macro('PG_KEKULE_N_COUNTS') == str(len(M.KEKULE_COUNTS))
    # argument errors are refused before any launch, without a GPU: oversize, negative sizes, null tables
    tab = hip.C.cast((hip.C.c_uint8 * 44)(), hip.C.c_void_p)

    def args(B, n_lig, n_bond, max_n, F=1, tables=(tab, tab, tab, tab)):
        return (None, None, None, None, B, F, n_lig, n_bond, max_n, *tables, 1, None, None, None, None, None, None)
    assert lib.pg_mol_kekule(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_kekule' in lib.pg_last_error()
    for bad in (args(1, 4, 12, -1), args(-1, 4, 12, 4), args(1, -4, 12, 4), args(1, 4, -12, 4), args(1, 4, 12, 4, F=-1), args(1, 4, 11, 4)):
        assert lib.pg_mol_kekule(*bad) != 0 and b'pg_mol_kekule' in lib.pg_last_error()
    for k in range(4):
        assert lib.pg_mol_kekule(*args(1, 4, 12, 4, tables=tuple(None if j == k else tab for j in range(4)))) != 0
        assert b'pg_mol_kekule' in lib.pg_last_error() and b'null' in lib.pg_last_error()
    assert lib.pg_mol_kekule(*args(0, 0, 0, 0)) == 0 and lib.pg_mol_kekule(*args(3, 4, 12, 4, F=0)) == 0
