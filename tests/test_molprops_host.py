"""CPU: the property descriptors' definition (restated in tests/props_reference.py from DESIGN.md 2.9 "Properties") on the named
molecules with hand-written answers, the saturation of every field, the tables' first-match rule, the limits, the shipped tables'
coverage, csrc/props_core.h compiled for the host under the sanitizers against the restatement, the binding's argument errors, the
option validation, `env_fields`, and the analysis record on CPU arrays.  No device."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import props_reference as PR
from mol_support import C_, CL_, F_, N_, O_, S_, ROOT, arg_count, build_host_check, header_macro, header_text, mol_result, batch_from
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import properties as P

HAND = PR.rows_from_fields(PR.HAND_ROWS)
DEFAULT = [list(t.rows) for t in P.DEFAULT_TABLES]


@pytest.fixture(scope='module')
def family():
    """The named molecules and the random family with their inputs from the CPU restatements; built once, changed by no test."""
    graphs = PR.named_graphs() + PR.random_family()
    return graphs, [PR.cpu_inputs(c, b) for c, b in graphs]


# ---- the definition on the named molecules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(PR.NAMED))
def test_named_molecules_by_hand(name):
    classes, bonds, fields, rows, counts, weight = PR.NAMED[name]
    got = PR.properties_of(classes, bonds, [HAND])
    assert got['atom_env'].tolist() == [PR.pack(f) for f in fields], [PR.unpack(w) for w in got['atom_env'].tolist()]
    assert got['atom_row'][0].tolist() == [255 if r is None else r for r in rows] and (got['atom_row'][1:] == 255).all()
    untyped = sum(r is None for r in rows)
    want = dict(dict.fromkeys(PR.COUNTS, 0), **counts, untyped=untyped)
    assert dict(zip(PR.COUNTS, got['counts'].tolist())) == want
    assert got['weight_milli'] == weight
    hand_sum = sum(PR.HAND_ROWS[r][1] + f.get('h', 0) * PR.HAND_ROWS[r][2] for r, f in zip(rows, fields) if r is not None)
    assert got['sums'].tolist() == [hand_sum, 0, 0, 0]
    assert got['status'] == (PR.UNTYPED if untyped else 0) and got['ok'] and got['violated'] == 0
    # the module's own constants say the same: the weights, the word's layout, the count names
    assert P.weight_table() == PR.WEIGHTS and P.PROPERTY_COUNTS == PR.COUNTS
    assert P.ENV_FIELDS == {k: (first, bits) for k, first, bits in PR.FIELDS}


def test_amide_and_rotatable_bonds():
    count = lambda name, k: dict(zip(PR.COUNTS, PR.properties_of(*PR.NAMED[name][:2])['counts'].tolist()))[k]    # noqa: E731
    assert count('acetamide', 'amide_bonds') == 1 and count('acetamide', 'rotatable') == 0
    assert count('N-methylacetamide', 'amide_bonds') == 1 and count('N-methylacetamide', 'rotatable') == 0
    assert count('butane', 'rotatable') == 1 and count('ethanol', 'rotatable') == 0
    # pentane 2, 2-butyne 0 (a triple bond at an end), cyclohexane 0 (ring bonds), N-propylacetamide: the amide bond apart, N-C and C-C
    c = lambda classes, bonds: dict(zip(PR.COUNTS, PR.properties_of(classes, bonds)['counts'].tolist()))          # noqa: E731
    assert c([C_] * 5, PR.chain(5, 1))['rotatable'] == 2
    assert c([C_] * 4, {(0, 1): 1, (1, 2): 3, (2, 3): 1})['rotatable'] == 0
    assert c([C_] * 5, {(0, 1): 1, (1, 2): 1, (2, 3): 3, (3, 4): 1})['rotatable'] == 0
    assert c([C_] * 6, PR.cycle(6, 1))['rotatable'] == 0
    got = c([C_, C_, O_, N_, C_, C_, C_], {(0, 1): 1, (1, 2): 2, (1, 3): 1, (3, 4): 1, (4, 5): 1, (5, 6): 1})
    assert got['amide_bonds'] == 1 and got['rotatable'] == 2


def _star(centre, leaves, order=1, h=0):
    """Synthetic rows: one atom bonded to all others, as the restatement's inputs (no Kekulé run: the orders are given)."""
    n = len(leaves) + 1
    cls = np.array([centre] + list(leaves), dtype=np.int8)
    pairs = n * (n - 1) // 2
    o = np.zeros(pairs, dtype=np.int8)
    o[:n - 1] = 1
    k = np.zeros(pairs, dtype=np.int8)
    k[:n - 1] = order
    return cls, o, k, np.array([h] + [0] * (n - 1), dtype=np.uint8), np.zeros(n, dtype=np.int8), 0, np.zeros(pairs, dtype=np.uint8), np.zeros(n, dtype=np.uint8)


def test_every_field_saturates():
    word = lambda rows: PR.unpack(int(PR.properties_of_rows(*rows)['atom_env'][0]))            # noqa: E731
    for leaves in (7, 8, 9):
        f = word(_star(C_, [O_] * leaves, h=leaves))
        assert (f['deg'], f['nb_het'], f['nb_no'], f['h'], f['nb_hal']) == (7, 7, 7, 7, 0), leaves
    assert word(_star(C_, [O_] * 6, h=6))['deg'] == 6 and word(_star(C_, [N_] * 6))['nb_no'] == 6
    for leaves in (3, 4, 5):
        f = word(_star(C_, [F_, CL_, F_, CL_, F_][:leaves], order=2))
        assert (f['nb_hal'], f['n_dbl'], f['dbl_o'], f['dbl_het']) == (3, 3, 0, 0), leaves
    assert word(_star(C_, [CL_] * 2, order=2))['n_dbl'] == 2
    # nb_arom: a centre with four neighbours that each have an aromatic ring bond
    n = 13                                                             # atom 0, then four triangles 1-2-3, 4-5-6, .. whose first atom is bonded to 0
    cls = np.full(n, C_, dtype=np.int8)
    a, b = np.triu_indices(n, 1)
    row = {(int(x), int(y)): i for i, (x, y) in enumerate(zip(a, b))}
    o, k, rs = (np.zeros(len(a), dtype=dt) for dt in (np.int8, np.int8, np.uint8))
    for t in range(4):
        x = 1 + 3 * t
        o[row[(0, x)]] = k[row[(0, x)]] = 1
        for e in ((x, x + 1), (x + 1, x + 2), (x, x + 2)):
            o[row[e]], k[row[e]], rs[row[e]] = 4, 1, 3
    got = PR.properties_of_rows(cls, o, k, np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int8), 0, rs, np.array([0] + [3] * 12, dtype=np.uint8))
    f0, f1 = PR.unpack(int(got['atom_env'][0])), PR.unpack(int(got['atom_env'][1]))
    assert (f0['nb_arom'], f0['arom'], f0['deg']) == (3, 0, 4) and (f1['arom'], f1['ring3'], f1['nb_arom']) == (1, 1, 2)
    assert all(0 <= int(w) < 1 << 30 for w in got['atom_env'])
    # an aromatic order on a bond that is no ring bond is neither aromatic nor a single or double bond
    cls, o, k, h, q, st, rs, ar = _star(C_, [O_], order=2)
    o[0] = 4
    f = PR.unpack(int(PR.properties_of_rows(cls, o, k, h, q, st, rs, ar)['atom_env'][0]))
    assert (f['arom'], f['n_dbl'], f['dbl_o'], f['deg']) == (0, 0, 0, 1)


def test_first_match_priority_and_untyped():
    classes, bonds = PR.NAMED['acetic acid'][:2]
    general, special = ({'el': C_}, 10000, 0), ({'el': C_, 'dbl_o': 1}, 70000, 0)
    a = PR.properties_of(classes, bonds, [PR.rows_from_fields([special, general])])
    b = PR.properties_of(classes, bonds, [PR.rows_from_fields([general, special])])
    assert a['sums'][0] == 80000 and b['sums'][0] == 20000 and a['atom_row'][0].tolist() == [1, 0, 255, 255] and b['atom_row'][0].tolist() == [0, 0, 255, 255]
    # the two oxygens have no row: they add 0, are counted once per table and set the informational bit only
    assert a['counts'][PR.COUNTS.index('untyped')] == 2 and a['status'] == PR.UNTYPED and a['ok']
    two = PR.properties_of(classes, bonds, [PR.rows_from_fields([general]), []])
    assert two['counts'][PR.COUNTS.index('untyped')] == 2 + 4 and two['sums'].tolist() == [20000, 0, 0, 0]
    # per_h multiplies the atom's own hydrogens: CH3 and OH
    h = PR.properties_of(classes, bonds, [PR.rows_from_fields([({}, 0, 100)])])
    assert h['sums'][0] == 400 and h['status'] == 0


def test_the_family_meets_its_conditions_and_the_default_tables_type_every_atom(family):
    graphs, inputs = family
    assert len(graphs) - len(PR.NAMED) >= 40 and max(len(c) for c, _ in graphs) <= PR.FAMILY_MAX
    random_part = inputs[len(PR.NAMED):]
    assert sum(not st & PR.KEKULE_FAILED for *_, st, _, _ in random_part) * 2 >= len(random_part)
    seen_set, seen_clear, untyped, n_atoms = 0, 0, 0, 0
    for rows in inputs:
        got = PR.properties_of_rows(*rows, DEFAULT)
        untyped += int(got['counts'][PR.COUNTS.index('untyped')])
        assert not got['status'] & PR.UNTYPED
        for w in got['atom_env'].tolist():
            if w >= 0:
                seen_set, seen_clear, n_atoms = seen_set | w, seen_clear | ~w, n_atoms + 1
    assert untyped == 0 and n_atoms > 500
    every = (1 << 30) - 1
    assert seen_set == every and seen_clear & every == every, (bin(seen_set), bin(seen_clear & every))
    # LOGP and MR end with one catch-all row per element, TPSA with one for every atom
    for t in (P.LOGP, P.MR):
        assert sorted(v for m, v, _, _ in t.rows[-11:]) == list(range(11)) and all(m == 15 for m, _, _, _ in t.rows[-11:])
    assert P.TPSA.rows[-1][:2] == (0, 0) and P.TPSA_SP.rows[-1][:2] == (0, 0)
    assert not any(PR.unpack(v)['el'] in (PR.S_, PR.P_) and m for m, v, _, _ in P.TPSA.rows)
    assert [t.name for t in P.DEFAULT_TABLES] == ['tpsa', 'logp', 'mr'] and P.TPSA_SP.name == 'tpsa_sp'


def test_shipped_values_on_simple_molecules():
    """Sums that follow from the tables by hand: ethanol's TPSA is the hydroxyl's 20.23, benzene's logP six aromatic CH."""
    eth = PR.properties_of(*PR.NAMED['ethanol'][:2], DEFAULT)
    assert eth['sums'][0] == 202300
    assert eth['sums'][1] == (1441 + 3 * 1230) + (-2035 + 2 * 1230) + (-2893 - 2677)
    ben = PR.properties_of(*PR.NAMED['benzene'][:2], DEFAULT)
    assert ben['sums'].tolist() == [0, 6 * (1581 + 1230), 6 * (33500 + 10570), 0]
    nma = PR.properties_of(*PR.NAMED['N-methylacetamide'][:2], DEFAULT)
    assert nma['sums'][0] == 170700 + 120300


# ---- limits ---------------------------------------------------------------------------------------------------------------------------
def _pairs(limits, tables=P.DEFAULT_TABLES):
    return limits.pairs(tables)


def test_each_limit_alone_and_both_sides():
    classes, bonds = PR.NAMED['N-methylacetamide'][:2]                 # weight 73.095, 5 heavy atoms, nhoh 1, no_count 2, rotatable 0
    base = PR.properties_of(classes, bonds, DEFAULT)
    values = dict(mol_weight=73.095, heavy_atoms=5, nhoh=1, no_count=2, rotatable=0)
    for bit, (k, v) in enumerate(values.items()):
        step = 0.001 if k == 'mol_weight' else 1
        for pair, hit in (((None, v), False), ((v, None), False), ((v, v), False), ((None, v - step), True), ((v + step, None), True)):
            lim = P.PropertyLimits(**{k: pair})
            got = PR.properties_of(classes, bonds, DEFAULT, _pairs(lim), lim.max_violations)
            assert got['violated'] == (1 << bit if hit else 0), (k, pair)
            assert got['status'] == (PR.LIMITS if hit else 0) and got['ok'] == (not hit)
            assert got['counts'][PR.COUNTS.index('violations')] == int(hit)
    for t, name in enumerate(('tpsa', 'logp', 'mr')):
        v = int(base['sums'][t]) / 1e4
        for pair, hit in (((None, v), False), ((v, None), False), ((None, v - 1e-4), True), ((v + 1e-4, None), True)):
            lim = P.PropertyLimits(sums={name: pair})
            assert PR.properties_of(classes, bonds, DEFAULT, _pairs(lim))['violated'] == (1 << (5 + t) if hit else 0), (name, pair)
    # max_violations: two violated quantities pass with 2, fail with 0 and 1; the bits are the same
    for allowed, ok in ((0, False), (1, False), (2, True)):
        lim = P.PropertyLimits(heavy_atoms=(6, None), no_count=(None, 1), max_violations=allowed)
        got = PR.properties_of(classes, bonds, DEFAULT, _pairs(lim), allowed)
        assert got['violated'] == 0b1010 and got['ok'] == ok and got['counts'][PR.COUNTS.index('violations')] == 2


def test_presets():
    lip, veb = P.PropertyLimits.lipinski(), P.PropertyLimits.veber()
    none, top = PR.INT_MIN, PR.INT_MAX
    assert _pairs(lip) == [(none, 500000), (none, top), (none, 5), (none, 10), (none, top), (none, top), (none, 50000), (none, top), (none, top)]
    assert lip.max_violations == 1
    assert _pairs(veb) == [(none, top)] * 4 + [(none, 10), (none, 1400000)] + [(none, top)] * 3 and veb.max_violations == 0
    assert _pairs(P.PropertyLimits()) == PR.NO_LIMITS and P.PropertyLimits().max_violations == 0
    # a long alkyl chain with twelve hydroxyls: nhoh 12 and no_count 12 are two violations of Lipinski's four, eleven rotatable bonds one of Veber's
    n = 13
    classes = [C_] * n + [O_] * 12
    bonds = {**PR.chain(n, 1), **{(i, n + i): 1 for i in range(12)}}
    got = PR.properties_of(classes, bonds, DEFAULT, _pairs(lip), lip.max_violations)
    assert got['violated'] == 0b1100 and not got['ok'] and got['status'] == PR.LIMITS
    got = PR.properties_of(classes, bonds, DEFAULT, _pairs(veb), veb.max_violations)
    assert got['counts'][PR.COUNTS.index('rotatable')] == 11 and got['violated'] == 0b10000 | 1 << 5 and not got['ok']
    assert PR.properties_of(*PR.NAMED['phenol'][:2], DEFAULT, _pairs(lip), 1)['ok']


def test_options_are_validated():
    for kw in (dict(mol_weight=500), dict(nhoh=(1, 2, 3)), dict(rotatable=(3, 1)), dict(heavy_atoms=(None, float('nan'))), dict(no_count=(True, None)),
               dict(sums=[('logp', (None, 5))]), dict(sums={'logp': 5}), dict(max_violations=-1), dict(max_violations=1.0), dict(mol_weight=(None, 1e9))):
        with pytest.raises(ValueError, match='PropertyLimits'):
            P.PropertyLimits(**kw)
    with pytest.raises(ValueError, match="names the table 'logp'"):
        P.PropertyLimits.lipinski().pairs((P.TPSA,))
    assert P.PropertyLimits(mol_weight=(0.0004, 0.0006)).pairs(())[0] == (0, 1)       # (converted once, with round)
    for rows, word in (([(0, 0, 1 << 20, 0)], 'atom'), ([(0, 0, 0, -(1 << 20))], 'per_h'), ([(0, 0, 0)], 'must be'), ([(0.5, 0, 0, 0)], 'mask'),
                       ([(0, 0, 0, 0)] * 129, 'MAX_ROWS = 128')):
        with pytest.raises(ValueError, match=word):
            P.PropertyTable('x', rows)
    for name in ('', 'two words', 'rotatable', 'mol_weight', 'status', 5):
        with pytest.raises(ValueError, match='PropertyTable'):
            P.PropertyTable(name, [])
    assert P.PropertyTable('x', [(0, 0, (1 << 20) - 1, 1 - (1 << 20))] * 128).rows[127] == (0, 0, 1048575, -1048575)
    assert P.table_row(1.23456, -0.5, el=C_, h=7) == (0x7f, 0x71, 12346, -5000) and P.table_row(0.0) == (0, 0, 0, 0)
    for kw in (dict(el=16), dict(h=-1), dict(charge=1), dict(q=2)):
        with pytest.raises(ValueError, match='table_row'):
            P.table_row(0.0, **kw)
    with pytest.raises(ValueError, match='at most MAX_TABLES = 4'):
        P._check_tables('who', [P.PropertyTable('t%d' % i) for i in range(5)])
    with pytest.raises(ValueError, match='share a name'):
        P._check_tables('who', [P.TPSA, P.TPSA])
    with pytest.raises(ValueError, match='sequence of PropertyTable'):
        P._check_tables('who', [P.TPSA.rows])
    assert (P.PROP_NO_KEKULE, P.PROP_LIMITS, P.PROP_UNTYPED, P.PROP_FAIL_MASK) == (1, 2, 4, 3)
    assert P.status_names(5) == ('NO_KEKULE', 'UNTYPED') and P.violation_names(0b100101, P.DEFAULT_TABLES) == ('mol_weight', 'nhoh', 'tpsa')
    # sample_valid's reader
    assert P._read(False) is None and P._read(True) == (P.DEFAULT_TABLES, P.PropertyLimits())
    assert P._read(P.PropertyLimits.veber()) == (P.DEFAULT_TABLES, P.PropertyLimits.veber())
    assert P._read(([P.LOGP], P.PropertyLimits())) == ((P.LOGP,), P.PropertyLimits())
    for bad in (1, 'lipinski', (P.DEFAULT_TABLES,), ((P.TPSA,), P.PropertyLimits.lipinski())):
        with pytest.raises(ValueError):
            P._read(bad)


def test_env_fields():
    f = P.env_fields(PR.pack(dict(el=N_, h=2, q=1, deg=3, arom=1, n_dbl=2, triple=1, ring=1, ring3=1, nb_het=5, nb_arom=3, dbl_o=1, dbl_het=1,
                                  nb_dbl_het=1, nb_hal=2, nb_no=6)))
    assert f == dict(el=N_, h=2, q=1, deg=3, arom=1, n_dbl=2, triple=1, ring=1, ring3=1, nb_het=5, nb_arom=3, dbl_o=1, dbl_het=1, nb_dbl_het=1,
                     nb_hal=2, nb_no=6) and list(f) == [k for k, _, _ in PR.FIELDS]
    assert P.env_fields(-1) is None and P.env_fields(np.int32(-1)) is None and P.env_fields(0) == dict.fromkeys(f, 0)
    assert P.env_fields(PR.pack(PR.NAMED['phenol'][2][6])) == dict(dict.fromkeys(f, 0), el=O_, h=1, deg=1, nb_arom=1)


# ---- props_core.h on the host, under the sanitizers --------------------------------------------------------------------------------------
def test_host_compiled_rules_against_the_restatement(family, tmp_path):
    graphs, inputs = family
    exe = build_host_check('props_host_check', tmp_path)
    lip, veb = P.PropertyLimits.lipinski(), P.PropertyLimits(rotatable=(1, 3), heavy_atoms=(4, 30), sums={'tpsa': (10.0, 140.0)})
    last = [(1 << 30, 1 << 30, 1, 1)] * 127 + [(0, 0, 70, 3)]          # 128 rows, the last one the only match
    cases = []
    for rows in inputs:
        cases.append((rows, DEFAULT, _pairs(lip), 1))
        cases.append((rows, [HAND, [], last, DEFAULT[1]], _pairs(veb, (P.TPSA, P.PropertyTable('b'), P.PropertyTable('c'), P.LOGP)), 0))
    failed = list(inputs[5])
    failed[5] = PR.KEKULE_FAILED
    cases += [(tuple(failed), DEFAULT, _pairs(lip), 1), (inputs[0], [], PR.NO_LIMITS, 0)]
    cases += [(_star(C_, [O_] * 9, h=9), DEFAULT, PR.NO_LIMITS, 0), (_star(S_, [CL_] * 5, order=2), [HAND], PR.NO_LIMITS, 0)]
    got = PR.run_host_check(exe, cases, tmp_path)
    assert len(got) == 3 * len(cases) + 1 and got[-1] == ''
    for i, (rows, tables, pairs, allowed) in enumerate(cases):
        want = PR.properties_of_rows(*rows, tables, pairs, allowed)
        assert got[3 * i:3 * i + 3] == PR.expected_lines(want, len(tables)), (i, len(rows[0]))
    assert got[3 * (len(cases) - 4)].split()[0] == '1'                   # the graph without a Kekulé structure


# ---- the binding and the argument errors ---------------------------------------------------------------------------------------------------
def test_binding_exports_the_entry_point_and_the_header_documents_it():
    header = header_text()
    assert 'pg_mol_props' in hip.EXPORTS and hip.ABI_VERSION == 11
    res, args = hip._PROTOS['pg_mol_props']
    assert len(args) == arg_count('pg_mol_props') == 29
    doc = header[header.index('Property descriptors and drug-likeness limits'):header.index('int pg_mol_props(')]
    for word in ('DESIGN.md 2.9 "Properties"', 'atom_env', 'atom_row', 'weight_milli', 'violated', 'first row', 'error before anything is launched',
                 'Every element of every output is written', 'do not depend on its batch'):
        assert word in doc, word
    for name in dir(hip):
        if name.startswith('PG_PROP_'):
            assert int(header_macro(name)) == getattr(hip, name), name
    for k, first, bits in PR.FIELDS:
        assert int(header_macro('PG_PROP_ENV_' + k.upper())) == first
    for i, k in enumerate(PR.COUNTS[:-1]):
        assert int(header_macro('PG_PROP_C_' + k.upper())) == i
    assert int(header_macro('PG_PROP_N_COUNTS')) == len(PR.COUNTS) and (P.MAX_ROWS, P.MAX_TABLES) == (128, 4)
    for i, k in enumerate(P.LIMITED):
        assert int(header_macro('PG_PROP_L_' + ('WEIGHT' if k == 'mol_weight' else k.upper()))) == i
    lib = hip.load_library()
    assert lib.pg_mol_props.argtypes == args
    makefile = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert ' mol_props.hip' in makefile and '$(OUT)/mol_props.o: mol_common.h props_core.h' in makefile
    kernel = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'mol_props.hip')).read()
    assert all(w in kernel for w in ('mol_frame(', 'for_each_pair(', 'MolAdjRow', '#include "mol_common.h"', '#include "props_core.h"'))


def test_argument_errors_without_a_device():
    node, pos, edge, sizes = batch_from(PR.named_graphs()[:2])
    res = mol_result(node, pos, edge, sizes, dev='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.properties(res)
    lib = hip.load_library()
    ok = dict(B=1, F=1, n_lig=2, n_bond=2, max_n=2, rows=[3, 0], max_violations=0)
    lim = (ctypes.c_int * 18)(*[x for p in PR.NO_LIMITS for x in p])

    def call(limits=lim, **kw):
        a = {**ok, **kw}
        rows = (ctypes.c_int * max(len(a['rows']), 1))(*a['rows'])
        return lib.pg_mol_props(*([None] * 10), a['B'], a['F'], a['n_lig'], a['n_bond'], a['max_n'], None, rows, len(a['rows']), None, limits,
                                a['max_violations'], *([None] * 8))
    for kw, word in ((dict(max_n=129), 'PG_MOL_MAX_ATOMS'), (dict(n_lig=-1), 'n_lig -1'), (dict(n_bond=3), 'both directions'),
                     (dict(rows=[1] * 5), '5 tables'), (dict(rows=[0, 129]), 'table 1 has 129 rows'), (dict(rows=[-1]), 'table 0 has -1 rows'),
                     (dict(max_violations=-1), 'max_violations -1'), (dict(limits=None), 'limits null'), (dict(), 'an array is null')):
        assert call(**kw) != 0, kw
        message = lib.pg_last_error().decode()
        assert message.startswith('pg_mol_props') and word in message, (kw, message)
    assert call(B=0) == 0 and call(F=0) == 0 and call(B=0, rows=[]) == 0   # nothing to launch


# ---- the analysis record on CPU arrays ------------------------------------------------------------------------------------------------------
def test_analysis_parts_entry_and_sdf(tmp_path):
    names = ['N-methylacetamide', 'benzene', 'acetic acid']
    graphs = [PR.NAMED[k][:2] for k in names]
    graphs[1] = (graphs[1][0] + [11], graphs[1][1])                      # benzene with a dropped seventh atom
    sizes = [len(c) for c, _ in graphs]
    lim = P.PropertyLimits(heavy_atoms=(None, 5), nhoh=(1, None))
    tables = (P.TPSA, P.LOGP, P.PropertyTable('hand', HAND))
    inputs = [PR.cpu_inputs(c, b) for c, b in graphs]
    wants = [PR.properties_of_rows(*rows, [list(t.rows) for t in tables], lim.pairs(tables), 0) for rows in inputs]
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.atleast_1d(w[k]) for w in wants]).astype(dt))[None]    # noqa: E731
    na = torch.tensor(sizes)
    off = lambda v: torch.cat([torch.zeros(1, dtype=torch.long), v.cumsum(0)]).int()                           # noqa: E731
    cls = torch.from_numpy(np.concatenate([r[0] for r in inputs]))[None]
    order = torch.from_numpy(np.concatenate([r[1] for r in inputs]))[None]
    compact = torch.from_numpy(np.concatenate([np.where(r[0] >= 0, np.cumsum(r[0] >= 0) - 1, -1) for r in inputs]).astype(np.int16))[None]
    N = sum(sizes)
    sc = M.Screen(status=torch.zeros(1, 3, dtype=torch.int32), counts=torch.zeros(1, 3, 4, dtype=torch.int32), valid=torch.ones(1, 3, dtype=torch.bool),
                  cls=cls, compact=compact, valence2=torch.zeros(1, N, dtype=torch.uint8), comp=torch.zeros(1, N, dtype=torch.int16), order=order,
                  lig_off=off(na), bond_off=off(na * (na - 1)), num_atoms=sizes)
    status = cat('status', np.int32)
    pr = P.Properties(status=status, counts=torch.from_numpy(np.stack([w['counts'] for w in wants]))[None], ok=(status & P.PROP_FAIL_MASK) == 0,
                      atom_env=cat('atom_env', np.int32), atom_row=torch.from_numpy(np.concatenate([w['atom_row'] for w in wants], axis=1))[None],
                      sums=torch.from_numpy(np.stack([w['sums'] for w in wants]))[None], weight_milli=cat('weight_milli', np.int32),
                      violated=cat('violated', np.int32), tables=tables, limits=lim, screen=sc, kekule=None, rings=None)
    assert pr.mol_weight.dtype == torch.float64 and pr.mol_weight[0].tolist() == [73.095, 78.114, 60.052]
    assert pr.value('tpsa')[0].tolist() == [29.1, 0.0, 37.3] and pr.value('hand').dtype == torch.float64
    assert pr.fsp3[0].tolist() == [2 / 3, 0.0, 0.5]
    with pytest.raises(ValueError, match="no table 'mr'"):
        pr.value('mr')
    rec = P.ANALYSIS
    assert (rec.keyword, rec.key, rec.holder, rec.also) == ('properties', 'properties', P.Properties, ())
    assert [(name, tuple(t.shape), dt) for name, t, dt in rec.parts(pr)] == [
        ('d_status', (3,), np.int32), ('d_counts', (3, 16), np.int32), ('d_sums', (3, 4), np.int32), ('d_weight', (3,), np.int32),
        ('d_violated', (3,), np.int32), ('d_env', (N,), np.int32), ('d_row', (4, N), np.uint8)]
    assert [a.keyword for a in M._carried(lambda a: True)][-1] == 'properties' and M._carried(lambda a: a.keyword == 'properties') == [rec]
    res = {'pred': [torch.zeros(N, 12), torch.arange(3 * N, dtype=torch.float32).reshape(N, 3), torch.zeros(2 * order.size(1), 6)]}
    mols = M.assemble(res, properties=pr)
    for m, w, (classes, _) in zip(mols, wants, graphs):
        q = m['properties']
        keep = np.array(classes) <= 10
        assert list(q)[:2] == ['status', 'properties_ok'] and list(q)[2:17] == list(PR.COUNTS[:-1])
        assert list(q)[17:] == ['mol_weight', 'tpsa', 'logp', 'hand', 'fsp3', 'violated', 'violated_names', 'env', 'row']
        assert q['status'] == w['status'] and q['properties_ok'] == w['ok'] and q['violated'] == w['violated']
        assert [q[k] for k in PR.COUNTS[:-1]] == w['counts'][:-1].tolist()
        assert q['mol_weight'] == w['weight_milli'] / 1000 and [q['tpsa'], q['logp'], q['hand']] == [s / 1e4 for s in w['sums'][:3].tolist()]
        assert q['env'].dtype == np.int32 and q['env'].tolist() == w['atom_env'][keep].tolist() and len(q['env']) == len(m['element'])
        assert q['row'].dtype == np.uint8 and q['row'].tolist() == w['atom_row'][:3].T[keep].tolist()
    assert [m['properties']['violated_names'] for m in mols] == [(), ('heavy_atoms', 'nhoh'), ()]
    assert [m['properties']['properties_ok'] for m in mols] == [True, False, True] and mols[0]['properties']['fsp3'] == 2 / 3
    assert [rec.verdict(m) for m in mols] == [True, False, True]
    text = rec.sdf(mols[1])
    assert text == P.sdf_item(mols[1]['properties']) and text.startswith('> <PHOREGEN_PROPERTIES>\nstatus 0x02\nmol_weight 78.114\ntpsa 0.0000\n')
    assert text.endswith('violations 2\nviolated heavy_atoms nhoh\n\n') and 'fsp3 0.0000\nheavy_atoms 6\nhydrogens 6\n' in text
    assert rec.sdf(mols[0]).endswith('violated -\n\n')
    path = tmp_path / 'p.sdf'
    M.write_sdf(str(path), mols)
    tags = [ln for ln in path.read_text().split('\n') if ln.startswith('> <')]
    assert tags == ['> <PHOREGEN_PROPERTIES>'] * 3
    bare = tmp_path / 'bare.sdf'
    M.write_sdf(str(bare), [{k: v for k, v in m.items() if k != 'properties'} for m in mols])
    assert 'PHOREGEN_PROPERTIES' not in bare.read_text()
    # sample_valid's keyword reaches the record's reader before anything is sampled
    with pytest.raises(ValueError, match='properties= must be True, a PropertyLimits'):
        M.sample_valid(SimpleNamespace(), None, 1, properties='lipinski')
