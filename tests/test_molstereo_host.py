"""CPU: the stereo perception's and the isomeric SMILES' definition (restated in tests/stereo_reference.py from DESIGN.md 2.9 "Stereo")
on the hand examples and the generated family, the kernels' cores compiled for the host under ASan / UBSan
(tools/stereo_host_check.cpp) against the restatement with `==`, every text read back by the independent reader and held against the
coordinates in float64, the functions that carry the labels, the binding and its argument errors.

The kernels themselves are held against the restatement in tests/test_gpu_molstereo.py."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import mol_reference as R
import mol_support as MS
import smiles_reference as S
import stereo_reference as T
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return MS.build_host_check('stereo_host_check', tmp_path_factory.mktemp('stereo_host'))


@pytest.fixture(scope='module')
def family():
    """The generated family: built once, read by several tests, changed by none."""
    return T.family()


def _restated(rows, limits=None):
    st = T.restate(rows, limits)
    return st, T.smiles_of_rows(*rows.smiles_inputs(), st['atom_parity'], st['bond_stereo'])


def test_constants_and_limits():
    assert (M.STEREO_NO_KEKULE, M.STEREO_UNDEFINED, M.STEREO_HAS_CENTRE, M.STEREO_HAS_BOND, M.STEREO_NONFINITE) == (1, 2, 4, 8, 16)
    assert M.STEREO_FAIL_MASK == 19 and sorted(M.STEREO_NAMES) == [1, 2, 4, 8, 16] and len(M.STEREO_COUNTS) == 8
    assert M.SMILES_STEREO_DROPPED == 64 and M.SMILES_STEREO_DROPPED & M.SMILES_FAIL_MASK == 0 and len(M.SMILES_STEREO_COUNTS) == 4
    assert (M.STEREO_KEY_A, M.STEREO_KEY_B) == (0x243F6A8885A308D3, 0x13198A2E03707344)
    assert (M.STEREO_KEY_C, M.STEREO_KEY_D) == (0xA4093822299F31D0, 0x082EFA98EC4E6C89)
    lim = M.StereoLimits()
    assert (lim.vol_min, lim.planar_min, lim.max_undefined) == (0.5, 0.25, 2 ** 31 - 1)
    for bad in (dict(vol_min=0.0), dict(vol_min=float('nan')), dict(planar_min=-0.1), dict(planar_min=float('inf')), dict(max_undefined=-1),
                dict(max_undefined=1.5), dict(vol_min=True)):
        with pytest.raises(ValueError, match='StereoLimits'):
            M.StereoLimits(**bad)
    with pytest.raises(ValueError, match='stereo='):
        M.sample_valid(None, None, 1, stereo=M.KekuleOptions())
    # an ideal tetrahedron and an ideal sp2 bond, the values the thresholds are a sixth and a third of
    tet = np.array([[0, 0, 0], [1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
    assert abs(abs(T.centre_volume(tet, 0, [1, 2, 3, 4])) - 16 / (3 * 3 ** 0.5)) < 1e-12
    assert abs(T.centre_volume(tet, 0, [1, 2, 3]) - T.centre_volume(tet, 0, [1, 2, 3, 4])) < 1e-12   # the hydrogen opposite the other three
    assert T.centre_volume(tet, 0, [1, 2, 3, 4]) == -T.centre_volume(tet, 0, [2, 1, 3, 4])
    c, b, p, _ = T.EXAMPLES['cis-1,2-difluoroethene skeleton']
    assert abs(T.bond_planarity(np.array(p), 1, 2, 0, 3) - 0.75) < 2e-3
    assert T.perm_sign([3, 1, 2]) == 1 and T.perm_sign([2, 1, 3]) == -1 and T.perm_sign([4, 3, 2, 1]) == 1


def test_census_of_the_family_before_any_kernel(family):
    assert [len(c) for c, _, _ in family[:11]] == [1, 2, 4, 5, 9, 10, 63, 64, 65, 127, 128]
    c, at, around = T.census(family)
    for k in ('centres+', 'centres-', 'centres_undefined', 'centres_h', 'cis', 'trans', 'bonds_undefined'):
        assert c[k] >= 10, (k, c)
    assert c['no_kekule'] == 2 and set(T.CENTRE_AT) <= at and around, (c, sorted(at))
    lim = M.StereoLimits()
    for classes, bonds, pos in family:                                 # no value within MARGIN of its threshold
        r = T.stereo_of(classes, bonds, pos)
        assert all(abs(abs(v) - lim.vol_min) > T.MARGIN for v in r['volumes'].values())
        assert all(abs(abs(t) - lim.planar_min) > T.MARGIN for t in r['planarities'].values())


@pytest.mark.parametrize('name', list(T.EXAMPLES))
def test_example_by_hand(name):
    classes, bonds, pos, text = T.EXAMPLES[name]
    rows = T.all_rows(classes, bonds, pos)
    st, tx = _restated(rows)
    _, _, at = T.graph_of_rows(rows.cls, rows.order)
    assert tx['text'] == text and tx['ok'] and st['ok']
    n_centres, n_read, n_extra = T.check_text_against_geometry(text, tx['atom_rank'], rows.pos, st, at, where=name)
    assert (n_centres, n_read, n_extra) == (text.count('[') if '@' in text else 0, st['counts'][6], 0)
    assert tx['stereo_counts'].tolist() == [n_centres, text.count('@@'), text.count('/') + text.count('\\'), n_read]
    # without its stereo the text is the plain writer's, and reads back to the molecule
    plain = S.smiles_of_rows(*rows.smiles_inputs(), capacity=12 * 8)
    zero = T.smiles_of_rows(*rows.smiles_inputs(), np.zeros_like(st['atom_parity']), np.zeros_like(st['bond_stereo']))
    S.same_answer(zero, plain, where=name)
    if '@' not in text:
        assert T.plain_text(text) == plain['text']
    # the mirror image: every atom label flips, the bond labels stay
    ms, mt = _restated(T.all_rows(classes, bonds, T.mirrored(pos)))
    assert ms['atom_label'].tolist() == [-x if abs(x) == 1 else x for x in st['atom_label'].tolist()]
    assert ms['bond_label'].tolist() == st['bond_label'].tolist() and ms['bond_stereo'].tolist() == st['bond_stereo'].tolist()
    assert (ms['stereo_key'] == st['stereo_key']) == (sorted(ms['atom_label'].tolist()) == sorted(st['atom_label'].tolist()))


def test_example_details_by_hand():
    by = {name: _restated(T.all_rows(c, b, p))[0] for name, (c, b, p, _) in T.EXAMPLES.items()}
    key = {name: T.all_rows(c, b, p).key for name, (c, b, p, _) in T.EXAMPLES.items()}
    for name in ('ring double bond', 'allene'):                        # nothing stereogenic: the key is the identity key
        assert not by[name]['counts'][[1, 5]].any() and by[name]['stereo_key'] == key[name] and by[name]['status'] == 0
    assert by['ring double bond']['counts'].tolist() == [0] * 8 and by['allene']['counts'].tolist() == [0] * 8
    assert by['conjugated triene']['counts'].tolist() == [0, 0, 0, 0, 3, 3, 3, 0] and by['conjugated triene']['status'] == M.STEREO_HAS_BOND
    assert by['quaternary N+']['counts'].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and by['quaternary N+']['status'] == M.STEREO_HAS_CENTRE
    # the oxime: trans by its lowest-index substituents; the carbon's largest substituent is its hydrogen, so the label is the opposite
    ox = by['oxime']
    assert ox['bond_stereo'][ox['bond_stereo'] != 0].tolist() == [-1] and ox['bond_label'][ox['bond_label'] != 0].tolist() == [1]
    # the two difluoroethenes differ in the key and from the identity key; meso and chiral tartaric too
    cis, trans = by['cis-1,2-difluoroethene skeleton'], by['trans-1,2-difluoroethene skeleton']
    assert len({cis['stereo_key'], trans['stereo_key'], key['cis-1,2-difluoroethene skeleton']}) == 3
    meso, chiral = by['meso-tartaric skeleton'], by['chiral tartaric skeleton']
    assert key['meso-tartaric skeleton'] == key['chiral tartaric skeleton'] and meso['stereo_key'] != chiral['stereo_key']
    assert sorted(meso['atom_label'][[3, 5]].tolist()) == [-1, 1] and abs(int(chiral['atom_label'][[3, 5]].sum())) == 2
    # thresholds: a planar centre and a perpendicular double bond are undefined, and counted against max_undefined
    c, b, p, _ = T.EXAMPLES['CHFClBr skeleton']
    flat = [[0, 0, 0], [1, 0, 0], [-0.5, 0.9, 0], [-0.5, -0.9, 0.01]]
    r = T.stereo_of(c, b, flat)
    assert r['atom_parity'].tolist() == [2, 0, 0, 0] == r['atom_label'].tolist() and r['status'] == 0 and r['stereo_key'] == T.all_rows(c, b, flat).key
    assert T.stereo_of(c, b, flat, M.StereoLimits(max_undefined=0))['status'] == M.STEREO_UNDEFINED
    assert T.stereo_of(c, b, flat, M.StereoLimits(vol_min=0.01))['atom_parity'][0] in (1, -1)
    # a neighbour that lies on the centre has no direction: undefined
    assert T.stereo_of(c, b, [p[0], p[0], p[2], p[3]])['atom_parity'][0] == 2
    c, b, p, _ = T.EXAMPLES['cis-1,2-difluoroethene skeleton']
    twisted = [p[0], p[1], p[2], [2.0, 0.1, 1.16]]
    r = T.stereo_of(c, b, twisted)
    assert r['counts'].tolist() == [0, 0, 0, 0, 1, 1, 0, 1] and r['bond_stereo'][r['bond_stereo'] != 0].tolist() == [2]
    assert T.stereo_of(c, b, twisted, M.StereoLimits(planar_min=0.001))['counts'].tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    nan = [p[0], p[1], p[2], [float('nan'), 0.0, 0.0]]
    r = T.stereo_of(c, b, nan)
    assert r['status'] == M.STEREO_NONFINITE and r['counts'][7] == 1 and not r['ok']


def test_reader_on_its_own():
    """What the reader accepts and derives, by the OpenSMILES text alone."""
    atoms, bonds, centres, sides = T.read_isomeric('N[C@@H](C)C(=O)O')
    assert atoms[1] == (6, 1, 0) and centres == {1: ('@@', [0, 'H', 2, 3])} and bonds[(3, 4)] == 2 and not sides
    assert T.read_isomeric('[C@]1(F)(Cl)CCO1')[2] == {0: ('@', [5, 1, 2, 3])}       # the digit stands before the branches
    assert T.read_isomeric('F[C@](Cl)(Br)I')[2] == {1: ('@', [0, 2, 3, 4])}
    _, _, _, sides = T.read_isomeric('F/C=C/F')
    assert sides == {(0, 1): 1, (1, 0): -1, (2, 3): 1, (3, 2): -1}     # F below the first carbon, F above the second: trans
    _, _, _, sides = T.read_isomeric('C/1=C/CCCC1')
    assert sides[(0, 5)] == 1 and sides[(5, 0)] == -1 and sides[(1, 2)] == 1
    assert T.read_isomeric('C1=C/CCCC/1')[3][(5, 0)] == 1               # at the closing digit the symbol reads from the closer
    for bad in ('F/C=C/', 'C/1=CCCCC/1', '[C@H2](F)Cl', 'C//C', '[C@@', 'F/C(/Cl'):
        with pytest.raises(ValueError):
            T.read_isomeric(bad)
    assert T.plain_text('F/C=C\\[C@@H](Cl)Br') == 'FC=C[CH](Cl)Br'


@needs_gxx
def test_examples_through_the_host_program(exe, tmp_path):
    rows = [T.all_rows(c, b, p) for c, b, p, _ in T.EXAMPLES.values()]
    rows += [T.all_rows(c, b, T.mirrored(p)) for c, b, p, _ in T.EXAMPLES.values()]
    got = T.run_host_check(exe, rows, tmp_path)
    assert [tx['text'] for _, tx in got[:len(T.EXAMPLES)]] == [t for _, _, _, t in T.EXAMPLES.values()]
    for k, (r, (st, tx)) in enumerate(zip(rows, got)):
        want_st, want_tx = _restated(r)
        T.same_stereo(st, want_st, where=k)
        T.same_text(tx, want_tx, where=k)


@needs_gxx
def test_cores_on_the_host_under_sanitizers(exe, tmp_path, family):
    """The text the kernels compile (csrc/stereo_core.h, the stereo part of csrc/smiles_core.h, mol_common.h's pair walk), built as a
    stand-alone host program with ASan + UBSan, on the family and three hundred further random graphs: every output `==` the
    restatement's, and every text agrees with the coordinates under the independent reader."""
    graphs = list(family)
    rng = np.random.default_rng(91)
    for _ in range(300):
        classes, bonds = T.random_graph(rng, int(rng.integers(1, 41)))
        graphs.append((classes, bonds, (rng.normal(size=(len(classes), 3)) * 1.5).astype(np.float32)))
    rows = [T.all_rows(*g) for g in graphs]
    got = T.run_host_check(exe, rows, tmp_path)
    assert len(got) == len(rows)
    centres = doubles = 0
    lim = M.StereoLimits()
    for k, (r, (st, tx)) in enumerate(zip(rows, got)):
        want_st, want_tx = _restated(r)
        if k >= len(family) and not (all(v is not None and abs(abs(v) - lim.vol_min) > T.MARGIN for v in want_st['volumes'].values())
                                     and all(t is not None and abs(abs(t) - lim.planar_min) > T.MARGIN for t in want_st['planarities'].values())):
            continue                                                   # (a further graph with a value at its threshold: fp32 may differ)
        T.same_stereo(st, want_st, where=k)
        T.same_text(tx, want_tx, where=k)
        assert tx['status'] & M.SMILES_STEREO_DROPPED == 0
        if tx['ok']:
            _, _, at = T.graph_of_rows(r.cls, r.order)
            a, b, _ = T.check_text_against_geometry(tx['text'], tx['atom_rank'], r.pos, want_st, at, where=k)
            centres, doubles = centres + a, doubles + b
            S.same_answer(T.smiles_of_rows(*r.smiles_inputs(), 0 * st['atom_parity'], 0 * st['bond_stereo'], capacity=12 * 128),
                          S.smiles_of_rows(*r.smiles_inputs(), capacity=12 * 128), where=k)
    assert centres >= 200 and doubles >= 100


@needs_gxx
def test_stereo_handed_in_contradiction_and_zero(exe, tmp_path):
    """Stereo values that no perception gives: three cis double bonds around a six-ring contradict each other and are dropped, three
    trans ones do not; values on atoms and pairs that cannot carry them are not read; all zeros give the plain text."""
    classes, bonds = [T.C_] * 6, {(0, 1): 2, (1, 2): 1, (2, 3): 2, (3, 4): 1, (4, 5): 2, (0, 5): 1}
    rows = T.all_rows(classes, bonds, np.arange(18).reshape(6, 3) * 0.3)
    h = len(rows.order)
    at = {p: R.pair_row(*p, 6) for p in bonds}
    zero_a, zero_b = np.zeros(6, dtype=np.int8), np.zeros(h, dtype=np.int8)
    cis, trans, wrong = zero_b.copy(), zero_b.copy(), np.ones(h, dtype=np.int8)
    for p, o in bonds.items():
        if o == 2:
            cis[at[p]], trans[at[p]], wrong[at[p]] = 1, -1, 0
    cases = {0: (zero_a, cis), 1: (zero_a, trans), 2: (zero_a + 1, wrong), 3: (zero_a, zero_b), 4: (zero_a + 2, zero_b + 2)}
    got = T.run_host_check(exe, [rows] * 5, tmp_path, stereo_in=cases)
    plain = S.smiles_of_rows(*rows.smiles_inputs(), capacity=12 * 8)
    for k, (_, tx) in enumerate(got):
        T.same_text(tx, T.smiles_of_rows(*rows.smiles_inputs(), *cases[k]), where=k)
        if k != 1:
            assert tx['text'] == plain['text'] == 'C1=CC=CC=C1' and tx['stereo_counts'].tolist() == [0] * 4
            assert tx['status'] == (M.SMILES_STEREO_DROPPED if k == 0 else 0) and np.array_equal(tx['counts'], plain['counts'])
    assert got[1][1]['text'] == 'C/1=C\\C=C\\C=C1' and got[1][1]['stereo_counts'].tolist() == [0, 0, 3, 3] and got[1][1]['status'] == 0


def test_labels_in_same_molecule_unique_and_sdf(tmp_path):
    c, b, p, _ = T.EXAMPLES['CHFClBr skeleton']
    left, right = T.assembled(c, b, p), T.assembled(c, b, T.mirrored(p))
    perm = [2, 0, 3, 1]
    moved = T.assembled(*T.renumbered(c, b, np.array(p), perm))
    assert M.same_molecule(left, right) and not M.same_molecule(left, right, stereo=True)
    assert M.same_molecule(left, moved, stereo=True) and moved['stereo']['stereo_key'] == left['stereo']['stereo_key'] != right['stereo']['stereo_key']
    c, b, p, _ = T.EXAMPLES['meso-tartaric skeleton']
    meso, meso_mirror = T.assembled(c, b, p), T.assembled(c, b, T.mirrored(p))
    c, b, p, _ = T.EXAMPLES['chiral tartaric skeleton']
    chiral, chiral_mirror = T.assembled(c, b, p), T.assembled(c, b, T.mirrored(p))
    c, b, p, _ = T.EXAMPLES['cis-1,2-difluoroethene skeleton']
    cis, trans = T.assembled(c, b, p), T.assembled(*T.EXAMPLES['trans-1,2-difluoroethene skeleton'][:3])
    mols = [left, right, moved, meso, meso_mirror, chiral, chiral_mirror, cis, trans]
    assert M.unique_molecules(mols)[1] == [0, 0, 0, 1, 1, 1, 1, 2, 2]
    assert M.unique_molecules(mols, stereo=True)[1] == [0, 1, 0, 2, 2, 3, 4, 5, 6]
    keys = torch.tensor([m['stereo']['stereo_key'] - (1 << 64) if m['stereo']['stereo_key'] >> 63 else m['stereo']['stereo_key'] for m in mols])
    assert M.duplicate_groups(keys)[2].tolist() == [0, 1, 0, 2, 2, 3, 4, 5, 6]
    with pytest.raises(ValueError, match='stereo'):
        M.same_molecule(left, {k: v for k, v in right.items() if k != 'stereo'}, stereo=True)
    path = tmp_path / 's.sdf'
    M.write_sdf(str(path), [left, trans, {k: v for k, v in left.items() if k != 'stereo'}])
    text = path.read_text()
    assert text.count('> <PHOREGEN_STEREO>') == 2 and text.startswith(M.mol_block(left))       # the mol block itself is unchanged
    item = text.split('> <PHOREGEN_STEREO>\n')[1].split('\n\n')[0].split('\n')
    assert item[:2] == ['status 0x04', 'stereo_key %016x' % left['stereo']['stereo_key']] and item[-1] == 'centre 1 - +'
    assert item[2:10] == ['%s %d' % (k, left['stereo'][k]) for k in M.STEREO_COUNTS]
    assert text.split('> <PHOREGEN_STEREO>\n')[2].split('\n\n')[0].split('\n')[-1] == 'bond 2 3 - -'


def test_stereo_needs_the_device():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    res = {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.stereo(res)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.smiles(res)


def test_binding_declares_the_stereo_kernels():
    lib = hip.load_library()
    header = MS.header_text()
    assert lib.pg_abi_version() == 11 == hip.ABI_VERSION
    for name, n_args in (('pg_mol_stereo', 29), ('pg_mol_smiles_stereo', 23), ('pg_mol_smiles', 20)):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in hip.EXPORTS and hasattr(lib, name)
        assert len(hip._PROTOS[name][1]) == n_args == MS.arg_count(name), name
    makefile = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert 'mol_stereo.hip' in makefile and re.search(r'mol_stereo\.o:.*stereo_core\.h', makefile) and re.search(r'mol_stereo\.o.*: mol_common\.h', makefile)
    for bit, name in M.STEREO_NAMES.items():
        assert MS.header_macro('PG_STEREO_' + name) == str(bit), name
    assert MS.header_macro('PG_STEREO_N_COUNTS') == str(len(M.STEREO_COUNTS))
    assert MS.header_macro('PG_SMILES_N_STEREO_COUNTS') == str(len(M.SMILES_STEREO_COUNTS))
    assert MS.header_macro('PG_SMILES_STEREO_DROPPED') == str(M.SMILES_STEREO_DROPPED)
    for word in ('STEREO_KEY_A', 'STEREO_KEY_B', 'STEREO_KEY_C', 'STEREO_KEY_D'):
        assert '0x%016X' % getattr(M, word) in header, word
    tab = hip.C.cast((hip.C.c_uint8 * 64)(), hip.C.c_void_p)

    # ---- pg_mol_stereo: argument errors are refused before any launch, without a GPU
    def args(B, n_lig, n_bond, max_n, F=1, arrays=None, vol=0.5, planar=0.25, undef=0):
        return (arrays, 0) + (arrays,) * 11 + (B, F, n_lig, n_bond, max_n, vol, planar, undef) + (arrays,) * 7 + (None,)
    assert lib.pg_mol_stereo(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_stereo' in lib.pg_last_error()
    for bad in (args(1, 4, 12, -1), args(-1, 4, 12, 4), args(1, -4, 12, 4), args(1, 4, -12, 4), args(1, 4, 12, 4, F=-1), args(1, 4, 11, 4)):
        assert lib.pg_mol_stereo(*bad) != 0 and b'pg_mol_stereo' in lib.pg_last_error()
    for kw in (dict(vol=0.0), dict(vol=float('nan')), dict(planar=-1.0), dict(planar=float('inf')), dict(undef=-1)):
        assert lib.pg_mol_stereo(*args(1, 4, 12, 4, arrays=tab, **kw)) != 0
        assert b'pg_mol_stereo' in lib.pg_last_error() and b'vol_min' in lib.pg_last_error()
    assert lib.pg_mol_stereo(*args(1, 4, 12, 4)) != 0                  # something to launch and no arrays
    assert b'pg_mol_stereo' in lib.pg_last_error() and b'null' in lib.pg_last_error()
    assert lib.pg_mol_stereo(*args(0, 0, 0, 0)) == 0 and lib.pg_mol_stereo(*args(3, 4, 12, 4, F=0)) == 0

    # ---- pg_mol_smiles_stereo: as pg_mol_smiles
    def sargs(B, n_lig, n_bond, max_n, F=1, table=tab, capacity=64, arrays=None, stereo='same'):
        st = arrays if stereo == 'same' else stereo
        return (arrays,) * 5 + (st, st, arrays, arrays, B, F, n_lig, n_bond, max_n, table, capacity) + (arrays,) * 5 + (st, None)
    assert lib.pg_mol_smiles_stereo(*sargs(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_smiles_stereo' in lib.pg_last_error()
    for bad in (sargs(1, 4, 12, -1), sargs(-1, 4, 12, 4), sargs(1, 4, 12, 4, F=-1), sargs(1, 4, 11, 4), sargs(1, 4, 12, 4, capacity=0, arrays=tab),
                sargs(1, 4, 12, 4, table=None, arrays=tab), sargs(1, 4, 12, 4), sargs(1, 4, 12, 4, arrays=tab, stereo=None)):
        assert lib.pg_mol_smiles_stereo(*bad) != 0 and b'pg_mol_smiles_stereo' in lib.pg_last_error()
    assert b'atom_parity' in lib.pg_last_error() and b'null' in lib.pg_last_error()
    assert lib.pg_mol_smiles_stereo(*sargs(0, 0, 0, 0)) == 0 and lib.pg_mol_smiles_stereo(*sargs(3, 4, 12, 4, F=0)) == 0
