"""CPU: the SMILES writer's definition (restated in tests/smiles_reference.py from DESIGN.md 2.9 "SMILES") on the hand-checked
examples, the kernel's core compiled for the host under ASan / UBSan (tools/smiles_host_check.cpp) against the restatement byte for
byte, every text read back by the independent reader, the label and capacity boundaries, the SDF item, the binding and its argument
errors.

The kernel itself is held against the restatement in tests/test_gpu_molsmiles.py."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import kekule_reference as K
import mol_reference as R
import smiles_reference as S
from mol_support import arg_count, build_host_check, header_macro, header_text, mol_dict as _mol
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CI = M.SMILES_COUNTS.index
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build_host_check('smiles_host_check', tmp_path_factory.mktemp('smiles_host'))


def test_tables_and_constants():
    from phoregen_amd.utils.sample_utils import ATOM_TYPES
    assert [M.SMILES_VALENCES[z] for z in ATOM_TYPES] == [(3,), (4,), (3, 5), (2,), (1,), (), (3, 5), (2, 4, 6), (1,), (1,), (1,)]
    assert (M.SMILES_NO_KEKULE, M.SMILES_RING_LABELS, M.SMILES_TOO_LONG, M.SMILES_DISCONNECTED, M.SMILES_EMPTY, M.SMILES_BRACKET) == (1, 2, 4, 8, 16, 32)
    assert M.SMILES_FAIL_MASK == 7 and sorted(M.SMILES_NAMES) == [1, 2, 4, 8, 16, 32] and M.SMILES_MAX_LABEL == 99
    assert M.SMILES_COUNTS == ('length', 'atoms', 'bonds', 'components', 'ring_closures', 'branches', 'max_label', 'bracket_atoms')
    # the notation's table is a second table on purpose: where it and the hydrogen rule disagree the atom is bracketed
    assert M.SMILES_VALENCES[7] != M.H_VALENCES[7] and M.SMILES_VALENCES[53] != M.H_VALENCES[53]
    assert S.atom_token(7, 3, 0, 0) == ('N', False) and S.atom_token(7, 4, 0, 1) == ('[N+]', True) and S.atom_token(7, 2, 1, 0) == ('N', False)
    assert S.atom_token(53, 2, 1, 0) == ('[IH]', True) and S.atom_token(14, 1, 3, 0) == ('[SiH3]', True) and S.atom_token(16, 3, 1, 0) == ('S', False)
    assert S.atom_token(6, 5, 0, 0) == ('C', False)                    # no valence left: the reader gives 0 hydrogens, and so does the rule
    with pytest.raises(ValueError, match='smiles='):
        M.sample_valid(None, None, 1, smiles=M.KekuleOptions())


@pytest.mark.parametrize('name', list(S.EXAMPLES))
def test_example_by_hand(name):
    classes, bonds, text = S.EXAMPLES[name]
    rows = S.kekule_rows(classes, bonds)
    w = S.smiles_of_rows(*rows)
    assert w['text'] == text and w['ok'] and w['length'] == len(text)
    c = dict(zip(M.SMILES_COUNTS, w['counts'].tolist()))
    assert c['length'] == len(text) and c['atoms'] == sum(k <= 10 for k in classes) and c['components'] == text.count('.') + 1
    assert c['ring_closures'] == c['bonds'] - c['atoms'] + c['components'] and c['branches'] == text.count('(')
    assert bool(w['status'] & M.SMILES_DISCONNECTED) == ('.' in text) and bool(w['status'] & M.SMILES_BRACKET) == ('[' in text)
    S.check_read_back(text, *rows[:4], w['atom_rank'], where=name)


def test_example_details_by_hand():
    by = {name: S.smiles_of_rows(*S.kekule_rows(c, b)) for name, (c, b, _) in S.EXAMPLES.items()}
    assert by['norbornane']['atom_rank'].tolist() == [0, 1, 2, 3, 4, 5, 6] and by['norbornane']['counts'][CI('max_label')] == 2
    assert by['dimethyl ether with a dropped atom']['atom_rank'].tolist() == [0, -1, 1, 2]
    assert by['tetrahedrane skeleton']['counts'].tolist() == [10, 4, 6, 1, 3, 0, 3, 0]
    assert by['two cyclopropanes joined by a bond']['counts'][CI('max_label')] == 1     # the label is free again after the first ring
    assert by['spiro[2.2]pentane']['counts'][CI('max_label')] == 2                      # ... but not at the atom where it closes
    assert by['tetramethylammonium']['counts'].tolist() == [14, 5, 4, 1, 0, 3, 0, 1]
    # the reader, on its own: what it accepts and what it refuses
    assert S.read_smiles('C=1CCCCC1') == ([(6, 1, 0)] + [(6, 2, 0)] * 4 + [(6, 1, 0)], {(0, 1): 1, (1, 2): 1, (2, 3): 1, (3, 4): 1, (4, 5): 1, (0, 5): 2})
    assert S.read_smiles('[N+](C)(C)(C)C')[0][0] == (7, 0, 1) and S.read_smiles('C%12CC%12')[1] == {(0, 1): 1, (1, 2): 1, (0, 2): 1}
    assert S.read_smiles('ClC(Br)[SiH3]')[0] == [(17, 0, 0), (6, 1, 0), (35, 0, 0), (14, 3, 0)] and S.read_smiles('') == ([], {})
    assert S.read_smiles('N(=O)(=O)C')[0][0] == (7, 0, 0) and S.read_smiles('SC')[0][0] == (16, 1, 0) and S.read_smiles('[S]C')[0][0] == (16, 0, 0)
    for bad in ('C1CC', 'C(C', 'C)C', 'C=', '=C', 'C..C', 'c1ccccc1', '[Na]', 'C11', 'C1C1', 'C%1C', '[CH-]', 'C(.C)'):
        with pytest.raises(ValueError):
            S.read_smiles(bad)
    # no Kekulé structure: no text
    w = S.smiles_of_rows(*S.kekule_rows(*K.NAMED['all-carbon five-ring'][:2]))
    assert (w['status'], w['text'], w['length'], w['counts'].tolist(), w['atom_rank'].tolist()) == (M.SMILES_NO_KEKULE, '', 0, [0] * 8, [-1] * 5)
    # nothing kept
    w = S.smiles_of_rows(*S.kekule_rows([11, 11], {(0, 1): 1}))
    assert (w['status'], w['text'], w['ok'], w['counts'].tolist()) == (M.SMILES_EMPTY, '', True, [0] * 8)


@needs_gxx
def test_examples_through_the_host_program(exe, tmp_path):
    rows = [S.kekule_rows(c, b) for c, b, _ in S.EXAMPLES.values()]
    got = S.run_host_check(exe, [(*r, None) for r in rows], tmp_path)
    assert [g['text'] for g in got] == [t for _, _, t in S.EXAMPLES.values()]
    for name, g, r in zip(S.EXAMPLES, got, rows):
        S.same_answer(g, S.smiles_of_rows(*r), where=name)


@needs_gxx
def test_core_on_the_host_under_sanitizers(exe, tmp_path):
    """The text the kernel compiles (csrc/smiles_core.h, mol_common.h's pair walk), built as a stand-alone host program with ASan +
    UBSan, on the random family and two thousand further random graphs: byte-equal to the restatement, and every text read back."""
    graphs = list(K.random_family())
    rng = np.random.default_rng(78)
    graphs += [K.random_graph(rng, int(rng.integers(1, 41))) for _ in range(2000)]
    rows = [S.kekule_rows(c, b) for c, b in graphs]
    got = S.run_host_check(exe, [(*r, None) for r in rows], tmp_path)
    assert len(got) == len(rows)
    n_ok = n_none = largest = 0
    for k, (g, r) in enumerate(zip(got, rows)):
        S.same_answer(g, S.smiles_of_rows(*r), where='case %d' % k)
        if g['ok']:
            S.check_read_back(g['text'], *r[:4], g['atom_rank'], where='case %d' % k)
            c = dict(zip(M.SMILES_COUNTS, g['counts'].tolist()))
            assert c['ring_closures'] == c['bonds'] - c['atoms'] + c['components'] and c['length'] == len(g['text'])
            n_ok, largest = n_ok + 1, max(largest, c['max_label'])
        else:
            assert g['status'] == M.SMILES_NO_KEKULE and bool(r[4] & M.KEKULE_FAILED)
            n_none += 1
    assert n_ok >= 1000 and n_none >= 300 and largest >= 3


@needs_gxx
def test_label_boundary(exe, tmp_path):
    at, over = S.kekule_rows(*S.label_boundary(99)), S.kekule_rows(*S.label_boundary(100))
    g_at, g_over = S.run_host_check(exe, [(*at, None), (*over, None)], tmp_path)
    for got in (g_at, S.smiles_of_rows(*at)):
        first = 'C' + ''.join(S.label_text(k) for k in range(1, 100))
        assert got['text'].startswith(first + 'C') and first.endswith('%99') and got['ok']
        assert got['counts'][CI('max_label')] == 99 and got['counts'][CI('ring_closures')] == 99 and got['length'] <= 8 * 128
        S.check_read_back(got['text'], *at[:4], got['atom_rank'], where='99 labels')
    S.same_answer(g_at, S.smiles_of_rows(*at))
    for got in (g_over, S.smiles_of_rows(*over)):
        assert (got['status'], got['text'], got['length'], got['counts'].tolist()) == (M.SMILES_RING_LABELS, '', 0, [0] * 8)
        assert got['atom_rank'].tolist() == [-1] * 128
    # 99 labels in use, one closed and another opened at the same atom: the closed one is not free there, so that is one too many
    classes, bonds = S.label_boundary(99)
    bonds[(2, 127)] = 1                                                # atom 2 closes label 1, 2 .. 99 are open, and it opens one of its own
    one_more = S.kekule_rows(classes, bonds)
    (got,) = S.run_host_check(exe, [(*one_more, None)], tmp_path)
    assert got['status'] == M.SMILES_RING_LABELS == S.smiles_of_rows(*one_more)['status']
    bonds = dict(S.label_boundary(99)[1])
    bonds[(3, 127)] = 1                                                # ... opened one atom later it takes label 1 again
    later = S.kekule_rows(classes, bonds)
    (got,) = S.run_host_check(exe, [(*later, None)], tmp_path)
    S.same_answer(got, S.smiles_of_rows(*later))
    assert got['ok'] and got['counts'][CI('max_label')] == 99 and got['counts'][CI('ring_closures')] == 100


@needs_gxx
def test_capacity_boundary(exe, tmp_path):
    rows = S.kekule_rows(*S.EXAMPLES['norbornane'][:2])
    text = S.EXAMPLES['norbornane'][2]
    exact, short, one = S.run_host_check(exe, [(*rows, len(text)), (*rows, len(text) - 1), (*rows, 1)], tmp_path)
    assert exact['text'] == text and exact['status'] == 0 and exact['length'] == len(text)
    for got, cap in ((short, len(text) - 1), (one, 1)):
        S.same_answer(got, S.smiles_of_rows(*rows, capacity=cap))
        assert got['status'] == M.SMILES_TOO_LONG and got['text'] == '' and got['length'] == 0 and got['atom_rank'].tolist() == [-1] * 7
        assert got['counts'].tolist() == exact['counts'].tolist() and got['counts'][CI('length')] == len(text)


def test_sdf_item_and_formula(tmp_path):
    w = S.smiles_of_rows(*S.kekule_rows(*S.EXAMPLES['tetramethylammonium'][:2]))
    mol = _mol([7, 6, 6, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)], [1] * 4)
    item = dict(zip(M.SMILES_COUNTS, w['counts'].tolist()), status=w['status'], smiles_ok=True, text=w['text'], atom_rank=w['atom_rank'])
    failed = dict(item, status=M.SMILES_NO_KEKULE, smiles_ok=False, text='')
    path = tmp_path / 's.sdf'
    M.write_sdf(str(path), [dict(mol, smiles=item, key=0x2A), mol, dict(mol, smiles=failed)], names=['a', 'b', 'c'])
    text = path.read_text()
    assert text.count('> <PHOREGEN_SMILES>') == 1
    assert text.startswith(M.mol_block(mol, 'a') + '> <PHOREGEN_KEY>\n000000000000002a\n\n> <PHOREGEN_SMILES>\n[N+](C)(C)(C)C\n\n$$$$\n'
                           + M.mol_block(mol, 'b') + '$$$$\n' + M.mol_block(mol, 'c') + '$$$$\n')
    # the formula of what the text reads back to is the Kekulé form's
    for name in ('pyridine', 'N-methylpyridinium', 'thiopyrylium', 'indole', '2-pyridone', 'naphthalene'):
        cls, kek, h, q, st = S.kekule_rows(*K.NAMED[name][:2])
        want = M.formula_of([M.ATOM_TYPES[c] for c in cls.tolist()], h, int(q.sum()))[0]
        assert S.formula_of_text(S.smiles_of_rows(cls, kek, h, q, st)['text']) == want, name
    assert S.formula_of_text('[N+](C)(C)(C)C') == 'C4H12N+' and S.formula_of_text('C[IH]C') == 'C2H7I'


def test_smiles_needs_the_device():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    res = {'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.smiles(res)


def test_binding_declares_the_smiles_kernel():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_smiles\s*\(', header)
    assert 'pg_mol_smiles' in hip.EXPORTS and hasattr(lib, 'pg_mol_smiles')
    assert len(hip._PROTOS['pg_mol_smiles'][1]) == 20 == arg_count('pg_mol_smiles')
    makefile = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert 'mol_smiles.hip' in makefile and re.search(r'mol_smiles\.o:.*smiles_core\.h', makefile) and re.search(r'mol_smiles\.o.*: mol_common\.h', makefile)
    for bit, name in M.SMILES_NAMES.items():
        assert header_macro('PG_SMILES_' + name) == str(bit), name
    assert header_macro('PG_SMILES_N_COUNTS') == str(len(M.SMILES_COUNTS))
    # argument errors are refused before any launch, without a GPU: oversize, negative sizes, no capacity, a null table, null arrays
    tab = hip.C.cast((hip.C.c_uint8 * 44)(), hip.C.c_void_p)

    def args(B, n_lig, n_bond, max_n, F=1, table=tab, capacity=64, arrays=None):
        return (arrays, arrays, arrays, arrays, arrays, arrays, arrays, B, F, n_lig, n_bond, max_n, table, capacity, arrays, arrays, arrays,
                arrays, arrays, None)
    assert lib.pg_mol_smiles(*args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1)) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error() and b'pg_mol_smiles' in lib.pg_last_error()
    for bad in (args(1, 4, 12, -1), args(-1, 4, 12, 4), args(1, -4, 12, 4), args(1, 4, -12, 4), args(1, 4, 12, 4, F=-1), args(1, 4, 11, 4)):
        assert lib.pg_mol_smiles(*bad) != 0 and b'pg_mol_smiles' in lib.pg_last_error()
    for cap in (0, -5):
        assert lib.pg_mol_smiles(*args(1, 4, 12, 4, capacity=cap, arrays=tab)) != 0
        assert b'pg_mol_smiles' in lib.pg_last_error() and b'capacity' in lib.pg_last_error()
    assert lib.pg_mol_smiles(*args(1, 4, 12, 4, table=None, arrays=tab)) != 0
    assert b'pg_mol_smiles' in lib.pg_last_error() and b'null' in lib.pg_last_error()
    assert lib.pg_mol_smiles(*args(1, 4, 12, 4)) != 0                  # something to launch and no arrays
    assert b'pg_mol_smiles' in lib.pg_last_error() and b'null' in lib.pg_last_error()
    assert lib.pg_mol_smiles(*args(0, 0, 0, 0)) == 0 and lib.pg_mol_smiles(*args(3, 4, 12, 4, F=0)) == 0
