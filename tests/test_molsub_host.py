"""CPU: the substructure search (DESIGN.md 2.9 "Substructure") without a GPU.  The restatement of tests/sub_reference.py is held against
networkx's subgraph monomorphisms on the frozen corpus and against expectations written out by hand; `Pattern`, its table and
`find_matches` (phoregen_amd/substructure.py) against the restatement; the core the kernel compiles (csrc/sub_core.h) runs as a host
program under ASan / UBSan (tools/mol_sub_host_check.cpp) and must equal the restatement too.  The kernel itself:
tests/test_gpu_molsub.py."""
import json
import os
import re
import shutil

import numpy as np
import pytest

import molkey_reference as Q
import sub_reference as R
from mol_support import C_, N_, build_host_check, cycle, header_text, run_program
from phoregen_amd import hip
from phoregen_amd import substructure as S
from phoregen_amd.utils.sample_utils import ATOM_TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def corpus():
    targets, names = R.corpus_targets()
    assert len(targets) == 413 and max(len(t['atoms']) for t in targets) == 40
    return targets, names


@pytest.fixture(scope='module')
def corpus_results(corpus):
    """{pattern name: the restatement's result per corpus molecule}, default max_steps"""
    return {p['name']: [R.search(t, p) for t in corpus[0]] for p in R.PATTERNS}


def _pattern(name):
    return next(p for p in R.PATTERNS + R.PROPERTY_PATTERNS if p['name'] == name)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_counts_equal_networkx_on_the_corpus(corpus, corpus_results):
    assert {p['name'] for p in R.PATTERNS} >= {'any-atom', 'C-O', 'C=any', 'path-4', 'path-8', 'path-16', '5-cycle', '6-cycle',
                                               'aromatic-ring', '3-star', 'NO-C-NO', 'fused-bicycle'}
    for p in R.PATTERNS:
        for t, r, name in zip(corpus[0], corpus_results[p['name']], corpus[1]):
            assert r['embeddings'] == R.nx_count(t, p), (p['name'], name)
            assert len(set(r['all'])) == len(r['all']) and all(R.is_embedding(t, p, e) for e in r['all'][:3])


def test_corpus_conditions(corpus, corpus_results):
    want = {'any-atom': (413, 40), 'path-4': (397, 160), 'path-8': (333, 434), 'path-16': (117, 338), '6-cycle': (109, 24),
            '5-cycle': (85, None), '3-star': (329, 96), 'fused-bicycle': (14, 4), 'aromatic-ring': (3, 12)}
    for name, (matched, most) in want.items():
        res = corpus_results[name]
        assert sum(r['embeddings'] > 0 for r in res) == matched, name
        assert most is None or max(r['embeddings'] for r in res) == most, name
    steps = {name: max(max(r['steps'].values(), default=0) for r in res) for name, res in corpus_results.items()}
    assert max(steps.values()) == 836 and steps['fused-bicycle'] == 836
    assert not any(r['truncated'] for res in corpus_results.values() for r in res)             # nothing truncates at the default
    assert {name for name, s in steps.items() if s > 100} == {'fused-bicycle', '6-cycle', '5-cycle', 'path-16'}
    assert (steps['6-cycle'], steps['5-cycle'], steps['path-16']) == (144, 101, 189)
    # the order of `all` is the defined one: by the images in matching order, lexicographically
    for p in R.PATTERNS:
        order = R.parse(p)['order']
        for r in corpus_results[p['name']][:60]:
            keys = [tuple(e[q] for q in order) for e in r['all']]
            assert keys == sorted(keys) and r['first'][:len(order)] == (list(r['all'][0]) if r['all'] else [-1] * len(order))


def _named(name):
    return next((c, b) for n, c, b in Q.named_bases() if n == name)


def _row(target, name, **kw):
    r = R.search(target, _pattern(name), **kw)
    return r['embeddings'], r['anchors'], sorted(S.mask_atoms(R.mask_words(r['mask']))), S.status_names(r['status'])


def test_property_constraints_on_the_named_bases():
    decalin, bicyclopentyl, benzene, pyridine, ethanol_water = (R.target_of_classes(*_named(n)) for n in
                                                                ('decalin', 'bicyclopentyl', 'benzene', 'pyridine', 'ethanol_water'))
    ring10 = list(range(10))
    # degree and atom ring: the two fusion atoms of decalin, the two joined atoms of bicyclopentyl
    assert _row(decalin, 'ring-fusion-atom') == (2, 2, [0, 1], ('MATCHED',))
    assert _row(bicyclopentyl, 'ring-fusion-atom') == (2, 2, [0, 5], ('MATCHED',))
    assert _row(benzene, 'ring-fusion-atom') == (0, 0, [], ('OUT_OF_BOUNDS',))                 # (min = 1)
    # the bond ring flag: bicyclopentyl's 0 - 5 is a bridge between ring atoms (both directions), forbidden by max = 0
    assert _row(decalin, 'bridge-bond') == (0, 0, [], ())
    assert _row(bicyclopentyl, 'bridge-bond') == (2, 2, [0, 5], ('MATCHED', 'OUT_OF_BOUNDS'))
    assert _row(decalin, 'ring-bond') == (22, 10, ring10, ('MATCHED',))                        # 11 ring bonds, both directions
    assert _row(bicyclopentyl, 'ring-bond') == (20, 10, ring10, ('MATCHED',))
    assert _row(ethanol_water, 'ring-bond') == (0, 0, [], ('OUT_OF_BOUNDS',))                  # (min = 1)
    # aromatic
    assert _row(pyridine, 'aromatic-N') == (1, 1, [0], ('MATCHED',))
    assert _row(benzene, 'aromatic-N') == (0, 0, [], ())
    # hydrogens: decalin has eight CH2 and two CH, benzene six CH, ethanol + water CH3 CH2 OH OH2
    assert _row(decalin, 'CH2') == (8, 8, [2, 3, 4, 5, 6, 7, 8, 9], ('MATCHED',))
    assert _row(bicyclopentyl, 'CH2') == (8, 8, [1, 2, 3, 4, 6, 7, 8, 9], ('MATCHED',))
    assert _row(benzene, 'CH2') == (0, 0, [], ())
    assert _row(ethanol_water, 'CH2') == (1, 1, [1], ('MATCHED',))
    assert _row(ethanol_water, 'OH') == (2, 2, [2, 3], ('MATCHED',))
    assert _row(ethanol_water, 'neutral-chain-C') == (3, 2, [0, 1, 2], ('MATCHED',))           # C0-C1, C1-C0, C1-O2
    assert _row(decalin, 'neutral-chain-C') == (0, 0, [], ())
    # charge: a nitrogen with four single bonds is N+
    ammonium = R.target_of_classes([N_, C_, C_, C_, C_], {(0, i): 1 for i in (1, 2, 3, 4)})
    assert _row(ammonium, 'cation') == (1, 1, [0], ('MATCHED',))
    assert _row(ammonium, 'neutral-chain-C') == (4, 4, [0, 1, 2, 3, 4], ('MATCHED',))
    assert _row(ethanol_water, 'cation') == (0, 0, [], ())


def test_a_graph_without_a_kekule_structure():
    """Five aromatic carbons in a ring have no Kekulé structure: a pattern that reads hydrogens or charge has no embedding and says
    why, any other pattern is searched as always."""
    five = R.target_of_classes([C_] * 5, cycle(5, 4))
    assert five['kekule_failed']
    for name in ('CH2', 'cation', 'OH', 'neutral-chain-C'):
        assert _row(five, name) == (0, 0, [], ('NO_KEKULE',))
    assert _row(five, 'any-atom') == (5, 5, [0, 1, 2, 3, 4], ('MATCHED',))
    assert _row(five, '5-cycle') == (10, 5, [0, 1, 2, 3, 4], ('MATCHED',))
    assert _row(five, 'aromatic-N') == (0, 0, [], ())
    assert _row(R.target_of_classes([], {}), 'any-atom') == (0, 0, [], ())                     # no kept atom: no embedding


def test_renumbering_permutes_the_mask_and_nothing_else():
    mols, iso_pairs, _, _ = Q.corpus()
    rng = np.random.default_rng(5)
    for a, b in iso_pairs[:40]:
        classes = [ATOM_TYPES.index(z) for z in mols[a]['element']]
        bi, bt = mols[a]['bond_index'].numpy(), mols[a]['bond_type'].numpy()
        bonds = {(int(x), int(y)): int(t) for x, y, t in zip(bi[0], bi[1], bt)}
        perm = rng.permutation(len(classes)).tolist()
        ta, tb = R.target_of_classes(classes, bonds), R.target_of_classes(*Q.permuted(classes, bonds, perm))
        for p in R.PATTERNS[:5] + R.PATTERNS[6:] + R.PROPERTY_PATTERNS[:4]:                    # (Kekulé properties depend on the structure chosen)
            ra, rb = R.search(ta, p), R.search(tb, p)
            assert (ra['embeddings'], ra['anchors']) == (rb['embeddings'], rb['anchors']), p['name']
            assert sum(1 << perm[c] for c in S.mask_atoms(R.mask_words(ra['mask']))) == rb['mask'], p['name']


# ---- Pattern, its table, find_matches ----------------------------------------------------------------------------------------------------
def test_pattern_validation_names_the_field():
    ok = {'name': 'x', 'atoms': [{'elements': ['C']}, {}], 'bonds': [{'a': 0, 'b': 1}]}
    assert S.Pattern.from_dict(ok).match_order == (0, 1)
    bad = [
        (dict(ok, colour=1), r"unknown keys \['colour'\]"),
        (dict(ok, atoms=[{'elements': []}, {}]), r'atoms\[0\]\.elements must be a non-empty'),
        (dict(ok, atoms=[{'elements': ['Xx']}, {}]), r"atoms\[0\]\.elements: 'Xx' is not one"),
        (dict(ok, atoms=[{'valence': 3}, {}]), r"atoms\[0\]: unknown keys \['valence'\]"),
        (dict(ok, atoms=[{'degree': [3, 1]}, {}]), r'atoms\[0\]\.degree must satisfy'),
        (dict(ok, atoms=[{'charge': 2}, {}]), r'atoms\[0\]\.charge must be 0, 1 or null'),
        (dict(ok, atoms=[{'ring': 1}, {}]), r'atoms\[0\]\.ring must be true, false or null'),
        (dict(ok, bonds=[{'a': 0, 'b': 1, 'orders': []}]), r'bonds\[0\]\.orders must be a non-empty subset'),
        (dict(ok, bonds=[{'a': 0, 'b': 1, 'orders': [5]}]), r'bonds\[0\]\.orders must be a non-empty subset'),
        (dict(ok, bonds=[{'a': 0, 'b': 2}]), r'bonds\[0\] \(0, 2\) indexes outside the 2 query atoms'),
        (dict(ok, bonds=[{'a': 0, 'b': 1}, {'a': 1, 'b': 0}]), r'bonds: duplicate bond \(0, 1\)'),
        (dict(ok, bonds=[]), r'bonds: the pattern is disconnected: query atoms \[1\]'),
        (dict(ok, atoms=[{}] * 17, bonds=[{'a': i, 'b': i + 1} for i in range(16)]), r'atoms: a pattern has 1 \.\. 16 query atoms'),
        (dict(ok, name='a b'), r'name must be a non-empty string without white space'),
        (dict(ok, min=2, max=1), r'min / max must satisfy'),
    ]
    for d, message in bad:
        with pytest.raises(ValueError, match='pattern: ' + message):
            S.Pattern.from_dict(d)
    with pytest.raises(ValueError, match='names must be distinct'):
        S.pattern_table([S.Pattern.from_dict(ok), S.Pattern.from_dict(ok)])
    with pytest.raises(ValueError, match='1 .. 256 Pattern objects'):
        S.pattern_table([])


def test_match_order_is_breadth_first_from_atom_0():
    for p in R.PATTERNS + R.PROPERTY_PATTERNS:
        assert list(S.Pattern.from_dict(p).match_order) == R.parse(p)['order'], p['name']
    assert S.Pattern.from_dict(_pattern('5-cycle')).match_order == (0, 1, 4, 2, 3)
    assert S.Pattern.from_dict(_pattern('fused-bicycle')).match_order == (0, 1, 5, 6, 2, 9, 4, 7, 3, 8)


def test_table_round_trip_and_header_macros(tmp_path):
    macros = {k: int(v) for k, v in re.findall(r'#define (PG_SUB_\w+) (\d+)', header_text())}
    mine = {k: getattr(hip, k) for k in dir(hip) if k.startswith('PG_SUB_')}
    mine.update(PG_SUB_MATCHED=S.SUB_MATCHED, PG_SUB_NO_KEKULE=S.SUB_NO_KEKULE, PG_SUB_TRUNCATED=S.SUB_TRUNCATED,
                PG_SUB_OUT_OF_BOUNDS=S.SUB_OUT_OF_BOUNDS)
    assert macros == mine and len(macros) == 22
    assert (S.MAX_ATOMS, S.MAX_PATTERNS, S.PATTERN_BYTES, S.MAX_STEPS, S.DEFAULT_STEPS) == (16, 256, 416, 2 ** 30, 65536)
    patterns = [S.Pattern.from_dict(p) for p in R.PATTERNS + R.PROPERTY_PATTERNS]
    table = S.pattern_table(patterns)
    assert table.dtype == np.uint8 and table.shape == (len(patterns), S.PATTERN_BYTES)
    assert S.unpack_table(table, [p.name for p in patterns]) == patterns
    for p in patterns:
        assert S.Pattern.from_dict(p.to_dict()) == p and S.Pattern.from_dict(json.loads(json.dumps(p.to_dict()))) == p
    row = table[[p.name for p in patterns].index('ring-bond')]
    assert row[hip.PG_SUB_OFF_K] == 2 and row[hip.PG_SUB_OFF_MIN] == 1 and row[hip.PG_SUB_OFF_MAX] == 20
    assert row[hip.PG_SUB_OFF_BONDS + 1] == row[hip.PG_SUB_OFF_BONDS + 16] == 15 | hip.PG_SUB_YES << 4
    path = tmp_path / 'patterns.json'
    path.write_text(json.dumps([p.to_dict() for p in patterns]))
    assert S.load_patterns_json(str(path)) == patterns
    assert [p.name for p in S.load_patterns_json(os.path.join(ROOT, 'tools', 'patterns', 'example_patterns.json'))] == ['amide', 'peroxide', 'nitro']


def _assembled(classes, bonds):
    """An assembled-style dict with the 'rings' and 'kekule' entries `find_matches` reads, from the tests' references."""
    import kekule_reference as K
    import ring_reference as G
    m = Q.mol_from(classes, bonds)
    cls, order = G.rows_of(list(classes), dict(bonds))
    rings, kek = G.rings_of_rows(cls, order), K.kekule_of_rows(cls, order)
    nz = np.nonzero(order)[0]
    m['rings'] = {'bond_ring_size': rings['ring_size'][nz], 'atom_ring': rings['atom_ring']}
    m['kekule'] = {'hcount': kek['hcount'], 'charge': kek['charge'], 'kekule_ok': bool(kek['ok'])}
    return m


def test_find_matches_equals_the_restatement():
    graphs = [(c, b) for _, c, b in Q.named_bases()] + [([C_] * 5, cycle(5, 4)), ([N_, C_, C_, C_, C_], {(0, i): 1 for i in (1, 2, 3, 4)})]
    rng = np.random.default_rng(Q.CORPUS_SEED)
    graphs += [Q._random_base(rng) for _ in range(6)]
    for classes, bonds in graphs:
        mol, target = _assembled(classes, bonds), R.target_of_classes(classes, bonds)
        for p in R.PATTERNS + R.PROPERTY_PATTERNS:
            want = R.search(target, p)['all']
            assert S.find_matches(mol, S.Pattern.from_dict(p)) == want, p['name']
            assert S.find_matches(mol, S.Pattern.from_dict(p), limit=2) == want[:2]
    plain = Q.mol_from(*_named('decalin')[:2])
    with pytest.raises(ValueError, match='carries no rings'):
        S.find_matches(plain, S.Pattern.from_dict(_pattern('ring-bond')))
    with pytest.raises(ValueError, match='carries no kekule'):
        S.find_matches(plain, S.Pattern.from_dict(_pattern('CH2')))
    # from_molecule: a molecule contains itself, and the cut-out part where it was cut
    whole = S.Pattern.from_molecule(plain)
    assert len(S.find_matches(plain, whole)) == 4 and S.find_matches(plain, whole)[0] == tuple(range(10))       # decalin's symmetries
    part = S.Pattern.from_molecule(plain, atoms=[6, 0, 1])
    assert (6, 0, 1) in S.find_matches(plain, part) and part.match_order == (0, 1, 2)


def test_pattern_from_fragment():
    from phoregen_amd.fragment import Fragment
    frag = Fragment.from_dict({'element': [6, 7, 8], 'pos': [[0, 0, 0], [1.4, 0, 0], [-0.7, 1.2, 0]], 'bonds': [(0, 1, 1), (0, 2, 2)]})
    p = S.Pattern.from_fragment(frag, name='amide-core')
    assert p.to_dict() == {'name': 'amide-core', 'atoms': [{'elements': ['C']}, {'elements': ['N']}, {'elements': ['O']}],
                           'bonds': [{'a': 0, 'b': 1, 'orders': [1]}, {'a': 0, 'b': 2, 'orders': [2]}], 'min': 0, 'max': None}
    with pytest.raises(ValueError, match='disconnected'):
        S.Pattern.from_fragment({'element': [6, 7], 'pos': [[0, 0, 0], [1.4, 0, 0]], 'bonds': []})


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_keeps_its_abi():
    assert hip.ABI_VERSION == 11 and 'pg_mol_sub' in hip.EXPORTS
    lib = hip.load_library()
    assert lib.pg_abi_version() == 11 and lib.pg_mol_sub.restype is not None and len(lib.pg_mol_sub.argtypes) == 25


# ---- the core under the host sanitizers ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')
def test_core_under_the_host_sanitizers_equals_the_restatement(corpus, corpus_results, tmp_path):
    exe = build_host_check('mol_sub_host_check', tmp_path)
    patterns = R.PATTERNS + R.PROPERTY_PATTERNS
    rows = dict(zip((p['name'] for p in patterns), S.pattern_table([S.Pattern.from_dict(p) for p in patterns]).tolist()))
    cases, wants = [], []
    for p in R.PATTERNS:                                               # the corpus at the default bound and at 100
        for t, r in zip(corpus[0], corpus_results[p['name']]):
            cases.append((t, rows[p['name']], S.DEFAULT_STEPS))
            wants.append((t, p, r))
            if max(r['steps'].values(), default=0) > 60:
                cases.append((t, rows[p['name']], 100))
                wants.append((t, p, dict(r, truncated=max(r['steps'].values()) > 100)))
    extra = [R.target_of_classes(c, b) for _, c, b in Q.named_bases()]
    extra += [R.target_of_classes([C_] * 5, cycle(5, 4)), R.target_of_classes([N_, C_, C_, C_, C_], {(0, i): 1 for i in (1, 2, 3, 4)}),
              R.target_of_classes([], {}), R.target_of_classes([11, 11], {})]
    for t in extra:
        for p in patterns:
            for steps in (S.DEFAULT_STEPS, 1):
                cases.append((t, rows[p['name']], steps))
                wants.append((t, p, R.search(t, p, max_steps=steps)))
    assert sum(w[2]['truncated'] for w in wants) >= 40 and sum(w[2]['no_kekule'] for w in wants) >= 4
    malformed = []                                                     # rows the entry point refuses: the check's code, nothing searched
    for off, value, code in ((hip.PG_SUB_OFF_K, 17, 1), (hip.PG_SUB_OFF_K, 0, 1), (hip.PG_SUB_OFF_ATOMS, 0, 2), (hip.PG_SUB_OFF_BONDS + 1, 16, 5),
                             (hip.PG_SUB_OFF_ORDER, 1, 6), (hip.PG_SUB_OFF_BONDS + 16, 0, 5), (hip.PG_SUB_OFF_MAX, 0, 8)):
        row = list(rows['ring-bond'])
        row[off] = value
        if off == hip.PG_SUB_OFF_ATOMS:
            row[off + 1] = 0
        malformed.append((row, code))
        cases.append((extra[0], row, 10))
    no_parent = list(rows['C-O'])
    no_parent[hip.PG_SUB_OFF_BONDS + 1] = no_parent[hip.PG_SUB_OFF_BONDS + 16] = 0
    malformed.append((no_parent, 7))
    cases.append((extra[0], no_parent, 10))
    path = os.path.join(str(tmp_path), 'sub_cases.txt')
    R.write_host_cases(path, cases)
    got = R.read_host_answers('\n'.join(run_program(exe, path)))
    assert len(got) == len(cases) == len(wants) + len(malformed)
    for (code, row), (t, p, want) in zip(got, wants):
        assert code == 0
        R.check_row(row, want, t, p, p['name'])
    for (code, row), (_, want_code) in zip(got[len(wants):], malformed):
        assert code == want_code and row['embeddings'] == 0 and row['first'] == [-1] * S.MAX_ATOMS
