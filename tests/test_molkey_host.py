"""CPU: the identity key's definition (restated in tests/molkey_reference.py from DESIGN.md 2.9), the exact comparison and the
grouping of phoregen_amd/molecule.py against networkx on a frozen corpus, the SDF data item, the unique top-up loop, the binding.

The kernel itself is held against the restatement bit for bit in tests/test_gpu_molkey.py.  Everything is integer: every
comparison is `==`."""
import os
import re

import numpy as np
import pytest
import torch

import molkey_reference as K
from mol_support import header_text
from phoregen_amd import hip
from phoregen_amd import molecule as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def corpus():
    mols, iso_pairs, near_pairs, names = K.corpus()
    return {'mols': mols, 'iso_pairs': iso_pairs, 'near_pairs': near_pairs, 'names': names, 'classes': K.nx_partition(mols),
            'keyed': [K.with_key(m) for m in mols]}


def test_corpus_conditions(corpus):
    """Judged by networkx alone, before anything of the project is looked at."""
    mols, cls = corpus['mols'], corpus['classes']
    assert len(cls) == len(mols) >= 300 and max(len(m['element']) for m in mols) <= K.CORPUS_MAX_ATOMS
    graphs = [K.nx_graph(m) for m in mols]
    iso = [(a, b) for a, b in corpus['iso_pairs'] if K.nx_same(graphs[a], graphs[b])]
    near = [(a, b) for a, b in corpus['near_pairs'] if not K.nx_same(graphs[a], graphs[b])]
    print(f'corpus: {len(mols)} molecules, {max(cls) + 1} classes, {len(iso)} isomorphic pairs, {len(near)} non-isomorphic near-miss pairs')
    assert len(iso) == len(corpus['iso_pairs']) >= 100               # a renumbering is the same molecule
    assert len(near) >= 100
    assert max(cls) + 1 < len(mols)
    assert all((cls[a] == cls[b]) for a, b in iso) and all(cls[a] != cls[b] for a, b in near)
    kinds = {n.split('/')[1] for n in corpus['names'] if '/' in n}
    assert {'element', 'order', 'moved', 'perm0', 'perm1'} <= kinds


def test_restated_key_is_invariant_and_tells_near_misses_apart(corpus):
    keyed = corpus['keyed']
    for a, b in corpus['iso_pairs']:
        assert keyed[a]['key'] == keyed[b]['key'], (corpus['names'][a], corpus['names'][b])
        assert sorted(keyed[a]['atom_colour'].tolist()) == sorted(keyed[b]['atom_colour'].tolist())
    for a, b in corpus['near_pairs']:
        if corpus['classes'][a] != corpus['classes'][b]:
            assert keyed[a]['key'] != keyed[b]['key'], (corpus['names'][a], corpus['names'][b])
    by_name = {n: m['key'] for n, m in zip(corpus['names'], keyed)}
    assert by_name['decalin'] != by_name['bicyclopentyl']              # (neighbour refinement alone cannot tell these two apart)
    assert by_name['benzene'] != by_name['cyclohexane']
    assert by_name['benzene'] != by_name['benzene_kekule']             # no kekulisation: two spellings, two keys
    # fresh random renumberings of every molecule of the corpus, beyond the frozen pairs
    rng = np.random.default_rng(1)
    for m, km in zip(corpus['mols'], keyed):
        classes = [M.ATOM_TYPES.index(z) for z in m['element']]
        bonds = {(a, b): t for (a, b), t in zip(m['bond_index'].T.tolist(), m['bond_type'].tolist())}
        key, colour = K.key_of(*K.permuted(classes, bonds, rng.permutation(len(classes)).tolist()))
        assert key == km['key'] and sorted(colour) == sorted(km['atom_colour'].tolist())


def test_restated_key_of_hand_cases():
    assert K.mix(0) == M.KEY_EMPTY == 0xE220A8397B1DCDAF
    assert K.key_of([], {})[0] == M.KEY_EMPTY
    # dropped atoms, their place in the row order, bonds to them and class-5 rows have no influence
    plain = K.key_of_rows([1, 1, 3], [1, 0, 2])                        # C-C=O
    holes = K.key_of_rows([-1, 1, 1, -1, 3], [1, 1, 0, 1,  1, 0, 0,  3, 2,  4])
    assert plain[0] == holes[0] == K.key_of([1, 1, 3], {(0, 1): 1, (1, 2): 2})[0]
    assert holes[1][0] == holes[1][3] == 0 and [holes[1][i] for i in (1, 2, 4)] == plain[1]
    assert K.key_of_rows([1, 1, 3], [1, 5, 2])[0] == plain[0]
    # disconnected decodings still have a key, and it sees the pieces
    assert K.key_of([1, 1, 3, 3], {(0, 1): 1, (1, 2): 1})[0] != K.key_of([1, 1, 3, 3], {(0, 1): 1, (2, 3): 1})[0]
    # atoms the refinement cannot tell apart share a colour
    colours = K.key_of([1] * 6, {(i, (i + 1) % 6): 4 for i in range(6)})[1]
    assert len(set(colours)) == 1


def test_no_key_is_shared_by_different_molecules_of_the_corpus(corpus):
    cls_of_key = {}
    for m, c, name in zip(corpus['keyed'], corpus['classes'], corpus['names']):
        assert cls_of_key.setdefault(m['key'], c) == c, name
    assert len(cls_of_key) == max(corpus['classes']) + 1


def test_unique_molecules_is_the_partition_networkx_finds(corpus):
    want = corpus['classes']
    first = [want.index(c) for c in range(max(want) + 1)]
    # without keys or colours; with the restated ones; with every key and every colour forced to one value
    forced = [dict(m, key=7, atom_colour=np.zeros(len(m['element']), dtype=np.uint64)) for m in corpus['mols']]
    for mols in (corpus['mols'], corpus['keyed'], forced):
        reps, class_of = M.unique_molecules(mols)
        assert class_of == want
        assert len(reps) == len(first) and all(reps[k] is mols[i] for k, i in enumerate(first))
    # same_molecule pair by pair on the frozen pairs, either argument order, keyed against unkeyed included
    for a, b in corpus['iso_pairs']:
        assert M.same_molecule(corpus['mols'][a], forced[b]) and M.same_molecule(corpus['keyed'][b], corpus['keyed'][a])
    for a, b in corpus['near_pairs']:
        assert M.same_molecule(forced[a], forced[b]) == (want[a] == want[b]) == M.same_molecule(corpus['keyed'][b], corpus['mols'][a])


def test_same_molecule_small_cases():
    ethanol = K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 1})
    renumbered = K.mol_from([3, 1, 1], {(0, 1): 1, (1, 2): 1})
    ether = K.mol_from([1, 3, 1], {(0, 1): 1, (1, 2): 1})
    assert M.same_molecule(ethanol, renumbered) and not M.same_molecule(ethanol, ether)
    assert not M.same_molecule(ethanol, K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 2}))
    assert not M.same_molecule(ethanol, K.mol_from([1, 1, 3, 3], {(0, 1): 1, (1, 2): 1}))
    empty = K.mol_from([], {})
    assert M.same_molecule(empty, empty) and not M.same_molecule(empty, ethanol)
    # pieces pair off whatever their order; many equal pieces do not blow the search up
    a = K.mol_from([1] * 12 + [1, 3, 1, 1], {(12, 13): 1, (14, 15): 2})
    b = K.mol_from([1, 1, 3, 1] + [1] * 12, {(0, 1): 2, (2, 3): 1})
    c = K.mol_from([1, 1, 3, 1] + [1] * 12, {(0, 1): 1, (2, 3): 2})
    assert M.same_molecule(a, b) and not M.same_molecule(a, c)
    # a keyed and an unkeyed copy are still one class
    assert M.unique_molecules([K.with_key(ethanol), renumbered, ether, K.with_key(renumbered)])[1] == [0, 0, 1, 0]
    with pytest.raises(ValueError):
        M.same_molecule(dict(ethanol, atom_colour=np.zeros(2, dtype=np.uint64)), dict(ethanol, atom_colour=np.zeros(3, dtype=np.uint64)))


def test_write_sdf_key_item(tmp_path):
    from test_molecule_host import ETHANOL, ETHANOL_BLOCK
    plain, keyed = tmp_path / 'plain.sdf', tmp_path / 'keyed.sdf'
    M.write_sdf(str(plain), [ETHANOL, ETHANOL], names=['ethanol', 'ethanol'])
    assert plain.read_text() == (ETHANOL_BLOCK + '$$$$\n') * 2          # without a key: the text as it always was
    M.write_sdf(str(keyed), [dict(ETHANOL, key=0xE220A8397B1DCDAF), dict(ETHANOL, key=0x1F), ETHANOL], names=['ethanol'] * 3)
    assert keyed.read_text() == (ETHANOL_BLOCK + '> <PHOREGEN_KEY>\ne220a8397b1dcdaf\n\n$$$$\n'
                                 + ETHANOL_BLOCK + '> <PHOREGEN_KEY>\n000000000000001f\n\n$$$$\n' + ETHANOL_BLOCK + '$$$$\n')
    assert M.mol_block(dict(ETHANOL, key=5), 'ethanol') == ETHANOL_BLOCK
    # a key that came over as a signed 64-bit pattern is written as the unsigned one
    M.write_sdf(str(keyed), [dict(ETHANOL, key=-1)], names=['ethanol'])
    assert 'ffffffffffffffff\n' in keyed.read_text()


class _Rota:
    """Stand-in for the network: `.sample` returns the next n molecules of a fixed rota, already assembled (`assemble` is stubbed)."""

    def __init__(self, rota):
        self.rota, self.i, self.calls = rota, 0, []

    def sample(self, data, n, device, **kw):
        assert kw.pop('return_traj') is False
        self.calls.append((n, kw))
        out = [dict(self.rota[(self.i + j) % len(self.rota)]) for j in range(n)]
        self.i += n
        return out


def test_sample_valid_unique_loop(monkeypatch):
    asked = []

    def assemble(res, keys=False):
        asked.append(keys)
        return res if keys else [{k: v for k, v in m.items() if k not in ('key', 'atom_colour')} for m in res]
    monkeypatch.setattr(M, 'assemble', assemble)
    a = K.with_key(K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 1}))
    a2 = K.with_key(K.mol_from([3, 1, 1], {(0, 1): 1, (1, 2): 1}))      # a, renumbered
    b = K.with_key(K.mol_from([1, 3, 1], {(0, 1): 1, (1, 2): 1}))
    c = K.with_key(K.mol_from([1, 1, 2], {(0, 1): 1, (1, 2): 1}))
    d = K.with_key(K.mol_from([1, 1, 7], {(0, 1): 1, (1, 2): 1}))
    bad = dict(K.with_key(K.mol_from([1, 1, 3], {(0, 1): 1})), valid=False, status=M.STATUS_DISCONNECTED)
    dbl = _Rota([a, a2, bad, b, a, c, b, d])
    out = M.sample_valid(dbl, None, num_samples=4, batch_size=3, unique=True, seed_marker=1)
    # by hand: draw 3 (a a2 bad) -> finished a; 3 (b a c) -> a b c; 1 (b) -> repeat; 1 (d) -> a b c d
    assert [n for n, _ in dbl.calls] == [3, 3, 1, 1] and out['n_calls'] == 4 and asked == [True] * 4
    assert all(kw == {'seed_marker': 1} for _, kw in dbl.calls)
    assert [m['key'] for m in out['finished']] == [a['key'], b['key'], c['key'], d['key']]
    assert [m['key'] for m in out['duplicates']] == [a['key']] * 2 + [b['key']]
    assert [m['status'] for m in out['failed']] == [M.STATUS_DISCONNECTED]
    assert set(out) == {'finished', 'failed', 'duplicates', 'n_calls'}
    fin = out['finished']
    assert not any(M.same_molecule(fin[i], fin[j]) for i in range(len(fin)) for j in range(i))
    # a key shared by different molecules does not make them repeats: the exact comparison decides
    clash = _Rota([dict(a, key=1), dict(b, key=1), dict(a2, key=1)])
    out = M.sample_valid(clash, None, num_samples=3, batch_size=3, unique=True, max_failed_factor=1)
    assert len(out['finished']) == 2 and len(out['duplicates']) == 4 and [n for n, _ in clash.calls] == [3, 1, 1, 1]
    # a model that only ever repeats itself: draws of 2, then of 1; the check before a draw first sees more than 3 * 2 repeats
    # with 7 of them, after 7 draws
    stuck = _Rota([a, a2])
    out = M.sample_valid(stuck, None, num_samples=2, batch_size=4, unique=True)
    assert len(out['finished']) == 1 and out['failed'] == [] and len(out['duplicates']) == 7
    assert [n for n, _ in stuck.calls] == [2] + [1] * 6 and out['n_calls'] == 7
    # unique=False: the loop and the dict it returns are the previous ones
    asked.clear()
    plain = _Rota([a, a2, bad, b])
    out = M.sample_valid(plain, None, num_samples=3, batch_size=4)
    assert set(out) == {'finished', 'failed', 'n_calls'} and asked == [False, False] and [n for n, _ in plain.calls] == [3, 1]
    assert len(out['finished']) == 3 and len(out['failed']) == 1 and not any('key' in m for m in out['finished'])


def test_duplicate_groups_on_the_host_device():
    keys = torch.tensor([5, -3, 5, 7, -3, -3, 2 ** 63 - 1, 5])
    first, counts, group = M.duplicate_groups(keys)
    census = {}
    for i, k in enumerate(keys.tolist()):
        census.setdefault(k, []).append(i)
    assert first.tolist() == [v[0] for v in census.values()] and counts.tolist() == [len(v) for v in census.values()]
    assert group.tolist() == [list(census).index(k) for k in keys.tolist()]
    assert all(t.numel() == 0 for t in M.duplicate_groups(torch.zeros(0, dtype=torch.long)))


def test_molecule_keys_needs_the_device():
    sc = M.Screen(status=torch.zeros(1, 1, dtype=torch.int32), counts=torch.zeros(1, 1, 4, dtype=torch.int32),
                  valid=torch.ones(1, 1, dtype=torch.bool), cls=torch.zeros(1, 2, dtype=torch.int8),
                  compact=torch.zeros(1, 2, dtype=torch.int16), valence2=torch.zeros(1, 2, dtype=torch.uint8),
                  comp=torch.zeros(1, 2, dtype=torch.int16), order=torch.zeros(1, 1, dtype=torch.int8),
                  lig_off=torch.tensor([0, 2], dtype=torch.int32), bond_off=torch.tensor([0, 2], dtype=torch.int32), num_atoms=[2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.molecule_keys(sc)


def test_binding_declares_the_key():
    lib = hip.load_library()
    header = header_text()
    assert re.search(r'\bint pg_mol_key\s*\(', header)
    assert 'pg_mol_key' in hip.EXPORTS and hasattr(lib, 'pg_mol_key')
    assert len(hip._PROTOS['pg_mol_key'][1]) == 12 == header.split('int pg_mol_key(')[1].split(');')[0].count(',') + 1
    assert hip.ABI_VERSION == 11 == lib.pg_abi_version()
    assert len(hip._PROTOS['pg_mol_screen'][1]) == 22                   # the screen's call is untouched
    assert 'mol_key.hip' in open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert '%016x' % M.KEY_EMPTY in header.lower()
    # argument errors are refused before any launch, without a GPU: oversize and negative sizes
    assert lib.pg_mol_key(None, None, None, None, 1, 1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1, None, None, None) != 0
    assert b'PG_MOL_MAX_ATOMS' in lib.pg_last_error()
    assert lib.pg_mol_key(None, None, None, None, 1, 1, 4, 12, -1, None, None, None) != 0 and b'pg_mol_key' in lib.pg_last_error()
    assert lib.pg_mol_key(None, None, None, None, 0, 1, 0, 0, 0, None, None, None) == 0
