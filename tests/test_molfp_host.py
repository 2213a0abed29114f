"""No GPU needed: the fingerprints and the similarity of sets of them (DESIGN.md 2.9 "Fingerprints and similarity") -- the plain
restatement (tests/fp_reference.py) on the frozen identity corpus and by hand, the host/device core (csrc/fp_core.h) as a host
program under ASan / UBSan against the restatement with `==`, the binding, and the host logic of phoregen_amd.similarity and
phoregen_amd.molecule."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

import fp_reference as P
from mol_support import arg_count, build_host_check, cycle, header_macro, header_text
import molkey_reference as K
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import similarity as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')
NAMES = ('pg_mol_fp', 'pg_fp_tanimoto', 'pg_fp_nearest', 'pg_fp_maxmin')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return build_host_check('fp_host_check', tmp_path_factory.mktemp('fp_host'))


def test_constants():
    assert M.FP_BITS == 2048 and M.FP_WORDS == 32 and M.FP_MAX_RADIUS == 4 and M.FP_RADIUS == 2
    for name, v in (('PG_FP_BITS', M.FP_BITS), ('PG_FP_WORDS', M.FP_WORDS), ('PG_FP_MAX_RADIUS', M.FP_MAX_RADIUS),
                    ('PG_FP_TILE_A', S.TILE_A), ('PG_FP_TILE_B', S.TILE_B)):
        assert header_macro(name) == str(v), name
    assert 'not RDKit' in M.fingerprints.__doc__.replace('NOT', 'not')


# ---- the corpus, judged by the restatement alone ---------------------------------------------------------------------------------
def test_corpus_conditions():
    sets, iso, near, mat = P.corpus_sets()
    mols = K.corpus()[0]
    assert len(sets) == 413 and min(map(len, sets)) == 3 and max(map(len, sets)) == 101
    assert len(iso) == 230 and all(sets[a] == sets[b] for a, b in iso)
    graphs = {i: K.nx_graph(mols[i]) for pair in near for i in pair}
    apart = [(a, b) for a, b in near if not K.nx_same(graphs[a], graphs[b])]
    assert len(apart) == 133 and not any(mat[a, b] == np.float32(1.0) for a, b in apart)
    assert min(mat[a, b] for a, b in apart) == np.float32(1.0) / np.float32(11.0)
    # the ties that make the lowest-index rules testable
    assert len(np.unique(mat)) >= 1000
    assert P.nearest_ties(mat, same=True) >= 100
    assert P.maxmin(mat, 20, 0)[2] >= 10
    assert (mat == mat.T).all() and (np.diag(mat) == 1).all()


def test_renumbering_leaves_the_fingerprint_unchanged():
    rng = np.random.default_rng(77)
    sets = P.corpus_sets()[0]
    for m, want in zip(K.corpus()[0], sets):
        bi, bt = np.asarray(m['bond_index']).reshape(2, -1), np.asarray(m['bond_type']).reshape(-1)
        classes = [K.ATOM_TYPES.index(int(z)) for z in m['element']]
        bonds = {(int(a), int(b)): int(t) for a, b, t in zip(bi[0], bi[1], bt)}
        c2, b2 = K.permuted(classes, bonds, rng.permutation(len(classes)).tolist())
        assert P.bit_set(c2, b2) == want


def test_hand_cases():
    assert P.bit_set([], {}) == set() and P.words_of(set()) == [0] * M.FP_WORDS
    assert P.bits_of_rows([], []) == set() and P.bits_of_rows([11, -1], [1]) == set()
    # dropped atoms, their position, bonds to them and class-5 rows have no influence
    want = P.bit_set([1, 1, 3], {(0, 1): 1, (1, 2): 2})
    assert P.bits_of_rows([1, 1, 3], [1, 0, 2]) == want
    assert P.bits_of_rows([11, 1, 1, 3], [1, 2, 4, 1, 0, 2]) == want               # a dropped atom first, with bonds to it
    assert P.bits_of_rows([1, 11, 1, 3], [3, 1, 0, 1, 1, 2]) == want               # ... in the middle
    assert P.bits_of_rows([1, 1, 3, -1], [1, 0, 4, 2, 4, 4]) == want               # ... last
    assert P.bits_of_rows([1, 1, 3], [1, 5, 2]) == want                            # an absorbing row is no bond
    assert P.bits_of_rows([1, 1, 3], [1, 1, 2]) != want
    # the radius-r bits are a subset of the radius-(r + 1) bits; radius 0 sets at most one bit per distinct atom word
    for name, classes, bonds in K.named_bases():
        levels = [P.bit_set(classes, bonds, r) for r in range(M.FP_MAX_RADIUS + 1)]
        assert all(a <= b for a, b in zip(levels, levels[1:])), name
        assert len(levels[0]) <= len(set(P.identifiers(classes, bonds, 0)[0])), name
    benzene, cyclohexane = P.bit_set([1] * 6, cycle(6, 4)), P.bit_set([1] * 6, cycle(6, 1))
    assert len(P.bit_set([1] * 6, cycle(6, 4), 0)) == 1 and len(benzene) == 3      # one environment per radius
    kekule = {p: 1 + (i % 2) for i, p in enumerate([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5)])}
    assert P.bit_set([1] * 6, kekule) != benzene != cyclohexane
    # a disconnected graph has one fingerprint: the union of its parts' bits
    assert P.bit_set([1, 1, 3, 3], {(0, 1): 1}) == P.bit_set([1, 1], {(0, 1): 1}) | P.bit_set([3], {})
    with pytest.raises(AssertionError):
        P.bit_set([1], {}, M.FP_MAX_RADIUS + 1)
    # similarity by hand
    assert P.similarity(set(), set()) == 1 and P.similarity({1}, set()) == 0 and P.similarity({1, 2, 3}, {2, 3, 4}) == np.float32(0.5)
    assert P.similarity(set(range(1, 4)), set(range(3))) == np.float32(2) / np.float32(4)
    mat = P.matrix([{1}, {1}, {1, 2}, set()], [{1}, {1}, {1, 2}, set()])
    sim, idx, tot = P.nearest(mat, same=True)
    assert sim.tolist() == [1, 1, 0.5, 0] and idx.tolist() == [1, 0, 0, 0] and tot.tolist() == [1.5, 1.5, 1.0, 0.0]
    assert P.nearest(mat[:1, :1], same=True)[0].tolist() == [-1] and P.nearest(mat[:1, :1], same=True)[1].tolist() == [-1]
    picked, psim, tied = P.maxmin(mat, 4, 0)
    assert picked == [0, 3, 2, 1] and psim.tolist() == [-1, 0, 0.5, 1] and tied == 0      # the duplicate of row 0 comes last


# ---- the core under the host sanitizers ------------------------------------------------------------------------------------------
@needs_gxx
def test_core_on_the_host_under_sanitizers(exe, tmp_path):
    rng = np.random.default_rng(41)
    ids = [int(v) for v in rng.integers(0, 2 ** 64, 2000, dtype=np.uint64)] + [0, P.M64, 2047, 2048, 1 << 63]
    got = open(P.run_host_check(exe, 'bit', tmp_path, ['%x' % v for v in ids])).read().split('\n')
    for v, line in zip(ids, got):
        b = v & (M.FP_BITS - 1)
        assert line == '%d %d %x' % (b, b >> 6, 1 << (b & 63)), hex(v)
        assert P.words_of({b})[b >> 6] == 1 << (b & 63)
    # the Tanimoto value of every (c, u)
    got = np.fromfile(P.run_host_check(exe, 'tanimoto', tmp_path), dtype=np.uint32)
    want = [np.ones(1, dtype=np.float32)] + [np.arange(u + 1, dtype=np.float32) / np.float32(u) for u in range(1, M.FP_BITS + 1)]
    assert np.array_equal(got, np.concatenate(want).view(np.uint32))
    # the packed (sim, index) order, both senses, on sorted random pairs with planted ties
    sims = np.concatenate([rng.integers(0, 2049, 600).astype(np.float32) / rng.integers(1, 2049, 600).astype(np.float32),
                           np.array([0, 1, 0.5, 0.5, 0.5], dtype=np.float32)])
    sims = np.minimum(sims, np.float32(1)).astype(np.float32)
    index = [int(v) for v in rng.integers(0, 2 ** 31, sims.size)]
    index[-3:] = [7, 2 ** 31 - 1, 0]
    pairs = sorted(zip(sims.tolist(), index))                         # lexicographic (sim, index)
    bits = [int(np.float32(s).view(np.uint32)) for s, _ in pairs]
    got = [ln.split() for ln in open(P.run_host_check(exe, 'pack', tmp_path, ['%x %d' % (b, i) for b, (_, i) in zip(bits, pairs)])).read().split('\n') if ln]
    assert got[-1] == ['-1', '%x' % int(np.float32(-1).view(np.uint32))]
    lo, hi = [int(g[0], 16) for g in got[:-1]], [int(g[3], 16) for g in got[:-1]]
    assert lo == sorted(lo) and len(set(lo)) == len(set(pairs))       # MaxMin: the unsigned minimum is the lowest (sim, index)
    by_hi = sorted(range(len(pairs)), key=lambda k: hi[k], reverse=True)
    assert [pairs[k] for k in by_hi] == sorted(pairs, key=lambda p: (-p[0], p[1]))       # nearest: the maximum is the highest sim, lowest index
    assert min(hi) > 0
    for g, b, (_, i) in zip(got, bits, pairs):
        assert (int(g[1]), int(g[2], 16), int(g[4]), int(g[5], 16)) == (i, b, i, b)
    # the tile and row arithmetic for every na, nb in 0 .. 3 tile + 1
    cases = [(na, nb, t) for na in range(3 * S.TILE_A + 2) for nb in list(range(0, 3 * S.TILE_B + 2)) + [5000] for t in (1, 3)]
    cases += [(na, nb, 2048) for na in (0, 1, 3, S.TILE_A, S.TILE_A + 1, 102400) for nb in (0, 1, 2 * S.TILE_B + 1, 102400, 2 ** 31 - 1)]
    cases += [(2 ** 31 - 1, 2 ** 31 - 1, 1)]
    got = open(P.run_host_check(exe, 'tiles', tmp_path, ['%d %d %d' % c for c in cases])).read().split('\n')
    assert got[0].split() == [str(v) for v in (S.TILE_A, S.TILE_B, M.FP_WORDS, M.FP_MAX_RADIUS)]
    for (na, nb, target), line in zip(cases, got[1:]):
        v = [int(x) for x in line.split()]
        ta, tb, runs = P.split_runs(na, nb, target, S.TILE_A, S.TILE_B)
        assert v[:3] == [ta, tb, len(runs)], (na, nb, target)
        assert list(zip(v[4:4 + 2 * len(runs):2], v[5:5 + 2 * len(runs):2])) == runs, (na, nb, target)
        # by property too: the runs cover 0 .. nb in order, none is empty (unless nb is 0), every cut is on a tile
        assert runs[0][0] == 0 and runs[-1][1] == nb and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        assert all(j0 % S.TILE_B == 0 and (j1 > j0 or nb == 0) for j0, j1 in runs)
        if na <= 3 * S.TILE_A + 1:
            rows = v[4 + 2 * len(runs):-1]
            want_rows = []
            for t in range(ta):
                want_rows += [t * S.TILE_A, t * S.TILE_A + S.TILE_A - 1 if t * S.TILE_A + S.TILE_A - 1 < na else -1]
            assert rows == want_rows, (na, nb)
        assert v[-1] == ((na - 1) * nb + nb - 1 if na and nb else 0)


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_points():
    lib = hip.load_library()
    header = header_text()
    assert lib.pg_abi_version() == 11 == hip.ABI_VERSION
    for name, n_args in zip(NAMES, (13, 6, 9, 9)):
        assert re.search(r'\bint %s\s*\(' % name, header) and name in hip.EXPORTS and hasattr(lib, name)
        assert len(hip._PROTOS[name][1]) == n_args == arg_count(name), name
    makefile = open(os.path.join(ROOT, 'phoregen_amd', 'csrc', 'Makefile')).read()
    assert 'mol_fp.hip' in makefile and 'fp_sim.hip' in makefile and re.search(r'mol_fp\.o.*fp_sim\.o: fp_core\.h', makefile)
    assert re.search(r'mol_fp\.o: mol_common\.h', makefile)
    # one copy of the key's mix, shared by the key and the fingerprint
    csrc = os.path.join(ROOT, 'phoregen_amd', 'csrc')
    assert 'key_mix(unsigned long long x)' in open(os.path.join(csrc, 'mol_common.h')).read()
    for f in ('mol_key.hip', 'mol_fp.hip', 'fp_core.h'):
        assert '0x9E3779B97F4A7C15' not in open(os.path.join(csrc, f)).read(), f


def test_argument_errors_are_refused_without_a_gpu():
    lib = hip.load_library()
    tab = hip.C.cast((hip.C.c_uint64 * 64)(), hip.C.c_void_p)

    def refused(name, *args):
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert name.encode() in lib.pg_last_error(), lib.pg_last_error()
        return lib.pg_last_error()

    def fp_args(B, n_lig, n_bond, max_n, F=1, radius=2, arrays=None):
        return (arrays,) * 4 + (B, F, n_lig, n_bond, max_n, radius, arrays, arrays, None)
    assert b'PG_MOL_MAX_ATOMS' in refused('pg_mol_fp', *fp_args(1, M.MAX_ATOMS + 1, 0, M.MAX_ATOMS + 1, arrays=tab))
    for bad in (fp_args(1, 4, 12, -1), fp_args(-1, 4, 12, 4), fp_args(1, -4, 12, 4), fp_args(1, 4, -12, 4), fp_args(1, 4, 12, 4, F=-1),
                fp_args(1, 4, 11, 4), fp_args(1, 4, 12, 4)):
        refused('pg_mol_fp', *bad)
    for radius in (-1, M.FP_MAX_RADIUS + 1):
        assert b'radius' in refused('pg_mol_fp', *fp_args(1, 4, 12, 4, radius=radius, arrays=tab))
        assert b'radius' in refused('pg_mol_fp', *fp_args(0, 0, 0, 0, radius=radius))
    assert lib.pg_mol_fp(*fp_args(0, 0, 0, 0)) == 0 and lib.pg_mol_fp(*fp_args(3, 4, 12, 4, F=0)) == 0
    # the set kernels: negative sizes, null pointers with a positive size, a matrix above 2^31 - 1 elements
    for bad in ((tab, -1, tab, 1, tab, None), (tab, 1, tab, -1, tab, None), (None, 1, tab, 1, tab, None), (tab, 1, None, 1, tab, None),
                (tab, 1, tab, 1, None, None), (tab, 65536, tab, 32768, tab, None)):
        refused('pg_fp_tanimoto', *bad)
    assert lib.pg_fp_tanimoto(None, 0, tab, 5, None, None) == 0 and lib.pg_fp_tanimoto(tab, 5, None, 0, None, None) == 0
    for bad in ((tab, -1, tab, 1, 0, tab, tab, tab, None), (tab, 1, tab, -1, 0, tab, tab, tab, None), (None, 1, tab, 1, 0, tab, tab, tab, None),
                (tab, 1, None, 1, 0, tab, tab, tab, None), (tab, 1, tab, 1, 0, None, tab, tab, None), (tab, 1, tab, 1, 0, tab, None, tab, None),
                (tab, 1, tab, 1, 0, tab, tab, None, None), (tab, 2, tab, 1, 1, tab, tab, tab, None)):
        refused('pg_fp_nearest', *bad)
    assert lib.pg_fp_nearest(None, 0, tab, 5, 0, None, None, None, None) == 0
    for bad in ((tab, 3, 4, 0, tab, tab, tab, tab, None), (tab, 3, -1, 0, tab, tab, tab, tab, None), (tab, 3, 2, 3, tab, tab, tab, tab, None),
                (tab, 3, 2, -1, tab, tab, tab, tab, None), (tab, -1, 0, 0, tab, tab, tab, tab, None), (None, 3, 2, 0, tab, tab, tab, tab, None),
                (tab, 3, 2, 0, None, tab, tab, tab, None), (tab, 3, 2, 0, tab, None, tab, tab, None), (tab, 3, 2, 0, tab, tab, None, tab, None),
                (tab, 3, 2, 0, tab, tab, tab, None, None)):
        refused('pg_fp_maxmin', *bad)
    assert lib.pg_fp_maxmin(None, 0, 0, 0, None, None, None, None, None) == 0 and lib.pg_fp_maxmin(tab, 3, 0, 1, None, None, None, None, None) == 0


# ---- host logic ------------------------------------------------------------------------------------------------------------------------
def _with_fp(m, radius=M.FP_RADIUS):
    bits = P.bits_of_mol(m, radius)
    return dict(m, fingerprint=np.array(P.words_of(bits), dtype=np.uint64), fp_bits=len(bits), fp_radius=radius)


def test_stack_and_diversity_arithmetic():
    mols = [_with_fp(K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 1})), _with_fp(K.mol_from([1] * 6, cycle(6, 4)))]
    rows = S.stack(mols, 'cpu')
    assert rows.shape == (2, M.FP_WORDS) and rows.dtype == torch.int64
    assert np.array_equal(rows.numpy().view(np.uint64), P.rows_array([P.bits_of_mol(m) for m in mols]))
    assert P.sets_of_array(rows.numpy().view(np.uint64)) == [P.bits_of_mol(m) for m in mols]
    assert S.stack([], 'cpu').shape == (0, M.FP_WORDS)
    with pytest.raises(ValueError, match='fingerprint'):
        S.stack([K.mol_from([1], {})], 'cpu')
    assert np.isnan(S._diversity(0.0, 0)) and np.isnan(S._diversity(0.0, 1))
    assert S._diversity(0.5, 2) == 0.75 and S._diversity(6.0, 3) == 0.0
    mat = P.matrix([{1}, {1, 2}], [{1}, {1, 2}])
    assert P.diversity(mat) == 0.5 == S._diversity(P.nearest(mat, same=True)[2].sum(), 2)
    assert S.TILE_A % 64 == 0 and S.TILE_B > 0


def test_no_cpu_fallback_and_argument_checks():
    rows = S.stack([_with_fp(K.mol_from([1, 1], {(0, 1): 1}))] * 3, 'cpu')
    for call in (lambda: S.tanimoto(rows), lambda: S.nearest(rows), lambda: S.nearest(rows, rows), lambda: S.internal_diversity(rows),
                 lambda: S.maxmin_pick(rows, 2)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    for bad in (rows.int(), rows[:, :31], rows.reshape(-1), rows.numpy()):
        with pytest.raises(ValueError, match='int64 tensor'):
            S.tanimoto(bad)
    import mol_reference as R
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    sc_like = type('Sc', (), {'cls': torch.zeros(1, 2, dtype=torch.int8), 'status': torch.zeros(1, 1, dtype=torch.int32)})()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.fingerprints(sc_like)
    for radius in (-1, 5, 2.0, True):
        with pytest.raises(ValueError, match='radius'):
            M.fingerprints(sc_like, radius)
    with pytest.raises(ValueError, match='radius'):
        M.sample_valid(None, None, 1, fingerprints=9)
    with pytest.raises(ValueError, match='fingerprints='):
        M.assemble({'pred': [node, pos, edge], 'traj': [None] * 3, 'lig_info': [torch.tensor([2])]}, fingerprints=object())


def test_sdf_item_and_unchanged_text(tmp_path):
    plain = K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 1})
    mol = _with_fp(plain, 3)
    a, b = tmp_path / 'a.sdf', tmp_path / 'b.sdf'
    M.write_sdf(str(a), [mol, plain], names=['x', 'y'])
    M.write_sdf(str(b), [plain, plain], names=['x', 'y'])
    text = a.read_text()
    assert text.count('> <PHOREGEN_FINGERPRINT>') == 1
    item = text.split('> <PHOREGEN_FINGERPRINT>\n')[1].split('\n\n')[0].split('\n')
    assert len(item) == 2 and len(item[0]) == 512 and item[1] == 'radius 3'
    words = [int(item[0][16 * k:16 * k + 16], 16) for k in range(M.FP_WORDS)]
    assert words == P.words_of(P.bits_of_mol(plain, 3)) == mol['fingerprint'].tolist()
    assert text.replace('> <PHOREGEN_FINGERPRINT>\n%s\nradius 3\n\n' % item[0], '') == b.read_text()     # otherwise as it always was
    with pytest.raises(ValueError, match='words'):
        M.write_sdf(str(a), [dict(mol, fingerprint=mol['fingerprint'][:5])])


class _Model:
    def __init__(self):
        self.calls = 0

    def sample(self, data, n, device, **kw):
        self.calls += 1
        return [dict(K.mol_from([1, 1, 3], {(0, 1): 1, (1, 2): 1})) for _ in range(n)]


def test_sample_valid_passes_fingerprints_through(monkeypatch):
    seen = []

    def assemble(res, keys=False, **kw):
        seen.append(dict(kw))
        return res
    monkeypatch.setattr(M, 'assemble', assemble)
    monkeypatch.setattr(M, '_screen', lambda res, frames: 'screen-of-%d' % len(res))
    monkeypatch.setattr(M, '_fingerprints', lambda sc, radius: ('fps', sc, radius))
    out = M.sample_valid(_Model(), None, num_samples=3, batch_size=2, fingerprints=True)
    assert len(out['finished']) == 3 and seen == [{'fingerprints': ('fps', 'screen-of-2', M.FP_RADIUS)}, {'fingerprints': ('fps', 'screen-of-1', M.FP_RADIUS)}]
    del seen[:]
    M.sample_valid(_Model(), None, num_samples=1, fingerprints=0)
    assert seen == [{'fingerprints': ('fps', 'screen-of-1', 0)}]
    del seen[:]

    def two_arguments(res, keys=False):                                # unset: the keyword is not passed at all
        seen.append(keys)
        return res
    monkeypatch.setattr(M, 'assemble', two_arguments)
    M.sample_valid(_Model(), None, num_samples=1)
    M.sample_valid(_Model(), None, num_samples=1, fingerprints=None)
    assert seen == [False, False]
