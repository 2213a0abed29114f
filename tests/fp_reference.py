"""Plain restatement of the fingerprints and the similarity of sets of them (DESIGN.md 2.9 "Fingerprints and similarity";
phoregen_amd/molecule.py, phoregen_amd/similarity.py, csrc/mol_fp.hip, csrc/fp_sim.hip) for the tests, written from the text: Python
ints masked to 64 bits, sets of bit positions, np.float32 division, no device code.  It shares nothing with the kernels but the
named constants of phoregen_amd.molecule.  Also here: the calls of the host program tools/fp_host_check.cpp."""
import os

import numpy as np

import molkey_reference as K
from mol_support import M64, compact_bonds, run_program
from phoregen_amd import molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

mix = K.mix


# ---- the fingerprint ------------------------------------------------------------------------------------------------------------
def identifiers(classes, bonds, radius):
    """classes: atom class 0..10 of every (kept) atom; bonds {(a, b): order 1..4}, every pair once.  [[id_r[i] for i] for r]."""
    assert 0 <= radius <= M.FP_MAX_RADIUS
    n = len(classes)
    nbr = [[] for _ in range(n)]
    degree, valence2, aromatic = [0] * n, [0] * n, [0] * n
    for (a, b), t in bonds.items():
        assert a != b and 1 <= t <= 4 and (b, a) not in bonds
        nbr[a].append((b, t)), nbr[b].append((a, t))
        for x in (a, b):
            degree[x] += 1
            valence2[x] += 3 if t == 4 else 2 * t
            aromatic[x] += t == 4
    ids = [[mix(classes[i] | valence2[i] << 8 | degree[i] << 24 | aromatic[i] << 32) for i in range(n)]]
    for _ in range(radius):
        prev, nxt = ids[-1], []
        for i in range(n):
            s = 0
            for j, t in nbr[i]:
                s = (s + mix(prev[j] ^ mix(t))) & M64
            nxt.append(mix(prev[i] ^ mix(s)))
        ids.append(nxt)
    return ids


def bit_set(classes, bonds, radius=M.FP_RADIUS):
    """The set of bit positions of the molecule's fingerprint."""
    return {v & (M.FP_BITS - 1) for level in identifiers(classes, bonds, radius) for v in level}


def words_of(bits):
    """FP_WORDS unsigned ints: bit b is bit b & 63 of word b >> 6."""
    words = [0] * M.FP_WORDS
    for b in bits:
        words[b >> 6] |= 1 << (b & 63)
    return words


def bits_of_rows(cls, order, radius=M.FP_RADIUS):
    """One graph as the screen wrote it (molkey_reference.key_of_rows' conventions): cls int8 [n] (-1 = dropped), order int8 for the
    pairs a < b in row-major order.  The set of bit positions."""
    kept, bonds = compact_bonds(cls, order)
    return bit_set([int(cls[i]) for i in kept], bonds, radius)


def bits_of_mol(m, radius=M.FP_RADIUS):
    """An assembled molecule ('element', 'bond_index', 'bond_type'): the set of bit positions."""
    bi, bt = np.asarray(m['bond_index']).reshape(2, -1), np.asarray(m['bond_type']).reshape(-1)
    return bit_set([ATOM_TYPES.index(int(z)) for z in m['element']],
                   {(int(a), int(b)): int(t) for a, b, t in zip(bi[0], bi[1], bt)}, radius)


def rows_array(bit_sets):
    """np.uint64 [n, FP_WORDS] of a list of bit sets."""
    return np.array([words_of(b) for b in bit_sets], dtype=np.uint64).reshape(len(bit_sets), M.FP_WORDS)


def sets_of_array(rows):
    """The bit sets of np.uint64 [n, FP_WORDS]."""
    out = []
    for r in np.asarray(rows).astype(np.uint64).reshape(-1, M.FP_WORDS).tolist():
        out.append({64 * w + k for w, v in enumerate(r) for k in range(64) if v >> k & 1})
    return out


# ---- Tanimoto, nearest, MaxMin ------------------------------------------------------------------------------------------------------
def similarity(x, y):
    """Two bit sets: np.float32(c) / np.float32(u), 1 for two empty ones."""
    c = len(x & y)
    u = len(x) + len(y) - c
    return np.float32(c) / np.float32(u) if u > 0 else np.float32(1.0)


def _as_int(bits):
    v = 0
    for b in bits:
        v |= 1 << b
    return v


def matrix(a, b):
    """np.float32 [na, nb] of two lists of bit sets.  (The sets as 2048-bit Python ints: the same counts, quicker.)"""
    ai, bi = [_as_int(x) for x in a], [_as_int(y) for y in b]
    pa, pb = [len(x) for x in a], [len(y) for y in b]
    c = np.array([[bin(x & y).count('1') for y in bi] for x in ai], dtype=np.int64).reshape(len(a), len(b))
    u = np.array(pa, dtype=np.int64).reshape(-1, 1) + np.array(pb, dtype=np.int64).reshape(1, -1) - c
    with np.errstate(divide='ignore', invalid='ignore'):
        out = c.astype(np.float32) / u.astype(np.float32)
    out[u == 0] = np.float32(1.0)
    return out


def nearest(mat, same=False):
    """From the float32 matrix: (sim float32 [na], index [na], sum float64 [na]); the lowest index among equals; `same`: j = i is left
    out; without a candidate -1, -1, 0."""
    na, nb = mat.shape
    sim, index, total = np.full(na, -1, dtype=np.float32), np.full(na, -1, dtype=np.int64), np.zeros(na, dtype=np.float64)
    for i in range(na):
        row = mat[i].astype(np.float64).tolist()                      # (float32 values as Python floats: the same order, exact)
        cand = [(v, j) for j, v in enumerate(row) if not (same and j == i)]
        if cand:
            best = max(v for v, _ in cand)
            sim[i], index[i] = np.float32(best), min(j for v, j in cand if v == best)
        s = 0.0
        for v, _ in cand:
            s += v
        total[i] = s
    return sim, index, total


def nearest_ties(mat, same=False):
    """Rows whose largest similarity is attained by more than one candidate."""
    n = 0
    for i in range(mat.shape[0]):
        row = [mat[i, j] for j in range(mat.shape[1]) if not (same and j == i)]
        n += bool(row) and row.count(max(row)) > 1
    return n


def maxmin(mat, k, first=0):
    """From the square float32 matrix: (picked [k], pick_sim float32 [k], tied steps)."""
    n = mat.shape[0]
    assert 0 <= k <= n and (n == 0 or 0 <= first < n)
    if k == 0:
        return [], np.zeros(0, dtype=np.float32), 0
    picked, sims, tied = [first], [np.float32(-1.0)], 0
    m = {i: mat[i, first] for i in range(n) if i != first}
    for _ in range(1, k):
        best = min(m.values())
        at = [i for i in sorted(m) if m[i] == best]
        tied += len(at) > 1
        i = at[0]
        picked.append(i), sims.append(best)
        del m[i]
        for j in m:
            m[j] = max(m[j], mat[j, i])
    return picked, np.array(sims, dtype=np.float32), tied


def diversity(mat):
    """1 - (sum over i != j of the float32 values, in float64) / (n (n - 1)); nan below two rows."""
    n = mat.shape[0]
    if n < 2:
        return float('nan')
    return 1.0 - (float(mat.astype(np.float64).sum()) - float(np.trace(mat.astype(np.float64)))) / (n * (n - 1))


_CORPUS = {}


def corpus_sets(radius=M.FP_RADIUS):
    """(bit sets of molkey_reference.corpus(), iso_pairs, near_pairs, the all-pairs float32 matrix), computed once."""
    if radius not in _CORPUS:
        mols, iso, near, _ = K.corpus()
        sets = [bits_of_mol(m, radius) for m in mols]
        _CORPUS[radius] = (sets, iso, near, matrix(sets, sets))
    return _CORPUS[radius]


# ---- the split of a sweep, as DESIGN.md 2.9 states it -------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def split_runs(n_a, n_b, target, tile_a, tile_b):
    """(tiles_a, tiles_b, [(j0, j1) per run])"""
    ta, tb = _ceil(n_a, tile_a), _ceil(n_b, tile_b)
    want = min(max(_ceil(target, ta) if ta else 1, 1), tb)
    if want <= 1:
        return ta, tb, [(0, n_b)]
    per = _ceil(tb, want)
    return ta, tb, [(s * per * tile_b, min((s + 1) * per * tile_b, n_b)) for s in range(_ceil(tb, per))]


# ---- the host program -----------------------------------------------------------------------------------------------------------------
def run_host_check(exe, mode, work_dir, lines=None):
    """Runs one mode; `lines`: the input file's lines.  Returns the output file's path."""
    out = os.path.join(str(work_dir), mode + '.out')
    args = [exe, mode]
    if lines is not None:
        src = os.path.join(str(work_dir), mode + '.in')
        with open(src, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
        args.append(src)
    run_program(*args, out)
    return out
