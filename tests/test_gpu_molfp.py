"""-m gpu: the fingerprint kernel (csrc/mol_fp.hip through phoregen_amd/molecule.py) and the set kernels (csrc/fp_sim.hip through
phoregen_amd/similarity.py) against the plain restatement of tests/fp_reference.py.  Integer work and one correctly rounded division:
every comparison is `==`, except the fp64 row sums, which are held to nb^2 * 2^-53 (exact fp32 terms in [0, 1], added in double in
some order)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fp_reference as P
import mol_reference as R
from helpers import default_model
from mol_support import M64, mol_result as _result, permute_batch as _permute_batch
from phoregen_amd import molecule as M
from phoregen_amd import similarity as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


@pytest.fixture(scope='module')
def corpus():
    """(bit sets, near-miss half as bit sets, the float32 matrix, the set on the device, the near-miss half on the device)"""
    sets, _, near, mat = P.corpus_sets()
    half = [sets[b] for _, b in near]
    return sets, half, mat, _device(sets), _device(half)


def _device(sets):
    return torch.from_numpy(P.rows_array(sets).view(np.int64)).to(DEV)


def _rows(t):
    """[.., 32] int64 on the device -> list of rows of unsigned ints"""
    return [[v & M64 for v in r] for r in t.cpu().reshape(-1, M.FP_WORDS).tolist()]


def _restated(refs, radius):
    sets = [P.bits_of_rows(r['cls'], r['order'], radius) for r in refs]
    return [P.words_of(b) for b in sets], [len(b) for b in sets]


# ---- the fingerprint kernel ------------------------------------------------------------------------------------------------------
def test_kernel_equals_restatement_on_the_ragged_batch():
    node, pos, edge, sizes = R.generate_batch()
    for n in (1, 2, 3, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
    refs = R.screen_batch(node, pos, edge, sizes)
    c = R.census(refs)
    assert c['HAD_MASKED_ATOM'] >= 1 and c['NO_ATOMS'] >= 1 and c['HAD_ABSORBING_BOND'] >= 1 and c['DISCONNECTED'] >= 10, c
    sc = M.screen(_result(node, pos, edge, sizes))
    seen = []
    for radius in (0, 2, 4):
        want_rows, want_bits = _restated(refs, radius)
        assert want_bits.count(0) == c['NO_ATOMS']
        fps = M.fingerprints(sc, radius)
        torch.cuda.synchronize()
        assert fps.fp.shape == (1, len(sizes), M.FP_WORDS) and fps.fp.dtype == torch.int64 and fps.radius == radius
        assert fps.bits.shape == (1, len(sizes)) and fps.bits.dtype == torch.int32
        got = _rows(fps.fp)
        for g, (a, b) in enumerate(zip(got, want_rows)):
            assert a == b, (radius, g, sizes[g])
        assert fps.bits.reshape(-1).tolist() == want_bits
        # the outputs do not depend on what their buffers held: a call into recycled memory agrees
        del fps
        torch.full((len(sizes) * M.FP_WORDS,), -1, dtype=torch.int64, device=DEV)
        again = M.fingerprints(sc, radius)
        assert _rows(again.fp) == want_rows and again.bits.reshape(-1).tolist() == want_bits
        seen.append(want_rows)
    assert seen[0] != seen[1] != seen[2]
    assert M.fingerprints(sc).radius == M.FP_RADIUS and _rows(M.fingerprints(sc).fp) == seen[1]


def test_renumbered_batch_has_the_same_rows():
    node, pos, edge, sizes = R.generate_batch()
    node2, pos2, edge2, _ = _permute_batch(node, pos, edge, sizes, seed=5)
    assert not torch.equal(node, node2)
    fps = M.fingerprints(M.screen(_result(node, pos, edge, sizes)))
    fps2 = M.fingerprints(M.screen(_result(node2, pos2, edge2, sizes)))
    assert torch.equal(fps.fp, fps2.fp) and torch.equal(fps.bits, fps2.bits)
    # and the permuted batch equals its own restatement, so the agreement is not two equal mistakes
    want_rows, want_bits = _restated(R.screen_batch(node2, pos2, edge2, sizes), M.FP_RADIUS)
    assert _rows(fps2.fp) == want_rows and fps2.bits.reshape(-1).tolist() == want_bits


def test_trajectory_frames_and_strided_views():
    """frames='traj' in one launch == frame by frame; a strided [F, rows, .] view (every second frame) works too."""
    sizes = [5, 17, 64, 3, 30]
    rng = np.random.default_rng(3)
    N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
    node = torch.from_numpy(rng.normal(0, 1, (6, N, 12)).astype(np.float32))
    edge = torch.from_numpy(rng.normal(0, 1, (6, E, 6)).astype(np.float32))
    edge[..., 0] += 2.5                                                # mostly "no bond", else everything is one clique
    pos = torch.from_numpy(rng.normal(0, 3, (6, N, 3)).astype(np.float32))
    full = _result(node[-1], pos[-1], edge[-1], sizes, traj=(node.to(DEV), pos.to(DEV), edge.to(DEV)))
    fps = M.fingerprints(M.screen(full, frames='traj'), 3)
    assert fps.fp.shape == (6, len(sizes), M.FP_WORDS) and fps.bits.shape == (6, len(sizes))
    for f in range(6):
        one = M.fingerprints(M.screen(_result(node[f], pos[f], edge[f], sizes)), 3)
        assert torch.equal(one.fp[0], fps.fp[f]) and torch.equal(one.bits[0], fps.bits[f])
        want_rows, want_bits = _restated(R.screen_batch(node[f], pos[f], edge[f], sizes), 3)
        assert _rows(fps.fp[f]) == want_rows and fps.bits[f].tolist() == want_bits
    assert len({tuple(r) for r in _rows(fps.fp)}) > len(sizes)         # the frames differ
    strided = dict(full, traj=[t[::2] for t in full['traj']])
    assert not strided['traj'][0].is_contiguous()
    fps2 = M.fingerprints(M.screen(strided, frames='traj'), 3)
    assert torch.equal(fps2.fp, fps.fp[::2]) and torch.equal(fps2.bits, fps.bits[::2])


def test_oversize_graph_and_bad_radius_are_refused_before_any_launch():
    from phoregen_amd import hip
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    cls = torch.zeros(1, n, dtype=torch.int8, device=DEV)
    order = torch.zeros(1, h, dtype=torch.int8, device=DEV)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    boff = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    fp = torch.full((1, 1, M.FP_WORDS), 77, dtype=torch.int64, device=DEV)
    bits = torch.full((1, 1), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError) as err:
        M._launch_fp(hip.lib(), cls, order, off, boff, 1, 1, n, 2, fp, bits)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_fp'):
        M._launch_fp(hip.lib(), cls, order, off, boff, 1, 1, -1, 2, fp, bits)
    small = M.screen(_result(*R.scores_from_classes([1, 1, 3], {(0, 1): 1, (1, 2): 1})[:3], [3]))
    for radius in (-1, M.FP_MAX_RADIUS + 1):
        with pytest.raises(RuntimeError, match='radius'):
            M._launch_fp(hip.lib(), small.cls, small.order, small.lig_off, small.bond_off, 1, 1, 3, radius, fp, bits)
    torch.cuda.synchronize()
    assert (fp == 77).all() and (bits == 77).all()
    M._launch_fp(hip.lib(), small.cls, small.order, small.lig_off, small.bond_off, 1, 1, 3, 2, fp, bits)
    assert _rows(fp) == [P.words_of(P.bit_set([1, 1, 3], {(0, 1): 1, (1, 2): 1}))]
    # empty batches return without a launch
    empty = M.fingerprints(M.screen(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])))
    assert empty.fp.shape == (1, 0, M.FP_WORDS) and empty.bits.shape == (1, 0)


# ---- the Tanimoto matrix -------------------------------------------------------------------------------------------------------------
def test_matrix_on_the_prefix_rows_covers_every_fraction():
    """Row k has bits 0 .. k - 1: entry (i, j) is min / max, every reduced fraction c / u with c <= u <= 2048, and (0, 0) -> 1."""
    n = M.FP_BITS + 1
    rows = np.zeros((n, M.FP_WORDS), dtype=np.uint64)
    for k in range(n):
        for w in range(M.FP_WORDS):
            b = min(max(k - 64 * w, 0), 64)
            rows[k, w] = (1 << b) - 1
    got = S.tanimoto(torch.from_numpy(rows.view(np.int64)).to(DEV)).cpu().numpy()
    k = np.arange(n, dtype=np.int64)
    lo, hi = np.minimum(k[:, None], k[None, :]).astype(np.float32), np.maximum(k[:, None], k[None, :]).astype(np.float32)
    with np.errstate(invalid='ignore'):
        want = lo / hi
    want[0, 0] = 1.0
    assert got.dtype == np.float32 and got.shape == (n, n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _random_sets(rng, n):
    """Sparse random bit sets with planted duplicates, empty rows and a full row."""
    sets = [set(int(v) for v in rng.integers(0, M.FP_BITS, int(rng.integers(1, 120)))) for _ in range(n)]
    if n >= 1:
        sets[-1] = set()
    if n >= 3:
        sets[0] = set(range(M.FP_BITS))
    if n >= 5:
        sets[n // 2], sets[1] = set(), set(sets[n - 2])
    return sets


SIZES = sorted({0, 1} | {t + d for t in (S.TILE_A, S.TILE_B) for d in (-1, 0, 1)} | {2 * S.TILE_A + 1, 2 * S.TILE_B + 1})


@pytest.mark.parametrize('na', SIZES)
def test_matrix_on_rectangular_random_sets(na):
    rng = np.random.default_rng(1000 + na)
    a = _random_sets(rng, na)
    a_dev = _device(a)
    for nb in SIZES:
        b = _random_sets(rng, nb)
        if nb >= 7 and na >= 7:
            b[5] = set(a[3])                                           # a row of a planted in b
        got = S.tanimoto(a_dev, _device(b))
        assert got.shape == (na, nb) and got.dtype == torch.float32
        want = P.matrix(a, b)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (na, nb)
    if na:
        assert torch.equal(S.tanimoto(a_dev), S.tanimoto(a_dev, a_dev))


# ---- nearest ---------------------------------------------------------------------------------------------------------------------------
def _check_nearest(got, mat, same):
    sim, index, total = P.nearest(mat, same)
    assert np.array_equal(got.sim.cpu().numpy().view(np.uint32), sim.view(np.uint32))
    assert got.index.dtype == torch.int32 and got.index.cpu().tolist() == index.tolist()
    bound = mat.shape[1] ** 2 * 2.0 ** -53
    err = np.abs(got.sum.cpu().numpy() - total)
    assert got.sum.dtype == torch.float64 and (err <= bound).all(), (err.max(), bound)


def test_nearest_on_the_corpus(corpus):
    sets, half, mat, dev, half_dev = corpus
    assert P.nearest_ties(mat, same=True) >= 100                       # the lowest-index rule is exercised
    _check_nearest(S.nearest(dev), mat, True)
    _check_nearest(S.nearest(dev, dev), mat, False)                    # handed in twice: no exclusion, every row finds itself first
    against = P.matrix(sets, half)
    assert P.nearest_ties(against) >= 5 and P.nearest_ties(against.T.copy()) >= 100     # (the restatement alone: ties are exercised)
    _check_nearest(S.nearest(dev, half_dev), against, False)
    _check_nearest(S.nearest(half_dev, dev), against.T.copy(), False)
    want = P.diversity(mat)
    assert abs(S.internal_diversity(dev) - want) <= 1e-12 and 0.0 < want < 1.0


def test_nearest_edges_and_the_split(corpus):
    sets, _, mat, dev, _ = corpus
    one = S.nearest(dev[:1])
    assert one.sim.tolist() == [-1.0] and one.index.tolist() == [-1] and one.sum.tolist() == [0.0]
    none = S.nearest(dev[:3], dev[:0])
    assert none.sim.tolist() == [-1.0] * 3 and none.index.tolist() == [-1] * 3 and none.sum.tolist() == [0.0] * 3
    empty = S.nearest(dev[:0], dev)
    assert empty.sim.shape == (0,) and empty.index.shape == (0,) and empty.sum.shape == (0,)
    assert np.isnan(S.internal_diversity(dev[:1])) and np.isnan(S.internal_diversity(dev[:0]))
    # few rows against many: b is cut into runs that a second launch combines; sim and index do not depend on the cut
    nb = 2 * S.TILE_B + 1
    assert len(P.split_runs(3, nb, 2048, S.TILE_A, S.TILE_B)[2]) == 3
    _check_nearest(S.nearest(dev[200:203], dev[:nb].contiguous()), mat[200:203, :nb], False)
    _check_nearest(S.nearest(dev[:nb].contiguous()), mat[:nb, :nb], True)
    # ties across the runs: every row of b the same, the lowest index wins
    same_rows = dev[7:8].expand(nb, M.FP_WORDS).contiguous()
    got = S.nearest(dev[:3].contiguous(), same_rows)
    assert got.index.tolist() == [0, 0, 0] and got.sim.tolist() == [float(mat[i, 7]) for i in range(3)]
    for n in (S.TILE_B, S.TILE_B + 1, S.TILE_A - 1, S.TILE_A, S.TILE_A + 1):
        _check_nearest(S.nearest(dev[:n].contiguous()), mat[:n, :n], True)


# ---- MaxMin ----------------------------------------------------------------------------------------------------------------------------
def _check_maxmin(got, mat, k, first):
    picked, sims, _ = P.maxmin(mat, k, first)
    assert got.index.dtype == torch.int32 and got.index.tolist() == picked, (k, first)
    assert np.array_equal(got.sim.cpu().numpy().view(np.uint32), sims.view(np.uint32)), (k, first)


def test_maxmin_on_the_corpus(corpus):
    sets, _, mat, dev, _ = corpus
    n = len(sets)
    assert P.maxmin(mat, 20, 0)[2] >= 10                               # tied steps: the lowest-index rule is exercised
    _check_maxmin(S.maxmin_pick(dev, 20), mat, 20, 0)
    _check_maxmin(S.maxmin_pick(dev, n), mat, n, 0)
    _check_maxmin(S.maxmin_pick(dev, 5, first=n - 1), mat, 5, n - 1)
    zero, one = S.maxmin_pick(dev, 0), S.maxmin_pick(dev, 1, first=3)
    assert zero.index.shape == (0,) and zero.sim.shape == (0,)
    assert one.index.tolist() == [3] and one.sim.tolist() == [-1.0]
    assert S.maxmin_pick(dev[:0], 0).index.shape == (0,)
    for bad in (dict(k=n + 1), dict(k=-1), dict(k=2, first=n), dict(k=2, first=-1)):
        with pytest.raises(ValueError, match='picks from'):
            S.maxmin_pick(dev, **bad)


def test_maxmin_with_every_row_duplicated(corpus):
    sets, _, _, _, _ = corpus
    doubled = [s for s in sets[:40] for _ in range(2)]
    mat = P.matrix(doubled, doubled)
    got = S.maxmin_pick(_device(doubled), len(doubled))
    _check_maxmin(got, mat, len(doubled), 0)
    distinct = len({frozenset(s) for s in doubled})
    assert (got.sim[distinct:] == 1).all() and (got.sim[1:distinct] < 1).all()      # the duplicates come last ...
    tail = got.index[distinct:].tolist()
    assert tail == sorted(tail)                                        # ... lowest index first


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_assemble_with_fingerprints_end_to_end(model):
    from bench import ligphore_workload
    NA = [11, 9, 14, 8]
    w = ligphore_workload(len(NA), seed=11)
    centers = torch.randn(len(NA), 3, generator=torch.Generator().manual_seed(11)) * 2.0
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(NA), centers, rng='device',
                             seed=17, num_steps=10)
    torch.cuda.synchronize()
    fps = M.fingerprints(M.screen(res), 3)
    plain, with_fp = M.assemble(res), M.assemble(res, fingerprints=fps)
    assert len(plain) == len(with_fp) == len(NA)
    for p, k in zip(plain, with_fp):
        assert set(k) == set(p) | {'fingerprint', 'fp_bits', 'fp_radius'}
        for name in p:                                                 # the default output, key for key
            same = torch.equal(p[name], k[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], k[name])
            assert same, name
        want = P.bits_of_mol(k, 3)
        assert k['fingerprint'].dtype == np.uint64 and k['fingerprint'].tolist() == P.words_of(want)
        assert k['fp_bits'] == len(want) and k['fp_radius'] == 3
    keyed = M.assemble(res, keys=True, fingerprints=fps)
    assert [m['fingerprint'].tolist() for m in keyed] == [m['fingerprint'].tolist() for m in with_fp] and 'key' in keyed[0]
    assert torch.equal(S.stack(with_fp, DEV), fps.fp[0])
    both = M.assemble(res, rings=M.rings(res, screen=fps.screen), fingerprints=fps)
    assert [m['fingerprint'].tolist() for m in both] == [m['fingerprint'].tolist() for m in with_fp] and 'rings' in both[0]


def test_sample_cli_writes_the_fingerprint_files(tmp_path):
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    out = tmp_path / 'out'
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--outdir', str(out), '--fingerprints', '--diverse', '2', '--sdf', '--num_steps', '10'],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(out.glob('*.pt'))), weights_only=False)
    (path,) = out.glob('*_fingerprints.npy')
    rows = np.load(str(path))
    assert rows.dtype == np.uint64 and rows.shape == (len(done), M.FP_WORDS)
    assert [r.tolist() for r in rows] == [P.words_of(P.bits_of_mol(m)) for m in done]
    (path,) = out.glob('*_similarity.txt')
    line = path.read_text().split('\n')
    assert line[-1] == '' and len(line) == 2 and len(line[0].split()) == 3 and int(line[0].split()[0]) == len(done)
    (path,) = out.glob('*_diverse.txt')
    picks = [ln.split() for ln in path.read_text().split('\n')[:-1]]
    assert len(picks) == min(2, len(done)) and all(len(p) == 2 for p in picks)
    if picks:
        assert picks[0] == ['0', '-1.000000'] and len({p[0] for p in picks}) == len(picks)
    sdfs = sorted((out / 'sdf_results').glob('*.sdf'), key=lambda p: int(p.stem.rsplit('_', 1)[1]))
    assert len(sdfs) == len(done)
    for p, r in zip(sdfs, rows):
        item = p.read_text().split('> <PHOREGEN_FINGERPRINT>\n')[1].split('\n')
        assert item[0] == ''.join('%016x' % int(v) for v in r) and item[1] == 'radius %d' % M.FP_RADIUS
