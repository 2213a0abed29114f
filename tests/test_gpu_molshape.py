"""-m gpu: the shape kernels (csrc/shape_sim.hip through phoregen_amd/shape.py) against the float64 restatement of
tests/shape_reference.py.

Tolerances, measured on the corpus by the restatement (tests/test_molshape_host.py prints them), nothing tuned against the kernel: the
floor -- the largest relative deviation from float64 of an fp32 evaluation of the same formulas in two term orders -- is 2.25e-6; V and
C are held to 4 x floor = 9.0e-6 relative (an overlap below 1e-30 absolutely against 1e-30), ST and CT to 3 x that = 2.7e-5 absolute;
a combined score to the same plus 2^-23 for its two products and its sum; a row sum to nb^2 2^-53 plus nb times the score tolerance.
Statuses, indices of decided rows and everything the determinism rules promise are compared with `==` on the bits."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mol_reference as R
import shape_reference as SR
from helpers import default_model
from mol_support import batch_from, bits, mol_result
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import shape as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = SR.tables(S.VDW_RADIUS_PM, S.ShapeOptions().colour_radius_pm, S.KAPPA, S.P)
SIZES = sorted({0, 1} | {t + d for t in (S.TILE_A, S.TILE_B) for d in (-1, 0, 1)} | {2 * S.TILE_A + 1, 2 * S.TILE_B + 1})
COMBINE = 2.0 ** -23


def _fake_features(sc, fp):
    """A `Features` that carries the feature bytes alone (and the screen they belong to)."""
    blank = dict.fromkeys(('status', 'counts', 'ok', 'point_dist', 'point_atom', 'point_off', 'point_range', 'point_kind', 'limits', 'kekule', 'rings'))
    return M.Features(atom_fp=fp, screen=sc, **blank)


def _device_set(mols, colour=True, select='all'):
    """The molecules through the sampler's layout, the screen and `shape_set`."""
    graphs = [(np.where(SR.kept(m), m.cls, 11).tolist(), {}, m.pos) for m in mols]
    res = mol_result(*batch_from(graphs))
    sc = M.screen(res)
    fp = torch.from_numpy(np.concatenate([m.fp for m in mols] + [np.zeros(0, dtype=np.uint8)])).to(DEV).reshape(1, -1)
    sel = torch.ones(1, len(mols), dtype=torch.bool, device=DEV) if select == 'all' else select
    return S.shape_set(res, screen=sc, features=_fake_features(sc, fp) if colour else None, select=sel)


@pytest.fixture(scope='module')
def case():
    mols, notes = SR.corpus()
    pk = SR.pack(mols)
    v, c = SR.overlaps(pk, pk, T), SR.overlaps(pk, pk, T, colour=True)
    out = dict(mols=mols, notes=notes, pk=pk, v=v, c=c, st=SR.tanimoto(v, np.diag(v), np.diag(v)), ct=SR.tanimoto(c, np.diag(c), np.diag(c)),
               tol=SR.tolerances(pk, T), dev=_device_set(mols))
    full = S.similarity(out['dev'])
    out['full_st'], out['full_ct'] = full.shape.cpu(), full.colour.cpu()
    return out


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


def _check_self(s, pk, tol, colour=True):
    assert s.self_shape.dtype == torch.float32 and s.self_shape.shape == (len(pk.status),) == s.self_colour.shape
    assert s.status.dtype == torch.int32 and s.status.cpu().tolist() == pk.status.tolist()
    want_v = SR.self_overlaps(pk, T)
    want_c = SR.self_overlaps(pk, T, colour=True) if colour else np.zeros(len(pk.status))
    rel = lambda got, want: float((np.abs(got.cpu().numpy() - want)[want > 0] / want[want > 0]).max()) if (want > 0).any() else 0.0     # noqa: E731
    print('self overlaps: relative deviation V %.3e C %.3e (tolerance %.3e)' % (rel(s.self_shape, want_v), rel(s.self_colour, want_c), tol.overlap))
    assert SR.overlap_close(s.self_shape.cpu().numpy(), want_v, tol.overlap)
    assert SR.overlap_close(s.self_colour.cpu().numpy(), want_c, tol.overlap)
    assert (s.mol[:, 1].cpu().numpy() == pk.mask.sum(axis=1)).all() and s.has_colour == colour


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
def _mols_of(refs, pos, sizes, fp=None):
    out, n0 = [], 0
    for r, n in zip(refs, sizes):
        out.append(SR.Mol(np.asarray(r['cls'], dtype=np.int64).reshape(-1), pos[n0:n0 + n].numpy().astype(np.float32).reshape(-1, 3),
                          np.zeros(n, dtype=np.uint8) if fp is None else fp[n0:n0 + n]))
        n0 += n
    return out


def test_pack_on_the_ragged_batch(case):
    node, pos, edge, sizes = R.generate_batch()
    for n in (1, 2, 3, 63, 64, 65, M.MAX_ATOMS):
        assert n in sizes
    refs = R.screen_batch(node, pos, edge, sizes)
    cen = R.census(refs)
    assert cen['HAD_MASKED_ATOM'] >= 1 and cen['NO_ATOMS'] >= 1 and cen['NONFINITE'] >= 1 and 0 < cen['valid'] < len(sizes), cen
    fp = np.random.default_rng(4).integers(0, 256, sum(sizes)).astype(np.uint8)
    mols = _mols_of(refs, pos, sizes, fp)
    res = mol_result(node, pos, edge, sizes)
    sc = M.screen(res)
    feats = _fake_features(sc, torch.from_numpy(fp).to(DEV).reshape(1, -1))
    everything = torch.ones(1, len(sizes), dtype=torch.bool, device=DEV)
    by_default = S.shape_set(res, screen=sc, features=feats)                       # select = screen.valid
    _check_self(by_default, SR.pack(mols, [r['valid'] for r in refs]), case['tol'])
    assert (by_default.status.cpu().numpy() & S.SHAPE_UNSELECTED != 0).tolist() == [not r['valid'] for r in refs]
    whole = S.shape_set(res, features=feats, select=everything)
    pk = SR.pack(mols)
    _check_self(whole, pk, case['tol'])
    assert {S.SHAPE_EMPTY, S.SHAPE_NONFINITE} <= set(whole.status.cpu().tolist())
    plain = S.shape_set(res, screen=sc, select=everything)
    _check_self(plain, pk, case['tol'], colour=False)
    assert bits(plain.self_shape).equal(bits(whole.self_shape))                   # the shape part does not see the colour
    # the same molecules from assembled dicts: the same bits, self overlaps and similarities
    again = S.from_molecules(M.assemble(res, features=None), DEV)
    assert not again.has_colour and again.status.cpu().tolist() == pk.status.tolist()
    assert bits(again.self_shape).equal(bits(plain.self_shape))
    assert bits(S.similarity(again).shape).equal(bits(S.similarity(plain).shape))
    with_fp = [dict(m, features={'atom_fp': f.fp[SR.kept(f)]}) for m, f in zip(M.assemble(res), mols)]
    coloured = S.from_molecules(with_fp, DEV)
    assert coloured.has_colour and bits(coloured.self_colour).equal(bits(whole.self_colour))
    a, b = S.similarity(coloured, whole), S.similarity(whole)
    assert bits(a.shape).equal(bits(b.shape)) and bits(a.colour).equal(bits(b.colour))
    near_a, near_b = S.nearest(coloured, colour_weight=0.5), S.nearest(whole, colour_weight=0.5)
    assert bits(near_a.sim).equal(bits(near_b.sim)) and near_a.index.equal(near_b.index)


def test_pack_on_trajectory_frames_and_strided_views(case):
    sizes = [5, 17, 64, 3, 30]
    rng = np.random.default_rng(3)
    N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
    node = torch.from_numpy(rng.normal(0, 1, (6, N, 12)).astype(np.float32))
    edge = torch.from_numpy(rng.normal(0, 1, (6, E, 6)).astype(np.float32))
    edge[..., 0] += 2.5
    pos = torch.from_numpy(rng.normal(0, 3, (6, N, 3)).astype(np.float32))
    pos[4, 30, 2] = float('nan')
    full = mol_result(node[-1], pos[-1], edge[-1], sizes, traj=(node.to(DEV), pos.to(DEV), edge.to(DEV)))
    everything = torch.ones(6, len(sizes), dtype=torch.bool, device=DEV)
    got = S.shape_set(full, frames='traj', select=everything)
    assert got.n == 6 * len(sizes) and not got.has_colour
    mols, valid = [], []
    for f in range(6):
        refs = R.screen_batch(node[f], pos[f], edge[f], sizes)
        mols += _mols_of(refs, pos[f], sizes)
        valid += [r['valid'] for r in refs]
    pk = SR.pack(mols)
    assert (pk.status == SR.NONFINITE).sum() == 1
    _check_self(got, pk, case['tol'], colour=False)
    _check_self(S.shape_set(full, frames='traj'), SR.pack(mols, valid), case['tol'], colour=False)
    for f in (0, 4):                                                   # frame by frame: the same bits
        one = S.shape_set(mol_result(node[f], pos[f], edge[f], sizes), select=everything[:1])
        assert bits(one.self_shape).equal(bits(got.self_shape[f * len(sizes):(f + 1) * len(sizes)]))
    strided = dict(full, traj=[t[::2] for t in full['traj']])
    assert not strided['traj'][1].is_contiguous()
    half = S.shape_set(strided, frames='traj', select=everything[::2].contiguous())
    keep = [f * len(sizes) + g for f in (0, 2, 4) for g in range(len(sizes))]
    assert bits(half.self_shape).equal(bits(got.self_shape[keep])) and half.status.equal(got.status[keep])
    assert bits(S.similarity(half).shape).equal(bits(S.similarity(S.select_rows(got, keep)).shape))


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('na', SIZES)
def test_matrix_on_rectangular_sets(case, na):
    dev, tol, n = case['dev'], case['tol'], len(case['mols'])
    ia = list(range(na))
    a = S.select_rows(dev, ia)
    for nb in SIZES:
        ib = [(7 * k + 3) % n for k in range(nb)]
        got = S.similarity(a, S.select_rows(dev, ib))
        assert got.shape.shape == (na, nb) == got.colour.shape and got.shape.dtype == got.colour.dtype == torch.float32
        st, ct = got.shape.cpu(), got.colour.cpu()
        if na and nb:
            print('%d x %d: ST off by %.3e, CT by %.3e (tolerance %.3e)' % (na, nb, np.abs(st.numpy() - case['st'][np.ix_(ia, ib)]).max(),
                                                                          np.abs(ct.numpy() - case['ct'][np.ix_(ia, ib)]).max(), tol.sim))
            assert np.abs(st.numpy() - case['st'][np.ix_(ia, ib)]).max() <= tol.sim, (na, nb)
            assert np.abs(ct.numpy() - case['ct'][np.ix_(ia, ib)]).max() <= tol.sim, (na, nb)
        # a pair's value does not depend on where the two molecules sit or on what else the sets hold
        assert bits(st).equal(bits(case['full_st'][ia][:, ib])) and bits(ct).equal(bits(case['full_ct'][ia][:, ib]))


def test_matrix_determinism_and_empty_rows(case):
    dev, notes, full_st, full_ct = case['dev'], case['notes'], case['full_st'], case['full_ct']
    _check_self(dev, case['pk'], case['tol'])
    for src, dst in notes['duplicates']:                               # exact duplicates: bit-equal columns (and rows)
        for full in (full_st, full_ct):
            assert bits(full[:, src]).equal(bits(full[:, dst])) and bits(full[src]).equal(bits(full[dst]))
        assert full_st[src, dst] == 1.0 and full_st[dst, dst] == 1.0
    both = S.similarity(dev, dev)
    assert bits(both.shape.cpu()).equal(bits(full_st)) and bits(both.colour.cpu()).equal(bits(full_ct))
    for i in (notes['no_kept'], notes['no_atoms'], notes['nan']):
        assert (full_st[i] == 0).all() and (full_st[:, i] == 0).all() and (full_ct[i] == 0).all() and (full_ct[:, i] == 0).all()
    for i in notes['far']:
        assert full_st[i, 0] == 0 and full_st[0, i] == 0               # underflows to 0
    for src, dst in notes['shifted']:
        assert 0.0 < full_st[src, dst] < 1.0
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    del both
    torch.full((2 * dev.n * dev.n,), -1.0, dtype=torch.float32, device=DEV)
    again = S.similarity(dev)
    assert bits(again.shape.cpu()).equal(bits(full_st)) and bits(again.colour.cpu()).equal(bits(full_ct))
    # a set without colour: no colour matrix, the same shape bits
    plain = _device_set(case['mols'], colour=False)
    got = S.similarity(plain, dev)
    assert got.colour is None and bits(got.shape.cpu()).equal(bits(full_st))
    # two sets joined: the rows keep their bits
    joined = S.concat([S.select_rows(dev, [5, 6]), dev])
    assert joined.n == dev.n + 2 and bits(S.similarity(joined).shape.cpu()[2:, 2:]).equal(bits(full_st))


# ---- nearest ---------------------------------------------------------------------------------------------------------------------------
def _check_nearest(got, case, ia, ib, same, w):
    tol = case['tol'].sim + COMBINE
    mat = SR.score(case['st'], case['ct'], w)[np.ix_(ia, ib)]
    sim, index, total, _ = SR.nearest(mat, same)
    assert got.sim.dtype == torch.float32 and got.index.dtype == torch.int32 and got.sum.dtype == torch.float64
    bound = len(ib) ** 2 * 2.0 ** -53 + len(ib) * tol
    print('nearest %d x %d, w %.2f: sim off by %.3e (tolerance %.3e), sum by %.3e (bound %.3e)'
          % (len(ia), len(ib), w, np.abs(got.sim.cpu().numpy() - sim).max(), tol, np.abs(got.sum.cpu().numpy() - total).max(), bound))
    assert np.abs(got.sim.cpu().numpy() - sim).max() <= tol
    SR.check_nearest_index(got.index.cpu().tolist(), mat, same, tol)
    assert np.abs(got.sum.cpu().numpy() - total).max() <= bound
    # bit-identical to the row maxima of similarity(): the score is two rounded products and one rounded sum
    w32 = np.float32(w)
    sc = (np.float32(1) - w32) * case['full_st'].numpy()[np.ix_(ia, ib)] + w32 * case['full_ct'].numpy()[np.ix_(ia, ib)]
    if same:
        sc[np.arange(len(ia)), np.arange(len(ia))] = -1.0
    assert np.array_equal(got.sim.cpu().numpy().view(np.uint32), sc.max(axis=1).view(np.uint32))
    assert got.index.cpu().tolist() == np.argmax(sc, axis=1).tolist()                # (argmax: the first, so the lowest, maximum)
    return sc


def test_nearest_on_the_corpus(case):
    dev, notes, n = case['dev'], case['notes'], len(case['mols'])
    rows = list(range(n))
    for w in (0.0, 0.25):
        _check_nearest(S.nearest(dev, colour_weight=w), case, rows, rows, True, w)
        _check_nearest(S.nearest(dev, dev, colour_weight=w), case, rows, rows, False, w)
    self_free, with_self = S.nearest(dev), S.nearest(dev, dev)
    for src, dst in notes['duplicates']:                               # the lowest index among exact ties
        assert with_self.index[src] == src and with_self.index[dst] == src and with_self.sim[dst] == 1.0
        assert self_free.index[src] == dst and self_free.index[dst] == src
    for i in (notes['no_kept'], notes['nan']):                         # an empty row scores 0 everywhere: index 0 (or 1 without itself)
        assert with_self.sim[i] == 0 and with_self.index[i] == 0 and self_free.index[i] == 0 and self_free.sum[i] == 0
    mat = SR.score(case['st'], case['ct'], 0.25)
    got = S.internal_diversity(dev, colour_weight=0.25)
    assert abs(got - SR.diversity(mat, case['pk'].status)) <= case['tol'].sim + COMBINE and 0.0 < got < 1.0


def test_nearest_edges_and_the_split(case):
    dev = case['dev']
    one = S.nearest(S.select_rows(dev, [4]))
    assert one.sim.tolist() == [-1.0] and one.index.tolist() == [-1] and one.sum.tolist() == [0.0]
    none = S.nearest(S.select_rows(dev, [0, 1, 2]), S.select_rows(dev, []))
    assert none.sim.tolist() == [-1.0] * 3 and none.index.tolist() == [-1] * 3 and none.sum.tolist() == [0.0] * 3
    empty = S.nearest(S.select_rows(dev, []), dev)
    assert empty.sim.shape == (0,) and empty.index.shape == (0,) and empty.sum.shape == (0,)
    assert math.isnan(S.internal_diversity(S.select_rows(dev, [4]))) and math.isnan(S.internal_diversity(S.select_rows(dev, [8, 9, 4])))
    # few rows against 2T + 1: b is cut into three runs that a second launch combines; nothing depends on the cut
    nb = 2 * S.TILE_B + 1
    ia, ib = [20, 21, 22], list(range(nb))
    for w in (0.0, 0.25):
        _check_nearest(S.nearest(S.select_rows(dev, ia), S.select_rows(dev, ib), colour_weight=w), case, ia, ib, False, w)
    # ties across the runs: every row of b the same molecule, the lowest index wins
    same_rows = S.select_rows(dev, [7] * nb)
    got = S.nearest(S.select_rows(dev, ia), same_rows)
    assert got.index.tolist() == [0, 0, 0] and bits(got.sim.cpu()).equal(bits(case['full_st'][ia, 7]))
    for n in (S.TILE_B - 1, S.TILE_B, S.TILE_B + 1):
        _check_nearest(S.nearest(S.select_rows(dev, list(range(n)))), case, list(range(n)), list(range(n)), True, 0.0)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(case):
    lib, dev = hip.lib(), case['dev']
    good = S._alpha_arg(S.ShapeOptions())
    n = M.MAX_ATOMS + 1
    cls = torch.zeros(1, n, dtype=torch.int8, device=DEV)
    pos = torch.zeros(n, 3, device=DEV)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    atoms = torch.full((n, 4), 77.0, device=DEV)
    mol = torch.full((1, 2), 77, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError) as err:
        S._launch_pack(lib, cls, off, pos, 0, None, None, 1, 1, n, n, good, atoms, mol, status)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and str(n) in str(err.value)
    zero_radius = S._alpha_arg(S.ShapeOptions(radii_pm=(192, 0) + S.VDW_RADIUS_PM[2:]))
    small_off = torch.tensor([0, 3], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='positive and finite'):
        S._launch_pack(lib, cls[:, :3].contiguous(), small_off, pos[:3], 0, None, None, 1, 1, 3, 3, zero_radius, atoms[:3], mol, status)
    with pytest.raises(RuntimeError, match='pg_shape_pack'):
        S._launch_pack(lib, cls[:, :3].contiguous(), small_off, pos[:3], 0, None, None, 1, 1, 3, -1, good, atoms[:3], mol, status)
    self_v, self_c = torch.full((dev.n,), 77.0, device=DEV), torch.full((dev.n,), 77.0, device=DEV)
    with pytest.raises(RuntimeError, match='positive and finite'):
        S._launch_self(lib, dev.atoms, dev.mol, zero_radius, self_v, self_c)
    st, ct = torch.full((dev.n, dev.n), 77.0, device=DEV), torch.full((dev.n, dev.n), 77.0, device=DEV)
    with pytest.raises(RuntimeError, match='positive and finite'):
        S._launch_similarity(lib, dev, dev, zero_radius, st, ct)
    out = S.Nearest(sim=torch.full((dev.n,), 77.0, device=DEV), index=torch.full((dev.n,), 77, dtype=torch.int32, device=DEV),
                    sum=torch.full((dev.n,), 77.0, dtype=torch.float64, device=DEV))
    for w in (1.5, -0.25, float('nan')):
        with pytest.raises(RuntimeError, match='colour weight'):
            S._launch_nearest(lib, dev, dev, False, True, w, good, out)
        with pytest.raises(RuntimeError, match='colour weight'):
            S.nearest(dev, colour_weight=w)
    with pytest.raises(RuntimeError, match='positive and finite'):
        S._launch_nearest(lib, dev, dev, False, True, 0.5, zero_radius, out)
    with pytest.raises(RuntimeError, match='same is set'):
        S._launch_nearest(lib, dev, S.select_rows(dev, [0, 1]), True, True, 0.5, good, out)
    torch.cuda.synchronize()
    for t in (atoms, mol, status, self_v, self_c, st, ct, out.sim, out.index, out.sum):
        assert (t == 77).all()
    # sets of different options do not meet; a zero radius never becomes a set
    other = S.from_molecules([{'element': [6, 8], 'atom_pos': np.zeros((2, 3), dtype=np.float32)}], DEV, S.ShapeOptions(colour_radius_pm=120))
    for fn in (S.similarity, S.nearest):
        with pytest.raises(ValueError, match='different options'):
            fn(dev, other)
    with pytest.raises(ValueError, match='same options'):
        S.concat([dev, other])
    with pytest.raises(RuntimeError, match='positive and finite'):
        S.from_molecules([{'element': [6], 'atom_pos': np.zeros((1, 3))}], DEV, S.ShapeOptions(colour_radius_pm=0))
    # the calls above left the library usable
    S._launch_nearest(lib, dev, dev, False, True, 0.25, good, out)
    _check_nearest(out, case, list(range(dev.n)), list(range(dev.n)), False, 0.25)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_sampled_molecules_end_to_end(case, model, tmp_path):
    from bench import ligphore_workload
    NA = [11, 9, 14, 8]
    w = ligphore_workload(len(NA), seed=11)
    centers = torch.randn(len(NA), 3, generator=torch.Generator().manual_seed(11)) * 2.0
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(NA), centers, rng='device',
                             seed=17, num_steps=10)
    torch.cuda.synchronize()
    points = w['pos_phore'].to(DEV).float() + centers.to(DEV)[w['batch_phore'].to(DEV)]
    feats = M.features(res, points, torch.full((points.size(0),), -1, dtype=torch.int8), w['batch_phore'].to(DEV))
    everything = torch.ones(1, len(NA), dtype=torch.bool, device=DEV)
    got = S.shape_set(res, features=feats, select=everything)
    done = M.assemble(res, features=feats)
    mols = [SR.Mol(np.array([S.ATOM_TYPES.index(z) for z in m['element']], dtype=np.int64), m['atom_pos'].numpy().astype(np.float32).reshape(-1, 3),
                   np.asarray(m['features']['atom_fp'], dtype=np.uint8)) for m in done]
    pk, tol = SR.pack(mols), case['tol']
    _check_self(got, pk, tol)
    v, c = SR.overlaps(pk, pk, T), SR.overlaps(pk, pk, T, colour=True)
    sim = S.similarity(got)
    assert np.abs(sim.shape.cpu().numpy() - SR.tanimoto(v, np.diag(v), np.diag(v))).max() <= tol.sim
    assert np.abs(sim.colour.cpu().numpy() - SR.tanimoto(c, np.diag(c), np.diag(c))).max() <= tol.sim
    again = S.from_molecules(done, DEV)
    assert again.has_colour and bits(S.similarity(again).shape).equal(bits(sim.shape)) and bits(S.similarity(again).colour).equal(bits(sim.colour))
    # the files of tools/sample_cli.py --shape --shape_colour --shape_reference, written from these molecules (the tool's own run
    # below samples from noise weights and may finish none); the reference is molecule 1's own mol block
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import sample_cli
    sample_cli.write_shape_files(str(tmp_path), 'x', done, True, 0.25, sample_cli.first_mol_block_of(M.mol_block(done[1], 'ref') + '$$$$\n'))
    rows = [ln.split() for ln in (tmp_path / 'x_shape.txt').read_text().split('\n')[:-1] if not ln.startswith('#')]
    near = S.nearest(got, colour_weight=0.25)
    assert [int(r[0]) for r in rows] == list(range(len(NA))) and all(len(r) == 5 for r in rows)
    assert [r[1] for r in rows] == ['%.3f' % x for x in got.self_shape.tolist()] and [int(r[3]) for r in rows] == near.index.tolist()
    assert [r[2] for r in rows] == ['%.6f' % x for x in near.sim.tolist()]
    # ST is 1, its maximum, at the molecule itself: the four decimals of the block move it in second order only
    assert abs(float(rows[1][4]) - 1.0) <= tol.sim + 1e-6 and all(0.0 <= float(r[4]) < 1.0 for k, r in enumerate(rows) if k != 1)
    summary = dict(ln.split(': ') for ln in (tmp_path / 'x_shape_summary.txt').read_text().split('\n')[:-1])
    assert list(summary) == ['molecules', 'internal_shape_diversity', 'mean_nearest_shape_similarity', 'mean_reference_shape_similarity']
    assert summary['molecules'] == '4' and abs(float(summary['internal_shape_diversity']) - S.internal_diversity(got, 0.25)) <= 1e-6


def test_sample_cli_writes_the_shape_files(case, tmp_path):
    """Two runs with one seed, so with the same molecules: the second takes the first .sdf the first one wrote as its reference."""
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    cli = [sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3', '--batch_size', '3',
           '--num_steps', '10', '--shape', '--shape_colour', '--sdf']
    first = tmp_path / 'first'
    run = subprocess.run(cli + ['--outdir', str(first)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    sdfs = sorted((first / 'sdf_results').glob('*.sdf'), key=lambda p: int(p.stem.rsplit('_', 1)[1]))
    out = first
    if sdfs:
        out = tmp_path / 'out'
        run = subprocess.run(cli + ['--outdir', str(out), '--shape_reference', str(sdfs[0])], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
    done = torch.load(str(next(out.glob('*.pt'))), weights_only=False)
    print('%d finished molecules, %d .sdf files' % (len(done), len(sdfs)))
    (path,) = out.glob('*_shape.txt')
    print(path.read_text() + next(out.glob('*_shape_summary.txt')).read_text())
    rows = [ln.split() for ln in path.read_text().split('\n')[:-1] if not ln.startswith('#')]
    assert len(rows) == len(done) and all(len(r) == (5 if sdfs else 4) for r in rows)
    assert [int(r[0]) for r in rows] == list(range(len(done)))
    for r, m in zip(rows, done):
        assert float(r[1]) > 0 and -1 <= int(r[3]) < len(done) and int(r[3]) != int(r[0]) and 'features' in m
        assert (int(r[3]) == -1) == (len(done) < 2) == (float(r[2]) == -1.0)
    (path,) = out.glob('*_shape_summary.txt')
    names = [ln.split(':')[0] for ln in path.read_text().split('\n')[:-1]]
    assert names == ['molecules', 'internal_shape_diversity', 'mean_nearest_shape_similarity'] + (['mean_reference_shape_similarity'] if sdfs else [])
    if sdfs:
        i = int(sdfs[0].stem.rsplit('_', 1)[1])                        # the finished molecule that is the reference
        ref, mine = S.from_mol_block(sdfs[0].read_text(), DEV), S.from_molecules(done[i:i + 1], DEV)
        assert ref.mol.equal(mine.mol) and not ref.has_colour
        assert np.abs(ref.atoms[:, :3].cpu().numpy() - mine.atoms[:, :3].cpu().numpy()).max() <= 5.1e-5     # the .sdf's four decimals
        # ST is 1, its maximum, at the molecule itself: the four decimals move it in second order only (about 1e-9); the column has six
        assert abs(float(rows[i][4]) - 1.0) <= case['tol'].sim + 1e-6
