"""-m gpu: the geometry screen (csrc/mol_geom.hip through phoregen_amd/molecule.py) against the float64 restatement of
tests/geom_reference.py.

Tolerances.  Integer outputs (status, counts, point_atom) compare with `==`: the generated batch holds no float64 distance within
relative 1e-5 of a limit and no point whose two nearest atoms are that close, which is far outside what fp32 can move a distance by.
Distances (point_dist, metrics 0-4) and metric 6 are held to relative 16 * 2^-24: both sides start from the same fp32 values; three
subtractions, three squares, two additions and a square root have relative error <= 2^-24 each (<= 2 ulp for the root), under 8 ulp
together, and the factor 2 is margin for fma contraction.  Metric 6 is a mean of differences distance - limit; the kernel forms it in
fp64 and rounds once, so it meets the same bound.  Metric 5 is held to the sequential-sum bound of the two centroids,
(n_kept + n_points + 4) * 2^-24 * sqrt(3) * max|coordinate| absolute.  Infinities and NaNs must match exactly."""
import os

import numpy as np
import pytest
import torch

import geom_reference as G
import mol_reference as R
from phoregen_amd import hip
from helpers import default_model
from mol_support import bits as _bits, mol_result as _result
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 16.0 * 2.0 ** -24
OUT_KEYS = ('status', 'counts', 'metrics', 'point_dist', 'point_atom')


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


@pytest.fixture(scope='module')
def generated():
    """The generated batch and its restatement, computed once and only read by the tests; its conditions are asserted here, by the
    restatement alone, before any kernel output exists."""
    batch = G.generate_batch()
    refs = G.restate_batch(batch)
    census = G.check_batch(batch, refs)
    print('census of the generated batch:', census)
    return batch, refs


def _launch(res, point_pos, point_is_ex, ranges, frames='final', limits=None, out=None, max_n=None):
    """The kernel with explicit point ranges (which may coincide between graphs): dict of the five output tensors."""
    _, pos, _, F, (_, _, pos_fs) = M._frames(res, frames)
    sc = M.screen(res, frames)
    B = len(sc.num_atoms)
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(ranges[:, 1] - ranges[:, 0])])
    Q = int(off[-1])
    if out is None:
        out = _buffers(F, B, Q)
    M._launch_geom(hip.lib(), pos, pos_fs, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms) if max_n is None else max_n,
                   torch.as_tensor(np.asarray(point_pos, dtype=np.float32)).reshape(-1, 3).to(DEV),
                   torch.as_tensor(np.asarray(point_is_ex, dtype=np.uint8)).reshape(-1).to(DEV),
                   torch.as_tensor(ranges, dtype=torch.int32).to(DEV), torch.as_tensor(off, dtype=torch.int32).to(DEV), Q,
                   tuple(G.limits64(limits).tolist()), out)
    torch.cuda.synchronize()
    return out


def _buffers(F, B, Q, fill=None):
    shapes = {'status': ((F, B), torch.int32), 'counts': ((F, B, 6), torch.int32), 'metrics': ((F, B, 8), torch.float32),
              'point_dist': ((F, Q), torch.float32), 'point_atom': ((F, Q), torch.int16)}
    return {k: (torch.empty(s, dtype=dt, device=DEV) if fill is None else torch.full(s, fill, dtype=dt, device=DEV)) for k, (s, dt) in shapes.items()}


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in OUT_KEYS)


def _close(got, want, tol_rel, what):
    """got (fp32 from the kernel) against want (float64): non-finite values exactly, the rest within tol_rel relative."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    special = ~np.isfinite(want)
    assert np.array_equal(got[special], want[special], equal_nan=True), (what, got[special], want[special])
    err = np.abs(got[~special] - want[~special])
    print(what, 'largest relative error %.3g of %.3g allowed' % (float((err / np.maximum(np.abs(want[~special]), 1e-300)).max()) if err.size else 0.0, tol_rel))
    assert (err <= tol_rel * np.abs(want[~special])).all(), (what, got[~special][err > tol_rel * np.abs(want[~special])])


def _compare_frame(out, f, refs, pos_f, point_pos):
    """Frame f of the kernel's outputs against the restated graphs."""
    status, counts, metrics = (out[k][f].cpu().numpy() for k in ('status', 'counts', 'metrics'))
    dist, atom = out['point_dist'][f].cpu().numpy(), out['point_atom'][f].cpu().numpy()
    finite_pos, finite_pts = pos_f[np.isfinite(pos_f)], point_pos[np.isfinite(point_pos)]
    biggest = max(float(np.abs(finite_pos).max()) if finite_pos.size else 0.0, float(np.abs(finite_pts).max()) if finite_pts.size else 0.0)
    q0 = 0
    assert [int(s) for s in status] == [r['status'] for r in refs], (f, status.tolist(), [r['status'] for r in refs])
    for g, r in enumerate(refs):
        p = r['n_points']
        assert counts[g].tolist() == r['counts'].tolist(), (f, g, counts[g].tolist(), r['counts'].tolist())
        assert np.array_equal(atom[q0:q0 + p], r['point_atom']), (f, g, atom[q0:q0 + p], r['point_atom'])
        q0 += p
    _close(dist, np.concatenate([r['point_dist'] for r in refs]), REL, 'point_dist')
    for k in (0, 1, 2, 3, 4, 6):
        _close(metrics[:, k], [r['metrics'][k] for r in refs], REL, M.GEOM_METRICS[k])
    assert (metrics[:, 7] == 0).all()
    for g, r in enumerate(refs):
        want = r['metrics'][5]
        if np.isnan(want):
            assert np.isnan(metrics[g, 5]), (f, g, metrics[g, 5])
        else:
            bound = (r['n_kept'] + r['n_points'] + 4) * 2.0 ** -24 * np.sqrt(3.0) * biggest
            assert abs(float(metrics[g, 5]) - want) <= bound, (f, g, float(metrics[g, 5]), want, bound)


def test_kernel_equals_restatement_on_the_generated_batch(generated):
    batch, refs = generated
    res = _result(batch['node'], batch['pos'], batch['edge'], batch['sizes'])
    out = _launch(res, batch['point_pos'], batch['point_is_ex'], batch['ranges'])
    B, Q = len(batch['sizes']), sum(r['n_points'] for r in refs)
    assert out['status'].shape == (1, B) and out['point_dist'].shape == (1, Q) and Q > batch['point_pos'].shape[0]   # (a shared range)
    _compare_frame(out, 0, refs, batch['pos'].numpy(), batch['point_pos'])


def _three_frames(batch):
    """The generated batch as frame 0 of a trajectory; frame 1 with every coordinate moved a little; frame 2 with other bonds and
    other coordinates."""
    node, pos, edge = batch['node'], batch['pos'], batch['edge']
    g = torch.Generator().manual_seed(3)
    pos1 = pos + 0.2 * torch.randn(pos.shape, generator=g)
    pos2 = pos.flip(0) * 0.98
    return torch.stack([node, node, node.flip(0)]), torch.stack([pos, pos1, pos2]), torch.stack([edge, edge, edge.flip(0)])


def test_strided_frames_equal_single_calls(generated):
    batch, refs = generated
    node3, pos3, edge3 = _three_frames(batch)
    res = _result(batch['node'], batch['pos'], batch['edge'], batch['sizes'], traj=(node3, pos3, edge3))
    args = (batch['point_pos'], batch['point_is_ex'], batch['ranges'])
    all3 = _launch(res, *args, frames='traj')
    assert all3['status'].shape[0] == 3
    for f in range(3):
        one = _launch(_result(node3[f], pos3[f], edge3[f], batch['sizes']), *args)
        for k in OUT_KEYS:
            assert torch.equal(_bits(all3[k][f]), _bits(one[k][0])), (f, k)
    _compare_frame(all3, 0, refs, batch['pos'].numpy(), batch['point_pos'])
    # every element of every output is written: a call into buffers that held something else comes out identical
    B, Q = all3['status'].shape[1], all3['point_dist'].shape[1]
    for fill in (0x55, -1):
        again = _launch(res, *args, frames='traj', out=_buffers(3, B, Q, fill=fill))
        assert _same(all3, again), fill


def test_exact_ties_and_exact_limits():
    """Small-integer coordinates, so every fp32 distance is exact.  A point as far from two atoms as from each other's: the first in
    atom order wins, counted among the kept classes.  Distances exactly at bond_min, bond_max, clash_min and ex_clear set no bit;
    a feature exactly at feat_cut is not covered (`check_nearby_phore` compares with <), which is the informational bit alone."""
    tie = R.scores_from_classes([11, 1, 1, 3], {(1, 2): 1}, pos=torch.tensor([[3., 0, 1], [0, 0, 0], [6, 0, 0], [3, 4, 0]]))
    tri = R.scores_from_classes([1, 1, 1], {(0, 1): 1, (0, 2): 1}, pos=torch.tensor([[0., 0, 0], [3, 0, 0], [0, 4, 0]]))
    node, pos, edge = (torch.cat([a, b]) for a, b in zip(tie[:3], tri[:3]))
    res = _result(node, pos, edge, [4, 3])
    lim = M.GeomLimits(bond_min=3.0, bond_max=4.0, clash_min=5.0, ex_clear=5.0, feat_cut=2.0)
    pts = torch.tensor([[3., 0, 0], [0, 0, 1], [0, 0, -5], [0, 0, 2]])
    ex = torch.tensor([0, 0, 1, 0])
    geo = M.geometry(res, pts[:3], ex[:3], point_batch=torch.tensor([0, 1, 1]), limits=lim)
    torch.cuda.synchronize()
    assert geo.point_off.tolist() == [0, 1, 3] and geo.point_range.tolist() == [[0, 1], [1, 3]]
    assert geo.point_dist[0].tolist() == [3.0, 1.0, 5.0] and geo.point_atom[0].tolist() == [0, 0, 0]
    assert geo.status[0].tolist() == [M.GEOM_BOND_LONG | M.GEOM_FEATURE_MISSED, 0] and geo.ok[0].tolist() == [False, True]
    assert geo.counts[0, 1].tolist() == [0, 0, 0, 0, 1, 1] and geo.metrics[0, 1, :5].tolist() == [3.0, 4.0, 5.0, 5.0, 1.0]
    assert geo.metrics[0, 1, 6].item() == 0.0
    # graph 0: the bond 1-2 of length 6 is long, the non-bonded pairs of length 5 are no clash at clash_min 5, the feature is 3 away
    want = G.geom_graph(pos[:4].numpy(), [-1, 1, 1, 3], [0, 0, 0, 1, 0, 0], pts[:1].numpy(), [0], lim)
    assert want['status'] == geo.status[0, 0].item() and geo.counts[0, 0].tolist() == want['counts'].tolist() == [0, 1, 0, 0, 0, 1]
    # the feature exactly at feat_cut: not covered; every graph measured against all points (point_batch=None)
    geo = M.geometry(res, pts[1:], ex[1:], limits=lim)
    assert geo.point_off.tolist() == [0, 3, 6] and geo.status[0, 1].item() == M.GEOM_FEATURE_MISSED and geo.ok[0, 1].item()
    assert geo.counts[0, 1].tolist() == [0, 0, 0, 0, 1, 2] and geo.point_dist[0, 3:].tolist() == [1.0, 5.0, 2.0]
    # one representable step inside each limit sets its bit
    eps = 2.0 ** -20
    geo = M.geometry(res, pts[1:], ex[1:], limits=M.GeomLimits(3.0 + eps, 4.0 - eps, 5.0 + eps, 5.0 + eps, 2.0 + eps))
    assert geo.status[0, 1].item() == M.GEOM_BOND_SHORT | M.GEOM_BOND_LONG | M.GEOM_CLASH | M.GEOM_EX_CLASH
    assert geo.counts[0, 1].tolist() == [1, 1, 1, 1, 2, 2]


def test_a_graph_alone_equals_the_graph_in_its_batch(generated):
    batch, refs = generated
    res = _result(batch['node'], batch['pos'], batch['edge'], batch['sizes'])
    whole = _launch(res, batch['point_pos'], batch['point_is_ex'], batch['ranges'])
    sizes = batch['sizes']
    n_off = np.concatenate([[0], np.cumsum(sizes)])
    e_off = np.concatenate([[0], np.cumsum([n * (n - 1) for n in sizes])])
    q_off = np.concatenate([[0], np.cumsum([r['n_points'] for r in refs])])
    picked = [sizes.index(M.MAX_ATOMS), sizes.index(65), sizes.index(1)] + [g for g, fault in enumerate(batch['faults']) if fault in ('bond_long', 'clash', 'shares_previous', 'nan_atom')]
    for g in picked:
        alone = _result(batch['node'][n_off[g]:n_off[g + 1]], batch['pos'][n_off[g]:n_off[g + 1]], batch['edge'][e_off[g]:e_off[g + 1]], [sizes[g]])
        one = _launch(alone, batch['point_pos'], batch['point_is_ex'], [batch['ranges'][g]])
        for k in ('status', 'counts', 'metrics'):
            assert torch.equal(_bits(one[k][0, 0]), _bits(whole[k][0, g])), (g, k, one[k][0, 0], whole[k][0, g])
        for k in ('point_dist', 'point_atom'):
            assert torch.equal(_bits(one[k][0]), _bits(whole[k][0, q_off[g]:q_off[g + 1]])), (g, k)


NA = [11, 9, 14, 8]


def _near_a_limit(r, limits=None):
    """Does the restated graph hold a distance fp32 could put on the other side of a limit, or a point with two nearest atoms fp32
    could swap?  (Sampled molecules are not the generated batch: nothing keeps their distances away from the limits.)"""
    d = np.concatenate([r['pair_dist'], r['atom_point_dist']])
    d = d[np.isfinite(d)]
    near = any((np.abs(d - v) <= G.REL_GAP * v).any() for v in G.limits64(limits))
    first = r['point_dist']
    ok = np.isfinite(first) & np.isfinite(r['second'])
    return near or bool((r['second'][ok] - first[ok] <= G.REL_GAP * first[ok]).any())


def test_through_the_model(model):
    from phoregen_amd.data import parse_phore_file
    data = parse_phore_file(os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')).to(DEV)
    res = model.sample(data, len(NA), DEV, num_atoms=torch.tensor(NA), seed=17, num_steps=12, return_traj=True)
    torch.cuda.synchronize()
    before = [t.clone() for t in res['pred'] + res['traj']]
    sct = M.screen(res, frames='traj')
    geo = M.geometry_for(data, res, frames='traj', screen=sct, ex_col=model.ex_col)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, res['pred'] + res['traj'])) and geo.screen is sct
    F, P = res['traj'][1].shape[0], data['phore'].pos.shape[0]
    assert F == 13 and geo.status.shape == (F, 4) and geo.point_dist.shape == (F, 4 * P) and geo.point_off.tolist() == [0, P, 2 * P, 3 * P, 4 * P]
    pts = (data['phore'].pos.float() + data.center.float()).cpu().numpy()
    is_ex = (data['phore'].x[:, model.ex_col] == 1).cpu().numpy()
    assert 0 < is_ex.sum() < P
    pos, cls, order = res['traj'][1].cpu().numpy(), sct.cls.cpu().numpy(), sct.order.cpu().numpy()
    out = {k: getattr(geo, k) for k in OUT_KEYS}
    skipped = 0
    for f in range(F):
        refs = G.geom_batch(pos[f], cls[f], order[f], NA, pts, is_ex, [[0, P]] * 4)
        if any(_near_a_limit(r) for r in refs):
            skipped += 1
            continue
        _compare_frame(out, f, refs, pos[f], pts)
    print('frames with a distance within 1e-5 of a limit, not compared:', skipped)
    assert skipped <= 2

    # assemble carries the final frame's row in its one copy
    gf = M.geometry_for(data, res, ex_col=model.ex_col)
    mols, plain = M.assemble(res, keys=True, geometry=gf), M.assemble(res, keys=True)
    status, metrics, counts = gf.status[0].cpu().numpy(), gf.metrics[0].cpu().numpy(), gf.counts[0].cpu().numpy()
    dist, atom = gf.point_dist[0].cpu().numpy(), gf.point_atom[0].cpu().numpy()
    for g, (m, pm) in enumerate(zip(mols, plain)):
        assert set(m) == set(pm) | {'geom'} and m['key'] == pm['key'] and m['element'] == pm['element'] and torch.equal(m['atom_pos'], pm['atom_pos'])
        assert torch.equal(m['bond_index'], pm['bond_index']) and m['status'] == pm['status']
        gm = m['geom']
        assert gm['status'] == int(status[g]) and gm['geom_ok'] == ((int(status[g]) & M.GEOM_FAIL_MASK) == 0) == bool(gf.ok[0, g])
        assert np.array_equal(np.array([gm[k] for k in M.GEOM_METRICS], dtype=np.float32), metrics[g], equal_nan=True)
        assert [gm[k] for k in M.GEOM_COUNTS] == counts[g].tolist()
        assert np.array_equal(gm['point_dist'], dist[g * P:(g + 1) * P]) and np.array_equal(gm['point_atom'], atom[g * P:(g + 1) * P])
        # point_atom indexes this molecule's own atoms
        near = gm['point_atom'] >= 0
        d = np.linalg.norm(m['atom_pos'].numpy().astype(np.float64)[gm['point_atom'][near]] - pts[near], axis=1)
        assert np.allclose(d, gm['point_dist'][near], rtol=1e-5)
    with pytest.raises(ValueError, match='final frame'):
        M.assemble(res, geometry=geo)

    # sample_valid(geometry=True): one draw of 4 in either run (max_failed_factor=0 ends the loop after it unless all four passed),
    # the same draw (the Philox key comes from torch's generator); filtered by hand with the restatement
    def by_hand(m):
        n = len(m['element'])
        order_m = np.zeros(n * (n - 1) // 2, dtype=np.int8)
        for (a, b), t in zip(m['bond_index'].T.tolist(), m['bond_type'].tolist()):
            order_m[R.pair_row(a, b, n)] = t
        return G.geom_graph(m['atom_pos'].numpy(), [1] * n, order_m, pts, is_ex)
    torch.manual_seed(5)
    plain = M.sample_valid(model, data, num_samples=4, batch_size=4, max_failed_factor=0, num_steps=10)
    torch.manual_seed(5)
    fit = M.sample_valid(model, data, num_samples=4, batch_size=4, max_failed_factor=0, num_steps=10, geometry=True)
    assert plain['n_calls'] == fit['n_calls'] == 1 and len(fit['finished']) + len(fit['failed']) == 4
    hand = [by_hand(m) for m in plain['finished']]
    assert not any(_near_a_limit(r) for r in hand)
    want = [m for m, r in zip(plain['finished'], hand) if r['ok']]
    assert len(fit['finished']) == len(want) and all('geom' in m for m in fit['finished'] + fit['failed'])
    for m, w in zip(fit['finished'], want):
        assert m['valid'] and m['geom']['geom_ok'] and m['element'] == w['element'] and torch.equal(m['atom_pos'], w['atom_pos'])
        assert torch.equal(m['bond_index'], w['bond_index']) and torch.equal(m['bond_type'], w['bond_type'])
    assert all(not m['valid'] or not m['geom']['geom_ok'] for m in fit['failed'])


class _Rota:
    """Test double for the network: `.sample` returns device tensors that encode a fixed rota of three-atom molecules C-C-O, all valid
    for the screen, at different geometries."""
    KINDS = {'good': [[0, 0, 0], [1.5, 0, 0], [1.5, 1.4, 0]], 'long': [[0, 0, 0], [3.0, 0, 0], [3.0, 1.4, 0]],
             'clash': [[0, 0, 0], [1.5, 0, 0], [0.3, 1.0, 0]], 'in_sphere': [[0, 0, 4.0], [1.5, 0, 4.0], [1.5, 1.4, 4.0]]}

    def __init__(self, rota):
        self.rota, self.i, self.calls = rota, 0, []

    def sample(self, data, n, device, **kw):
        assert kw.pop('return_traj') is False
        self.calls.append(n)
        kinds = [self.rota[(self.i + j) % len(self.rota)] for j in range(n)]
        self.i += n
        parts = [R.scores_from_classes([1, 1, 3], {(0, 1): 1, (1, 2): 1}, pos=torch.tensor(self.KINDS[k], dtype=torch.float32) + 30.0) for k in kinds]
        node, pos, edge = (torch.cat([p[i] for p in parts]) for i in range(3))
        return _result(node, pos, edge, [3] * n)


def test_sample_valid_geometry_loop():
    pts = torch.tensor([[0.5, 0.5, 0], [1.5, 0, 6.0]]) + 30.0          # a feature beside the molecule, a sphere above it
    dbl = _Rota(['good', 'long', 'good', 'clash', 'in_sphere', 'good'])
    out = M.sample_valid(dbl, None, num_samples=4, batch_size=4, geometry=(pts, torch.tensor([0, 1]), M.GeomLimits()))
    # by hand: draw 4 (g l g c) -> 2 finished; 2 (s g) -> 3; 1 (g) -> 4
    assert dbl.calls == [4, 2, 1] and out['n_calls'] == 3 and len(out['finished']) == 4
    assert all(m['valid'] and m['geom']['status'] == 0 and m['geom']['features_covered'] == 1 for m in out['finished'])
    assert [m['geom']['status'] for m in out['failed']] == [M.GEOM_BOND_LONG, M.GEOM_CLASH, M.GEOM_EX_CLASH | M.GEOM_FEATURE_MISSED]
    assert all(m['valid'] for m in out['failed'])                      # the screen alone would have finished them
    # without geometry= the loop is the previous one: no 'geom', everything valid is finished
    dbl = _Rota(['good', 'long'])
    out = M.sample_valid(dbl, None, num_samples=3, batch_size=4)
    assert dbl.calls == [3] and len(out['finished']) == 3 and not any('geom' in m for m in out['finished'])


def test_errors_are_raised_before_any_launch(generated):
    batch, refs = generated
    res = _result(batch['node'], batch['pos'], batch['edge'], batch['sizes'])
    B, Q = len(batch['sizes']), sum(r['n_points'] for r in refs)
    out = _buffers(1, B, Q, fill=77)
    with pytest.raises(RuntimeError) as err:
        _launch(res, batch['point_pos'], batch['point_is_ex'], batch['ranges'], out=out, max_n=M.MAX_ATOMS + 1)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_geom' in str(err.value)
    with pytest.raises(ValueError, match='do not fit'):               # outputs sized for another batch
        _launch(res, batch['point_pos'], batch['point_is_ex'], batch['ranges'][:-1], out=out)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == 77).all(), k
    pts, ex = torch.zeros(5, 3), torch.zeros(5)
    for bad in (dict(point_pos=torch.zeros(5, 2)), dict(point_is_ex=torch.zeros(4)), dict(point_batch=torch.zeros(4, dtype=torch.long)),
                dict(point_batch=torch.tensor([0, 2, 1, 3, 3])), dict(point_batch=torch.tensor([0, 0, 1, 1, B])),
                dict(limits=M.GeomLimits(bond_max=float('nan'))), dict(frames='traj', screen=M.screen(res))):
        with pytest.raises(ValueError):
            M.geometry(res, **dict(dict(point_pos=pts, point_is_ex=ex), **bad))
    # an empty batch and a batch without points return without trouble
    empty = _result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])
    assert M.geometry(empty, pts, ex).status.shape == (1, 0)
    geo = M.geometry(res, torch.zeros(0, 3), torch.zeros(0))
    assert geo.point_dist.shape == (1, 0) and geo.counts[0, :, 5].sum().item() == 0
