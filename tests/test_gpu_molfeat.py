"""-m gpu: the feature kernel (csrc/mol_feat.hip through phoregen_amd/molecule.py) against the plain restatement of
tests/feature_reference.py, and the functions that carry its answers.

The typing is integer work: atom bytes, counts, status and point_atom compare with `==`.  The restatement types from the Kekulé form
and the ring sizes the kernel itself read (which Kekulé structure a graph gets is not canonical); those two kernels have suites of
their own.  Whether a point is matched never turns on rounding: the generator leaves no atom-point distance within 1e-3 of the cutoff
and no two atoms within 1e-3 of each other as seen from a point.  Distances are held to relative 16 * 2^-24, the bound the header of
tests/test_gpu_molgeom.py derives for the same fp32 expression: three subtractions, three squares, two additions and a square root,
under 8 ulp together, times 2 for fma contraction.  Infinities must match exactly."""
import dataclasses

import numpy as np
import pytest
import torch

import feature_reference as FR
import kekule_reference as K
import mol_reference as R
from phoregen_amd import hip
from mol_support import batch_from, renumbered_rows, split_frame, mol_result as _result
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REL = 16.0 * 2.0 ** -24
CI = M.FEATURE_COUNTS.index


def _batch(cases):
    """(node, pos, edge, sizes) of cases {'classes', 'bonds', 'pos'} as CPU tensors, one-hot scores."""
    return batch_from([(c['classes'], c['bonds'], c['pos']) for c in cases])


def _split(ft, sizes, f=0):
    """Frame f of a `Features` as one dict of numpy arrays per graph, with the inputs the kernel read."""
    sc, kk = ft.screen, ft.kekule
    parts = split_frame(sizes, f, per_atom={'atom_fp': ft.atom_fp, 'cls': sc.cls, 'hcount': kk.hcount, 'charge': kk.charge},
                        per_pair={'order': sc.order, 'kekule_order': kk.kekule_order, 'ring_size': ft.rings.ring_size},
                        per_graph={'counts': ft.counts, 'status': ft.status, 'ok': ft.ok, 'kekule_status': kk.status})
    dist, atom, off = ft.point_dist[f].cpu().numpy(), ft.point_atom[f].cpu().numpy(), ft.point_off.cpu().tolist()
    return [{'atom_fp': r['atom_fp'], 'point_dist': dist[off[g]:off[g + 1]], 'point_atom': atom[off[g]:off[g + 1]], 'counts': r['counts'],
             'status': r['status'], 'ok': r['ok'],
             'inputs': (r['cls'], r['order'], r['kekule_order'], r['hcount'], r['charge'], r['kekule_status'] & M.KEKULE_FAILED == 0, r['ring_size'])}
            for g, r in enumerate(parts)]


def _same(r, w, where):
    """One graph's kernel outputs against the restatement's."""
    assert r['atom_fp'].dtype == np.uint8 and np.array_equal(r['atom_fp'], w['atom_fp']), (where, r['atom_fp'].tolist(), w['atom_fp'].tolist())
    assert r['counts'].tolist() == w['counts'].tolist(), (where, dict(zip(M.FEATURE_COUNTS, zip(r['counts'].tolist(), w['counts'].tolist()))))
    assert r['status'] == w['status'] and r['ok'] == w['ok'], (where, r['status'], w['status'])
    assert r['point_atom'].dtype == np.int16 and np.array_equal(r['point_atom'], w['point_atom']), (where, r['point_atom'], w['point_atom'])
    d, e = r['point_dist'].astype(np.float64), w['point_dist']
    fin = np.isfinite(e)
    assert r['point_dist'].dtype == np.float32 and np.array_equal(np.isinf(d), ~fin) and (d[~fin] > 0).all(), where
    err = np.abs(d[fin] - e[fin])
    print(where, 'max relative distance error', float((err / np.maximum(e[fin], 1e-30)).max()) if fin.any() else 0.0, 'bound', REL)
    assert (err <= REL * e[fin]).all(), (where, float((err / e[fin]).max()))


def _check(cases, layout='own', limits=M.FeatureLimits(), where=''):
    """The kernel on one batch of cases against the restatement.  layout 'own': every graph has its own points (sorted point_batch);
    'shared': every graph has all points of the first case (point_batch=None)."""
    node, pos, edge, sizes = _batch(cases)
    res = _result(node, pos, edge, sizes)
    if layout == 'own':
        pts = torch.from_numpy(np.concatenate([c['points'].reshape(-1, 3) for c in cases]).astype(np.float32))
        kinds = torch.from_numpy(np.concatenate([c['kinds'] for c in cases]).astype(np.int8))
        pb = torch.repeat_interleave(torch.arange(len(cases)), torch.tensor([len(c['kinds']) for c in cases]))
    else:
        pts, kinds, pb = torch.from_numpy(cases[0]['points']), torch.from_numpy(cases[0]['kinds']), None
    ft = M.features(res, pts, kinds, pb, limits=limits)
    torch.cuda.synchronize()
    N, Q = sum(sizes), (len(kinds) if layout == 'own' else len(kinds) * len(cases))
    assert ft.status.shape == ft.ok.shape == (1, len(sizes)) and ft.counts.shape == (1, len(sizes), 25) and ft.atom_fp.shape == (1, N)
    assert ft.point_dist.shape == ft.point_atom.shape == (1, Q) and ft.limits == limits
    assert (ft.status.dtype, ft.counts.dtype, ft.ok.dtype, ft.atom_fp.dtype) == (torch.int32, torch.int32, torch.bool, torch.uint8)
    got = _split(ft, sizes)
    want = []
    for g, (c, r) in enumerate(zip(cases, got)):
        cls, order = K.rows_of(c['classes'], c['bonds'])
        assert np.array_equal(r['inputs'][0], cls) and np.array_equal(r['inputs'][1], order), (where, g)    # (what the screen decoded)
        src = c if layout == 'own' else cases[0]
        w = FR.features_of_rows(*r['inputs'], c['pos'], src['points'], src['kinds'], limits)
        _same(r, w, '%s %d' % (where, g))
        want.append(w)
    return ft, res, got, want


def _named_cases():
    """Every named molecule with a point on each atom of one of its types (matched), a point of a type the atom does not carry placed
    on it (matched only if another carrying atom is in reach: the restatement says), and an untyped and an ignored point."""
    rng = np.random.default_rng(5)
    cases = []
    for name, (classes, bonds, _) in FR.NAMED.items():
        n = len(classes)
        pos = (rng.random((n, 3)) * 12.0).astype(np.float32)
        answer = FR.named_answer(name)
        pts, kinds = [], []
        for i, types in enumerate(answer):
            for t in M.FEATURE_TYPES:
                if t in types or (i + M.FEATURE_TYPES.index(t)) % 3 == 0:
                    pts.append(pos[i] + np.float32([0.25, -0.125, 0.5]))
                    kinds.append(M.FEATURE_TYPES.index(t))
        pts += [pos[0], pos[0]]
        kinds += [-1, -2]
        pts, kinds = np.array(pts, dtype=np.float32), np.array(kinds, dtype=np.int8)
        assert FR.acceptable(pos, pts), name
        cases.append({'classes': classes, 'bonds': bonds, 'pos': pos, 'points': pts, 'kinds': kinds, 'name': name})
    return cases


def test_named_molecules_by_hand_and_by_the_restatement():
    cases = _named_cases()
    ft, _, got, want = _check(cases, where='named')
    for c, r, w in zip(cases, got, want):
        answer = FR.named_answer(c['name'])
        assert r['atom_fp'].tolist() == FR.fp_of(answer).tolist(), c['name']
        assert r['status'] == (M.FEAT_HAS_UNTYPED | (M.FEAT_NO_KEKULE if c['name'] == 'indene-like' else 0)), c['name']
        k = 0
        for i, types in enumerate(answer):                             # a point on an atom of the right type is matched by that atom
            for t in M.FEATURE_TYPES:
                if t in types or (i + M.FEATURE_TYPES.index(t)) % 3 == 0:
                    if t in types:
                        assert r['point_atom'][k] == i and r['point_dist'][k] < 0.6, (c['name'], i, t)
                    k += 1
        assert r['counts'][CI('untyped_points')] == 1 and r['counts'][CI('typed_points')] == k
    by = {c['name']: r for c, r in zip(cases, got)}
    assert by['indene-like']['counts'][CI('matched')] == 0 and np.isinf(by['indene-like']['point_dist']).all()
    assert by['acetic acid']['counts'][CI('atoms_NE')] == 2 and by['methanesulfonic acid']['counts'][CI('atoms_NE')] == 3
    assert by['pyridine']['counts'][CI('atoms_AR')] == 6 and by['N-methylpyridinium']['counts'][CI('atoms_PO')] == 1


def _family():
    rng = np.random.default_rng(FR.FAMILY_SEED + 1)
    sizes = (1, 2, 3, 63, 64, 65, 127, 128, 128, 65, 64, 3)
    graphs = [FR.typable_graph(rng, n) if k != 8 else FR.decorate(rng, *K.random_graph(rng, n)) for k, n in enumerate(sizes)]
    graphs += [FR.star_graph(n) for n in (65, 128)]
    graphs += [g for g in FR.graphs_from_generator(30) if any(c == 11 for c in g[0])][:3]
    counts = (0, 1, 70, 5, 70, 12, 70, 70, 0, 1, 12, 70, 70, 70, 12, 5, 70)
    assert len(counts) == len(graphs)
    return [FR.make_case(rng, c, b, p) for (c, b), p in zip(graphs, counts)]


@pytest.fixture(scope='module')
def family():
    """The mixed batch: computed once, read by several tests, changed by none."""
    return _family()


def test_random_family_with_its_own_points(family):
    ft, _, got, want = _check(family, where='family')
    assert sorted({len(c['classes']) for c in family[:12]}) == [1, 2, 3, 63, 64, 65, 127, 128]
    assert {0, 1, 70} <= {len(c['kinds']) for c in family} and any(11 in c['classes'] for c in family)
    total = sum(w['counts'].astype(np.int64) for w in want)
    assert total[CI('matched')] >= 20 and total[CI('unmatched')] >= 100 and total[CI('untyped_points')] >= 10
    sc = ft.screen
    assert (sc.status[0] & M.STATUS_VALENCE).bool().sum() >= 2        # the stars fail the valence rule and are typed all the same
    # tighter limits move the status alone
    _, _, tight, _ = _check(family, limits=M.FeatureLimits(feat_cut=2.0, max_unmatched=0), where='family, max_unmatched=0')
    for a, b in zip(got, tight):
        assert np.array_equal(a['counts'], b['counts']) and b['status'] == a['status'] | (M.FEAT_UNMATCHED if a['counts'][CI('unmatched')] else 0)


def _shared_cases():
    rng = np.random.default_rng(FR.FAMILY_SEED + 2)
    graphs = [FR.typable_graph(rng, n) for n in (1, 3, 64, 65, 128)] + [FR.star_graph(64)]
    types = sum((FR.types_of(c, b) for c, b in graphs), [])
    for _ in range(50):
        poss = [(rng.random((len(c), 3)) * 30.0).astype(np.float32) for c, _ in graphs]
        pts, kinds = FR.draw_points(rng, np.concatenate(poss), 70, types)
        if all(FR.acceptable(p, pts) for p in poss):
            break
    else:
        raise AssertionError('no acceptable draw')
    return [{'classes': c, 'bonds': b, 'pos': p, 'points': pts, 'kinds': kinds} for (c, b), p in zip(graphs, poss)]


def test_shared_points():
    """point_batch=None: every graph sees all P points (70: more than a wave)."""
    cases = _shared_cases()
    ft, _, got, want = _check(cases, layout='shared', where='shared')
    assert ft.point_off.tolist() == [70 * g for g in range(7)] and sum(int(w['counts'][CI('matched')]) for w in want) >= 5


def test_trajectory_frames(family):
    """frames='traj', F = 3 in one launch: frames 0 and 2 are equal, in frame 1 two molecules have their coordinates dealt to other
    atoms (the same set of positions, so the generator's margins still hold)."""
    a = [family[k] for k in (2, 5, 13)]
    b = [dict(a[0], pos=np.roll(a[0]['pos'], 1, axis=0)), dict(a[1], pos=a[1]['pos'][::-1].copy()), a[2]]
    per = [_batch(a), _batch(b), _batch(a)]
    sizes = per[0][3]
    traj = tuple(torch.stack([p[k] for p in per]) for k in range(3))
    res = _result(*per[-1][:3], sizes, traj=traj)
    pts = torch.from_numpy(np.concatenate([c['points'] for c in a]))
    kinds = torch.from_numpy(np.concatenate([c['kinds'] for c in a]))
    pb = torch.repeat_interleave(torch.arange(3), torch.tensor([len(c['kinds']) for c in a]))
    ft = M.features(res, pts, kinds, pb, frames='traj')
    assert ft.status.shape == (3, 3) and ft.atom_fp.shape == (3, sum(sizes)) and ft.point_dist.shape == (3, len(kinds))
    for k in ('status', 'counts', 'atom_fp', 'point_dist', 'point_atom'):
        assert torch.equal(getattr(ft, k)[0], getattr(ft, k)[2]), k
    assert not torch.equal(ft.point_dist[0], ft.point_dist[1])
    for f, cases in enumerate((a, b, a)):
        for g, (c, r) in enumerate(zip(cases, _split(ft, sizes, f))):
            _same(r, FR.features_of_rows(*r['inputs'], c['pos'], a[g]['points'], a[g]['kinds']), 'frame %d graph %d' % (f, g))
    final = M.features(res, pts, kinds, pb)
    for k in ('status', 'counts', 'atom_fp', 'point_dist', 'point_atom'):
        assert torch.equal(getattr(final, k)[0], getattr(ft, k)[2]), k
    # a screen handed in is reused; one of other frames is refused
    sc = M.screen(res, frames='traj')
    assert M.features(res, pts, kinds, pb, frames='traj', screen=sc).screen is sc
    with pytest.raises(ValueError, match='screen'):
        M.features(res, pts, kinds, pb, frames='final', screen=sc)


def test_renumbered_graphs(family):
    """Permuting a graph's atoms permutes atom_fp and leaves counts, status and distances; point_atom maps through the permutation."""
    cases = [c for c in family if len(c['classes']) >= 3][:10]
    rng = np.random.default_rng(9)
    moved, perms = [], []
    for c in cases:
        n = len(c['classes'])
        p = rng.permutation(n)                                         # atom i becomes atom p[i]
        classes, pos = [0] * n, np.zeros_like(c['pos'])
        for i in range(n):
            classes[p[i]], pos[p[i]] = c['classes'][i], c['pos'][i]
        bonds = {(int(min(p[a], p[b])), int(max(p[a], p[b]))): t for (a, b), t in c['bonds'].items()}
        moved.append(dict(c, classes=classes, bonds=bonds, pos=pos))
        perms.append(p)
    _, _, base, _ = _check(cases, where='numbering, base')
    _, _, other, _ = _check(moved, where='numbering, moved')
    for g, (a, b, p, c) in enumerate(zip(base, other, perms, cases)):
        # feasibility of the Kekulé form does not depend on the numbering; the structure may, and with it where the hydrogens sit
        assert a['status'] & M.FEAT_NO_KEKULE == b['status'] & M.FEAT_NO_KEKULE and a['counts'][CI('typed_points')] == b['counts'][CI('typed_points')], g
        if _same_structure(a, b, p):
            assert a['status'] == b['status'], g
            assert np.array_equal(b['atom_fp'][p], a['atom_fp']) and np.array_equal(a['counts'], b['counts']), g
            assert np.array_equal(a['point_dist'], b['point_dist']), g
            keep = [i for i in range(len(p)) if c['classes'][i] <= 10]
            to_compact_b = {int(p[i]): k for k, i in enumerate(sorted(keep, key=lambda i: p[i]))}
            want = [-1 if x < 0 else to_compact_b[int(p[keep[x]])] for x in a['point_atom'].tolist()]
            assert b['point_atom'].tolist() == want, g
    assert sum(_same_structure(a, b, p) for a, b, p in zip(base, other, perms)) >= 6


def _same_structure(a, b, p):
    """Did both numberings get the same Kekulé structure (double bonds, hydrogens and charges atom for atom)?"""
    return (np.array_equal(b['inputs'][2][renumbered_rows(p)], a['inputs'][2]) and np.array_equal(b['inputs'][3][p], a['inputs'][3])
            and np.array_equal(b['inputs'][4][p], a['inputs'][4]))


def test_assemble_and_sdf_carry_the_features(family, tmp_path):
    cases = _named_cases()[:6] + [family[13], family[14]]
    node, pos, edge, sizes = _batch(cases)
    res = _result(node, pos, edge, sizes)
    pts = torch.from_numpy(np.concatenate([c['points'] for c in cases]))
    kinds = torch.from_numpy(np.concatenate([c['kinds'] for c in cases]))
    pb = torch.repeat_interleave(torch.arange(len(cases)), torch.tensor([len(c['kinds']) for c in cases]))
    ft = M.features(res, pts, kinds, pb)
    got = _split(ft, sizes)
    plain, full = M.assemble(res), M.assemble(res, features=ft)
    for g, (p, m, r, c) in enumerate(zip(plain, full, got, cases)):
        assert set(m) == set(p) | {'features'}
        for name in p:                                                 # the default output, key for key
            assert torch.equal(p[name], m[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], m[name]), name
        f = m['features']
        assert set(f) == {'status', 'features_ok', 'atom_fp', 'atom_types', 'point_kind', 'point_dist', 'point_atom', 'point_matched'} | set(M.FEATURE_COUNTS)
        assert [f[k] for k in M.FEATURE_COUNTS] == r['counts'].tolist() and f['status'] == r['status'] and f['features_ok'] == r['ok']
        keep = r['inputs'][0] >= 0
        assert f['atom_fp'].dtype == np.uint8 and f['atom_fp'].tolist() == r['atom_fp'][keep].tolist() and len(f['atom_fp']) == len(m['element'])
        assert f['atom_types'] == [tuple(t for k, t in enumerate(M.FEATURE_TYPES) if b >> k & 1) for b in f['atom_fp'].tolist()]
        assert np.array_equal(f['point_dist'], r['point_dist']) and np.array_equal(f['point_atom'], r['point_atom'])
        assert f['point_kind'].tolist() == c['kinds'].tolist() and int(f['point_matched'].sum()) == f['matched']
    path = tmp_path / 'f.sdf'
    M.write_sdf(str(path), full)
    text = path.read_text()
    assert text.count('> <PHOREGEN_FEATURES>') == len(cases) and '\nHD ' in text and '\ntyped_points ' in text
    # keys, geometry, rings, the Kekulé form and the features ride in one copy, all from one screen
    geo = M.geometry(res, pts, kinds == -2, pb, screen=ft.screen)
    every = M.assemble(res, keys=True, geometry=geo, rings=ft.rings, kekule=ft.kekule, features=ft)
    without = M.assemble(res, keys=True, geometry=geo, rings=ft.rings, kekule=ft.kekule)
    for m, q, w in zip(every, without, full):
        assert set(m) == set(q) | {'features'} and m['key'] == q['key'] and m['geom']['status'] == q['geom']['status']
        assert m['rings']['status'] == q['rings']['status'] and m['kekule']['formula'] == q['kekule']['formula']
        assert all(np.array_equal(m['features'][k], w['features'][k]) if isinstance(w['features'][k], np.ndarray) else m['features'][k] == w['features'][k]
                   for k in w['features'])
    # features() takes the parts it is handed and refuses parts of another screen
    again = M.features(res, pts, kinds, pb, kekule=ft.kekule, rings=ft.rings)
    assert again.screen is ft.screen and torch.equal(again.atom_fp, ft.atom_fp) and torch.equal(again.counts, ft.counts)
    swapped = _result(node, pos, edge, sizes[:3] + sizes[:2:-1])       # as many atom and bond rows, other graphs
    with pytest.raises(ValueError, match='different results'):
        M.features(res, pts, kinds, pb, screen=ft.screen, rings=M.rings(swapped))
    with pytest.raises(ValueError, match='different results'):
        M.assemble(res, rings=M.rings(swapped), features=ft)
    with pytest.raises(ValueError, match='features='):                  # of more than the final frame
        M.assemble(res, features=dataclasses.replace(ft, status=ft.status.repeat(2, 1)))
    with pytest.raises(ValueError, match='FeatureLimits'):
        M.features(res, pts, kinds, pb, limits={'max_unmatched': 0})


def test_sample_valid_with_features():
    """A stand-in model that hands out ethanol: with a donor point on the O and an aromatic point nowhere near an aromatic atom it is
    finished under the default limits and failed under max_unmatched=0."""
    classes, bonds, _ = FR.NAMED['ethanol']
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.2, 1.2, 0.0]])
    part = R.scores_from_classes(classes, bonds, pos=pos)

    class Ethanol:
        def sample(self, data, n, device, **kw):
            return _result(*(torch.cat([part[k]] * n) for k in range(3)), [3] * n)
    pts, kinds = torch.tensor([[2.2, 1.2, 0.5], [2.2, 1.2, 0.0]]), torch.tensor([0, 1], dtype=torch.int8)
    out = M.sample_valid(Ethanol(), None, num_samples=3, batch_size=2, features=(pts, kinds, M.FeatureLimits()))
    assert len(out['finished']) == 3 and not out['failed'] and out['n_calls'] == 2
    m = out['finished'][0]
    assert set(m) >= {'features'} and 'kekule' not in m and 'rings' not in m
    assert m['features']['atom_types'] == [('HY',), (), ('HD', 'HA')] and (m['features']['matched'], m['features']['unmatched']) == (1, 1)
    out = M.sample_valid(Ethanol(), None, num_samples=2, batch_size=2, max_failed_factor=1, features=(pts, kinds, M.FeatureLimits(max_unmatched=0)))
    assert not out['finished'] and len(out['failed']) == 4
    assert all(m['valid'] and m['features']['status'] == M.FEAT_UNMATCHED and not m['features']['features_ok'] for m in out['failed'])
    out = M.sample_valid(Ethanol(), None, num_samples=2, batch_size=2, kekule=True, rings=True, unique=True, max_failed_factor=1,
                         features=(pts[:1], kinds[:1], M.FeatureLimits(max_unmatched=0)))
    assert len(out['finished']) == 1 and out['finished'][0]['kekule']['formula'] == 'C2H6O' and out['finished'][0]['rings']['rings_ok']


def test_cpu_result_and_oversize_graph_are_refused():
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.features({'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]}, torch.zeros(1, 3), torch.zeros(1, dtype=torch.int8))
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)     # noqa: E731
    sc = dataclasses.make_dataclass('S', ['cls', 'order', 'compact', 'lig_off', 'bond_off'])(
        z((1, n), torch.int8), z((1, h), torch.int8), z((1, n), torch.int16), torch.tensor([0, n], dtype=torch.int32, device=DEV),
        torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV))
    kk = dataclasses.make_dataclass('K', ['kekule_order', 'hcount', 'charge', 'status'])(
        z((1, h), torch.int8), z((1, n), torch.uint8), z((1, n), torch.int8), z((1, 1), torch.int32))
    rg = dataclasses.make_dataclass('R', ['ring_size'])(z((1, h), torch.uint8))
    pts, kinds = z((2, 3), torch.float32), z((2,), torch.int8)
    ranges, off = torch.tensor([[0, 2]], dtype=torch.int32, device=DEV), torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    out = dict(status=torch.full((1, 1), 77, dtype=torch.int32, device=DEV), counts=torch.full((1, 1, 25), 77, dtype=torch.int32, device=DEV),
               atom_fp=torch.full((1, n), 77, dtype=torch.uint8, device=DEV), point_dist=torch.full((1, 2), 77.0, device=DEV),
               point_atom=torch.full((1, 2), 77, dtype=torch.int16, device=DEV))
    xyz = z((n, 3), torch.float32)
    with pytest.raises(RuntimeError) as err:
        M._launch_feat(hip.lib(), xyz, 0, sc, kk, rg, 1, 1, n, pts, kinds, ranges, off, 2, M.FeatureLimits(), out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_feat' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_feat'):
        M._launch_feat(hip.lib(), xyz, 0, sc, kk, rg, 1, 1, -1, pts, kinds, ranges, off, 2, M.FeatureLimits(), out)
    with pytest.raises(ValueError, match='features'):
        M._launch_feat(hip.lib(), xyz, 0, sc, kk, rg, 1, 1, n, pts, kinds[:1], ranges, off, 2, M.FeatureLimits(), out)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values())
    # empty batches return without a launch
    empty = M.features(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), []), torch.zeros(0, 3), torch.zeros(0, dtype=torch.int8))
    assert empty.status.shape == (1, 0) and empty.atom_fp.shape == (1, 0) and empty.counts.shape == (1, 0, 25)
