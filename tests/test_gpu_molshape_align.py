"""-m gpu: the overlay kernels (csrc/shape_align.hip through phoregen_amd/shape.py) against the float64 restatement of
tests/shape_align_reference.py and against the module's own in-place `similarity()`.

Tolerances, measured on the corpus by the restatement (tests/test_molshape_align_host.py prints them), nothing tuned against the kernel:
frames to 4 x the fp32 rounding of the float64 frames (centroid 7.2e-6, axes 1.2e-7, rho 8.5e-7, eigenvalues 6.9e-6 absolute); the
returned rotation to |R^T R - I| <= 4 x 1.25e-6 and |det R - 1| <= 4 x 1.25e-6; consistency with `similarity()` at the returned
transform, V and C to 4 x 9.0e-8 + 9.0e-6 = 9.4e-6 relative, ST and CT to 4 x 7.6e-8 + 2.7e-5 = 2.73e-5 absolute; the score against
the restatement to max(4 x 1.7e-6, 2.7e-5) = 2.7e-5, at most 5 % of the pairs excused and only where the restatement's best two
starts lie within twice that; recovery of moved copies to 1 - ST <= max(4 x the fp32 run's worst, the ST tolerance) = 2.73e-5.
Everything the determinism rules promise is compared with `==` on the bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mol_reference as R
import shape_align_reference as AR
import shape_reference as SR
from mol_support import batch_from, bits, mol_result
from phoregen_amd import hip
from phoregen_amd import molecule as M
from phoregen_amd import shape as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = SR.tables(S.VDW_RADIUS_PM, S.ShapeOptions().colour_radius_pm, S.KAPPA, S.P)
W = AR.COLOUR_WEIGHT
FIELDS = ('shape_overlap', 'colour_overlap', 'shape', 'colour', 'score', 'rotation', 'translation', 'start', 'steps')


def _fake_features(sc, fp):
    """A `Features` that carries the feature bytes alone (and the screen they belong to)."""
    blank = dict.fromkeys(('status', 'counts', 'ok', 'point_dist', 'point_atom', 'point_off', 'point_range', 'point_kind', 'limits', 'kekule', 'rings'))
    return M.Features(atom_fp=fp, screen=sc, **blank)


def _device_set(mols, colour=True, select=None):
    """The molecules through the sampler's layout, the screen and `shape_set`."""
    graphs = [(np.where(SR.kept(m), m.cls, 11).tolist(), {}, m.pos) for m in mols]
    res = mol_result(*batch_from(graphs))
    sc = M.screen(res)
    fp = torch.from_numpy(np.concatenate([m.fp for m in mols] + [np.zeros(0, dtype=np.uint8)])).to(DEV).reshape(1, -1)
    sel = torch.ones(1, len(mols), dtype=torch.bool, device=DEV) if select is None else select
    return S.shape_set(res, screen=sc, features=_fake_features(sc, fp) if colour else None, select=sel)


def _pairs(rows):
    return torch.tensor([p[:2] for p in rows], dtype=torch.int32, device=DEV).reshape(-1, 2)


def _same(x, y, rows_x=slice(None), rows_y=slice(None)):
    return all(bits(getattr(x, k)[rows_x]).equal(bits(getattr(y, k)[rows_y])) for k in FIELDS)


@pytest.fixture(scope='module')
def case():
    ref = AR.reference(T)
    dev = _device_set(ref['mols'])
    out = dict(ref, dev=dev, plain=S.align(dev, pairs=_pairs(ref['pairs'])),
               colour=S.align(dev, pairs=_pairs(ref['colour_pairs']), colour_weight=W), sim=S.similarity(dev))
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
def test_frames_against_the_restatement(case):
    dev, sides, tol = case['dev'], case['sides'], case['tol'].frame
    got = S.frames(dev)
    assert got.dtype == torch.float32 and got.shape == (dev.n, hip.PG_SHAPE_FRAME_FLOATS)
    got = _np(got)
    worst = np.zeros(16)
    for i, s in enumerate(sides):
        want = AR.frame64(s.pos)
        e = got[i, 3:12].reshape(3, 3)
        assert np.isfinite(got[i]).all() and np.abs(e @ e.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(e) - 1) <= 1e-6, i
        assert np.abs(np.cross(e[0], e[1]) - e[2]).max() <= 1e-6, i
        err = np.abs(got[i] - want)
        if len(s.pos) < 3:                                             # one or two atoms, or none: the axes are not decided
            err[3:12] = 0.0
        worst = np.maximum(worst, err)
        assert (err <= tol).all(), (i, len(s.pos), err, tol)
    print('frames: centroid off by %.3e, axes %.3e, rho %.3e, eigenvalues %.3e (tolerances %.3e %.3e %.3e %.3e)'
          % (worst[:3].max(), worst[3:12].max(), worst[12], worst[13:].max(), tol[0], tol[3], tol[12], tol[13]))
    identity = [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0, 0, 0]
    for i in (case['notes']['empty'], case['notes']['nan']):
        assert got[i].tolist() == identity
    assert got[case['notes']['sizes'][1], 3:13].tolist() == identity[3:13]
    # a frame depends on its row alone
    rows = [5, 0, case['notes']['empty'], 8, 5]
    assert bits(S.frames(S.select_rows(dev, rows))).equal(bits(S.frames(dev)[rows]))


# ---- the returned values -----------------------------------------------------------------------------------------------------------------
def _live(rows):
    return [k for k, p in enumerate(rows) if p[2] != 'empty']


def test_returned_transform_is_rigid(case):
    tol = case['tol']
    for name in ('plain', 'colour'):
        r = _np(case[name].rotation)
        orth = np.abs(np.einsum('nki,nkj->nij', r, r) - np.eye(3)).max()
        det = np.abs(np.linalg.det(r) - 1.0).max()
        print('%s: |R^T R - I| %.3e (tolerance %.3e), |det R - 1| %.3e (tolerance %.3e)' % (name, orth, tol.orthogonal, det, tol.det))
        assert orth <= tol.orthogonal and det <= tol.det
        assert case[name].rotation.shape[1:] == (3, 3) and case[name].translation.shape[1:] == (3,)


@pytest.mark.parametrize('name', ['plain', 'colour'])
def test_consistency_with_similarity_at_the_returned_transform(case, name):
    """The strongest check: B moved by the reported transform (`transformed`), then the in-place `similarity()`, and a float64
    evaluation at the same transform."""
    dev, tol, got = case['dev'], case['tol'], case[name]
    rows = case['pairs'] if name == 'plain' else case['colour_pairs']
    colour = name == 'colour'
    moved = S.transformed(dev, got.pairs[:, 1], got.rotation, got.translation)
    assert moved.n == len(rows) and bits(moved.self_shape).equal(bits(dev.self_shape[got.pairs[:, 1].long()]))
    sim = S.similarity(S.select_rows(dev, got.pairs[:, 0].long()), moved)
    st, ct = _np(sim.shape.diagonal()), _np(sim.colour.diagonal())
    worst = dict(v=0.0, c=0.0, st=0.0, ct=0.0)
    for k in _live(rows):
        ia, ib = rows[k][:2]
        a, b = case['sides'][ia], case['sides'][ib]
        y = b.pos.astype(np.float64) @ _np(got.rotation[k]).T + _np(got.translation[k])
        v8, c8, st8, ct8 = AR.overlaps_at(a, y, b, T, colour)
        v, c = float(got.shape_overlap[k]), float(got.colour_overlap[k])
        worst['v'] = max(worst['v'], abs(v - v8) / v8)
        if c8 >= SR.TINY:
            worst['c'] = max(worst['c'], abs(c - c8) / c8)
        else:
            assert c == 0.0 or not colour
        worst['st'] = max(worst['st'], abs(float(got.shape[k]) - st8), abs(float(got.shape[k]) - st[k]))
        if colour:
            worst['ct'] = max(worst['ct'], abs(float(got.colour[k]) - ct8), abs(float(got.colour[k]) - ct[k]))
    print('%s: V off by %.3e, C by %.3e relative (tolerance %.3e); ST by %.3e, CT by %.3e (tolerance %.3e)'
          % (name, worst['v'], worst['c'], tol.overlap, worst['st'], worst['ct'], tol.sim))
    assert worst['v'] <= tol.overlap and worst['c'] <= tol.overlap and worst['st'] <= tol.sim and worst['ct'] <= tol.sim
    if not colour:                                                     # w = 0: CT = 0 and the colour terms are skipped
        assert (got.colour == 0).all() and (got.colour_overlap == 0).all()
    # the score is the combination of the two reported similarities, two rounded products and one rounded sum
    w32 = np.float32(W if colour else 0.0)
    want = (np.float32(1) - w32) * got.shape.cpu().numpy() + w32 * got.colour.cpu().numpy()
    assert np.array_equal(got.score.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize('name', ['plain', 'colour'])
def test_score_against_the_restatement(case, name):
    tol, got = case['tol'].score, case[name]
    rows = case['pairs'] if name == 'plain' else case['colour_pairs']
    runs = case[name + '64']
    live = _live(rows)
    off = {k: abs(float(got.score[k]) - runs[k].best.score) for k in live}
    excused = [k for k in live if off[k] > tol and AR.best_two_gap(runs[k]) <= 2 * tol]
    print('%s: score off by at most %.3e (tolerance %.3e, floor %.3e); %d of %d pairs excused' % (name, max(off.values()), tol, case['tol'].score_floor,
                                                                                            len(excused), len(live)))
    for k in live:
        print('  pair %s: device %.7f start %d steps %d, restatement %.7f start %d steps %d' % (rows[k], float(got.score[k]), int(got.start[k]),
              int(got.steps[k]), runs[k].best.score, runs[k].best.start, runs[k].best.steps))
    assert all(off[k] <= tol or k in excused for k in live), {k: off[k] for k in live if off[k] > tol}
    assert len(excused) <= 0.05 * len(live)
    assert (got.steps[live] >= 1).all() and (got.steps <= AR.MAX_STEPS).all() and (got.start[live] >= 0).all() and (got.start <= 4).all()


def test_exact_properties(case):
    dev, notes, got, sim_tol = case['dev'], case['notes'], case['plain'], case['tol'].sim
    rows = case['pairs']
    live = _live(rows)
    # never worse than where the molecules lie (start 0 is enabled), up to the consistency tolerance
    in_place = case['sim'].shape[got.pairs[:, 0].long(), got.pairs[:, 1].long()]
    assert (got.score[live] >= in_place[live] - sim_tol).all()
    # start 0 alone with one evaluation: similarity()'s values bit for bit, the identity exactly
    for w, name in ((0.0, 'plain'), (W, 'colour')):
        one = S.align(dev, pairs=got.pairs, colour_weight=w, options=S.AlignOptions(max_steps=1, starts='in_place'))
        ia, ib = got.pairs[:, 0].long(), got.pairs[:, 1].long()
        assert bits(one.shape).equal(bits(case['sim'].shape[ia, ib]))
        if w:
            assert bits(one.colour).equal(bits(case['sim'].colour[ia, ib]))
        assert (one.rotation[live] == torch.eye(3, device=DEV)).all() and (one.translation == 0).all()
        assert (one.start[live] == 0).all() and (one.steps[live] == 1).all()
    # empty and NaN rows: zeros, the identity, no start
    for k, p in enumerate(rows):
        if p[2] == 'empty':
            assert [float(getattr(got, f)[k]) for f in FIELDS[:5]] == [0.0] * 5 and int(got.start[k]) == -1 and int(got.steps[k]) == 0
            assert got.rotation[k].equal(torch.eye(3, device=DEV)) and (got.translation[k] == 0).all()
    # ties go to the lowest start: one atom on itself scores the same from every start
    k = [p[2] for p in rows].index('self')
    assert int(got.start[k]) == 0 and float(got.score[k]) == 1.0
    inertial = S.align(dev, pairs=got.pairs[k:k + 1], options=S.AlignOptions(starts='inertial'))
    assert int(inertial.start[0]) == 1 and float(inertial.score[0]) == 1.0
    # steps <= max_steps
    few = S.align(dev, pairs=got.pairs, options=S.AlignOptions(max_steps=3))
    assert (few.steps <= 3).all() and (few.steps[live] >= 1).all() and (few.score[live] <= got.score[live] + sim_tol).all()
    # an unselected row is an empty row
    sel = torch.ones(1, 4, dtype=torch.bool, device=DEV)
    sel[0, 2] = False
    small = _device_set(case['mols'][3:7], select=sel)
    out = S.align(small, options=S.AlignOptions(max_steps=8))
    assert out.pairs.tolist() == [[i, j] for i in range(4) for j in range(4)] and out.pairs.dtype == torch.int32
    for k, (i, j) in enumerate(out.pairs.tolist()):
        assert (int(out.start[k]) == -1) == (i == 2 or j == 2) == (float(out.score[k]) == 0.0)


def test_position_duplication_and_permutation_change_no_bit(case):
    dev, got, n = case['dev'], case['plain'], len(case['pairs'])
    perm = torch.from_numpy(np.random.default_rng(9).permutation(n)).to(DEV)
    twice = torch.cat([got.pairs[perm], got.pairs[:7], got.pairs[perm[:5]]])
    again = S.align(dev, pairs=twice)
    assert _same(again, got, slice(0, n), perm) and _same(again, got, slice(n, n + 7), slice(0, 7)) and _same(again, got, slice(n + 7, None), perm[:5])
    # the grid of two sets is the listed grid; the rows of a set may stand anywhere
    ia, ib = [4, 40, 9, 41], [42, 5, 41]
    a, b = S.select_rows(dev, ia), S.select_rows(dev, ib)
    grid = S.align(a, b, colour_weight=W)
    listed = S.align(dev, pairs=_pairs([(i, j) for i in ia for j in ib]), colour_weight=W)
    assert grid.pairs.tolist() == [[i, j] for i in range(4) for j in range(3)] and _same(grid, listed)
    # recycled memory: the outputs do not depend on what their buffers held
    del again, grid, listed
    torch.full((64 * n,), -1.0, device=DEV)
    assert _same(S.align(dev, pairs=got.pairs), got)
    # the exact duplicate of a molecule scores as the molecule does
    src, dup = case['notes']['duplicate']
    two = S.align(dev, pairs=_pairs([(40, src), (40, dup), (src, 41), (dup, 41)]))
    assert _same(two, two, slice(0, 1), slice(1, 2)) and _same(two, two, slice(2, 3), slice(3, 4))


def test_recovery_of_moved_copies(case):
    """Rigidly moved copies under the default options, perturbed copies (20 degrees, 0.7 Angstrom) from the in-place start alone."""
    dev, tol = case['dev'], case['tol']
    kinds = [p[2] for p in case['pairs']]
    worst32 = {k: max(1.0 - (r.best.st if k == 'rigid' else r.ascents[0].st) for r, kk in zip(case['plain32'], kinds) if kk == k)
               for k in ('rigid', 'perturbed')}
    rigid = [k for k, kind in enumerate(kinds) if kind in ('rigid', 'far')]
    got = 1.0 - _np(case['plain'].shape[rigid])
    print('rigid copies: 1 - ST at most %.3e (bound %.3e)' % (got.max(), max(4 * worst32['rigid'], tol.sim)))
    assert got.max() <= max(4 * worst32['rigid'], tol.sim)
    assert (case['plain'].start[[kinds.index('far')]] >= 1).all()
    rows = [p for p in case['pairs'] if p[2] == 'perturbed']
    alone = S.align(dev, pairs=_pairs(rows), options=S.AlignOptions(starts='in_place'))
    got = 1.0 - _np(alone.shape)
    print('perturbed copies, in place: 1 - ST at most %.3e (bound %.3e), steps at most %d' % (got.max(), max(4 * worst32['perturbed'], tol.sim),
                                                                                          int(alone.steps.max())))
    assert got.max() <= max(4 * worst32['perturbed'], tol.sim) and (alone.start == 0).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(case):
    lib, dev = hip.lib(), case['dev']
    good = S._alpha_arg(S.ShapeOptions())
    zero_radius = S._alpha_arg(S.ShapeOptions(radii_pm=(192, 0) + S.VDW_RADIUS_PM[2:]))
    fr = S.frames(dev)
    n = 6
    pairs = _pairs([(i, i + 1) for i in range(n)])
    values, transform = torch.full((n, 5), 77.0, device=DEV), torch.full((n, 12), 77.0, device=DEV)
    start, steps = torch.full((n,), 77, dtype=torch.int32, device=DEV), torch.full((n,), 77, dtype=torch.int32, device=DEV)

    def call(pairs=pairs, n_pairs=n, w=0.25, alpha=good, max_steps=128, first=0.5, least=1e-4, mask=0x1f, a=dev, fa=fr, out=values):
        S._launch_align(lib, a, fa, dev, fr, pairs, n_pairs, True, w, alpha, max_steps, first, least, mask, out, transform, start, steps)

    outside = [_pairs([(0, 1), (dev.n, 2)] + [(1, 2)] * 4), _pairs([(0, 1), (3, -1)] + [(1, 2)] * 4), _pairs([(-1, 0)] + [(1, 2)] * 5),
               _pairs([(1, 2)] * 5 + [(0, dev.n)])]
    refused = [dict(pairs=p) for p in outside]
    refused += [dict(max_steps=m) for m in (0, -1, 1025)] + [dict(first=x) for x in (0.0, -0.5, float('inf'), float('nan'))]
    refused += [dict(least=x) for x in (0.0, -1e-4, float('nan'), 0.75)] + [dict(mask=m) for m in (0, 0x20, 0x3f, -1)]
    refused += [dict(w=x) for x in (1.5, -0.25, float('nan'))] + [dict(alpha=zero_radius), dict(n_pairs=-1), dict(pairs=None, n_pairs=n)]
    for kw in refused:
        with pytest.raises(RuntimeError, match='pg_shape_align'):
            call(**kw)
    null = torch.empty(0, device=DEV)
    for kw in (dict(fa=null), dict(out=null)):
        with pytest.raises(RuntimeError, match='null'):
            call(**kw)
    with pytest.raises(RuntimeError, match='pg_shape_frames'):
        hip.check(lib.pg_shape_frames(dev.atoms.data_ptr(), -1, dev.mol.data_ptr(), dev.n, fr.data_ptr(), hip.stream_ptr()), 'pg_shape_frames')
    with pytest.raises(RuntimeError, match='null'):
        hip.check(lib.pg_shape_frames(dev.atoms.data_ptr(), dev.atoms.size(0), dev.mol.data_ptr(), dev.n, None, hip.stream_ptr()), 'pg_shape_frames')
    torch.cuda.synchronize()
    for t in (values, transform, start, steps):
        assert (t == 77).all()
    # the Python side: options, weights, pair lists, sets of different options
    with pytest.raises(ValueError, match='AlignOptions'):
        S.align(dev, options='fast')
    with pytest.raises(ValueError, match='pairs'):
        S.align(dev, pairs=pairs.long())
    with pytest.raises(RuntimeError, match='colour weight'):
        S.align(dev, pairs=pairs, colour_weight=1.5)
    with pytest.raises(RuntimeError, match='max_steps'):
        S.align(dev, pairs=pairs, options=S.AlignOptions(max_steps=2000))
    with pytest.raises(RuntimeError, match=r'pair 1 is \(%d, 2\)' % dev.n):
        S.align(dev, pairs=outside[0])
    other = S.from_molecules([{'element': [6, 8], 'atom_pos': np.zeros((2, 3), dtype=np.float32)}], DEV, S.ShapeOptions(colour_radius_pm=120))
    with pytest.raises(ValueError, match='different options'):
        S.align(dev, other)
    with pytest.raises(ValueError, match='rotation'):
        S.transformed(dev, [0, 1], torch.eye(3, device=DEV)[None], torch.zeros(2, 3, device=DEV))
    # n_pairs = 0 is nothing to do, and the library is still usable
    none = S.align(dev, pairs=pairs[:0])
    assert none.score.shape == (0,) and none.rotation.shape == (0, 3, 3) and S.align(S.select_rows(dev, []), dev).pairs.shape == (0, 2)
    call()
    assert _same(S.align(dev, pairs=pairs, colour_weight=0.25), S.ShapeAlignment(pairs, values[:, 0], values[:, 1], values[:, 2], values[:, 3], values[:, 4],
                                                                               transform[:, :9].reshape(n, 3, 3), transform[:, 9:], start, steps))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_sampled_molecules_onto_a_reference_in_another_frame(case, tmp_path):
    """`generate_batch()` through the screen and `from_molecules`; the reference is one of the molecules, written as a mol block in
    another frame (turned and shifted), so in place nothing matches it and after the overlay the molecule itself does."""
    node, pos, edge, sizes = R.generate_batch()
    res = mol_result(node, pos, edge, sizes)
    done = [m for m in M.assemble(res) if m['valid'] and 4 <= len(m['element']) <= 60]
    assert len(done) >= 3
    mols = S.from_molecules(done, DEV)
    src = max(range(len(done)), key=lambda i: len(done[i]['element']))
    rot, shift = AR._rotation(np.random.default_rng(1)), np.array([7.0, -5.0, 6.0])
    away = dict(done[src], atom_pos=torch.as_tensor(np.asarray(done[src]['atom_pos'], dtype=np.float64) @ rot.T + shift, dtype=torch.float32))
    ref = S.from_mol_block(M.mol_block(away, 'ref'), DEV)
    got = S.align(ref, mols)
    assert got.pairs.tolist() == [[0, j] for j in range(len(done))]
    in_place = S.similarity(ref, mols).shape[0]
    assert (got.shape >= in_place - case['tol'].sim).all() and float(in_place[src]) < 0.5
    # the block's four decimals move the copy by at most 5e-5 Angstrom per coordinate: ST is 1 to second order in that
    assert 1.0 - float(got.shape[src]) <= case['tol'].sim + 1e-6 and int(got.start[src]) >= 1
    moved = S.transformed(mols, got.pairs[:, 1], got.rotation, got.translation)
    assert np.abs(_np(S.similarity(ref, moved).shape[0]) - _np(got.shape)).max() <= case['tol'].sim
    # the overlay undoes the move: R y + t puts the molecule onto the reference's atoms
    back = _np(moved.atoms[moved.mol[src, 0]:moved.mol[src, 0] + moved.mol[src, 1], :3])
    assert np.abs(back - _np(ref.atoms[:, :3])).max() <= 5e-2
    # the files of tools/sample_cli.py --shape --shape_reference --shape_align, written from these molecules (the tool's own run
    # below samples from noise weights and may finish none): there the molecule stays and the reference moves
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import sample_cli
    block = sample_cli.first_mol_block_of(M.mol_block(away, 'ref') + '$$$$\n')
    assert sample_cli.write_shape_files(str(tmp_path), 'old', done, False, 0.5, block) is None
    overlay = sample_cli.write_shape_files(str(tmp_path), 'new', done, False, 0.5, block, align=True)
    old, new = ((tmp_path / (name + '_shape.txt')).read_text().split('\n') for name in ('old', 'new'))
    assert new[0] == old[0] + ' aligned_shape_sim aligned_start' and len(old) == len(new) == len(done) + 2
    for k, (x, y) in enumerate(zip(old[1:-1], new[1:-1])):
        extra = y[len(x):].split()
        assert y.startswith(x + ' ') and len(extra) == 2 and extra[0] == '%.6f' % float(overlay.shape[k]) and int(extra[1]) == int(overlay.start[k])
        assert float(extra[0]) >= float(x.split()[4]) - case['tol'].sim - 1e-6
    assert 1.0 - float(new[1 + src].split()[5]) <= case['tol'].sim + 2e-6 and float(old[1 + src].split()[4]) < 0.5
    old_sum, new_sum = ((tmp_path / (name + '_shape_summary.txt')).read_text() for name in ('old', 'new'))
    assert new_sum == old_sum + 'mean_aligned_reference_shape_similarity: %.6f\n' % overlay.shape.double().mean().item()
    # --shape_align_sdf: the molecule moved by the inverse transform lies on the reference's atoms, and is written as any molecule is
    onto = sample_cli.overlaid_onto_reference(done[src], overlay.rotation[src].tolist(), overlay.translation[src].tolist())
    assert np.abs(_np(onto['atom_pos']) - _np(away['atom_pos'])).max() <= 5e-2 and onto['element'] == done[src]['element']
    M.write_sdf(str(tmp_path / 'onto.sdf'), [onto], names=['onto'])
    again = S.from_mol_block((tmp_path / 'onto.sdf').read_text(), DEV)
    assert 1.0 - float(S.similarity(ref, again).shape[0, 0]) <= case['tol'].sim + 2e-3


def _cli(tmp_path, out, *flags):
    lst = tmp_path / 'files.json'
    lst.write_text(json.dumps([os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')]))
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_cli.py'), '--phore_file_list', str(lst), '--num_samples', '3',
                          '--batch_size', '3', '--num_steps', '10', '--outdir', str(out), *flags], capture_output=True, text=True, timeout=600)
    return run


def test_sample_cli_aligns_to_the_reference(case, tmp_path):
    """Two runs with one seed, so with the same molecules: without the new flags the files are what they were, with them every line
    gains its columns and the aligned .sdf files appear."""
    mol = {'element': [6, 6, 7, 6, 8, 6, 6, 16], 'atom_pos': np.asarray(SR.walk(np.random.default_rng(2), 8)) + [30.0, 0.0, -20.0],
           'bond_index': np.array([[0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7]]), 'bond_type': np.array([1] * 7)}
    ref_file = tmp_path / 'reference.sdf'
    ref_file.write_text(M.mol_block(mol, 'ref') + '$$$$\n')
    base = ['--shape', '--shape_colour', '--shape_reference', str(ref_file), '--sdf']
    plain, aligned = tmp_path / 'plain', tmp_path / 'aligned'
    for out, flags in ((plain, base), (aligned, base + ['--shape_align', '--shape_align_sdf'])):
        run = _cli(tmp_path, out, *flags)
        assert run.returncode == 0, run.stderr[-2000:]
    refused = _cli(tmp_path, tmp_path / 'refused', '--shape', '--shape_align')
    assert refused.returncode != 0 and '--shape_reference' in refused.stderr
    done = torch.load(str(next(aligned.glob('*.pt'))), weights_only=False)
    old = next(plain.glob('*_shape.txt')).read_text().split('\n')
    new = next(aligned.glob('*_shape.txt')).read_text().split('\n')
    print('%d finished molecules\n%s' % (len(done), '\n'.join(new)))
    assert len(old) == len(new) == len(done) + 2 and new[0] == old[0] + ' aligned_shape_sim aligned_start aligned_colour_sim aligned_score'
    for a, b in zip(old[1:-1], new[1:-1]):
        extra = b[len(a):].split()
        assert b.startswith(a + ' ') and len(extra) == 4 and 0 <= int(extra[1]) <= 4
        assert float(extra[0]) >= float(a.split()[4]) - case['tol'].sim - 1e-6       # never worse than in place
    old_sum = next(plain.glob('*_shape_summary.txt')).read_text()
    new_sum = next(aligned.glob('*_shape_summary.txt')).read_text()
    assert new_sum.startswith(old_sum) and (new_sum[len(old_sum):].startswith('mean_aligned_reference_shape_similarity: ') or not done)
    assert not (plain / 'sdf_aligned').exists()
    files = sorted(p.name for p in (aligned / 'sdf_aligned').glob('*.sdf')) if done else []
    assert files == sorted(p.name for p in (aligned / 'sdf_results').glob('*.sdf'))
    for name in ('sdf_results',):                                      # every file both runs write is the same, byte for byte
        for p in (plain / name).glob('*'):
            assert p.read_bytes() == (aligned / name / p.name).read_bytes()
    if done:
        # an aligned file holds the molecule moved by the inverse of the reported transform: scored where it lies against the
        # reference (no overlay), it reaches the aligned similarity, up to the file's four decimals
        i = int(files[0].rsplit('_', 1)[1].split('.')[0])
        moved = S.from_mol_block((aligned / 'sdf_aligned' / files[0]).read_text(), DEV)
        st = float(S.similarity(S.from_mol_block(ref_file.read_text(), DEV), moved).shape[0, 0])
        assert abs(st - float(new[1 + i].split()[5])) <= case['tol'].sim + 2e-3
