"""No GPU: the mirrors of the overlay's constants, the float64 restatement of tests/shape_align_reference.py on hand cases (the frame
against numpy.linalg.eigh, the degenerate frames, the gradient against finite differences), the stand-alone host program over
csrc/shape_align_core.h (tools/shape_align_host_check.cpp, compiled with g++ under ASan + UBSan and run as a child process) against
the restatement, and the conditions the corpus must meet, judged by the restatement alone.

Tolerances (shape_align_reference.reference, measured on the corpus, nothing tuned against the kernel): a frame's numbers to 4 x the
largest fp32 rounding of the float64 frames (centroid 7.2e-6, axes 1.2e-7, rho 8.5e-7, eigenvalues 6.9e-6 absolute); the fp32
quaternion-to-matrix formula leaves |R^T R - I| <= 1.25e-6 and |det R - 1| <= 1.25e-6 on 1e5 random unit quaternions, held to 4 x;
moving B in fp32 instead of float64 moves V and C by 9.0e-8 relative and ST, CT by 7.6e-8, so the consistency check holds V and C to
4 x 9.0e-8 + 9.0e-6 = 9.4e-6 relative and ST, CT to 4 x 7.6e-8 + 2.7e-5 = 2.73e-5; the fp32 and the float64 run of the restatement
end within 1.7e-6 of each other in score on every pair, so the score is held to max(4 x 1.7e-6, 2.7e-5) = 2.7e-5.  A value the host
program computes with a handful of fp32 operations is compared at 4e-6: a dozen roundings of numbers of magnitude at most 2 on either
side."""
import numpy as np
import pytest
import torch

import shape_align_reference as AR
import shape_reference as SR
from mol_support import arg_count, build_host_check, header_macro, hex32, run_program
from phoregen_amd import hip
from phoregen_amd import shape as S

T = SR.tables(S.VDW_RADIUS_PM, S.ShapeOptions().colour_radius_pm, S.KAPPA, S.P)
FEW = 4e-6


@pytest.fixture(scope='module')
def ref():
    return AR.reference(T)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    return build_host_check('shape_align_host_check', tmp_path_factory.mktemp('shape_align_host'))


def _degenerate():
    """name -> float32 [n, 3]: no atom, one, two, five on a line, four in a plane, the corners of a cube (three equal eigenvalues),
    a square antiprism-like set with two equal eigenvalues."""
    line = np.outer(np.arange(5.0), [0.6, -0.48, 0.64]) + [1.0, 2.0, -3.0]
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * 0.75 + [0.5, 0.25, -4.0]
    disc = np.array([[np.cos(a), np.sin(a), h] for h in (-2.0, 2.0) for a in np.arange(4) * np.pi / 2]) + [3.0, 0.0, 1.0]
    return {'none': np.zeros((0, 3)), 'one': np.array([[1.5, -2.25, 0.125]]), 'two': np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.5]]),
            'line': line, 'plane': np.array([[0, 0, 1.0], [1.5, 0, 1.0], [0, 1.25, 1.0], [2.0, 2.0, 1.0]]), 'cube': cube, 'disc': disc}


def _proper(frame, tol=1e-6):
    e = np.asarray(frame[3:12], dtype=np.float64).reshape(3, 3)
    return bool(np.isfinite(np.asarray(frame)).all() and np.abs(e @ e.T - np.eye(3)).max() <= tol and abs(np.linalg.det(e) - 1.0) <= tol
                and np.abs(np.cross(e[0], e[1]) - e[2]).max() <= tol)


def test_constants_and_mirrors():
    for name, value in (('PG_SHAPE_FRAME_FLOATS', AR.FRAME), ('PG_SHAPE_ALIGN_N_STARTS', 5), ('PG_SHAPE_ALIGN_IN_PLACE', 0x01),
                        ('PG_SHAPE_ALIGN_INERTIAL', 0x1e), ('PG_SHAPE_ALIGN_MAX_STEPS', 1024)):
        assert int(header_macro(name), 0) == value == getattr(hip, name), name
    for name in ('pg_shape_frames', 'pg_shape_align'):
        assert name in hip.EXPORTS and arg_count(name) == len(hip._PROTOS[name][1]), name
    assert hip.ABI_VERSION == 11
    o = S.AlignOptions()
    assert (o.max_steps, o.first_step, o.min_step, o.starts) == (AR.MAX_STEPS, AR.FIRST_STEP, AR.MIN_STEP, 'both')
    assert S.START_NAMES == tuple(AR.STARTS) and [S.AlignOptions(starts=s).mask() for s in S.START_NAMES] == [0x01, 0x1e, 0x1f]
    for s, ks in AR.STARTS.items():
        assert S.AlignOptions(starts=s).mask() == sum(1 << k for k in ks)


def test_python_side_refusals():
    with pytest.raises(ValueError, match='ShapeSet'):
        S.align('x')
    with pytest.raises(ValueError, match='ShapeSet'):
        S.frames(None)
    with pytest.raises(ValueError, match='colour_weight'):
        S.align(None, colour_weight='a')
    with pytest.raises(ValueError, match='starts'):
        S.AlignOptions(starts='all').mask()
    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt)         # noqa: E731
    cpu = S.ShapeSet(atoms=z(2, 4), mol=z(1, 2, dt=torch.int32), status=z(1, dt=torch.int32), self_shape=z(1), self_colour=z(1), has_colour=False)
    for call in (lambda: S.align(cpu), lambda: S.frames(cpu), lambda: S.transformed(cpu, [0], z(1, 3, 3), z(1, 3))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_frame_against_eigh(ref):
    """On every corpus molecule of three atoms and more: the eigenvalues of the restatement's Jacobi are numpy.linalg.eigh's, its
    axes eigh's up to sign, the frame right-handed and its conventions kept."""
    seen = 0
    for s in ref['sides']:
        if len(s.pos) < 3:
            continue
        x = s.pos.astype(np.float64)
        cov = np.cov(x.T, bias=True)
        lam, vec = np.linalg.eigh(cov)
        fr = AR.frame64(s.pos)
        assert np.allclose(fr[13:], lam[::-1], rtol=0, atol=1e-12 * lam[-1]) and np.allclose(fr[:3], x.mean(axis=0), rtol=0, atol=1e-13)
        assert abs(fr[12] - max(np.sqrt(((x - x.mean(axis=0)) ** 2).sum(axis=1).mean()), 0.5)) <= 1e-13
        e = fr[3:12].reshape(3, 3)
        assert _proper(fr, 1e-13)
        for k in range(3):
            assert min(np.abs(e[k] - vec[:, 2 - k]).max(), np.abs(e[k] + vec[:, 2 - k]).max()) <= 1e-9, k
        for k in (0, 1):
            assert e[k][np.argmax(np.abs(e[k]))] > 0
        seen += 1
    assert seen >= 40


def test_degenerate_frames_are_proper():
    for name, pos in _degenerate().items():
        fr = AR.frame64(pos.astype(np.float32))
        assert _proper(fr, 1e-12), name
        assert fr[12] >= 0.5 and (fr[13:] >= -1e-12).all() and fr[13] >= fr[14] >= fr[15], name
    none = AR.frame64(np.zeros((0, 3), dtype=np.float32))
    assert none.tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0, 0, 0]
    one = AR.frame64(_degenerate()['one'].astype(np.float32))
    assert one[:3].tolist() == [1.5, -2.25, 0.125] and one[3:12].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and one[12] == 0.5
    line = AR.frame64(_degenerate()['line'].astype(np.float32))
    assert np.abs(np.abs(line[3:6]) - [0.6, 0.48, 0.64]).max() <= 1e-6 and line[3] > 0 and abs(line[14]) <= 1e-12


def test_gradient_is_the_derivative(ref):
    """The force and the torque of the restatement against central differences of its own objective, with colour."""
    f = np.float64
    a, b = (ref['sides'][i] for i in ref['notes']['different'][1])
    tm = AR.terms_of(a, b, T, f)
    (av, ac), (bv, bc) = AR.self_overlaps(a, T, True, f), AR.self_overlaps(b, T, True, f)
    q, p, w, h = AR.quat_normalised([0.9, 0.1, -0.3, 0.2], f), np.array([0.3, -0.2, 0.5]), f(0.25), 1e-6
    at = lambda q_, p_: AR.evaluate(a.pos.astype(f), AR.posed(b, q_, p_, f), p_, tm, (av, bv, ac, bc), w, True, f)        # noqa: E731
    e = at(q, p)
    assert e.c > 0 and e.v > 0
    for i in range(3):
        dp = np.zeros(3)
        dp[i] = h
        assert abs((at(q, p + dp).f - at(q, p - dp).f) / (2 * h) - e.force[i]) <= 1e-8
        turned = (at(AR.quat_mul(AR.quat_exp(dp, f), q, f), p).f - at(AR.quat_mul(AR.quat_exp(-dp, f), q, f), p).f) / (2 * h)
        assert abs(turned - e.torque[i]) <= 1e-8


def _frames_file(path, sets):
    rows = ['mols %d' % len(sets)]
    for pos in sets:
        rows.append('mol %d' % len(pos))
        rows += [' '.join(hex32(x) for x in p) for p in pos]
    path.write_text('\n'.join(rows) + '\n')


def test_host_program_frames_and_starts(ref, program, tmp_path):
    """align_frame and align_start of the core header against the restatement: corpus molecules in pairs (A, B), then the
    degenerate sets."""
    pairs = [p[:2] for p in ref['pairs'] if p[2] in ('rigid', 'different', 'far')][::3]
    sets = [ref['sides'][i].pos for pair in pairs for i in pair] + [p.astype(np.float32) for p in _degenerate().values()]
    _frames_file(tmp_path / 'frames.txt', sets)
    out = [ln.split() for ln in run_program(program, 'frames', tmp_path / 'frames.txt')]
    frames = {int(f[1]): np.array([float.fromhex(x) for x in f[2:]]) for f in out if f and f[0] == 'frame'}
    starts = {(int(f[1]), int(f[2])): np.array([float.fromhex(x) for x in f[3:]]) for f in out if f and f[0] == 'start'}
    assert len(frames) == len(sets) and len(starts) == 5 * (len(sets) // 2)
    tol = ref['tol'].frame
    for i, pos in enumerate(sets):
        want = AR.frame64(pos)
        assert _proper(frames[i]), i
        worst = np.abs(frames[i] - want)
        assert (worst[:3] <= tol[:3]).all() and (worst[12:] <= tol[12:]).all(), (i, worst)
        if i < 2 * len(pairs) and len(pos) >= 3:                       # the gaps are at least 0.05 there: the axes are decided
            assert (worst[3:12] <= tol[3:12]).all(), (i, worst)
    f = np.float32
    for i, (ia, ib) in enumerate(pairs):
        for k in range(5):
            q, p = AR.start_pose(k, ref['sides'][ia], ref['sides'][ib], f)
            got = starts[(i, k)]
            assert np.abs(AR.quat_matrix(got[:4], np.float64) - AR.quat_matrix(q, np.float64)).max() <= FEW, (i, k)
            assert np.array_equal(got[4:].astype(f), p), (i, k)
            if k == 0:
                assert got[:4].tolist() == [1, 0, 0, 0]


def test_host_program_quaternions(ref, program, tmp_path):
    rng = np.random.default_rng(3)
    f, f8 = np.float32, np.float64
    quats = [np.array(q, dtype=f) for q in ([1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0.5, 0.5, 0.5, 0.5], [0, 0.6, 0.8, 0],
                                            [1e-4, 1, 0, 0], [0.7071, -0.7071, 0, 0])] + [rng.normal(size=4).astype(f) * 3 for _ in range(40)]
    vecs = [np.array(v, dtype=f) for v in ([0, 0, 0], [1e-8, 0, 0], [2e-6, -1e-6, 0], [np.pi, 0, 0], [0, 6.0, 0], [0.3, -0.2, 0.1])]
    vecs += [rng.normal(size=3).astype(f) for _ in range(20)]
    trials = [(AR.quat_normalised(rng.normal(size=4), f), rng.normal(size=3).astype(f) * 5, d / np.linalg.norm(d), f(s), f(rho))
              for d, s, rho in ((rng.normal(size=6), 0.5 * 1.5 ** k, 0.5 + k) for k in range(8))]
    grads = [(rng.normal(size=3).astype(f), rng.normal(size=3).astype(f), f(2.5)), (np.zeros(3, f), np.zeros(3, f), f(1.0)),
             (np.array([1e-30, 0, 0], f), np.zeros(3, f), f(1.0))]
    rows = ['q ' + ' '.join(hex32(x) for x in q) for q in quats] + ['e ' + ' '.join(hex32(x) for x in v) for v in vecs]
    rows += ['t ' + ' '.join(hex32(x) for x in np.concatenate([q, p, d.astype(f), [s, rho]])) for q, p, d, s, rho in trials]
    rows += ['g ' + ' '.join(hex32(x) for x in np.concatenate([fo, to, [rho]])) for fo, to, rho in grads]
    (tmp_path / 'quat.txt').write_text('\n'.join(rows) + '\n')
    out = [ln.split() for ln in run_program(program, 'quat', tmp_path / 'quat.txt') if ln]
    vals = lambda tag: [np.array([float.fromhex(x) for x in ln[1:]]) for ln in out if ln[0] == tag]       # noqa: E731
    orth, det = ref['rigidity_floor']
    for q, m, back in zip(quats, vals('matrix'), vals('back')):
        unit = q.astype(f8) / np.linalg.norm(q.astype(f8))
        r = m.reshape(3, 3)
        assert np.abs(r - AR.quat_matrix(unit, f8)).max() <= FEW
        assert np.abs(r.T @ r - np.eye(3)).max() <= 4 * orth and abs(np.linalg.det(r) - 1) <= 4 * det
        assert min(np.abs(back - unit).max(), np.abs(back + unit).max()) <= FEW, q      # the round trip, up to the sign of q
    assert vals('matrix')[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for v, e in zip(vecs, vals('exp')):
        assert np.abs(e - AR.quat_exp(v.astype(f8), f8)).max() <= FEW and abs(np.linalg.norm(e) - 1) <= FEW, v
    assert vals('exp')[0].tolist() == [1, 0, 0, 0]
    for (q, p, d, s, rho), got in zip(trials, vals('trial')):
        d8 = d.astype(f).astype(f8)
        want_q = AR.quat_normalised(AR.quat_mul(AR.quat_exp(f8(s) / f8(rho) * d8[3:], f8), q.astype(f8), f8), f8)
        assert np.abs(got[:4] - want_q).max() <= FEW and np.abs(got[4:] - (p.astype(f8) + f8(s) * d8[:3])).max() <= FEW * 8
    (ok0, d0), (ok1, _), (ok2, _) = [(int(g[0]), g[1:]) for g in vals('direction')]
    g6 = np.concatenate([grads[0][0], grads[0][1] / grads[0][2]]).astype(f8)
    assert ok0 == 1 and np.abs(d0 - g6 / np.linalg.norm(g6)).max() <= FEW
    assert ok1 == 0 and ok2 == 0                                       # |g6| = 0, in fp32 as the kernel computes it


@pytest.mark.parametrize('first,least,most,scores', [
    (0.5, 1e-4, 128, [0.2, 0.3, 0.3, 0.25, 0.31, 0.4, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]),
    (0.5, 1e-4, 1, [0.7]),
    (0.5, 1e-4, 4, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]),
    (1.0, 0.25, 128, [0.5, 0.5, 0.5, 0.5, 0.5]),
    (0.5, 0.5, 128, [0.0, float('nan'), 1.0]),
])
def test_host_program_step_rule(program, first, least, most, scores):
    """The accept / reject sequence on a scripted objective: a strictly better trial is accepted and lengthens the step by 1.5, any
    other (an equal one, a NaN) shortens it by 0.5; the walk ends below min_step or after max_steps evaluations, the first counting."""
    want_seq, want_steps, want_s, want_f = AR.scripted(scores, first, least, most)
    out = run_program(program, 'steps', hex32(first), hex32(least), most, *[hex32(x) for x in scores])
    got_seq = [ln == 'accept' for ln in out if ln in ('accept', 'reject')]
    end = next(ln.split() for ln in out if ln.startswith('end'))
    assert got_seq == want_seq and int(end[1]) == want_steps <= most
    assert float.fromhex(end[2]) == want_s and float.fromhex(end[3]) == want_f
    if most == 1:
        assert got_seq == []
    if least == 0.25:
        assert got_seq == [False, False, False]                        # equal scores: never accepted; 1 -> 0.5 -> 0.25 -> 0.125 < min


def test_corpus_conditions(ref):
    """Judged by the restatement alone: the sizes and variants, the eigenvalue gaps, the recovery of moved copies, the far pair, and
    that the fp32 and the float64 run agree on every pair of different molecules."""
    mols, notes, sides, tol = ref['mols'], ref['notes'], ref['sides'], ref['tol']
    counts = [len(s.pos) for s in sides]
    assert {0, 1, 2, 3, 5, 17, 63, 64, 65, 128} <= set(counts)
    first, middle, last = (mols[i] for i in notes['dropped'])
    assert first.cls[0] == 11 and middle.cls[9] == middle.cls[10] == 11 and last.cls[-1] == 11
    assert SR.status_of(mols[notes['nan']]) == SR.NONFINITE and SR.status_of(mols[notes['empty']]) == SR.EMPTY
    src, dup = notes['duplicate']
    assert np.array_equal(mols[src].pos, mols[dup].pos)
    assert any((m.fp != 0).any() for m in mols) and any((m.fp == 0).all() and len(m.fp) > 1 for m in mols)
    # 1. eigenvalue gaps of every molecule that a frame comparison or a recovery test uses (one and two atoms: properness only)
    for ia, ib, kind in ref['pairs']:
        for i in (ia, ib):
            if kind in ('rigid', 'perturbed', 'different', 'far') and counts[i] >= 3:
                assert min(AR.eigen_gaps(sides[i].pos)) >= 0.05, (i, AR.eigen_gaps(sides[i].pos))
    # the far pair: nothing overlaps in place, in float64 too, and the inertial starts find the copy
    (ia, ib), = notes['far']
    far = ref['plain64'][[p[:2] for p in ref['pairs']].index((ia, ib))]
    assert far.ascents[0].v == 0.0 and far.ascents[0].steps == 1 and far.best.start >= 1 and 1.0 - far.best.st <= 1e-9
    # recovery, float64: the inertial starts on the rigid copies, the in-place start on the perturbed ones
    kinds = [p[2] for p in ref['pairs']]
    worst = {k: max(1.0 - (r.best.st if k == 'rigid' else r.ascents[0].st) for r, kk in zip(ref[run], kinds) if kk == k)
             for run in ('plain64', 'plain32') for k in ('rigid', 'perturbed')}
    print('recovery, worst 1 - ST of the fp32 run: rigid %.3e, perturbed in place %.3e' % (worst['rigid'], worst['perturbed']))
    for r, k in zip(ref['plain64'], kinds):
        if k == 'rigid':
            assert 1.0 - r.best.st <= 1e-9
        if k == 'perturbed':
            assert 1.0 - r.ascents[0].st <= 1e-6 and r.ascents[0].steps <= AR.MAX_STEPS
    assert worst['rigid'] <= tol.sim and worst['perturbed'] <= tol.sim
    # 2. the two runs agree on the winning score of every pair of different molecules: none to excuse
    print('floors: score %.3e, transform %.3e relative %.3e absolute, rigidity %.3e %.3e' % (tol.score_floor, *ref['transform_floor'], *ref['rigidity_floor']))
    print('tolerances: overlap %.3e sim %.3e score %.3e frame %s' % (tol.overlap, tol.sim, tol.score, tol.frame[[0, 3, 12, 13]]))
    for name in ('plain', 'colour'):
        for (ia, ib, kind), lo, hi in zip(ref['pairs'] if name == 'plain' else ref['colour_pairs'], ref[name + '32'], ref[name + '64']):
            if kind == 'different':
                assert abs(lo.best.score - hi.best.score) <= tol.score, (name, ia, ib)
                assert all(x.steps <= AR.MAX_STEPS for x in hi.ascents)
    assert 1e-8 < tol.score_floor < 1e-5 and tol.score == max(4 * tol.score_floor, AR.SIM_TOL)
    assert any(hi.best.ct > 0 for hi in ref['colour64']) and any(hi.best.ct == 0 for hi in ref['colour64'])
    # empty rows have no overlay; a one-atom molecule on itself ties all five starts
    for (ia, ib, kind), hi in zip(ref['pairs'], ref['plain64']):
        assert (hi.best is None) == (kind == 'empty')
        if kind == 'self':
            assert [x.score for x in hi.ascents] == [1.0] * 5 and hi.best.start == 0
