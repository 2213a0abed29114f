"""The float64 restatement of the rigid overlay (DESIGN.md 2.9 "Shape alignment"; phoregen_amd/shape.py, csrc/shape_align.hip): the
frame of a molecule, the five starts, the objective with its gradient written as the definition states it (the force on every atom of
B, the torque about p), the step rule and the winner -- plain numpy.  It is handed the tables of phoregen_amd.shape
(`shape_reference.tables`) and shares nothing else with it.  Every function takes the number type: the float64 run is the yardstick,
the numpy-fp32 run of the same algorithm is what the tolerance floors are measured from (`tolerances`).  The frame is computed in
double in both, as defined.  Beside them the corpus.  CPU only."""
from typing import NamedTuple

import numpy as np

import shape_reference as SR

FRAME = 16
JACOBI_SWEEPS = 8
GROW, SHRINK, MIN_RHO = 1.5, 0.5, 0.5
MAX_STEPS, FIRST_STEP, MIN_STEP = 128, 0.5, 1e-4
SIGNS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))
STARTS = {'in_place': (0,), 'inertial': (1, 2, 3, 4), 'both': (0, 1, 2, 3, 4)}
_POP = np.array([bin(i).count('1') for i in range(256)], dtype=np.float64)


# ---- the frame (always double) ----------------------------------------------------------------------------------------------------------
def jacobi(a):
    """(eigenvalues descending, eigenvectors as columns, right-handed) of a symmetric 3 x 3 matrix: cyclic Jacobi over (0,1), (0,2),
    (1,2) with a fixed number of sweeps, a stable sort, the largest-magnitude component of e1 and e2 positive (the first such
    component decides a tie), e3 = e1 x e2."""
    a, v = np.array(a, dtype=np.float64), np.eye(3)
    with np.errstate(over='ignore'):
        for _ in range(JACOBI_SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                if a[p, q] == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * a[p, q])
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                j = np.eye(3)
                j[p, p] = j[q, q] = c
                j[p, q], j[q, p] = s, -s
                a, v = j.T @ a @ j, v @ j
    lam = np.diag(a).copy()
    for i, k in ((0, 1), (1, 2), (0, 1)):
        if lam[k] > lam[i]:
            lam[[i, k]], v[:, [i, k]] = lam[[k, i]], v[:, [k, i]]
    for i in (0, 1):
        big = 0
        for k in (1, 2):
            if abs(v[k, i]) > abs(v[big, i]):
                big = k
        if v[big, i] < 0.0:
            v[:, i] = -v[:, i]
    v[:, 2] = np.cross(v[:, 0], v[:, 1])
    return lam, v


def frame64(pos):
    """The 16 numbers of a frame in float64 from the fp32 coordinates [n, 3] of the kept atoms: centroid 3, axes 9 (axis k at
    3 + 3 k), rho, eigenvalues 3.  The sums add the atoms in order.  No atoms: origin, identity, rho 0.5, zeros."""
    x = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    c = np.cumsum(x, axis=0)[-1] / n if n else np.zeros(3)
    d = x - c
    cov = np.cumsum(d[:, :, None] * d[:, None, :], axis=0)[-1] / n if n else np.zeros((3, 3))
    lam, v = jacobi(cov)
    return np.concatenate([c, v.T.reshape(-1), [max(np.sqrt(np.trace(cov)), MIN_RHO)], lam])


def frame(pos):
    """The frame as the device holds it: float64, rounded once."""
    return frame64(pos).astype(np.float32)


def eigen_gaps(pos):
    """The two gaps of the covariance's eigenvalues, relative to the largest (0 for fewer than two atoms)."""
    lam = frame64(pos)[13:]
    return ((lam[0] - lam[1]) / lam[0], (lam[1] - lam[2]) / lam[0]) if lam[0] > 0 else (0.0, 0.0)


# ---- quaternions (w, x, y, z) in the number type f ----------------------------------------------------------------------------------------
def quat_matrix(q, f):
    w, x, y, z = (f(c) for c in q)
    one, two = f(1), f(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=f)


def quat_normalised(q, f):
    q = np.asarray(q, dtype=f)
    return (q / np.sqrt((q * q).sum(dtype=f))).astype(f)


def matrix_quat(r, f):
    r = np.asarray(r, dtype=f)
    tr, one = r[0, 0] + r[1, 1] + r[2, 2], f(1)
    if tr >= r[0, 0] and tr >= r[1, 1] and tr >= r[2, 2]:
        q = [one + tr, r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]]
    elif r[0, 0] >= r[1, 1] and r[0, 0] >= r[2, 2]:
        q = [r[2, 1] - r[1, 2], one + r[0, 0] - r[1, 1] - r[2, 2], r[0, 1] + r[1, 0], r[0, 2] + r[2, 0]]
    elif r[1, 1] >= r[2, 2]:
        q = [r[0, 2] - r[2, 0], r[0, 1] + r[1, 0], one - r[0, 0] + r[1, 1] - r[2, 2], r[1, 2] + r[2, 1]]
    else:
        q = [r[1, 0] - r[0, 1], r[0, 2] + r[2, 0], r[1, 2] + r[2, 1], one - r[0, 0] - r[1, 1] + r[2, 2]]
    return quat_normalised(q, f)


def quat_mul(a, b, f):
    aw, ax, ay, az = (f(c) for c in a)
    bw, bx, by, bz = (f(c) for c in b)
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dtype=f)


def quat_exp(rv, f):
    """The rotation by |rv| about rv / |rv|."""
    rv = np.asarray(rv, dtype=f)
    angle = np.sqrt((rv * rv).sum(dtype=f))
    k = np.sin(f(0.5) * angle) / angle if angle > f(1e-6) else f(0.5)
    return np.concatenate([[np.cos(f(0.5) * angle)], k * rv]).astype(f)


# ---- one molecule as the optimiser sees it ----------------------------------------------------------------------------------------------
class Side(NamedTuple):
    pos: np.ndarray              # float32 [n, 3] kept atoms in packed order (n = 0: an empty row)
    cls: np.ndarray              # int [n]
    fp: np.ndarray               # int [n]
    frame: np.ndarray            # float32 [16]


def side(m):
    k = SR.kept(m) if SR.status_of(m) == 0 else np.zeros(len(m.cls), dtype=bool)
    pos = m.pos[k].astype(np.float32)
    return Side(pos, m.cls[k].astype(np.int64), m.fp[k].astype(np.int64), frame(pos))


class Eval(NamedTuple):
    v: float
    c: float
    st: float
    ct: float
    f: float
    force: np.ndarray
    torque: np.ndarray


def _tanimoto(ab, aa, bb, f):
    den = (aa + bb) - ab
    return ab / den if den > 0 else f(0)


def _slope(ab, aa, bb, f):
    den = (aa + bb) - ab
    return (aa + bb) / (den * den) if den > 0 else f(0)


def _score(st, ct, w, f):
    return f(f(f(1) - w) * st) + f(w * ct)


class Terms(NamedTuple):
    """The pair tables of A against B in the number type: weight and exponent factor of every shape term, the popcounts, and the
    colour weight and factor."""
    wv: np.ndarray
    kv: np.ndarray
    pop: np.ndarray
    wc: float
    kc: float


def terms_of(a, b, t, f):
    ai, aj = t.alpha.astype(f)[a.cls][:, None], t.alpha.astype(f)[b.cls][None, :]
    s = ai + aj
    p, pi, ac = f(t.p), f(np.pi), f(t.alpha_c)
    return Terms((p * p * (pi / s) ** f(1.5)).astype(f), (ai * aj / s).astype(f), _POP[a.fp[:, None] & b.fp[None, :]].astype(f),
                 f(p * p * (pi / (ac + ac)) ** f(1.5)), f(ac * ac / (ac + ac)))


def overlap(xa, yb, tm, colour, f):
    """(V, C, g [na, nb], gc [na, nb], d [na, nb, 3]) at A's and B's positions, all in f."""
    d = (xa[:, None, :] - yb[None, :, :]).astype(f)
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    with np.errstate(under='ignore'):
        g = (tm.wv * np.exp(-tm.kv * d2)).astype(f)
        gc = (tm.pop * (tm.wc * np.exp(-tm.kc * d2))).astype(f) if colour else None
    return g.sum(dtype=f), (gc.sum(dtype=f) if colour else f(0)), g, gc, d


def evaluate(xa, yb, p, tm, self4, w, colour, f):
    """The objective and its gradient at B's posed positions yb: the force on B's atom j is sum_i 2 k g (x_i - y'_j), F their sum,
    tau = sum_j (y'_j - p) x f_j; shape and colour parts weighted by the chain rule through the two Tanimoto values."""
    aa_v, bb_v, aa_c, bb_c = self4
    v, c, g, gc, d = overlap(xa, yb, tm, colour, f)
    st, ct = _tanimoto(v, aa_v, bb_v, f), (_tanimoto(c, aa_c, bb_c, f) if colour else f(0))
    fj = f(f(1) - w) * _slope(v, aa_v, bb_v, f) * ((f(2) * tm.kv * g)[..., None] * d).sum(axis=0, dtype=f)
    if colour:
        fj = fj + w * _slope(c, aa_c, bb_c, f) * ((f(2) * tm.kc * gc)[..., None] * d).sum(axis=0, dtype=f)
    fj = fj.astype(f)
    return Eval(v, c, st, ct, _score(st, ct, w, f), fj.sum(axis=0, dtype=f), np.cross((yb - p).astype(f), fj).sum(axis=0, dtype=f).astype(f))


def posed(b, q, p, f):
    """R(q) (y - c_B) + p."""
    return ((b.pos.astype(f) - b.frame[:3].astype(f)) @ quat_matrix(q, f).T + p).astype(f)


def start_pose(k, a, b, f):
    if k == 0:
        return np.array([1, 0, 0, 0], dtype=f), b.frame[:3].astype(f)
    ea, eb = a.frame[3:12].astype(f).reshape(3, 3), b.frame[3:12].astype(f).reshape(3, 3)        # rows: the axes
    r = sum(f(SIGNS[k - 1][m]) * np.outer(ea[m], eb[m]) for m in range(3)).astype(f)
    return matrix_quat(r, f), a.frame[:3].astype(f)


class Ascent(NamedTuple):
    """Where one start ended."""
    start: int
    v: float
    c: float
    st: float
    ct: float
    score: float
    rotation: np.ndarray
    translation: np.ndarray
    steps: int
    accepted: list               # the accept / reject sequence, one bool per trial


def ascend(k, a, b, tm, self4, w, colour, f, max_steps=MAX_STEPS, first_step=FIRST_STEP, min_step=MIN_STEP):
    q, p = start_pose(k, a, b, f)
    w, rho, xa = f(w), f(b.frame[12]), a.pos.astype(f)
    cur = evaluate(xa, b.pos.astype(f) if k == 0 else posed(b, q, p, f), p, tm, self4, w, colour, f)       # start 0: B as stored
    steps, s, accepted = 1, f(first_step), []
    while not (s < f(min_step) or steps >= max_steps):
        g6 = np.concatenate([cur.force, cur.torque / rho]).astype(f)
        norm = np.sqrt((g6 * g6).sum(dtype=f))
        if not (norm > 0 and np.isfinite(norm)):
            break
        d = (g6 / norm).astype(f)
        pt = (p + s * d[:3]).astype(f)
        qt = quat_normalised(quat_mul(quat_exp((s / rho) * d[3:], f), q, f), f)
        trial = evaluate(xa, posed(b, qt, pt, f), pt, tm, self4, w, colour, f)
        steps += 1
        better = bool(trial.f > cur.f)
        accepted.append(better)
        if better:
            cur, q, p = trial, qt, pt
        s = f(s * f(GROW if better else SHRINK))
    r = quat_matrix(q, f)
    return Ascent(k, float(cur.v), float(cur.c), float(cur.st), float(cur.ct), float(cur.f), r.astype(np.float64),
                  (p - r @ b.frame[:3].astype(f)).astype(np.float64), steps, accepted)


class Overlay(NamedTuple):
    best: Ascent                 # the winner: the largest final score, ties to the lowest start; None for a pair with an empty row
    ascents: list                # every start's end, in start order


def self_overlaps(s, t, colour, f):
    if len(s.pos) == 0:
        return f(0), f(0)
    v, c, *_ = overlap(s.pos.astype(f), s.pos.astype(f), terms_of(s, s, t, f), colour, f)
    return v, c


def overlay(a, b, t, w=0.0, colour=False, f=np.float64, starts='both', **step):
    """The overlay of B onto A.  colour: both sets have colour; with w = 0 the colour terms are skipped and C = CT = 0."""
    if len(a.pos) == 0 or len(b.pos) == 0:
        return Overlay(None, [])
    colour = bool(colour) and w > 0
    (aa_v, aa_c), (bb_v, bb_c) = self_overlaps(a, t, colour, f), self_overlaps(b, t, colour, f)
    tm = terms_of(a, b, t, f)
    ascents = [ascend(k, a, b, tm, (aa_v, bb_v, aa_c, bb_c), w, colour, f, **step) for k in STARTS[starts]]
    best = ascents[0]
    for x in ascents[1:]:
        if x.score > best.score:
            best = x
    return Overlay(best, ascents)


def overlaps_at(a, yb, b, t, colour):
    """float64 (V, C, ST, CT) of A against B's atoms at the positions yb."""
    f = np.float64
    tm = terms_of(a, b, t, f)
    v, c, *_ = overlap(a.pos.astype(f), np.asarray(yb, dtype=f), tm, colour, f)
    (aa_v, aa_c), (bb_v, bb_c) = self_overlaps(a, t, colour, f), self_overlaps(b, t, colour, f)
    return float(v), float(c), float(_tanimoto(v, aa_v, bb_v, f)), float(_tanimoto(c, aa_c, bb_c, f)) if colour else 0.0


# ---- tolerances, measured -----------------------------------------------------------------------------------------------------------------
def rigidity_floor(n=100000, seed=5):
    """max |R^T R - I| and max |det R - 1| of the fp32 quaternion-to-matrix formula on n random unit quaternions (normalised in
    fp32), judged in float64."""
    f = np.float32
    q = np.random.default_rng(seed).normal(size=(n, 4)).astype(f)
    q = (q / np.sqrt((q * q).sum(axis=1, dtype=f))[:, None]).astype(f)
    w, x, y, z = q.T
    one, two = f(1), f(2)
    r = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y), two * (x * y + w * z), one - two * (x * x + z * z),
                  two * (y * z - w * x), two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    assert r.dtype == f
    r = r.astype(np.float64)
    return float(np.abs(np.einsum('nki,nkj->nij', r, r) - np.eye(3)).max()), float(np.abs(np.linalg.det(r) - 1.0).max())


class Tolerances(NamedTuple):
    frame: np.ndarray            # [16] absolute: 4 x the largest fp32 rounding of the float64 frames, per group of numbers
    orthogonal: float            # max |R^T R - I|: 4 x the fp32 floor
    det: float                   # |det R - 1|: 4 x the fp32 floor
    overlap: float               # relative, V and C against similarity() at the returned transform: 4 x the transform floor + 9.0e-6
    sim: float                   # absolute, ST and CT likewise: 4 x the transform floor + 2.7e-5
    score_floor: float           # the largest |score fp32 - score float64| of the two restatement runs
    score: float                 # absolute, against the restatement: max(4 x score_floor, 2.7e-5)


OVERLAP_TOL, SIM_TOL = 9.0e-6, 2.7e-5      # the in-place module's measured tolerances (tests/test_molshape_host.py)


def frame_tolerance(frames64):
    """Per number of a frame: 4 x the largest |fp32(x) - x| over the corpus within its group (centroid, axes, rho, eigenvalues)."""
    err = np.abs(np.asarray(frames64).astype(np.float32).astype(np.float64) - np.asarray(frames64))
    out = np.zeros(FRAME)
    for lo, hi in ((0, 3), (3, 12), (12, 13), (13, 16)):
        out[lo:hi] = 4.0 * err[:, lo:hi].max()
    return out


def transform_floor(sides, pairs, runs32, t, colour):
    """(relative on V and C, absolute on ST and CT): over the pairs, two float64 evaluations of the overlaps -- at B's coordinates
    moved by the fp32 run's (R, t) in fp32 arithmetic and in float64 arithmetic."""
    rel = ab = 0.0
    for (ia, ib), run in zip(pairs, runs32):
        if run.best is None:
            continue
        a, b = sides[ia], sides[ib]
        r32, t32 = run.best.rotation.astype(np.float32), run.best.translation.astype(np.float32)
        y32 = (b.pos @ r32.T + t32).astype(np.float32)
        assert y32.dtype == np.float32
        y64 = b.pos.astype(np.float64) @ r32.astype(np.float64).T + t32.astype(np.float64)
        lo, hi = overlaps_at(a, y32, b, t, colour), overlaps_at(a, y64, b, t, colour)
        for k in (0, 1):
            if hi[k] >= SR.TINY:
                rel = max(rel, abs(lo[k] - hi[k]) / hi[k])
        ab = max(ab, abs(lo[2] - hi[2]), abs(lo[3] - hi[3]))
    return rel, ab


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------------
def _rotation(rng, angle=None):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0.3, np.pi) if angle is None else angle
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def _direction(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def _mol(rng, n_kept, dropped=(), ring=False, coloured=True, need_gap=True):
    """n_kept kept atoms of mixed elements on a random walk and dropped atoms (class 11) at the rows `dropped`; drawn again until the
    eigenvalue gaps of the kept atoms are at least 0.05 (three atoms and more)."""
    n = n_kept + len(dropped)
    while True:
        cls = rng.choice(11, size=n, p=np.array([1, 30, 8, 8, 2, 1, 1, 2, 2, 1, 1]) / 57.0)
        cls[list(dropped)] = 11
        pos = (SR.walk(rng, n, ring) + rng.normal(0, 1.0, size=3)).astype(np.float32)
        fp = rng.integers(0, 256, size=n).astype(np.uint8) if coloured else np.zeros(n, dtype=np.uint8)
        m = SR.Mol(cls.astype(np.int64), pos, fp)
        if n_kept < 3 or not need_gap or min(eigen_gaps(pos[SR.kept(m)])) >= 0.05:
            return m


def _moved(m, rot, shift):
    """The molecule turned by `rot` about the centroid of all its rows and shifted, rounded to fp32."""
    x = m.pos.astype(np.float64)
    c = x.mean(axis=0) if len(x) else np.zeros(3)
    return SR.Mol(m.cls.copy(), ((x - c) @ rot.T + c + shift).astype(np.float32), m.fp.copy())


SIZES = (1, 2, 3, 5, 17, 63, 64, 65, 128)


def corpus(seed=23):
    """(molecules, notes).  Kept-atom counts 0, 1, 2 (collinear), 3 (planar), 5, 17, 63, 64, 65, 128; dropped atoms first, in the
    middle and last; a NaN row; an exact duplicate; of every one of those molecules a rigidly moved copy (a random rotation, a shift of
    up to 3 Angstrom) and a perturbed copy (20 degrees about a random axis, 0.7 Angstrom); ten different molecules of 8 to 50 atoms; a
    far-away copy.  Feature bytes on part of the corpus (the others carry 0).  notes: 'sizes' {n: row}, 'empty', 'nan', 'dropped',
    'duplicate' (src, copy), and the pair lists 'rigid', 'perturbed', 'different', 'far' of (row of a, row of b)."""
    rng = np.random.default_rng(seed)
    mols, notes = [], {'sizes': {}}
    for k, n in enumerate(SIZES):
        notes['sizes'][n] = len(mols)
        mols.append(_mol(rng, n, ring=bool(k & 1), coloured=n not in (2, 63)))
    notes['empty'] = len(mols)
    mols.append(_mol(rng, 0, dropped=(0, 1, 2)))
    notes['dropped'] = [len(mols), len(mols) + 1, len(mols) + 2]
    mols += [_mol(rng, 20, dropped=(0,)), _mol(rng, 20, dropped=(9, 10)), _mol(rng, 20, dropped=(20,), ring=True)]
    nan = _mol(rng, 12)
    nan.pos[5, 1] = np.nan
    notes['nan'] = len(mols)
    mols.append(nan)
    notes['duplicate'] = (notes['sizes'][17], len(mols))
    mols.append(SR.Mol(*(x.copy() for x in mols[notes['sizes'][17]])))
    sources = [notes['sizes'][n] for n in SIZES] + notes['dropped']
    notes['rigid'], notes['perturbed'] = [], []
    for src in sources:
        notes['rigid'].append((src, len(mols)))
        mols.append(_moved(mols[src], _rotation(rng), rng.uniform(0.5, 3.0) * _direction(rng)))
        notes['perturbed'].append((src, len(mols)))
        mols.append(_moved(mols[src], _rotation(rng, np.deg2rad(20.0)), 0.7 * _direction(rng)))
    first = len(mols)
    for k, n in enumerate((8, 12, 19, 23, 27, 31, 36, 41, 46, 50)):
        mols.append(_mol(rng, n, ring=bool(k & 1), coloured=k != 3))
    notes['different'] = [(first + i, first + (i + d) % 10) for d in (1, 3) for i in range(10)]
    notes['far'] = [(first + 2, len(mols))]
    mols.append(_moved(mols[first + 2], _rotation(rng), np.array([60.0, -60.0, 60.0])))
    return mols, notes


# ---- the step rule on a scripted objective ------------------------------------------------------------------------------------------------
def scripted(scores, first_step, min_step, max_steps, f=np.float32):
    """(accept / reject sequence, evaluations, final step, final score) of the step rule fed the scores of the start and of its
    trials from a list."""
    cur, s, steps, seq = f(scores[0]), f(first_step), 1, []
    while not (s < f(min_step) or steps >= max_steps):
        trial = f(scores[steps])
        steps += 1
        better = bool(trial > cur)
        seq.append(better)
        if better:
            cur = trial
        s = f(s * f(GROW if better else SHRINK))
    return seq, steps, float(s), float(cur)


# ---- the reference runs over the corpus, computed once per process -------------------------------------------------------------------------
_REFERENCE = {}
COLOUR_WEIGHT = 0.25


def reference(t):
    """Everything the tests share: the corpus, its sides, the pair list with the kind of every pair, the float64 and the fp32 run
    over all pairs at w = 0 ('plain') and over the pairs of different molecules with colour at w = COLOUR_WEIGHT ('colour'), and the
    tolerances measured from them."""
    if 'ref' in _REFERENCE:
        return _REFERENCE['ref']
    mols, notes = corpus()
    sides = [side(m) for m in mols]
    pairs = [(ia, ib, kind) for kind in ('rigid', 'perturbed', 'different', 'far') for ia, ib in notes[kind]]
    one = notes['sizes'][1]
    pairs += [(one, one, 'self'), (notes['duplicate'][0], notes['duplicate'][1], 'duplicate'), (notes['empty'], 3, 'empty'),
              (3, notes['nan'], 'empty')]
    run = lambda ia, ib, w, colour, f: overlay(sides[ia], sides[ib], t, w, colour, f)        # noqa: E731
    out = dict(mols=mols, notes=notes, sides=sides, pairs=pairs,
               plain64=[run(ia, ib, 0.0, False, np.float64) for ia, ib, _ in pairs],
               plain32=[run(ia, ib, 0.0, False, np.float32) for ia, ib, _ in pairs])
    out['colour_pairs'] = [(ia, ib, kind) for ia, ib, kind in pairs if kind == 'different']
    out['colour64'] = [run(ia, ib, COLOUR_WEIGHT, True, np.float64) for ia, ib, _ in out['colour_pairs']]
    out['colour32'] = [run(ia, ib, COLOUR_WEIGHT, True, np.float32) for ia, ib, _ in out['colour_pairs']]
    floor = max(abs(lo.best.score - hi.best.score) for lo, hi in zip(out['plain32'] + out['colour32'], out['plain64'] + out['colour64'])
                if hi.best is not None)
    rel0, abs0 = transform_floor(sides, [p[:2] for p in pairs], out['plain32'], t, False)
    rel1, abs1 = transform_floor(sides, [p[:2] for p in out['colour_pairs']], out['colour32'], t, True)
    orth, det = rigidity_floor()
    out['transform_floor'] = (max(rel0, rel1), max(abs0, abs1))
    out['rigidity_floor'] = (orth, det)
    out['tol'] = Tolerances(frame_tolerance([frame64(s.pos) for s in sides]), 4.0 * orth, 4.0 * det, 4.0 * max(rel0, rel1) + OVERLAP_TOL,
                            4.0 * max(abs0, abs1) + SIM_TOL, floor, max(4.0 * floor, SIM_TOL))
    _REFERENCE['ref'] = out
    return out


def best_two_gap(run):
    """The winner's score minus the best score of another start (inf with one start)."""
    rest = sorted((x.score for x in run.ascents), reverse=True)
    return rest[0] - rest[1] if len(rest) > 1 else np.inf
