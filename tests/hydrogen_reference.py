"""Plain float64 restatement of the hydrogen placement (DESIGN.md 2.9 "Hydrogens"; phoregen_amd/hydrogens.py, csrc/mol_hydrogens.hip,
csrc/hydrogen_core.h) for the tests: numpy vectors, Python lists and dicts, one site at a time.  It shares the definition with the
document and the core and nothing else.  Besides the outputs it returns, per hydrogen, the smallest norm `s` of any vector it
normalised on the way to that hydrogen, and every quantity a float comparison decided (`decisions`), so that the tests can keep their
inputs away from the thresholds by the restatement alone.  Also here: the hand examples with ideal float64 skeletons, the generator
of the family, the position bound, and the case format of tools/hydrogen_host_check.cpp.  Nothing here holds device code.  What the
kernel reads for one graph comes from stereo_reference.all_rows, without the keys and rings that this kernel does not read.

The position bound.  A hydrogen is p + L dir.  With e = 2^-24 (round to nearest, fp32; the build's divisions and square roots are
correctly rounded) and the fp32 coordinates taken as exact, count the roundings of the longest path, the d = 1 rule, to first order:
  u0 = (p_j - p) / |p_j - p|: the difference 1 (relative, so no coordinate magnitude enters), the squared norm 3, its root 1/2 + 1,
      the quotient 1                                                                                       |du0| <= 4.5 e
  r^ likewise                                                                                              |dr|  <= 4.5 e
  c = u0 . r^: three products and two sums of terms below 1, plus what u0 and r^ carry                     |dc|  <= 3 e + 9 e
  t = r^ - u0 c: a product and a difference per component (3 sqrt(3) e), plus dr, du0 |c| and |u0| dc      |dt|  <= 5.2 e + 21 e
  e1 = t / |t|: dt / s with s = |t|, plus the 4.5 e of the normalisation itself                            |de1| <= 26.2 e / s + 4.5 e
  e2 = u0 x e1: two products and a difference per component (5.2 e), plus du0 and de1                      |de2| <= 9.7 e + |de1|
  dir = cos u0 + sin (cp e1 + sp e2): four rounded constants (4 e), six operations per component (10.4 e), |cos| du0 (1.5 e),
      sin (|cp| de1 + |sp| de2) <= 1.29 |de1| + 7.9 e                                                      |ddir| <= 29.6 e + 33.8 e / s
  p + L dir: the product (L e) and the sum ((max|coordinate| + L) e)
so |error| <= e (max|coordinate| + L (32 + 34 / s)) <= K e (max|coordinate| + L (1 + 1 / s)) with K = 34 from the count; K_BOUND = 40
leaves the second-order terms a sixth.  The other rules are shorter: (3, 1) and trigonal (2, 1) normalise one sum of unit vectors,
tetrahedral (2, h) a sum and a cross product, a vertex of the generic rule nothing at all.  `s` here is the smallest norm of ANY
vector normalised for the hydrogen, bond vectors included, which can only widen the bound where a bond is shorter than the sum."""
import functools
import math
import os

import numpy as np

import kekule_reference as K
import mol_support as MS
import stereo_reference
from mol_support import B_, C_, N_, O_, F_, SI_, P_, S_, CL_, BR_, I_, batch_from, mirrored  # noqa: F401  (read from here by the tests)
from phoregen_amd import hydrogens as HY
from phoregen_amd import molecule as M

K_BOUND = 40                     # 34 roundings on the longest path (module docstring), the rest for second-order terms
EPS32 = 2.0 ** -24
TET, TRIG, LIN, GEN = HY.SHAPE_TETRAHEDRAL, HY.SHAPE_TRIGONAL, HY.SHAPE_LINEAR, HY.SHAPE_GENERIC
VERTICES = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) / math.sqrt(3.0)
TET_COS = -1.0 / 3.0
TIE_MARGIN = 1e-4                # an argmin (axis, vertex) decided by less than this, but not by exactly 0, may flip in fp32


def position_bound(max_coordinate, length, s):
    return K_BOUND * EPS32 * (max_coordinate + length * (1.0 + 1.0 / s))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def graph_of_rows(cls, kekule_order, order):
    """kept [n]; heavy neighbours [n] ascending (pair rows of Kekulé order 1..3 between kept atoms); per atom the number of Kekulé
    double bonds, whether it has a triple bond, whether it has a bond of the screen's order 4."""
    n = len(cls)
    assert len(order) == len(kekule_order)
    w = MS.pair_walk(cls, kekule_order, (1, 2, 3))
    ndbl, triple, arom = [0] * n, [False] * n, [False] * n
    for (a, b), row in w.rows.items():
        if w.order[row] == 2:
            ndbl[a], ndbl[b] = ndbl[a] + 1, ndbl[b] + 1
        if w.order[row] == 3:
            triple[a] = triple[b] = True
    for a, b in MS.pair_walk(cls, order, (4,)).rows:                   # (the screen's order 4, whatever the Kekulé order of the pair)
        arom[a] = arom[b] = True
    return w.kept, w.nbrs, ndbl, triple, arom


def shape_of(cls, ndbl, triple, arom, d, h, conj):
    if triple or ndbl >= 2:
        return LIN
    if ndbl >= 1 or arom or (cls == N_ and d + h == 3 and conj):
        return TRIG
    return TET


class _Site:
    """The arithmetic of one site with its book-keeping: norms normalised (for `s`) and decisions taken."""

    def __init__(self, decisions):
        self.norms, self.decisions = [], decisions

    def unit(self, v, degenerate_below=None):
        """v / |v|, or None: a bond vector (degenerate_below None) needs a positive finite squared norm, a vector of unit inputs one of
        at least DEG_EPS^2."""
        q = float(np.dot(v, v))
        if degenerate_below is not None:
            self.decisions.append(('deg', math.sqrt(q) if q >= 0 and math.isfinite(q) else float('nan')))
        if not (q > 0.0 and math.isfinite(q)) or (degenerate_below is not None and not q >= degenerate_below ** 2):
            return None
        self.norms.append(math.sqrt(q))
        return v / math.sqrt(q)

    def argmin_first(self, values, kind):
        k = int(np.argmin(values))                                     # (numpy's argmin is the first minimum)
        rest = sorted(values)
        self.decisions.append((kind, float(rest[1] - rest[0])))
        return k


def _vertex_dots(e):
    x, y, z = (float(c) for c in e)
    c = 1.0 / math.sqrt(3.0)
    return np.array([c * ((x + y) + z), c * ((x - y) - z), c * ((y - x) - z), c * ((z - x) - y)])


def place_site(i, pos, nbrs, cls, h, ndbl, triple, arom, decisions):
    """(directions [h, 3], shape used, s per hydrogen) of site i, whose own and whose neighbours' coordinates are finite."""
    st = _Site(decisions)
    p, d = pos[i], len(nbrs[i])
    conj = any(ndbl[j] >= 1 or arom[j] for j in nbrs[i])
    shape = shape_of(cls[i], ndbl[i], triple[i], arom[i], d, h, conj)
    us = []
    for j in nbrs[i]:
        u = st.unit(pos[j] - p)
        if u is not None:
            us.append(u)
    bond_norms = list(st.norms)
    total = np.zeros(3)
    for u in us:
        total = total + u
    dirs, s_of = None, None
    inf = float('inf')

    def smallest(*extra):
        return min(bond_norms + list(extra)) if bond_norms or extra else inf

    if len(us) == d:
        if d == 0:
            dirs, s_of = [VERTICES[k] for k in range(h)], [inf] * h
        elif d == 1 and ((shape == TET and h <= 3) or (shape == TRIG and h <= 2)):
            u0, j = us[0], nbrs[i][0]
            others = [w for w in nbrs[j] if w != i]
            ok, r_norm = True, []
            if others:
                before = len(st.norms)
                r = st.unit(pos[others[0]] - pos[j])
                ok, r_norm = r is not None, st.norms[before:]
            else:
                r = np.eye(3)[st.argmin_first([abs(float(c)) for c in u0], 'axis')] * (1.0 if i < j else -1.0)
            e1 = st.unit(r - u0 * float(np.dot(u0, r)), HY.DEG_EPS) if ok else None
            if e1 is not None:
                e2 = np.cross(u0, e1)
                cs, sn = (-1.0 / 3.0, 2.0 * math.sqrt(2.0) / 3.0) if shape == TET else (-0.5, math.sqrt(3.0) / 2.0)
                h3 = math.sqrt(3.0) / 2.0
                phis = [(-1.0, 0.0), (0.5, -h3), (0.5, h3)] if shape == TET else [(-1.0, 0.0), (1.0, 0.0)]
                dirs = [cs * u0 + sn * (cp * e1 + sp * e2) for cp, sp in phis[:h]]
                s_of = [min([bond_norms[0], st.norms[-1]] + r_norm)] * h
        elif shape == LIN and d == 1 and h == 1:
            dirs, s_of = [-us[0]], [smallest()]
        elif (shape == TET and d == 3 and h == 1) or (shape == TRIG and d == 2 and h == 1):
            t = st.unit(total, HY.DEG_EPS)
            if t is not None:
                dirs, s_of = [-t], [smallest(st.norms[-1])]
        elif shape == TET and d == 2 and h <= 2:
            t, nn = st.unit(total, HY.DEG_EPS), st.unit(np.cross(us[0], us[1]), HY.DEG_EPS)
            if t is not None and nn is not None:
                c, s = 1.0 / math.sqrt(3.0), math.sqrt(2.0 / 3.0)
                dirs, s_of = [-c * t + s * nn, -c * t - s * nn][:h], [smallest(st.norms[-1], st.norms[-2])] * h
    if dirs is not None:
        return np.array(dirs).reshape(h, 3), shape, s_of
    # the generic rule
    vmax = np.full(4, -np.inf)
    for u in us:
        vmax = np.maximum(vmax, _vertex_dots(u))
    dirs, s_of = [], []
    t = st.unit(total, HY.DEG_EPS)
    for k in range(h):
        if k == 0 and t is not None:
            e, s = -t, smallest(st.norms[-1])
        else:
            e, s = VERTICES[st.argmin_first(list(vmax), 'vertex')], inf
        vmax = np.maximum(vmax, _vertex_dots(e))
        dirs.append(e), s_of.append(s)
    return np.array(dirs).reshape(h, 3), GEN, s_of


def hydrogens_of_rows(cls, order, kekule_order, hcount, kekule_status, pos, options=None):
    """The outputs of pg_mol_hydrogens for one graph: status, ok, counts [8], h_pos [n, 4, 3] (float64), h_placed [n], site_shape [n],
    min_contact; and cls, s [n, 4] (inf where nothing was normalised), decisions [(kind, value)], contact_distances."""
    opt = HY.HydrogenOptions() if options is None else options
    n = len(cls)
    cls, hcount = [int(c) for c in cls], [int(x) for x in hcount]
    pos = np.asarray(pos, dtype=np.float64).reshape(n, 3)
    out = dict(status=0, counts=np.zeros(len(HY.HYD_COUNTS), dtype=np.int32), h_pos=np.zeros((n, 4, 3)), h_placed=np.zeros(n, dtype=np.uint8),
               site_shape=np.zeros(n, dtype=np.uint8), min_contact=float('inf'), s=np.full((n, 4), np.inf), decisions=[], contact_distances=[],
               cls=cls, ok=True)
    if int(kekule_status) & M.KEKULE_FAILED:
        out.update(status=HY.HYD_NO_KEKULE, min_contact=0.0, ok=False)
        return out
    kept, nbrs, ndbl, triple, arom = graph_of_rows(cls, kekule_order, order)
    finite = [bool(np.isfinite(pos[i]).all()) for i in range(n)]
    status = HY.HYD_NONFINITE if any(kept[i] and not finite[i] for i in range(n)) else 0
    out['counts'][7] = sum(kept)
    if any(kept[i] and hcount[i] > HY.MAX_PER_ATOM for i in range(n)):
        out.update(status=status | HY.HYD_TOO_MANY, ok=False)
        return out
    hydrogens = []                                                     # (position, parent) in (parent, slot) order
    for i in range(n):
        h = hcount[i] if kept[i] else 0
        if h < 1 or not finite[i] or not all(finite[j] for j in nbrs[i]):
            continue
        dirs, shape, s_of = place_site(i, pos, nbrs, cls, h, ndbl, triple, arom, out['decisions'])
        length = opt.xh_length[cls[i]]
        for k in range(h):
            out['h_pos'][i, k] = pos[i] + length * dirs[k]
            out['s'][i, k] = s_of[k]
            hydrogens.append((out['h_pos'][i, k], i))
        out['h_placed'][i], out['site_shape'][i] = h, shape
        out['counts'][0] += h
        out['counts'][1] += 1
        out['counts'][1 + shape] += 1
    # contacts: hydrogen against every kept atom but its parent, and against every later hydrogen of another parent
    dist = []
    if hydrogens:
        hp, par = np.array([x for x, _ in hydrogens]), np.array([a for _, a in hydrogens])
        heavy = [j for j in range(n) if kept[j] and finite[j]]
        if heavy:
            dd = np.sqrt(((hp[:, None, :] - pos[heavy][None, :, :]) ** 2).sum(-1))
            dist += dd[par[:, None] != np.array(heavy)[None, :]].tolist()
        dd = np.sqrt(((hp[:, None, :] - hp[None, :, :]) ** 2).sum(-1))
        q = np.arange(len(par))
        dist += dd[(q[:, None] < q[None, :]) & (par[:, None] != par[None, :])].tolist()
    out['contact_distances'] = dist
    out['counts'][6] = sum(x < opt.clash_min for x in dist)
    out['min_contact'] = min(dist, default=float('inf'))
    status |= HY.HYD_CONTACTS if out['counts'][6] > opt.max_contacts else 0
    status |= HY.HYD_GENERIC if out['counts'][5] else 0
    status |= HY.HYD_HAS_HYDROGEN if out['counts'][0] else 0
    out.update(status=status, ok=(status & HY.HYD_FAIL_MASK) == 0)
    return out


# everything the kernel reads for one (classes, {(a, b): bond class}, coordinates) graph, the Kekulé form by its own restatement
all_rows = functools.partial(stereo_reference.all_rows, with_keys_and_rings=False)


def restate(rows, options=None, pos=None):
    """`hydrogens_of_rows` on an `all_rows` record; pos: other coordinates than the record's."""
    return hydrogens_of_rows(rows.cls, rows.order, rows.kekule_order, rows.hcount, rows.kekule_status, rows.pos if pos is None else pos, options)


def hydrogens_of(classes, bonds, pos, options=None, exact=False):
    """The restatement on a graph; exact: on the float64 coordinates as they are, not on their fp32 rounding."""
    return restate(all_rows(classes, bonds, pos), options, np.asarray(pos, dtype=np.float64).reshape(-1, 3) if exact else None)


def is_safe(result, options=None):
    """No float comparison of the run can flip between fp32 and float64: every norm tested against DEG_EPS and every contact distance
    tested against clash_min is exactly 0 or outside a factor 2 of its threshold, every argmin is decided exactly or by TIE_MARGIN."""
    opt = HY.HydrogenOptions() if options is None else options
    for kind, x in result['decisions']:
        if kind == 'deg' and not (x == 0.0 or x < HY.DEG_EPS / 2 or x > 2 * HY.DEG_EPS):
            return False
        if kind in ('axis', 'vertex') and not (x == 0.0 or x >= TIE_MARGIN):
            return False
    return all(x == 0.0 or x < opt.clash_min / 2 or x > 2 * opt.clash_min for x in result['contact_distances'])


def compare(got, want, pos, options=None, where=''):
    """got: status, counts, h_pos, h_placed, site_shape, min_contact of a kernel or of the host core; want: the restatement on the same
    rows.  Integers `==`, positions within the bound; returns the largest error / bound."""
    opt = HY.HydrogenOptions() if options is None else options
    assert int(got['status']) == want['status'], (where, 'status', int(got['status']), want['status'])
    for k in ('counts', 'h_placed', 'site_shape'):
        assert np.asarray(got[k]).tolist() == np.asarray(want[k]).tolist(), (where, k, np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist())
    gp, n = np.asarray(got['h_pos'], dtype=np.float64).reshape(-1, 4, 3), len(want['h_placed'])
    pos = np.asarray(pos, dtype=np.float64).reshape(n, 3)
    finite = pos[np.isfinite(pos).all(1)]
    max_c = float(np.abs(finite).max()) if finite.size else 0.0
    worst, widest = 0.0, 0.0
    for i in range(n):
        for k in range(4):
            if k >= want['h_placed'][i]:
                assert not gp[i, k].any(), (where, 'an unused slot is not 0', i, k)
                continue
            b = position_bound(max_c, opt.xh_length[want['cls'][i]], want['s'][i, k])
            err = float(np.abs(gp[i, k] - want['h_pos'][i, k]).max())
            assert err <= b, (where, 'position', i, k, err, b)
            worst, widest = max(worst, err / b), max(widest, b)
    mc, wc = float(got['min_contact']), want['min_contact']
    if math.isfinite(wc) and wc > 0:
        assert abs(mc - wc) <= 2 * widest + 4 * EPS32 * wc, (where, 'min_contact', mc, wc)
    else:
        assert mc == wc, (where, 'min_contact', mc, wc)
    return worst


# ---- the hand examples: ideal skeletons in float64 ------------------------------------------------------------------------------------------
def _ring(k, bond):
    r = bond / (2.0 * math.sin(math.pi / k))
    return [[r * math.cos(2 * math.pi * i / k), r * math.sin(2 * math.pi * i / k), 0.0] for i in range(k)]


def _tetra(centre, dist, count=4):
    return [list(np.asarray(centre) + dist * VERTICES[k]) for k in range(count)]


def _acetamide():
    c1 = np.zeros(3)
    c0, o = np.array([1.52, 0.0, 0.0]), 1.23 * np.array([math.cos(math.radians(120)), math.sin(math.radians(120)), 0.0])
    nn = 1.34 * np.array([math.cos(math.radians(240)), math.sin(math.radians(240)), 0.0])
    return [list(c0), list(c1), list(o), list(nn)]


_CYC5, _CYC6 = K.cycle(5), K.cycle(6)
# name: (classes, bonds, coordinates, {atom: (hydrogens, shape)} expected of the sites)
EXAMPLES = {
    'methane': ([C_], {}, [[0.0, 0.0, 0.0]], {0: (4, TET)}),
    'ethane': ([C_, C_], {(0, 1): 1}, [[0.0, 0.0, 0.0], [1.54, 0.0, 0.0]], {0: (3, TET), 1: (3, TET)}),
    'ethene': ([C_, C_], {(0, 1): 2}, [[0.0, 0.0, 0.0], [1.34, 0.0, 0.0]], {0: (2, TRIG), 1: (2, TRIG)}),
    'ethyne': ([C_, C_], {(0, 1): 3}, [[0.0, 0.0, 0.0], [1.2, 0.0, 0.0]], {0: (1, LIN), 1: (1, LIN)}),
    'methanol': ([C_, O_], {(0, 1): 1}, [[0.0, 0.0, 0.0], [0.0, 1.43, 0.0]], {0: (3, TET), 1: (1, TET)}),
    'methylamine': ([C_, N_], {(0, 1): 1}, [[0.0, 0.0, 0.0], [0.0, 0.0, 1.47]], {0: (3, TET), 1: (2, TET)}),
    'formaldehyde': ([C_, O_], {(0, 1): 2}, [[0.0, 0.0, 0.0], [1.21, 0.0, 0.0]], {0: (2, TRIG)}),
    'hydrogen cyanide': ([C_, N_], {(0, 1): 3}, [[0.0, 0.0, 0.0], [1.16, 0.0, 0.0]], {0: (1, LIN)}),
    'water': ([O_], {}, [[0.5, -0.25, 2.0]], {0: (2, TET)}),
    'ammonia': ([N_], {}, [[-1.0, 3.0, 0.125]], {0: (3, TET)}),
    'benzene': ([C_] * 6, _CYC6, _ring(6, 1.39), {i: (1, TRIG) for i in range(6)}),
    'pyridine': ([N_] + [C_] * 5, _CYC6, _ring(6, 1.39), {i: (1, TRIG) for i in range(1, 6)}),
    'pyrrole': ([N_] + [C_] * 4, _CYC5, _ring(5, 1.38), {i: (1, TRIG) for i in range(5)}),
    'acetamide': ([C_, C_, O_, N_], {(0, 1): 1, (1, 2): 2, (1, 3): 1}, _acetamide(), {0: (3, TET), 3: (2, TRIG)}),
    'tetramethylammonium': ([N_, C_, C_, C_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1}, [[0.0, 0.0, 0.0]] + _tetra([0.0, 0.0, 0.0], 1.5),
                            {i: (3, TET) for i in range(1, 5)}),
    'isobutane': ([C_, C_, C_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1}, [[0.0, 0.0, 0.0]] + _tetra([0.0, 0.0, 0.0], 1.54, 3),
                  {0: (1, TET), 1: (3, TET), 2: (3, TET), 3: (3, TET)}),
    'propane': ([C_, C_, C_], {(0, 1): 1, (1, 2): 1}, _tetra([0.0, 0.0, 0.0], 1.54, 1) + [[0.0, 0.0, 0.0]] + [_tetra([0.0, 0.0, 0.0], 1.54, 2)[1]],
                {0: (3, TET), 1: (2, TET), 2: (3, TET)}),
    'dimethylamine': ([C_, N_, C_], {(0, 1): 1, (1, 2): 1}, _tetra([0.0, 0.0, 0.0], 1.47, 1) + [[0.0, 0.0, 0.0]] + [_tetra([0.0, 0.0, 0.0], 1.47, 2)[1]],
                      {0: (3, TET), 1: (1, TET), 2: (3, TET)}),
    # P with four carbons has one hydrogen (valence 5): d + h = 5, the generic rule; the carbons lean away from +z, so the hydrogen is there
    'tetramethylphosphorane': ([P_, C_, C_, C_, C_], {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1},
                               [[0.0, 0.0, 0.0], [1.75, 0.0, -0.5], [-1.75, 0.0, -0.5], [0.0, 1.75, -0.5], [0.0, -1.75, -0.5]],
                               {0: (1, GEN), 1: (3, TET), 2: (3, TET), 3: (3, TET), 4: (3, TET)}),
    # exactly collinear, from integers: the amine's two rules have no direction, the methyls' reference is along their own bond
    'collinear dimethylamine': ([C_, N_, C_], {(0, 1): 1, (1, 2): 1}, [[-2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]],
                                {0: (3, GEN), 1: (1, GEN), 2: (3, GEN)}),
}
IDEAL_SKELETONS = ('methane', 'ethane', 'ethene', 'ethyne', 'methanol', 'methylamine', 'formaldehyde', 'hydrogen cyanide', 'water', 'ammonia',
                   'benzene', 'pyridine', 'pyrrole', 'acetamide', 'tetramethylammonium', 'isobutane', 'propane', 'dimethylamine')
# the clash_min values the examples are run with: below half of every distance a small ideal molecule has (no contact), and above
# twice every one (every pair a contact); the default 1.5 lies inside a factor 2 of the 1-3 distances of every molecule
EXAMPLE_CLASH = (0.4, 16.0)


def example_graphs():
    """[(classes, bonds, pos float32)] of EXAMPLES, in its order."""
    return [(c, b, np.array(p, dtype=np.float32)) for c, b, p, _ in EXAMPLES.values()]


def angle(a, b, c):
    """The angle a - b - c in degrees."""
    u, v = np.asarray(a) - np.asarray(b), np.asarray(c) - np.asarray(b)
    return math.degrees(math.acos(max(-1.0, min(1.0, float(np.dot(u, v) / (np.linalg.norm(u) * np.linalg.norm(v)))))))


def torsion(a, b, c, d):
    """The torsion a - b - c - d in degrees, -180 .. 180."""
    a, b, c, d = (np.asarray(x, dtype=np.float64) for x in (a, b, c, d))
    b1, b2, b3 = b - a, c - b, d - c
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return math.degrees(math.atan2(float(np.dot(np.cross(n1, n2), b2 / np.linalg.norm(b2))), float(np.dot(n1, n2))))


# ---- the generated family -------------------------------------------------------------------------------------------------------------------
FAMILY_SIZES = (1, 2, 3, 5, 9, 10, 63, 64, 65, 127, 128)
FAMILY_SEED = 20250611
FAMILY_GRAPHS = 66
FAMILY_CLASH = 0.1               # grown atoms keep 2 A apart, so a hydrogen inside 0.05 .. 0.2 A of anything is rare (and redrawn)
MIN_SEPARATION = 2.0             # of two atoms that are not bonded: a site's neighbours then stand at least 83 degrees apart
BOND_LENGTH = 1.5
_CAPACITY = {B_: 3, C_: 4, N_: 3, O_: 2, F_: 1, SI_: 4, P_: 5, S_: 6, CL_: 1, BR_: 1, I_: 1}   # bonds' orders summed, while growing
_MAX_DEGREE = {P_: 4, S_: 5}     # (P with four and S with five neighbours have one hydrogen: the generic rule)
_POOL = [C_] * 10 + [N_] * 4 + [O_] * 3 + [P_] * 2 + [S_] * 2 + [F_, CL_, BR_, I_, SI_, B_]


_SINGLE = (C_, N_, O_, F_, S_, P_)   # the single-atom graphs in turn: methane, ammonia, water, HF, ...


def random_graph(rng, n, turn=0):
    """A random tree of n atoms with single, double and triple bonds, grown in space: every atom BOND_LENGTH from its parent in a
    random direction that keeps it MIN_SEPARATION from every other atom.  (classes, bonds, pos float32 [n, 3]).  n = 1: the turn-th
    of _SINGLE."""
    if n == 1:
        return [_SINGLE[turn % len(_SINGLE)]], {}, (rng.normal(size=(1, 3)) * 3).astype(np.float32)
    for _ in range(200):
        classes = [int(v) for v in rng.choice(_POOL, n)]
        classes[0] = int(rng.choice([C_, N_, P_, S_]))
        pos, bonds, used, degree = [rng.normal(size=3) * 2], {}, [0] * n, [0] * n
        for v in range(1, n):
            for _ in range(400):
                u = int(rng.integers(max(0, v - 6), v))
                o = int(rng.choice([1, 1, 1, 2, 2, 3]))
                o = min(o, _CAPACITY[classes[u]] - used[u], _CAPACITY[classes[v]])
                if o < 1 or degree[u] >= _MAX_DEGREE.get(classes[u], 4):
                    continue
                x = rng.normal(size=3)
                x = pos[u] + BOND_LENGTH * x / np.linalg.norm(x)
                if all(np.linalg.norm(x - pos[w]) >= MIN_SEPARATION for w in range(v) if w != u):
                    break
            else:
                break
            pos.append(x)
            bonds[(u, v)] = o
            used[u], used[v], degree[u], degree[v] = used[u] + o, used[v] + o, degree[u] + 1, degree[v] + 1
        else:
            return classes, bonds, np.array(pos).astype(np.float32)
    raise AssertionError('no tree of %d atoms grown' % n)


def family(seed=FAMILY_SEED, n_graphs=FAMILY_GRAPHS, sizes=FAMILY_SIZES, options=None):
    """([(classes, bonds, pos float32 [n, 3])], graphs drawn): the sizes in turn; a graph of which the restatement says that a float
    comparison could flip in fp32 (`is_safe`) is drawn again.  The last two have no Kekulé structure."""
    opt = HY.HydrogenOptions(clash_min=FAMILY_CLASH) if options is None else options
    rng = np.random.default_rng(seed)
    out, drawn = [], 0
    for k in range(n_graphs):
        for _ in range(100):
            g = random_graph(rng, sizes[k % len(sizes)], k // len(sizes))
            drawn += 1
            if is_safe(hydrogens_of(*g, options=opt), opt):
                break
        else:
            raise AssertionError('no graph clear of the thresholds')
        out.append(g)
    five = K.NAMED['all-carbon five-ring']
    out += [(list(five[0]), dict(five[1]), np.array(_ring(5, 1.4), dtype=np.float32) + np.float32(k)) for k in range(2)]
    return out, drawn


def census(graphs, options=None):
    """{(shape, d, h): sites} over the graphs, by the restatement alone."""
    rows = {}
    for classes, bonds, pos in graphs:
        r = all_rows(classes, bonds, pos)
        got = restate(r, options)
        _, nbrs, _, _, _ = graph_of_rows(r.cls, r.kekule_order, r.order)
        for i, (h, s) in enumerate(zip(got['h_placed'].tolist(), got['site_shape'].tolist())):
            if h:
                rows[(s, len(nbrs[i]), h)] = rows.get((s, len(nbrs[i]), h), 0) + 1
    return rows


# every row of the definition's table: (shape, d, h)
TABLE_ROWS = ([(TET, 3, 1), (TET, 2, 2), (TET, 2, 1), (TRIG, 2, 1), (LIN, 1, 1)] + [(TET, 1, h) for h in (1, 2, 3)] + [(TRIG, 1, h) for h in (1, 2)]
              + [(TET, 0, h) for h in (1, 2, 3, 4)])


# ---- tools/hydrogen_host_check.cpp: the core compiled for the host --------------------------------------------------------------------------
def run_host_check(exe, cases, work_dir, options=None):
    """cases: [`all_rows` records].  Returns per case the dict `compare` takes."""
    opt = HY.HydrogenOptions() if options is None else options
    path = os.path.join(str(work_dir), 'hydrogen_cases.txt')
    with open(path, 'w') as fh:
        fh.write(' '.join(MS.hex32(v) for v in opt.xh_length) + '\n')
        fh.write('%s %d\n' % (MS.hex32(opt.clash_min), opt.max_contacts))
        for m in cases:
            n = len(m.cls)
            rows, a, b = MS.listed_pairs(n, m.order, m.kekule_order)
            fh.write('%d %d %d\n' % (n, m.kekule_status, len(rows)))
            for i in range(n):
                fh.write('%d %d %s %s %s\n' % (m.cls[i], m.hcount[i], *(MS.hex32(x) for x in m.pos[i])))
            for x, y, r in zip(a, b, rows):
                fh.write('%d %d %d %d\n' % (x, y, m.order[r], m.kekule_order[r]))
    out = MS.run_program(exe, path)
    got = []
    for c, case in enumerate(cases):
        n = len(case.cls)
        head, atoms, coords = (out[3 * c + k].split() for k in range(3))
        got.append({'status': int(head[0]), 'min_contact': float.fromhex(head[1]) if head[1] not in ('inf', 'nan') else float(head[1]),
                    'counts': np.array([int(v) for v in head[2:]], dtype=np.int32),
                    'h_placed': np.array([int(v) for v in atoms[0::2]], dtype=np.uint8).reshape(n),
                    'site_shape': np.array([int(v) for v in atoms[1::2]], dtype=np.uint8).reshape(n),
                    'h_pos': np.array([float.fromhex(v) for v in coords], dtype=np.float64).reshape(n, 4, 3)})
    return got
