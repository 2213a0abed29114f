"""Plain restatement of the feature typing and the typed match (DESIGN.md 2.9 "Features"; phoregen_amd/molecule.py, csrc/mol_feat.hip,
csrc/feature_core.h) for the tests, written from the text in another form than the kernel: neighbour dicts, sets of type names, every
pattern of rule 6 enumerated atom by atom with distinct atoms, distances in float64.  No device code; it shares nothing with the
kernel but the named constants of phoregen_amd.molecule.  The Kekulé form and the ring sizes are inputs: on the CPU they come from
kekule_reference / ring_reference, on the GPU from the kernels that the feature kernel reads (which Kekulé structure a graph gets
is not canonical, so the typing is always restated for the structure at hand).  Also here: the named molecules with their
hand-written answers, the random family, and the case format of tools/feature_host_check.cpp."""
import itertools
import os

import numpy as np

import kekule_reference as K
import mol_reference as R
import mol_support as MS
import ring_reference as G
from mol_support import B_, C_, N_, O_, F_, SI_, P_, S_, CL_, BR_, I_  # noqa: F401
from phoregen_amd import molecule as M

ONPS = (O_, N_, P_, S_)
T = M.FEATURE_TYPES


# ---- typing -------------------------------------------------------------------------------------------------------------------------
def _graph(cls, order, kek_order, hcount, charge, ring_size):
    cls = [int(c) for c in cls]
    n = len(cls)
    kept, _, rows, order = MS.pair_walk(cls, order)
    nbr = [dict() for _ in range(n)]                                   # neighbour -> (Kekulé order, screen order is 4, ring bond)
    for (a, b), row in rows.items():
        nbr[a][b] = nbr[b][a] = (int(kek_order[row]), order[row] == 4, int(ring_size[row]) > 0)
    h = [int(hcount[i]) if kept[i] else 0 for i in range(n)]
    q = [int(charge[i]) if kept[i] else 0 for i in range(n)]
    arom = [any(a4 and ring for _, a4, ring in nbr[i].values()) for i in range(n)]
    v = [sum(k for k, _, _ in nbr[i].values()) + h[i] for i in range(n)]
    return {'n': n, 'cls': cls, 'kept': kept, 'nbr': nbr, 'h': h, 'q': q, 'arom': arom, 'v': v, 'deg': [len(x) for x in nbr]}


def _single(bond):
    return bond[0] == 1


def _double(bond):
    return bond[0] == 2 and not bond[1]


def type_atoms(cls, order, kek_order, hcount, charge, ring_size, kekule_ok=True):
    """The set of type names of every atom (empty for a dropped atom; all empty without a Kekulé structure)."""
    g = _graph(cls, order, kek_order, hcount, charge, ring_size)
    n, el, nbr, h, q, arom, v, deg = g['n'], g['cls'], g['nbr'], g['h'], g['q'], g['arom'], g['v'], g['deg']
    out = [set() for _ in range(n)]
    if not kekule_ok:
        return out
    aliph = lambda i, els: el[i] in els and not arom[i]                                  # noqa: E731
    has_dbl = lambda x, open_only=False: any(_double(b) and aliph(z, ONPS) and not (open_only and b[2]) for z, b in nbr[x].items())  # noqa: E731
    for i in range(n):
        if not g['kept'][i]:
            continue
        X = deg[i] + h[i]
        # rule 1
        if el[i] in (N_, O_, S_) and h[i] >= 1:
            out[i].add('HD')
        # rule 2
        if arom[i]:
            out[i].add('AR')
        # rule 3
        if q[i] > 0:
            out[i].add('PO')
        if aliph(i, (C_,)):
            ns = [z for z in nbr[i] if aliph(z, (N_,))]
            if any(_single(nbr[i][a]) and _single(nbr[i][b]) and _double(nbr[i][c]) for a, b, c in itertools.permutations(ns, 3)):
                out[i].add('PO')
        # rule 4
        if aliph(i, (O_, S_)) and v[i] == 2:
            if h[i] == 0 or (h[i] == 1 and any(_single(b) and not has_dbl(x) for x, b in nbr[i].items())):
                out[i].add('HA')
        if aliph(i, (N_,)) and v[i] == 3 and not any(_single(b) and has_dbl(x, True) for x, b in nbr[i].items()):
            out[i].add('HA')
        if arom[i] and q[i] == 0 and ((el[i] == N_ and h[i] == 0) or el[i] in (O_, S_)):
            out[i].add('HA')
        # rule 5
        if ((arom[i] and el[i] in (C_, S_)) or (aliph(i, (S_,)) and h[i] == 0 and v[i] == 2) or el[i] in (BR_, I_)
                or (el[i] == C_ and q[i] == 0 and not any(el[z] in (N_, O_, F_) for z in nbr[i]))):
            out[i].add('HY')
        # rule 7
        if el[i] in (CL_, BR_, I_) and X == 1 and any(_single(b) and el[z] == C_ for z, b in nbr[i].items()):
            out[i].add('XB')
    # rule 6: every pattern, from its centre, over all assignments of distinct atoms
    for c in range(n):
        if not g['kept'][c] or arom[c]:
            continue
        X = deg[c] + h[c]
        dbl = [z for z, b in nbr[c].items() if _double(b) and aliph(z, (O_, S_))]
        oh = [z for z, b in nbr[c].items() if _single(b) and aliph(z, (O_,)) and h[z] == 1]
        o_any = [z for z, b in nbr[c].items() if _single(b) and aliph(z, (O_,))]
        if (el[c] == C_ and X == 3) or (el[c] == S_ and X == 3) or (el[c] == P_ and deg[c] == 3):          # 6a
            for x, y in itertools.product(dbl, oh):
                out[x].add('NE'), out[y].add('NE')
        if el[c] == P_ and X == 4:
            for x, y1, y2 in itertools.product(dbl, oh, oh):                                                # 6b
                if y1 != y2:
                    out[x].add('NE'), out[y1].add('NE'), out[y2].add('NE')
            for x, y, o in itertools.product(dbl, oh, o_any):                                               # 6c
                if o != y and any(t not in (c, x, y, o) and _single(b) and h[t] != 1 for t, b in nbr[o].items()):
                    out[x].add('NE'), out[y].add('NE')
        if el[c] == S_ and X == 4:                                                                          # 6d
            for x1, x2, y in itertools.product(dbl, dbl, oh):
                if x1 != x2:
                    out[x1].add('NE'), out[x2].add('NE'), out[y].add('NE')
    return out


def fp_of(types):
    return np.array([sum(1 << T.index(t) for t in s) for s in types], dtype=np.uint8)


# ---- the match ------------------------------------------------------------------------------------------------------------------------
def features_of_rows(cls, order, kek_order, hcount, charge, kekule_ok, ring_size, pos, points, kinds, limits=None):
    """One graph: the kernel's outputs for it -- 'atom_fp' uint8 [n], 'point_dist' float64 [p], 'point_atom' int16 [p] (compact index),
    'counts' int32 [25], 'status', 'ok' -- plus 'types' (the sets) and 'margin' (per typed point, how far the second nearest carrying
    atom is behind the nearest; inf without two)."""
    limits = M.FeatureLimits() if limits is None else limits
    types = type_atoms(cls, order, kek_order, hcount, charge, ring_size, kekule_ok)
    n = len(types)
    kept = [0 <= int(c) <= 10 for c in cls]
    compact, k = [], 0
    for i in range(n):
        compact.append(k if kept[i] else -1)
        k += kept[i]
    pos = np.asarray(pos, dtype=np.float64).reshape(n, 3)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    finite = [kept[i] and bool(np.isfinite(pos[i]).all()) for i in range(n)]
    bad = any(kept[i] and not finite[i] for i in range(n))
    c = dict.fromkeys(M.FEATURE_COUNTS, 0)
    for s in types:
        for t in s:
            c['atoms_' + t] += 1
    dist, atom, margin = np.full(len(points), np.inf), np.full(len(points), -1, dtype=np.int16), np.full(len(points), np.inf)
    for p, kind in enumerate(int(x) for x in kinds):
        if not -1 <= kind < len(T):
            continue
        if not np.isfinite(points[p]).all():
            bad = True
            continue
        if kind == -1:
            c['untyped_points'] += 1
            continue
        t = T[kind]
        c['typed_points'] += 1
        c['points_' + t] += 1
        cand = sorted((float(np.sqrt(((pos[i] - points[p]) ** 2).sum())), i) for i in range(n) if finite[i] and t in types[i])
        if cand:
            dist[p], atom[p] = cand[0][0], compact[cand[0][1]]
            margin[p] = cand[1][0] - cand[0][0] if len(cand) > 1 else np.inf
        if dist[p] < limits.feat_cut:
            c['matched'] += 1
            c['matched_' + t] += 1
        else:
            c['unmatched'] += 1
    status = 0 if kekule_ok else M.FEAT_NO_KEKULE
    status |= M.FEAT_UNMATCHED if c['unmatched'] > limits.max_unmatched else 0
    status |= M.FEAT_HAS_UNTYPED if c['untyped_points'] else 0
    status |= M.FEAT_NONFINITE if bad else 0
    return {'atom_fp': fp_of(types), 'point_dist': dist, 'point_atom': atom, 'counts': np.array([c[k] for k in M.FEATURE_COUNTS], dtype=np.int32),
            'status': status, 'ok': status & M.FEAT_FAIL_MASK == 0, 'types': types, 'margin': margin}


def cpu_inputs(classes, bonds):
    """(cls, order, kek_order, hcount, charge, kekule_ok, ring_size) of one graph from the restatements of the Kekulé form and the rings."""
    cls, order = K.rows_of(classes, {k: v for k, v in bonds.items()})
    kk = K.kekule_of_rows(cls, order)
    rr = G.rings_of_rows(cls, order)
    return cls, order, kk['kekule_order'], kk['hcount'], kk['charge'], bool(kk['ok']), rr['ring_size']


def types_of(classes, bonds):
    cls, order, kek, h, q, ok, rs = cpu_inputs(classes, bonds)
    return type_atoms(cls, order, kek, h, q, rs, ok)


# ---- the named molecules: (classes, bonds, {atom: set of types}) -- the answers by hand from the rules; ring carbons that are not listed
# are {AR, HY} ---------------------------------------------------------------------------------------------------------------------------
def _benzene_x(x):
    return [C_] * 6 + [x], {**K.cycle(6), (0, 6): 1}


_S = lambda *names: set(names)                                                            # noqa: E731
NAMED = {
    'acetic acid': ([C_, C_, O_, O_], {(0, 1): 1, (1, 2): 2, (1, 3): 1}, {0: _S('HY'), 1: _S(), 2: _S('HA', 'NE'), 3: _S('HD', 'NE')}),
    'ethanol': ([C_, C_, O_], {(0, 1): 1, (1, 2): 1}, {0: _S('HY'), 1: _S(), 2: _S('HD', 'HA')}),
    'acetamide': ([C_, C_, O_, N_], {(0, 1): 1, (1, 2): 2, (1, 3): 1}, {0: _S('HY'), 1: _S(), 2: _S('HA'), 3: _S('HD')}),
    'acetonitrile': ([C_, C_, N_], {(0, 1): 1, (1, 2): 3}, {0: _S('HY'), 1: _S(), 2: _S('HA')}),
    'methylguanidine': ([C_, N_, C_, N_, N_], {(0, 1): 1, (1, 2): 1, (2, 3): 2, (2, 4): 1},
                        {0: _S(), 1: _S('HD'), 2: _S('PO'), 3: _S('HD', 'HA'), 4: _S('HD')}),
    'methanesulfonic acid': ([C_, S_, O_, O_, O_], {(0, 1): 1, (1, 2): 2, (1, 3): 2, (1, 4): 1},
                             {0: _S('HY'), 1: _S(), 2: _S('HA', 'NE'), 3: _S('HA', 'NE'), 4: _S('HD', 'NE')}),
    'chlorobenzene': (*_benzene_x(CL_), {6: _S('XB')}),
    'bromobenzene': (*_benzene_x(BR_), {6: _S('XB', 'HY')}),
    'pyridine': (*K.NAMED['pyridine'][:2], {0: _S('AR', 'HA')}),
    'pyrrole': (*K.NAMED['pyrrole'][:2], {0: _S('AR', 'HD')}),
    'thiophene': (*K.NAMED['thiophene'][:2], {0: _S('AR', 'HA', 'HY')}),
    'N-methylpyridinium': (*K.NAMED['N-methylpyridinium'][:2], {0: _S('AR', 'PO'), 6: _S()}),
    # an aromatic bond class on a chain: no ring bond, so every atom is aliphatic, and a Kekulé double bond on such a bond is no "double"
    'aromatic bonds on a chain': (*K.NAMED['three aromatic bonds in a chain'][:2], {i: _S('HY') for i in range(4)}),
    'indene-like': (*K.NAMED['indene-like'][:2], {i: _S() for i in range(9)}),
    # rule 6b and 6c: methyl phosphate C-O-P(=O)(OH)(OH); 6c alone: dimethyl phosphate; neither: the ester O's carbon has exactly one H
    'methyl phosphate': ([C_, O_, P_, O_, O_, O_], {(0, 1): 1, (1, 2): 1, (2, 3): 2, (2, 4): 1, (2, 5): 1},
                         {0: _S(), 1: _S('HA'), 2: _S(), 3: _S('HA', 'NE'), 4: _S('HD', 'NE'), 5: _S('HD', 'NE')}),
    'dimethyl phosphate': ([C_, O_, P_, O_, O_, O_, C_], {(0, 1): 1, (1, 2): 1, (2, 3): 2, (2, 4): 1, (2, 5): 1, (5, 6): 1},
                           {0: _S(), 1: _S('HA'), 2: _S(), 3: _S('HA', 'NE'), 4: _S('HD', 'NE'), 5: _S('HA'), 6: _S()}),
    'isopropyl methylphosphonate': ([C_, O_, P_, O_, O_, C_, C_, C_],
                                    {(0, 1): 1, (1, 2): 1, (2, 3): 2, (2, 4): 1, (2, 5): 1, (0, 6): 1, (0, 7): 1},
                                    {0: _S(), 1: _S('HA'), 2: _S(), 3: _S('HA'), 4: _S('HD'), 5: _S('HY'), 6: _S('HY'), 7: _S('HY')}),
}


def named_answer(name):
    """The full hand answer: the listed atoms, and {AR, HY} for every other (ring carbon) atom."""
    classes, _, listed = NAMED[name]
    return [set(listed[i]) if i in listed else {'AR', 'HY'} for i in range(len(classes))]


# ---- the random family ----------------------------------------------------------------------------------------------------------------
FAMILY_SEED = 20250917
GAP = 1e-3                                                             # no atom-point distance within GAP of feat_cut
TIE = 1e-3                                                             # the two nearest atoms of a point differ by more than this
HETERO = [C_, C_, C_, C_, N_, N_, O_, O_, S_, P_, F_, CL_, BR_, I_]


def graphs_from_generator(n_graphs=40, seed=R.GEN_SEED):
    """mol_reference's generator, decoded to (classes, bonds) by its own restatement of the screen."""
    node, pos, edge, sizes = R.generate_batch(seed, n_graphs)
    out = []
    for r in R.screen_batch(node, pos, edge, sizes):
        rows, a, b = MS.listed_pairs(len(r['cls']), r['order'])
        out.append(([int(c) if c >= 0 else 11 for c in r['cls']], {(int(x), int(y)): int(r['order'][k]) for x, y, k in zip(a, b, rows)}))
    return out


def star_graph(n):
    """One atom bonded to all others: far above its valence."""
    classes = [C_] + [(C_, N_, O_, S_)[i % 4] for i in range(n - 1)]
    return classes, {(0, i): 1 for i in range(1, n)}


def typable_graph(rng, n, tries=40):
    """A decorated graph of kekule_reference's family of n atoms that has a Kekulé structure (by the restatement of the Kekulé form)."""
    for _ in range(tries):
        classes, bonds = decorate(rng, *K.random_graph(rng, n))
        if cpu_inputs(classes, bonds)[5]:
            return classes, bonds
    raise AssertionError('no graph of %d atoms with a Kekulé structure in %d draws' % (n, tries))


def decorate(rng, classes, bonds):
    """Hetero atoms and terminal groups on a graph of kekule_reference's family: the ballast (non-aromatic) atoms get random elements,
    some single bonds become double."""
    classes, bonds = list(classes), dict(bonds)
    in_arom = {x for (a, b), t in bonds.items() if t == 4 for x in (a, b)}
    for i, c in enumerate(classes):
        if c <= 10 and i not in in_arom and rng.random() < 0.6:
            classes[i] = int(rng.choice(HETERO))
    for e, t in list(bonds.items()):
        if t == 1 and rng.random() < 0.2:
            bonds[e] = 2
    return classes, bonds


def place(rng, n):
    """n atom positions, uniform in a box that grows with n: sparse enough that a point near one atom rarely has another atom within GAP
    of the cutoff."""
    side = 6.0 * max(n, 1) ** (1.0 / 3.0) + 4.0
    return (rng.random((n, 3)) * side).astype(np.float32)


def draw_points(rng, pos, p, types=None):
    """p points: most at an atom's position plus an offset of length 0 .. 3 (either side of the cutoff), some far away; kinds 0..6,
    -1 (untyped) and -2 (ignored).  types (a set of names per atom, optional): half of the points near an atom that has a type ask for
    one of its types, so that matches are not rare."""
    n = len(pos)
    pts = np.zeros((p, 3), dtype=np.float32)
    kinds = rng.choice(np.arange(-2, 7), size=p, p=[0.08, 0.08] + [0.12] * 7).astype(np.int8)
    for k in range(p):
        if n and rng.random() < 0.8:
            d = rng.normal(size=3)
            i = int(rng.integers(0, n))
            pts[k] = pos[i] + (d / np.linalg.norm(d) * rng.random() * 3.0).astype(np.float32)
            if types is not None and types[i] and rng.random() < 0.5:
                kinds[k] = T.index(sorted(types[i])[int(rng.integers(0, len(types[i])))])
        else:
            pts[k] = (rng.random(3) * 40.0 + 60.0).astype(np.float32)
    return pts, kinds


def acceptable(pos, pts, feat_cut=2.0):
    """No atom-point distance within GAP of the cutoff, no two atoms within TIE of each other as seen from a point."""
    if len(pos) == 0 or len(pts) == 0:
        return True
    d = np.sqrt(((pos.astype(np.float64)[None] - pts.astype(np.float64)[:, None]) ** 2).sum(-1))      # [p, n]
    if (np.abs(d - feat_cut) <= GAP).any():
        return False
    if d.shape[1] > 1:
        s = np.sort(d, axis=1)
        near = s[:, 0] < 2 * feat_cut + 1.0                            # (only where a match or a reported atom could turn on it)
        if ((s[:, 1] - s[:, 0])[near] <= TIE).any():
            return False
    return True


def make_case(rng, classes, bonds, p, stats=None):
    """One case: the graph with positions and p accepted points.  stats [drawn, accepted] counts the point draws."""
    pos = place(rng, len(classes))
    types = types_of(classes, bonds)
    while True:
        pts, kinds = draw_points(rng, pos, p, types)
        ok = acceptable(pos, pts)
        if stats is not None:
            stats[0] += 1
            stats[1] += ok
        if ok:
            return {'classes': list(classes), 'bonds': dict(bonds), 'pos': pos, 'points': pts, 'kinds': kinds}


FAMILY_POINTS = (0, 1, 5, 12, 70)


def random_family(seed=FAMILY_SEED, n_aromatic=48, n_generator=40, stats=None):
    """Cases from kekule_reference's aromatic family (decorated with hetero atoms), mol_reference's generator and a few stars."""
    rng = np.random.default_rng(seed)
    graphs = [decorate(rng, c, b) for c, b in K.random_family(n_graphs=n_aromatic)]
    graphs += graphs_from_generator(n_generator)
    graphs += [star_graph(n) for n in (5, 64, 65, 128)]
    return [make_case(rng, c, b, FAMILY_POINTS[k % len(FAMILY_POINTS)], stats) for k, (c, b) in enumerate(graphs)]


def restate_case(case, inputs=None, limits=None):
    inputs = cpu_inputs(case['classes'], case['bonds']) if inputs is None else inputs
    cls, order, kek, h, q, ok, rs = inputs
    return features_of_rows(cls, order, kek, h, q, ok, rs, case['pos'], case['points'], case['kinds'], limits)


# ---- tools/feature_host_check.cpp: the kernel's rules compiled for the host ---------------------------------------------------------------
def run_host_check(exe, cases, work_dir):
    """cases: [(cls, order, kek_order, hcount, charge, kekule_ok, ring_size)] of graphs WITH a Kekulé structure -> one uint8 array of
    atom bytes per case."""
    path = os.path.join(str(work_dir), 'feature_cases.txt')
    with open(path, 'w') as fh:
        for cls, order, kek, h, q, ok, rs in cases:
            assert ok
            n = len(cls)
            rows, a, b = MS.listed_pairs(n, order)
            fh.write('%d %d\n' % (n, rows.size) + ' '.join('%d %d %d' % (cls[i], h[i], q[i]) for i in range(n)) + '\n'
                     + ' '.join('%d %d %d %d %d' % (x, y, order[r], kek[r], rs[r]) for x, y, r in zip(a, b, rows)) + '\n')
    out = MS.run_program(exe, path)
    return [np.array([int(v) for v in out[c].split()], dtype=np.uint8) for c in range(len(cases))]
