"""Plain restatement of the Kekulé form (DESIGN.md 2.9 "Kekulé form"; phoregen_amd/molecule.py, csrc/mol_kekule.hip) for the tests,
written from the text in another form than the kernel: classification and per-atom arithmetic in Python, feasibility and the maximum
cardinality by exhaustive search over the allowed graph, memoised on the set of atoms still free -- no augmenting paths, no blossoms.
A matching the kernel returns is validated by its properties (`check_assignment`), not compared with the restatement's own.  No
device code; it shares nothing with the kernel but the named constants and tables of phoregen_amd.molecule.  Also here: the named
molecules of the tests with their hand-written answers, the random family, and the case format of tools/kekule_host_check.cpp.  The
graph builders (here with the aromatic order as the default), `rows_of` and the walk over the pair rows are tests/mol_support.py's."""
import os
import sys

import numpy as np

import mol_support as MS
from mol_support import B_, C_, N_, O_, F_, SI_, P_, S_, CL_, BR_, I_, rows_of  # noqa: F401  (read from here by other modules)
from phoregen_amd import molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

NONE, NOT, MAY, MUST = 'none', 'not', 'may', 'must'


def _table(d):
    return [d[z] for z in ATOM_TYPES]


def graph_of_rows(cls, order):
    """One graph as the screen wrote it -> kept flags, s and a per atom, the aromatic bonds [(a, b, row)]."""
    w = MS.pair_walk(cls, order)
    n = len(w.kept)
    s, a, arom = [0] * n, [0] * n, []
    for (i, j), row in w.rows.items():
        o = w.order[row]
        if o == 4:
            a[i] += 1
            a[j] += 1
            arom.append((i, j, row))
        else:
            s[i] += o
            s[j] += o
    return {'n': n, 'cls': [int(c) for c in cls], 'order': w.order, 'kept': w.kept, 's': s, 'a': a, 'arom': arom}


def classify(g, pas):
    neutral, charged, must = _table(M.KEKULE_DBL_NEUTRAL), _table(M.KEKULE_DBL_CHARGED), _table(M.KEKULE_MUST)
    kinds = []
    for i in range(g['n']):
        if not g['kept'][i] or g['a'][i] < 1:
            kinds.append(NONE)
            continue
        el = g['cls'][i]
        cap = neutral[el] if pas == 0 else max(neutral[el], charged[el])
        kinds.append(NOT if g['s'][i] + g['a'][i] + 1 > cap else MUST if must[el] else MAY)
    return kinds


def allowed_edges(g, kinds):
    return [(i, j) for i, j, _ in g['arom'] if kinds[i] in (MAY, MUST) and kinds[j] in (MAY, MUST)]


def best_matching(n, edges, kinds):
    """Exhaustive: the largest matching of `edges` that covers every MUST atom, as a set of pairs; None if there is none."""
    nbr = [[] for _ in range(n)]
    for i, j in edges:
        nbr[i].append(j)
        nbr[j].append(i)
    verts = [i for i in range(n) if kinds[i] in (MAY, MUST)]
    memo = {}
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))

    def best(free):                                                   # free: frozen as an int bitmask over atoms
        if free == 0:
            return 0, ()
        if free in memo:
            return memo[free]
        v = (free & -free).bit_length() - 1
        rest = free & ~(1 << v)
        res = None
        if kinds[v] != MUST:
            sub = best(rest)
            if sub is not None:
                res = sub
        for u in nbr[v]:
            if rest >> u & 1:
                sub = best(rest & ~(1 << u))
                if sub is not None and (res is None or sub[0] + 1 > res[0]):
                    res = (sub[0] + 1, sub[1] + ((min(u, v), max(u, v)),))
        memo[free] = res
        return res

    out = best(sum(1 << i for i in verts))
    return None if out is None else set(out[1])


def solve(g, allow_charged=True):
    """The matching-independent answer: {'feasible', 'pass' (the deciding pass, or the last one tried), 'kinds' (of that pass),
    'size' (|M|, 0 on failure), 'matching' (one maximum matching of the restatement's own, empty on failure)}."""
    for pas in (0, 1):
        kinds = classify(g, pas)
        m = best_matching(g['n'], allowed_edges(g, kinds), kinds)
        if m is not None or pas == 1 or not allow_charged:
            return {'feasible': m is not None, 'pass': pas, 'kinds': kinds, 'size': len(m or ()), 'matching': m or set()}


def results_for(g, sol, matching):
    """Section 1's outputs for this matching (a set of pairs a < b; the empty set on failure)."""
    neutral, hval = _table(M.KEKULE_DBL_NEUTRAL), _table(M.H_VALENCES)
    n = g['n']
    d = [0] * n
    for i, j in matching:
        d[i] += 1
        d[j] += 1
    kek = np.array(g['order'], dtype=np.int8)
    if sol['feasible']:
        for i, j, row in g['arom']:
            kek[row] = 2 if (i, j) in matching else 1
    h, q = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int8)
    for i in range(n):
        if not g['kept'][i]:
            continue
        el = g['cls'][i]
        v = g['s'][i] + g['a'][i] + d[i]
        q[i] = 1 if (el == N_ and v == 4) or (d[i] == 1 and v > neutral[el]) else 0
        x = v - int(q[i])
        t = [t for t in hval[el] if t >= x]
        h[i] = min(t) - x if t else 0
    kinds = sol['kinds']
    no = [g['kept'][i] and g['cls'][i] in (N_, O_) for i in range(n)]
    counts = {'aromatic_atoms': sum(k != NONE for k in kinds), 'aromatic_bonds': len(g['arom']), 'doubled': len(matching),
              'must_atoms': sum(k == MUST for k in kinds), 'may_matched': sum(d[i] == 1 and kinds[i] == MAY for i in range(n)),
              'hydrogens': int(h.sum()), 'charge': int(q.sum()), 'hbd': sum(no[i] and h[i] >= 1 for i in range(n)), 'hba': sum(no),
              'heavy_atoms': sum(g['kept'])}
    status = 0 if sol['feasible'] else M.KEKULE_FAILED
    status |= M.KEKULE_CHARGED if sol['feasible'] and sol['pass'] == 1 else 0
    status |= M.KEKULE_HAS_AROMATIC if counts['aromatic_atoms'] else 0
    status |= M.KEKULE_CATION if counts['charge'] else 0
    return {'kekule_order': kek, 'hcount': h, 'charge': q, 'counts': np.array([counts[k] for k in M.KEKULE_COUNTS], dtype=np.int32),
            'status': status, 'ok': status & M.KEKULE_FAIL_MASK == 0}


INDEPENDENT = ('aromatic_atoms', 'aromatic_bonds', 'doubled', 'must_atoms', 'hba', 'heavy_atoms')   # counts that no choice of M moves


def kekule_of_rows(cls, order, allow_charged=True):
    """The restatement's answer for one graph: `results_for` its own matching, plus 'solution' and 'h_minus_q'."""
    g = graph_of_rows(cls, order)
    sol = solve(g, allow_charged)
    r = results_for(g, sol, sol['matching'])
    return dict(r, solution=sol, graph=g, h_minus_q=int(r['hcount'].sum()) - int(r['charge'].sum()))


def check_assignment(cls, order, got, allow_charged=True, expect=None, where=''):
    """Validate what the code under test returned for one graph -- got: 'kekule_order', 'hcount', 'charge', 'counts', 'status' -- by
    the properties of its matching: every doubled bond is an allowed bond of order 4, no atom is matched twice, every MUST atom is
    covered, |M| is the restated maximum, and every output equals what section 1 gives FOR THAT MATCHING.
    expect=(feasible, pass, size): for graphs too large for the exhaustive search, whose answer is known by construction.
    Returns the restated solution."""
    g = graph_of_rows(cls, order)
    if expect is None:
        sol = solve(g, allow_charged)
    else:
        sol = {'feasible': expect[0], 'pass': expect[1], 'kinds': classify(g, expect[1]), 'size': expect[2], 'matching': set()}
    failed = bool(int(got['status']) & M.KEKULE_FAILED)
    assert failed == (not sol['feasible']), (where, 'feasible', sol['feasible'], int(got['status']))
    assert bool(int(got['status']) & M.KEKULE_CHARGED) == (sol['feasible'] and sol['pass'] == 1), (where, 'pass', sol['pass'], int(got['status']))
    kek = np.asarray(got['kekule_order'])
    assert kek.shape == (len(g['order']),), (where, kek.shape)
    matching = set()
    if sol['feasible']:
        ok = {(i, j) for i, j in allowed_edges(g, sol['kinds'])}
        seen = set()
        for i, j, row in g['arom']:
            assert kek[row] in (1, 2), (where, 'an aromatic bond left', i, j, int(kek[row]))
            if kek[row] == 2:
                assert (i, j) in ok, (where, 'doubled bond outside the allowed graph', i, j)
                assert i not in seen and j not in seen, (where, 'an atom with two double bonds', i, j)
                seen.update((i, j))
                matching.add((i, j))
        missed = [i for i in range(g['n']) if sol['kinds'][i] == MUST and i not in seen]
        assert not missed, (where, 'MUST atoms uncovered', missed)
        assert len(matching) == sol['size'], (where, 'cardinality', len(matching), sol['size'])
    want = results_for(g, sol, matching)
    for k in ('kekule_order', 'hcount', 'charge'):
        assert np.asarray(got[k]).dtype == want[k].dtype and np.array_equal(np.asarray(got[k]), want[k]), \
            (where, k, np.nonzero(np.asarray(got[k]) != want[k])[0][:8])
    assert np.asarray(got['counts']).tolist() == want['counts'].tolist(), \
        (where, dict(zip(M.KEKULE_COUNTS, zip(np.asarray(got['counts']).tolist(), want['counts'].tolist()))))
    assert int(got['status']) == want['status'], (where, int(got['status']), want['status'])
    return sol


def has_odd_cycle(n, edges):
    """Is the graph not bipartite?"""
    nbr = [[] for _ in range(n)]
    for i, j in edges:
        nbr[i].append(j)
        nbr[j].append(i)
    side = [-1] * n
    for s in range(n):
        if side[s] >= 0:
            continue
        side[s] = 0
        todo = [s]
        for u in todo:
            for v in nbr[u]:
                if side[v] < 0:
                    side[v] = 1 - side[u]
                    todo.append(v)
                elif side[v] == side[u]:
                    return True
    return False


# ---- building inputs ------------------------------------------------------------------------------------------------------------
def cycle(n, order=4, off=0):
    return MS.cycle(n, order, off)


def chain(n, order=4, off=0):
    return MS.chain(n, order, off)


def ladder(rungs, order=4):
    """A linear polyacene-like ladder: two rails of `rungs` atoms (0 .. rungs-1 and rungs .. 2 rungs-1), a rung at every even index:
    six-rings fused in a row.  Degree <= 3."""
    bonds = {**chain(rungs, order), **chain(rungs, order, off=rungs)}
    bonds.update({(i, rungs + i): order for i in range(0, rungs, 2)})
    return bonds


_AZULENE = {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 4): 4, (0, 4): 4, (4, 5): 4, (5, 6): 4, (6, 7): 4, (7, 8): 4, (8, 9): 4, (3, 9): 4}
_INDOLE = {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 8): 4, (0, 8): 4, (3, 4): 4, (4, 5): 4, (5, 6): 4, (6, 7): 4, (7, 8): 4}
_NAPHTHALENE = {**cycle(6), (0, 6): 4, (6, 7): 4, (7, 8): 4, (8, 9): 4, (1, 9): 4}
A_, CH_, CA_, F_BIT = M.KEKULE_HAS_AROMATIC, M.KEKULE_CHARGED, M.KEKULE_CATION, M.KEKULE_FAILED

# name: (classes, bonds, allow_charged, status, doubled, hydrogens, charge, {atom: (h, q)} for the atoms whose answer every maximum
# matching shares) -- all by hand
NAMED = {
    'benzene': ([C_] * 6, cycle(6), True, A_, 3, 6, 0, {i: (1, 0) for i in range(6)}),
    'pyridine': ([N_] + [C_] * 5, cycle(6), True, A_, 3, 5, 0, {0: (0, 0)}),
    'pyrrole': ([N_] + [C_] * 4, cycle(5), True, A_, 2, 5, 0, {0: (1, 0)}),
    'imidazole': ([N_, C_, N_, C_, C_], cycle(5), True, A_, 2, 4, 0, {1: (1, 0), 3: (1, 0), 4: (1, 0)}),
    'furan': ([O_] + [C_] * 4, cycle(5), True, A_, 2, 4, 0, {0: (0, 0)}),
    'thiophene': ([S_] + [C_] * 4, cycle(5), True, A_, 2, 4, 0, {0: (0, 0)}),
    '2-pyridone': ([N_] + [C_] * 5 + [O_], {**cycle(6), (1, 6): 2}, True, A_, 2, 5, 0, {0: (1, 0), 1: (0, 0), 6: (0, 0)}),
    'naphthalene': ([C_] * 10, _NAPHTHALENE, True, A_, 5, 8, 0, {0: (0, 0), 1: (0, 0)}),
    'azulene': ([C_] * 10, _AZULENE, True, A_, 5, 8, 0, {3: (0, 0), 4: (0, 0)}),
    'indole': ([N_] + [C_] * 8, _INDOLE, True, A_, 4, 7, 0, {0: (1, 0), 3: (0, 0), 8: (0, 0)}),
    'all-carbon five-ring': ([C_] * 5, cycle(5), True, A_ | F_BIT, 0, 10, 0, {i: (2, 0) for i in range(5)}),
    'indene-like': ([C_] * 9, _INDOLE, True, A_ | F_BIT, 0, 16, 0, {3: (1, 0), 8: (1, 0)}),
    'N-methylpyridinium': ([N_] + [C_] * 6, {**cycle(6), (0, 6): 1}, True, A_ | CH_ | CA_, 3, 8, 1, {0: (0, 1), 6: (3, 0)}),
    'thiopyrylium': ([S_] + [C_] * 5, cycle(6), True, A_ | CH_ | CA_, 3, 5, 1, {0: (0, 1)}),
    'thiopyrylium, neutral only': ([S_] + [C_] * 5, cycle(6), False, A_ | F_BIT, 0, 10, 0, {0: (0, 0)}),
    'pyridazine': ([N_, N_] + [C_] * 4, cycle(6), True, A_, 3, 4, 0, {0: (0, 0), 1: (0, 0)}),
    'three aromatic bonds in a chain': ([C_] * 4, chain(4), True, A_, 2, 6, 0, {0: (2, 0), 1: (1, 0), 2: (1, 0), 3: (2, 0)}),
    'a lone aromatic bond': ([C_] * 2, chain(2), True, A_, 1, 4, 0, {0: (2, 0), 1: (2, 0)}),
}

# graphs on which a search without blossom contraction goes wrong: the first search meets an odd cycle of matched and unmatched bonds
BLOSSOM = {
    'triangle with a tail': ([C_] * 4, {**cycle(3), (2, 3): 4}),
    'two five-rings sharing a bond': ([C_] * 8, {**cycle(5), (3, 5): 4, (5, 6): 4, (6, 7): 4, (4, 7): 4}),
    'azulene, seven-ring first': ([C_] * 10, {(min(a, b), max(a, b)): 4 for a, b in
                                              ((9 - a, 9 - b) for a, b in _AZULENE)}),
    'azulene, shuffled': ([C_] * 10, {(min(a, b), max(a, b)): 4 for a, b in
                                      (((7 * a + 3) % 10, (7 * b + 3) % 10) for a, b in _AZULENE)}),
}


# ---- the random family: sparse aromatic subgraphs among non-aromatic ballast --------------------------------------------------------
FAMILY_SIZES = (1, 2, 3, 5, 6, 9, 10, 63, 64, 65, 127, 128)
FAMILY_SEED, FAMILY_GRAPHS = 20240811, 96
MAX_AROMATIC = 20


def random_graph(rng, n):
    """One graph of n atoms as (classes, bonds): up to MAX_AROMATIC atoms form a sparse aromatic subgraph of degree <= 3 -- rings of
    3 to 7 atoms, fused along a bond or joined by a bond, with tails -- of mixed C / N / S / O / P; some carry a substituent (a
    single or double bond to a ballast atom), which moves them between MUST / MAY and NOT; the other atoms are ballast on a chain of
    single bonds.  The aromatic atoms lie anywhere in the numbering.  A few graphs get a dropped atom or a class-5 row."""
    k = int(min(n, rng.integers(2, MAX_AROMATIC + 1)))
    where = rng.permutation(n)                                          # where[i]: the atom that the i-th made vertex becomes
    arom, deg, made = set(), [0] * k, 0

    def bond(i, j):
        if i != j and deg[i] < 3 and deg[j] < 3 and (min(i, j), max(i, j)) not in arom:
            arom.add((min(i, j), max(i, j)))
            deg[i] += 1
            deg[j] += 1
            return True
        return False

    while made < k:
        left = k - made
        kind = rng.random()
        if made == 0 or kind < 0.25:                                    # a new ring, joined to the old part by a bond
            r = int(min(left, rng.choice([3, 5, 5, 5, 6, 6, 7, 7])))
            ring = list(range(made, made + r))
            for t in range(r - 1):
                bond(ring[t], ring[t + 1])
            if r >= 3:
                bond(ring[0], ring[-1])
            if made and rng.random() < 0.7:
                bond(int(rng.integers(0, made)), ring[0])
            made += r
        elif kind < 0.75 and arom:                                      # a ring fused along an existing bond
            edges = sorted(arom)
            i, j = edges[int(rng.integers(0, len(edges)))]
            r = int(min(left, rng.choice([1, 3, 3, 3, 4, 4, 5, 5])))    # new atoms: the ring has r + 2
            path = [i] + list(range(made, made + r)) + [j]
            for t in range(len(path) - 1):
                bond(path[t], path[t + 1])
            made += r
        else:                                                           # a tail atom
            bond(int(rng.integers(0, made)), made)
            made += 1
    classes = [int(c) for c in rng.choice([C_, C_, C_, O_], n, p=[0.4, 0.3, 0.2, 0.1])]
    for i in range(k):
        classes[where[i]] = int(rng.choice([C_, N_, S_, O_, P_], p=[0.62, 0.2, 0.08, 0.06, 0.04]))
    bonds = {(int(min(where[i], where[j])), int(max(where[i], where[j]))): 4 for i, j in arom}
    ballast = [int(a) for a in where[k:]]
    for t in range(len(ballast) - 1):                                   # the ballast chain
        if rng.random() < 0.85:
            a, b = sorted((ballast[t], ballast[t + 1]))
            bonds[(a, b)] = 1
    for i in range(k):                                                  # substituents
        if ballast and rng.random() < 0.22:
            a, b = sorted((int(where[i]), ballast[int(rng.integers(0, len(ballast)))]))
            bonds.setdefault((a, b), int(rng.choice([1, 1, 1, 2])))
    if n >= 5 and rng.random() < 0.15:
        classes[int(rng.integers(0, n))] = 11
    if n >= 5 and rng.random() < 0.15:
        a, b = sorted(int(v) for v in rng.choice(n, 2, replace=False))
        bonds[(a, b)] = 5
    return classes, bonds


def random_family(seed=FAMILY_SEED, n_graphs=FAMILY_GRAPHS, sizes=FAMILY_SIZES):
    """[(classes, bonds)]: the sizes of FAMILY_SIZES in turn."""
    rng = np.random.default_rng(seed)
    return [random_graph(rng, sizes[g % len(sizes)]) for g in range(n_graphs)]


def outcome(sol):
    return 'failed' if not sol['feasible'] else 'charged' if sol['pass'] == 1 else 'neutral'


# ---- tools/kekule_host_check.cpp: the kernel's core compiled for the host ------------------------------------------------------------
def run_host_check(exe, cases, work_dir):
    """cases: [(cls, order, allow_charged)] as rows -> one dict per case in `check_assignment`'s form."""
    path = os.path.join(str(work_dir), 'kekule_cases.txt')
    listed = []
    with open(path, 'w') as fh:
        for t in (_table(M.KEKULE_DBL_NEUTRAL), _table(M.KEKULE_DBL_CHARGED), _table(M.KEKULE_MUST), MS.padded_valences(M.H_VALENCES)):
            fh.write(' '.join(str(int(v)) for v in t) + '\n')
        for cls, order, allow in cases:
            n = len(cls)
            rows, a, b = MS.listed_pairs(n, order)
            listed.append(rows)
            fh.write('%d %d %d\n' % (n, int(allow), rows.size) + ' '.join(str(int(c)) for c in cls) + '\n'
                     + ' '.join('%d %d %d' % (x, y, order[r]) for x, y, r in zip(a, b, rows)) + '\n')
    out = MS.run_program(exe, path)
    got = []
    for c, ((cls, order, _), rows) in enumerate(zip(cases, listed)):
        head, kek_rows, hq = ([int(v) for v in out[3 * c + k].split()] for k in range(3))
        kek = np.array(order, dtype=np.int8)
        kek[rows] = kek_rows
        got.append({'status': head[0], 'counts': np.array(head[1:], dtype=np.int32), 'kekule_order': kek,
                    'hcount': np.array(hq[0::2], dtype=np.uint8), 'charge': np.array(hq[1::2], dtype=np.int8)})
    return got
