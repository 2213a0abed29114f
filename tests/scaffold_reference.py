"""Plain restatement of the scaffold (DESIGN.md 2.9 "Scaffolds"; phoregen_amd/scaffold.py, csrc/mol_scaffold.hip) for the tests, written
from the definition in another form than the kernel: sets of atoms and one leaf at a time for the pruning, a bridge test that deletes
the bond and searches for its other end, union-find for components and ring systems.  No device code; it shares nothing with the
kernel but the named constants of phoregen_amd.molecule / phoregen_amd.scaffold.  Also here: the named molecules of the scaffold tests
(their hand-written answers are in tests/test_molscaffold_host.py) and the seeded family with chosen atoms at the word and lane
boundaries.  The graph builders, `rows_of`, `batch_from` and the walk over the pair rows are tests/mol_support.py's."""
import numpy as np

import mol_support as MS
from mol_support import B_, C_, N_, O_, S_, chain, cycle, pair_walk, rows_of
from phoregen_amd import molecule as M
from phoregen_amd import scaffold as SC

OPTIONS = [(True, False), (False, False), (True, True), (False, True)]       # (exocyclic, generic), the default first


def _reaches(nbrs, src, dst, without):
    """Is dst reachable from src when the bond `without` = (a, b) is taken out?"""
    seen, todo = {src}, [src]
    while todo:
        u = todo.pop()
        for v in nbrs[u]:
            if {u, v} == set(without) or v in seen:
                continue
            if v == dst:
                return True
            seen.add(v)
            todo.append(v)
    return False


def _roots(n, members, bonds):
    """Union-find over `bonds` restricted to `members`: {atom: smallest atom of its class}."""
    up = list(range(n))

    def find(x):
        while up[x] != x:
            x = up[x]
        return x

    for a, b in bonds:
        if a in members and b in members:
            ra, rb = find(a), find(b)
            up[max(ra, rb)] = min(ra, rb)
    return {i: find(i) for i in members}


def scaffold_of_rows(cls, order, exocyclic=True, generic=False):
    """One graph as the screen wrote it (cls int8 [n], -1 = dropped; order int8 [n (n - 1) / 2]).  Returns the kernel's outputs for
    it: 'part' uint8 [n], 'counts' int32 [8] (SC.SCAFFOLD_COUNTS), and the scaffold screen's 'cls', 'compact', 'valence2', 'comp' [n],
    'order' [h], 's_counts' int32 [4], 'status', 'valid'; plus the sets 'core', 'ring_bonds', 'linker_bonds' for the tests."""
    n = len(cls)
    w = pair_walk(cls, order)
    kept = {i for i in range(n) if w.kept[i]}
    bonds = {ab: w.order[row] for ab, row in w.rows.items()}
    # core: one leaf at a time (the 2-core does not depend on the order of the removals)
    core = set(kept)
    while True:
        leaf = next((i for i in sorted(core) if sum(v in core for v in w.nbrs[i]) <= 1), None)
        if leaf is None:
            break
        core.discard(leaf)
    core_bonds = [ab for ab in bonds if ab[0] in core and ab[1] in core]
    ring_bonds = [ab for ab in core_bonds if _reaches(w.nbrs, ab[0], ab[1], ab)]
    linker_bonds = [ab for ab in core_bonds if ab not in ring_bonds]
    ring_atoms = {x for ab in ring_bonds for x in ab}
    exo = set()
    if exocyclic:
        exo = {x for (a, b), o in bonds.items() if o == 2 for x, y in ((a, b), (b, a)) if x not in core and y in core}
    scaffold = core | exo
    part = np.zeros(n, dtype=np.uint8)
    for i in kept:
        part[i] = (SC.PART_RING if i in ring_atoms else SC.PART_LINKER if i in core else SC.PART_EXOCYCLIC if i in exo
                   else SC.PART_SIDE_CHAIN)
    s_bonds = {ab: (1 if generic else o) for ab, o in bonds.items() if ab[0] in scaffold and ab[1] in scaffold}
    s_cls = np.full(n, -1, dtype=np.int8)
    compact = np.full(n, -1, dtype=np.int16)
    for c, i in enumerate(sorted(scaffold)):
        s_cls[i] = C_ if generic else cls[i]
        compact[i] = c
    s_order = np.zeros(len(w.order), dtype=np.int8)
    val2 = np.zeros(n, dtype=np.int64)
    for (a, b), o in s_bonds.items():
        s_order[w.rows[(a, b)]] = o
        val2[a] += 3 if o == 4 else 2 * o
        val2[b] += 3 if o == 4 else 2 * o
    roots = _roots(n, scaffold, s_bonds)
    comp = np.full(n, -1, dtype=np.int16)
    for i, r in roots.items():
        comp[i] = r
    sizes = {}
    for r in roots.values():
        sizes[r] = sizes.get(r, 0) + 1
    systems = set(_roots(n, ring_atoms, ring_bonds).values())
    status = (M.STATUS_NO_ATOMS if not scaffold else 0) | (M.STATUS_DISCONNECTED if len(sizes) > 1 else 0)
    counts = [len(scaffold), len(s_bonds), len(ring_atoms), len(core - ring_atoms), len(exo), len(kept - scaffold), len(systems),
              len(linker_bonds)]
    return {'part': part, 'counts': np.array(counts, dtype=np.int32), 'cls': s_cls, 'compact': compact,
            'valence2': np.minimum(val2, 255).astype(np.uint8), 'comp': comp, 'order': s_order,
            's_counts': np.array([len(scaffold), len(s_bonds), len(sizes), max(sizes.values(), default=0)], dtype=np.int32),
            'status': status, 'valid': (status & M.FAIL_MASK) == 0,
            'core': core, 'ring_bonds': sorted(ring_bonds), 'linker_bonds': sorted(linker_bonds)}


ARRAYS = ('part', 'counts', 'cls', 'compact', 'valence2', 'comp', 'order', 's_counts', 'status', 'valid')    # what the kernel writes


def scaffold_of_graphs(graphs, exocyclic=True, generic=False):
    """`scaffold_of_rows` of every (classes 0..11, {(a, b): bond class 1..5}) graph, through `rows_of`."""
    return [scaffold_of_rows(*rows_of(g[0], g[1]), exocyclic=exocyclic, generic=generic) for g in graphs]


# ---- the named molecules: name -> (atom classes 0..11, {(a, b): bond class 1..5}) -----------------------------------------------------
def _named():
    tail = {**cycle(3, 1), **chain(126, 1, off=2)}                         # atoms 0..2 the ring, 2 - 3 - .. - 127 the tail
    toluene = {**cycle(6, 4), (0, 6): 1}
    biphenyl = {**cycle(6, 4), **cycle(6, 4, off=6), (0, 6): 1}
    # two phenyls on carbon 12, which also carries the methyl 13
    diphenylmethane_me = {**cycle(6, 4), **cycle(6, 4, off=6), (0, 12): 1, (6, 12): 1, (12, 13): 1}
    spiro = {**cycle(5, 1), (0, 5): 1, (5, 6): 1, (6, 7): 1, (7, 8): 1, (8, 9): 1, (0, 9): 1}
    fused = {**cycle(6, 4), (0, 6): 4, (6, 7): 4, (7, 8): 4, (8, 9): 4, (1, 9): 4}
    bridged = {**cycle(6, 1), (0, 6): 1, (3, 6): 1}
    ring_co = {**cycle(6, 1), (0, 6): 2}                                   # cyclohexanone
    linker_co = {**cycle(6, 4), **cycle(6, 4, off=6), (0, 12): 1, (6, 12): 1, (12, 13): 2}    # benzophenone
    ring_exo_c = {**cycle(6, 1), (0, 6): 2, (6, 7): 1, (6, 8): 1}          # ring =C(-C)-C
    triple = {**cycle(6, 1), (0, 6): 3, (6, 7): 1}
    two_systems = {**cycle(6, 4), **cycle(5, 1, off=6), (0, 11): 1}        # benzene with a methyl, and a separate five-ring
    dropped = {**cycle(6, 1), (0, 6): 1}                                   # atom 3 of the ring is class 11: the ring is open
    absorbing = {**cycle(6, 1), (2, 3): 5, (0, 6): 1}                      # the ring bond 2 - 3 is an absorbing row
    named = {
        'none': ([], {}),
        'one_atom': ([C_], {}),
        'two_atoms': ([C_, O_], {(0, 1): 1}),
        'three_atoms': ([C_, C_, O_], {(0, 1): 1, (1, 2): 2}),
        'chain128': ([C_] * 128, chain(128, 1)),
        'ring3_tail125': ([C_] * 128, tail),
        'benzene': ([C_] * 6, cycle(6, 4)),
        'toluene': ([C_] * 7, toluene),
        'biphenyl': ([C_] * 12, biphenyl),
        'diphenylmethane_methyl': ([C_] * 14, diphenylmethane_me),
        'spiro': ([C_] * 10, spiro),
        'fused': ([C_] * 10, fused),
        'bridged': ([C_] * 7, bridged),
        'ring_carbonyl': ([C_] * 6 + [O_], ring_co),
        'linker_carbonyl': ([C_] * 13 + [O_], linker_co),
        'ring_exocyclic_carbon': ([C_] * 9, ring_exo_c),
        'ring_triple': ([C_] * 7 + [N_], triple),
        'two_ring_systems': ([C_] * 12, two_systems),
        'dropped_in_ring': ([C_, C_, C_, 11, C_, C_, C_], dropped),
        'absorbing_on_ring': ([C_] * 7, absorbing),
    }
    return named


NAMED = _named()


# ---- the seeded family ----------------------------------------------------------------------------------------------------------------
FAMILY_SEED = 20241105
FAMILY_SIZES = (63, 64, 65, 127, 128)
BOUNDARY = (62, 63, 64, 65, 127)                                           # local indices at the word and lane boundaries
ROLES = (SC.PART_RING, SC.PART_LINKER, SC.PART_EXOCYCLIC)


def _boundary_graph(rng, n, shift):
    """A graph of n atoms: two ring systems joined by a linker chain with an `=O` on a linker atom and on ring atoms, side chains and
    substituents on the exocyclic atoms up to n atoms, numbered so that the boundary indices below n hold a ring atom, a linker atom or
    an exocyclic atom in turn (which one first: `shift`).  Returns (classes, bonds, {index: role})."""
    atoms, bonds = [], []                                                  # roles in an abstract numbering; bonds as (a, b, order)

    def add(role, cls):
        atoms.append((role, cls))
        return len(atoms) - 1

    def ring(size, order):
        ids = [add(SC.PART_RING, int(rng.choice([C_, C_, C_, N_, S_]))) for _ in range(size)]
        bonds.extend((ids[i], ids[(i + 1) % size], order) for i in range(size))
        return ids

    ra, rb = ring(6, 4), ring(5, 1)
    fused = [add(SC.PART_RING, C_) for _ in range(3)]                      # a second ring fused onto ra
    bonds.extend([(ra[0], fused[0], 1), (fused[0], fused[1], 1), (fused[1], fused[2], 1), (fused[2], ra[1], 1)])
    link = [add(SC.PART_LINKER, int(rng.choice([C_, N_, O_]))) for _ in range(int(rng.integers(4, 8)))]
    bonds.extend((a, b, 1) for a, b in zip([ra[3]] + link, link + [rb[0]]))
    exos = []
    for host in [link[1], link[2], rb[2], rb[3], fused[1]]:
        x = add(SC.PART_EXOCYCLIC, int(rng.choice([O_, C_, S_])))
        bonds.append((host, x, 2))
        exos.append(x)
    while len(atoms) < n:                                                  # side chains anywhere, the exocyclic atoms' own included
        host = int(rng.integers(0, len(atoms)))
        x = add(SC.PART_SIDE_CHAIN, int(rng.choice([C_, C_, N_, O_, 9 if rng.random() < 0.1 else C_])))
        bonds.append((host, x, int(rng.choice([1, 1, 1, 3])) if atoms[host][0] != SC.PART_SIDE_CHAIN or rng.random() < 0.8 else 2))
    # numbering: the boundary indices take a ring, a linker, an exocyclic atom in turn; everything else at random
    want = {b: ROLES[(k + shift) % 3] for k, b in enumerate(BOUNDARY) if b < n}
    free = {role: [i for i, (r, _) in enumerate(atoms) if r == role] for role in ROLES}
    number, used = {}, set()
    for b, role in want.items():
        pool = free[role]
        i = pool.pop(int(rng.integers(0, len(pool))))
        number[i] = b
        used.add(b)
    rest = [i for i in range(n) if i not in used]
    rng.shuffle(rest)
    for i in range(len(atoms)):
        if i not in number:
            number[i] = rest.pop()
    classes = [0] * n
    for i, (_, c) in enumerate(atoms):
        classes[number[i]] = c
    out = {}
    for a, b, o in bonds:
        out[(min(number[a], number[b]), max(number[a], number[b]))] = o
    return classes, out, want


def _random_graph(rng, n):
    """A small graph with no plan: a random forest plus a few extra bonds, mixed orders and classes, now and then a dropped atom or an
    absorbing row."""
    classes = [int(c) for c in rng.choice([B_, C_, C_, C_, N_, O_, S_], size=n)]
    if rng.random() < 0.3:
        classes[int(rng.integers(0, n))] = 11
    bonds = {}
    for b in range(1, n):
        if rng.random() < 0.92:
            bonds[(int(rng.integers(0, b)), b)] = int(rng.choice([1, 1, 1, 2, 2, 3, 4]))
    for _ in range(int(rng.integers(0, 5))):
        a, b = sorted(int(v) for v in rng.choice(n, size=2, replace=False))
        bonds[(a, b)] = int(rng.choice([1, 2, 4, 5]))
    return classes, bonds


def family(seed=FAMILY_SEED):
    """[(classes, bonds)] and, per graph, the {index: role} that its numbering was built for ({} for the random graphs)."""
    rng = np.random.default_rng(seed)
    graphs, wants = [], []
    for n in FAMILY_SIZES:
        for shift in range(3):
            classes, bonds, want = _boundary_graph(rng, n, shift)
            graphs.append((classes, bonds))
            wants.append(want)
    for n in [int(v) for v in rng.integers(4, 40, 24)]:
        graphs.append(_random_graph(rng, n))
        wants.append({})
    return graphs, wants


# ---- the host-check program (tools/scaffold_host_check.cpp) ------------------------------------------------------------------------------
def write_cases(path, graphs, options=OPTIONS):
    """One case per graph and option pair: `n flags n_rows`, the n classes (-1 = dropped), n_rows triples `a b order` (every pair row
    that is not 0, absorbing rows included)."""
    with open(path, 'w') as fh:
        for classes, bonds in graphs:
            cls = [c if c <= 10 else -1 for c in classes]
            rows = sorted(bonds.items())
            for exo, gen in options:
                fh.write(f'{len(cls)} {int(exo) | 2 * int(gen)} {len(rows)}\n')
                fh.write(' '.join(str(c) for c in cls) + '\n')
                fh.write(' '.join(f'{a} {b} {o}' for (a, b), o in rows) + '\n')


def expected_lines(graphs, options=OPTIONS):
    """What the program prints for `write_cases`: per case a line with the status, the four screen counts and the eight counts; a line
    `part cls compact valence2 comp` per atom, flattened; a line with the scaffold order of every listed row."""
    lines = []
    for classes, bonds in graphs:
        cls, order = rows_of(classes, bonds)
        rows = sorted(bonds.items())
        n = len(classes)
        for exo, gen in options:
            r = scaffold_of_rows(cls, order, exo, gen)
            lines.append(' '.join(str(int(v)) for v in [r['status'], *r['s_counts'], *r['counts']]))
            lines.append(' '.join(f"{r['part'][i]} {r['cls'][i]} {r['compact'][i]} {r['valence2'][i]} {r['comp'][i]}" for i in range(n)))
            lines.append(' '.join(str(int(r['order'][MS.pair_row(a, b, n)])) for (a, b), _ in rows))
    return lines
