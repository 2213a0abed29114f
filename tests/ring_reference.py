"""Plain restatement of the ring screen (DESIGN.md 2.9 "Rings"; phoregen_amd/molecule.py, csrc/mol_rings.hip) for the tests, written
from the text in another form than the kernel: adjacency lists, a queue breadth-first search per bond on a copy of the graph with that
bond taken out, union-find for ring systems and components.  No device code; it shares nothing with the kernel but the named
constants of phoregen_amd.molecule.  Also here: the named molecules of the ring tests with their hand-written answers, and the
networkx graph of a graph's rows.  The graph builders, `rows_of`, `batch_from` and the walk over the pair rows are
tests/mol_support.py's."""
from collections import deque

import numpy as np

import mol_support as MS
from mol_support import C_, batch_from, pair_walk, rows_of  # noqa: F401  (batch_from and rows_of are read from here by the tests)
from phoregen_amd import molecule as M


def _shortest(nbrs, src, dst):
    """Bonds on a shortest path src -> dst over the adjacency lists, None if there is none (src != dst)."""
    dist = {src: 0}
    todo = deque([src])
    while todo:
        u = todo.popleft()
        for v in nbrs[u]:
            if v == dst:                                               # (first reached from the nearest atom that reaches it)
                return dist[u] + 1
            if v not in dist:
                dist[v] = dist[u] + 1
                todo.append(v)
    return None


class _Sets:
    def __init__(self, n):
        self.up = list(range(n))

    def find(self, x):
        while self.up[x] != x:
            self.up[x] = self.up[self.up[x]]
            x = self.up[x]
        return x

    def join(self, a, b):
        ra, rb = self.find(a), self.find(b)
        self.up[max(ra, rb)] = min(ra, rb)                             # the root of a set is its smallest member


def rings_of_rows(cls, order, limits=None):
    """One graph as the screen wrote it: cls int8 [n] (-1 = dropped), order int8 [n (n - 1) / 2] for the pairs a < b in row-major
    order.  Returns the kernel's outputs for it: 'ring_size' uint8 [h], 'atom_ring' uint8 [n], 'ring_sys' int16 [n], 'counts'
    int32 [10] (M.RING_COUNTS), 'status', 'ok'."""
    limits = M.RingLimits() if limits is None else limits
    n = len(cls)
    kept, nbrs, rows, order = pair_walk(cls, order)
    bonds = [(a, b, order[row], row) for (a, b), row in rows.items()]
    degree = [len(x) for x in nbrs]
    aromatic = [0] * n
    ring_size = np.zeros(len(order), dtype=np.uint8)
    comps, systems = _Sets(n), _Sets(n)
    in_ring = [False] * n
    atom_ring = np.zeros(n, dtype=np.uint8)
    rotatable = aromatic_outside = 0
    for a, b, o, r in bonds:
        cut = list(nbrs)                                               # the graph without this bond: the two ends get lists of their own
        cut[a], cut[b] = [v for v in nbrs[a] if v != b], [v for v in nbrs[b] if v != a]
        d = _shortest(cut, a, b)
        comps.join(a, b)
        if o == 4:
            aromatic[a] += 1
            aromatic[b] += 1
        if d is None:
            rotatable += o == 1 and degree[a] >= 2 and degree[b] >= 2
            aromatic_outside += o == 4
            continue
        assert 2 <= d <= 127
        ring_size[r] = 1 + d
        systems.join(a, b)
        for x in (a, b):
            atom_ring[x] = 1 + d if not in_ring[x] else min(int(atom_ring[x]), 1 + d)
            in_ring[x] = True
    ring_sys = np.full(n, -1, dtype=np.int16)
    members = {}
    for i in range(n):
        if in_ring[i]:
            ring_sys[i] = systems.find(i)
            members.setdefault(int(ring_sys[i]), []).append(i)
    n_kept = sum(kept)
    n_comp = len({comps.find(i) for i in range(n) if kept[i]})
    sizes = ring_size[ring_size > 0]
    counts = {'rings': len(bonds) - n_kept + n_comp, 'ring_bonds': int(sizes.size), 'ring_atoms': sum(in_ring), 'ring_systems': len(members),
              'ring_min': int(sizes.min()) if sizes.size else 0, 'ring_max': int(sizes.max()) if sizes.size else 0,
              'largest_system': max((len(v) for v in members.values()), default=0), 'rotatable': int(rotatable),
              'aromatic_outside_ring': int(aromatic_outside), 'aromatic_lone': sum(kept[i] and aromatic[i] == 1 for i in range(n))}
    status = 0
    status |= M.RING_AROMATIC_OUTSIDE if counts['aromatic_outside_ring'] > 0 else 0
    status |= M.RING_SMALL if 0 < counts['ring_min'] < limits.ring_min else 0
    status |= M.RING_LARGE if counts['ring_max'] > limits.ring_max else 0
    status |= M.RING_SYSTEM_LARGE if counts['largest_system'] > limits.system_max else 0
    status |= M.RING_ROTATABLE if counts['rotatable'] > limits.rotatable_max else 0
    status |= M.RING_AROMATIC_LONE if counts['aromatic_lone'] > 0 else 0
    return {'ring_size': ring_size, 'atom_ring': atom_ring, 'ring_sys': ring_sys,
            'counts': np.array([counts[k] for k in M.RING_COUNTS], dtype=np.int32), 'status': status,
            'ok': (status & M.RING_FAIL_MASK) == 0}


def rings_of_batch(refs, limits=None):
    """The rows of a restated batch (tests/mol_reference.screen_batch): one `rings_of_rows` result per graph."""
    return [rings_of_rows(r['cls'], r['order'], limits) for r in refs]


# ---- building inputs ------------------------------------------------------------------------------------------------------------
def cycle(n, order=1, off=0):
    return MS.cycle(n, order, off)


def chain(n, order=1, off=0):
    return MS.chain(n, order, off)


def _named():
    naphthalene = cycle(6, 4)
    naphthalene.update({(0, 6): 4, (6, 7): 4, (7, 8): 4, (8, 9): 4, (1, 9): 4})
    biphenyl = {**cycle(6, 4), **cycle(6, 4, off=6)}
    biphenyl[(0, 6)] = 1
    spiro = {**cycle(5), (0, 5): 1, (5, 6): 1, (6, 7): 1, (7, 8): 1, (8, 9): 1, (0, 9): 1}
    norbornane = {**cycle(6), (0, 6): 1, (3, 6): 1}
    cubane = {**cycle(4), **cycle(4, off=4), (0, 4): 1, (1, 5): 1, (2, 6): 1, (3, 7): 1}
    toluene = {**cycle(6, 4), (0, 6): 4}
    hexane = {**chain(6), (1, 2): 4, (2, 3): 4}
    # name: (classes, bonds, counts in M.RING_COUNTS order, status with the default limits, status with FILTER) -- all by hand
    A, L = M.RING_AROMATIC_OUTSIDE, M.RING_AROMATIC_LONE
    return {
        'benzene': ([C_] * 6, cycle(6, 4), [1, 6, 6, 1, 6, 6, 6, 0, 0, 0], 0, 0),
        'naphthalene': ([C_] * 10, naphthalene, [2, 11, 10, 1, 6, 6, 10, 0, 0, 0], 0, M.RING_SYSTEM_LARGE),
        'biphenyl': ([C_] * 12, biphenyl, [2, 12, 12, 2, 6, 6, 6, 1, 0, 0], 0, M.RING_ROTATABLE),
        'spiro[4.5]decane': ([C_] * 10, spiro, [2, 11, 10, 1, 5, 6, 10, 0, 0, 0], 0, M.RING_SYSTEM_LARGE),
        'norbornane': ([C_] * 7, norbornane, [2, 8, 7, 1, 5, 5, 7, 0, 0, 0], 0, 0),
        'cubane': ([C_] * 8, cubane, [5, 12, 8, 1, 4, 4, 8, 0, 0, 0], 0, M.RING_SMALL),
        'cyclopropane': ([C_] * 3, cycle(3), [1, 3, 3, 1, 3, 3, 3, 0, 0, 0], 0, M.RING_SMALL),
        'macrocycle14': ([C_] * 14, cycle(14), [1, 14, 14, 1, 14, 14, 14, 0, 0, 0], 0, M.RING_LARGE | M.RING_SYSTEM_LARGE),
        'toluene_aromatic_methyl': ([C_] * 7, toluene, [1, 6, 6, 1, 6, 6, 6, 0, 1, 1], A | L, A | L),
        'hexane_two_aromatic': ([C_] * 6, hexane, [0, 0, 0, 0, 0, 0, 0, 1, 2, 2], A | L, A | L | M.RING_ROTATABLE),
        'butane': ([C_] * 4, chain(4), [0, 0, 0, 0, 0, 0, 0, 1, 0, 0], 0, M.RING_ROTATABLE),
    }


NAMED = _named()
FILTER = dict(ring_min=5, ring_max=8, system_max=9, rotatable_max=0)     # the limits of the fifth column of NAMED


def nx_graph(cls, order):
    """networkx graph of one graph's rows (kept atoms as nodes, bonds as edges)."""
    import networkx as nx
    w = pair_walk(cls, order)
    g = nx.Graph()
    g.add_nodes_from(i for i, k in enumerate(w.kept) if k)
    g.add_edges_from(w.rows)
    return g
