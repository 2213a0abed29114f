"""Plain restatement of the molecule screen (phoregen_amd/molecule.py, csrc/mol_screen.hip) for the tests: `decode_data` of
phoregen_amd.utils.sample_utils (pinned to the reference's recorded fixture elsewhere in the suite) filtered to the pairs a < b, then
union-find, degree / valence and the status rule in Python.  No device code, nothing shared with the kernel but the constants of
phoregen_amd.molecule (the status bits and the one valence table)."""
import numpy as np
import torch

from phoregen_amd import molecule as M
from phoregen_amd.plan import make_edge_data
from phoregen_amd.utils.sample_utils import ATOM_TYPES, decode_data


def pair_row(a, b, n):
    """Row of the pair a < b among the first-half bond rows of a graph with n atoms (row-major upper triangle)."""
    return a * n - a * (a + 1) // 2 + (b - a - 1)


def screen_graph(node_scores, pos, edge_scores, edge_index, max_valence=None):
    """One graph: node_scores [n, 12], pos [n, 3], edge_scores [n(n-1), 6], edge_index [2, n(n-1)] local atom ids (CPU tensors).
    Returns the kernel's outputs for it as numpy arrays / ints, plus 'decoded' (decode_data's dict with bonds filtered to a < b)."""
    max_valence = M.MAX_VALENCE if max_valence is None else max_valence
    n = node_scores.shape[0]
    h = n * (n - 1) // 2
    d = decode_data([node_scores, pos, edge_scores], edge_index, include_bond=True)
    at = node_scores.argmax(-1).numpy() if n else np.zeros(0, dtype=np.int64)
    keep = at < len(ATOM_TYPES)
    kept_local = np.nonzero(keep)[0]                       # compact index -> local atom index
    assert [ATOM_TYPES[c] for c in at[keep]] == d['element']
    cls = np.where(keep, at, -1).astype(np.int8)
    compact = np.full(n, -1, dtype=np.int16)
    compact[keep] = np.arange(kept_local.size)
    bi, bt = d['bond_index'].numpy().reshape(2, -1), d['bond_type'].numpy().reshape(-1)
    half = bi[0] < bi[1]                                    # the reference builds bonds from node_i < node_j only
    bi, bt = bi[:, half], bt[half]
    d = dict(d, bond_index=torch.from_numpy(bi), bond_type=torch.from_numpy(bt))
    order = np.zeros(h, dtype=np.int8)
    val2 = np.zeros(n, dtype=np.int64)
    deg = np.zeros(n, dtype=np.int64)
    arom = np.zeros(n, dtype=bool)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for (ca, cb), t in zip(bi.T.tolist(), bt.tolist()):
        a, b = int(kept_local[ca]), int(kept_local[cb])
        assert a < b and 1 <= t <= 4
        order[pair_row(a, b, n)] = t
        for x in (a, b):
            val2[x] += 3 if t == 4 else 2 * t
            deg[x] += 1
            arom[x] |= t == 4
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)               # the root of a component is its smallest index
    comp = np.full(n, -1, dtype=np.int16)
    for i in kept_local.tolist():
        comp[i] = find(i)
    sizes = np.bincount(comp[keep].astype(np.int64), minlength=1) if kept_local.size else np.zeros(1, dtype=np.int64)
    n_comp = int((sizes > 0).sum())
    # first-half rows by their own argmax (class 5 there is informational; the second half is never looked at)
    ei = edge_index.numpy().reshape(2, -1)
    first = ei[0] < ei[1]
    et_first = edge_scores.argmax(-1).numpy()[first] if h else np.zeros(0, dtype=np.int64)
    assert et_first.size == h and (pair_row(ei[0][first], ei[1][first], n) == np.arange(h)).all()
    status = 0
    if kept_local.size == 0:
        status |= M.STATUS_NO_ATOMS
    if n_comp > 1:
        status |= M.STATUS_DISCONNECTED
    for i in kept_local.tolist():
        if val2[i] > 2 * max_valence[ATOM_TYPES[at[i]]] + (1 if arom[i] else 0):
            status |= M.STATUS_VALENCE
    if kept_local.size and not np.isfinite(pos.numpy()[keep]).all():
        status |= M.STATUS_NONFINITE
    if (at == len(ATOM_TYPES)).any():
        status |= M.STATUS_HAD_MASKED_ATOM
    if (et_first == 5).any():
        status |= M.STATUS_HAD_ABSORBING_BOND
    return {'status': status, 'counts': np.array([kept_local.size, bt.size, n_comp, int(sizes.max())], dtype=np.int32),
            'cls': cls, 'compact': compact, 'valence2': np.minimum(val2, 255).astype(np.uint8), 'comp': comp, 'order': order,
            'degree': deg, 'valid': (status & M.FAIL_MASK) == 0, 'decoded': d}


def screen_batch(node_scores, pos, edge_scores, num_atoms):
    """A batch in the sampler's layout (CPU tensors, one frame): list of `screen_graph` results."""
    out, n0, e0 = [], 0, 0
    for n in [int(v) for v in num_atoms]:
        e = n * (n - 1)
        ei = make_edge_data(torch.tensor([n]))[0]
        out.append(screen_graph(node_scores[n0:n0 + n], pos[n0:n0 + n], edge_scores[e0:e0 + e], ei))
        n0, e0 = n0 + n, e0 + e
    return out


# ---- building inputs ----------------------------------------------------------------------------------------------------------
def scores_from_classes(atom_cls, bonds, reversed_only=(), pos=None):
    """One graph as the sampler would hand it over, from classes: atom_cls (0..11 per atom), bonds {(a, b): class 1..5} for a < b
    (written to BOTH halves, as the sampler's symmetric bond state has them), reversed_only {(a, b): class}: written to the reversed
    half only.  Scores are one-hots, like the trajectory frames."""
    n = len(atom_cls)
    h = n * (n - 1) // 2
    node = torch.zeros(n, 12)
    node[torch.arange(n), torch.tensor(atom_cls, dtype=torch.long)] = 1.0
    et = torch.zeros(2 * h, dtype=torch.long)
    for (a, b), t in dict(bonds).items():
        assert a < b
        et[pair_row(a, b, n)] = t
        et[h + pair_row(a, b, n)] = t
    for (a, b), t in dict(reversed_only).items():
        et[h + pair_row(a, b, n)] = t
    edge = torch.zeros(2 * h, 6)
    edge[torch.arange(2 * h), et] = 1.0
    if pos is None:
        pos = torch.arange(3 * n, dtype=torch.float32).reshape(n, 3) * 0.25
    return node, pos.clone(), edge, make_edge_data(torch.tensor([n]))[0]


# frozen generator of the ragged GPU batch (tests/test_gpu_molecule.py): tuned on the CPU with this file alone so that the batch
# holds enough graphs of every kind; the counts are asserted on this restatement's output before the kernel is looked at
GEN_SEED = 20240607
GEN_SIZES = [1, 2, 3, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS]
GEN_GRAPHS = 160
P_TREE, EXTRA_PER_N, P_SINGLE = 0.7, 0.15, 0.9


def generate_batch(seed=GEN_SEED, n_graphs=GEN_GRAPHS):
    """Ragged batch of logits: carbon-heavy atom classes, a random spanning tree on P_TREE of the graphs plus extra bonds with
    probability EXTRA_PER_N / n per pair (uniformly random logits would bond almost every pair), mostly single; every third graph a long
    thin tree of C / N instead; a few rows forced to
    class 5, a few atoms to class 11, two graphs all-masked, one graph with a NaN coordinate.  The chosen class gets the largest
    logit by a margin, the rest is noise: first-maximum ties are exercised by the one-hot inputs of the other tests.
    Returns (node [N,12], pos [N,3], edge [E,6], num_atoms list) as CPU tensors."""
    rng = np.random.default_rng(seed)
    sizes = list(GEN_SIZES) + [int(v) for v in rng.integers(4, 40, n_graphs - len(GEN_SIZES))]
    atom_p = np.array([1, 60, 12, 12, 3, 1, 1, 4, 3, 2, 1], dtype=np.float64)
    atom_p /= atom_p.sum()
    nodes, poss, edges = [], [], []
    for g, n in enumerate(sizes):
        h = n * (n - 1) // 2
        ac = rng.choice(11, size=n, p=atom_p)
        if g % 9 == 4 and n > 2:
            ac[rng.integers(0, n, max(1, n // 10))] = 11
        if g in (20, 21):
            ac[:] = 11
        et = np.zeros(h, dtype=np.int64)
        a_idx, b_idx = np.triu_indices(n, 1)
        if h:
            extra = rng.random(h) < EXTRA_PER_N / n
            if g % 3 == 0:                                   # a long thin tree of C / N: large valid graphs, long label chains
                ac[ac != 11] = rng.choice([1, 2], size=int((ac != 11).sum()))
                extra[:] = False
                for b in range(1, n):
                    extra[pair_row(int(rng.integers(max(0, b - 2), b)), b, n)] = True
            elif rng.random() < P_TREE or n >= 63:
                for b in range(1, n):
                    extra[pair_row(int(rng.integers(0, b)), b, n)] = True
            kinds = np.where(rng.random(h) < P_SINGLE, 1, rng.integers(2, 5, h))
            et[extra] = kinds[extra]
            if g % 5 == 2:
                et[rng.integers(0, h, max(1, h // 50))] = 5
        et_full = np.concatenate([et, et])
        node = rng.normal(0, 1, (n, 12)).astype(np.float32)
        node[np.arange(n), ac] += 8.0
        edge = rng.normal(0, 1, (2 * h, 6)).astype(np.float32)
        edge[np.arange(2 * h), et_full] += 8.0
        pos = rng.normal(0, 3, (n, 3)).astype(np.float32)
        if g == 30:
            pos[n // 2, 1] = np.nan
        nodes.append(node), poss.append(pos), edges.append(edge)
    return (torch.from_numpy(np.concatenate(nodes)), torch.from_numpy(np.concatenate(poss)),
            torch.from_numpy(np.concatenate(edges)), sizes)


def census(refs):
    """How many graphs of a restated batch are valid / carry each status bit."""
    c = {'valid': sum(r['valid'] for r in refs)}
    for bit, name in M.STATUS_NAMES.items():
        c[name] = sum(bool(r['status'] & bit) for r in refs)
    return c
