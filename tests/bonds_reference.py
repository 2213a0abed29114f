"""Plain restatement of the distance bond screen (phoregen_amd/molecule.py screen(bonds='distance'), csrc/mol_screen_dist.hip) for the
tests: fp32 distances, the nested strict rule of the reference's utils/predict_bonds.py over the thresholds of
`molecule.bond_thresholds`, then the screen's own phases by handing the perceived orders, as one-hot edge scores, to
tests/mol_reference.py.  No device code; nothing shared with the kernel but the constants and the one table of phoregen_amd.molecule.

Every input built here keeps 100 * distance at least MARGIN_PM away from every threshold of its pair (measured in float64 on the fp32
coordinates).  The fp32 error of 100 * d at these distances (below 3 Angstrom: an ulp of 300 is 3e-5, a few of them from the three
squares, the root and the product) stays below 2e-4 pm whichever way the sum is rounded or contracted, so every comparison with the
kernel and with the reference's recorded answers is exact."""
import numpy as np
import torch

import mol_reference as R
from phoregen_amd import molecule as M
from phoregen_amd.plan import make_edge_data
from phoregen_amd.utils.sample_utils import ATOM_TYPES

MARGIN_PM = 1e-3
UNMAPPED_CLASSES = (ATOM_TYPES.index(5), ATOM_TYPES.index(14))       # B, Si


def pair_d100(pos):
    """100 * distance of the pairs a < b in row-major order, in fp32 as the kernel computes it."""
    n = pos.shape[0]
    a, b = np.triu_indices(n, 1)
    p = np.asarray(pos, dtype=np.float32)
    d = p[a] - p[b]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.float32(100.0) * np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=np.float32)


def usable(cls, pos):
    """Atoms that take part in the rule: kept (class 0..10) and all three coordinates finite."""
    cls = np.asarray(cls)
    return (cls >= 0) & (cls < len(ATOM_TYPES)) & np.isfinite(np.asarray(pos, dtype=np.float32)).all(1)


def distance_orders(cls, pos, thresholds):
    """int8 [n (n - 1) / 2]: the order of every pair a < b.  cls [n] (anything outside 0..10: dropped), pos fp32 [n, 3],
    thresholds [11, 11, 3]."""
    cls = np.asarray(cls, dtype=np.int64)
    n = cls.size
    a, b = np.triu_indices(n, 1)
    ok = usable(cls, pos)
    d100 = pair_d100(pos)
    order = np.zeros(a.size, dtype=np.int8)
    for p in np.nonzero(ok[a] & ok[b])[0].tolist():
        t = thresholds[cls[a[p]], cls[b[p]]]
        if d100[p] < t[0]:
            order[p] = 1
            if d100[p] < t[1]:
                order[p] = 2
                if d100[p] < t[2]:
                    order[p] = 3
    return order


def min_margin_pm(cls, pos, thresholds):
    """The smallest |100 d - t| in pm, in float64 on the fp32 coordinates, over the pairs of usable atoms and the thresholds t > 0
    of their two elements (inf without one)."""
    cls = np.asarray(cls, dtype=np.int64)
    a, b = np.triu_indices(cls.size, 1)
    ok = usable(cls, pos)
    sel = ok[a] & ok[b]
    if not sel.any():
        return np.inf
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    d100 = 100.0 * np.sqrt(((p[a[sel]] - p[b[sel]]) ** 2).sum(1))
    t = thresholds[cls[a[sel]], cls[b[sel]]].astype(np.float64)
    gap = np.where(t > 0, np.abs(d100[:, None] - t), np.inf)
    return float(gap.min()) if gap.size else np.inf


def agreement(pred, order, both):
    """The six BOND_AGREE_COUNTS.  pred: argmax class of the pair rows (5 counts as no bond), order: the distance order, both: the
    pair's two atoms are usable."""
    pr = np.where((pred >= 1) & (pred <= 4), pred, 0)[both]
    o = order[both].astype(np.int64)
    bb = (pr > 0) & (o > 0)
    same, arom = bb & (pr == o), bb & (pr == 4) & (o <= 2)
    return np.array([same.sum(), arom.sum(), (bb & ~same & ~arom).sum(), ((pr > 0) & (o == 0)).sum(), ((pr == 0) & (o > 0)).sum(),
                     ((pr == 0) & (o == 0)).sum()], dtype=np.int32)


def onehot_edges(order):
    """Edge scores [2 h, 6] whose argmax is `order` in both halves."""
    et = torch.from_numpy(np.concatenate([order, order]).astype(np.int64))
    edge = torch.zeros(et.numel(), 6)
    edge[torch.arange(et.numel()), et] = 1.0
    return edge


def screen_graph(node_scores, pos, edge_scores=None, margins=None):
    """One graph: node_scores [n, 12], pos [n, 3], edge_scores [n (n - 1), 6] or None (CPU tensors).  The kernel's outputs for it,
    as tests/mol_reference.py's `screen_graph` returns them, plus 'agree' (None without edge scores)."""
    thresholds = M.bond_thresholds(margins)
    n = node_scores.shape[0]
    h = n * (n - 1) // 2
    at = node_scores.argmax(-1).numpy() if n else np.zeros(0, dtype=np.int64)
    order = distance_orders(at, pos.numpy(), thresholds)
    out = R.screen_graph(node_scores, pos, onehot_edges(order), make_edge_data(torch.tensor([n]))[0])
    assert np.array_equal(out['order'], order) and not out['status'] & M.STATUS_HAD_ABSORBING_BOND
    if np.isin(at, UNMAPPED_CLASSES).any():
        out['status'] |= M.STATUS_DIST_UNMAPPED_ELEMENT
    out['agree'] = None
    if edge_scores is not None:
        a, b = np.triu_indices(n, 1)
        ok = usable(at, pos.numpy())
        pred = edge_scores[:h].argmax(-1).numpy() if h else np.zeros(0, dtype=np.int64)
        out['agree'] = agreement(pred, order, ok[a] & ok[b])
    return out


def screen_batch(node_scores, pos, edge_scores, num_atoms, margins=None):
    """A batch in the sampler's layout (CPU tensors, one frame; edge_scores may be None): list of `screen_graph` results."""
    out, n0, e0 = [], 0, 0
    for n in [int(v) for v in num_atoms]:
        e = n * (n - 1)
        out.append(screen_graph(node_scores[n0:n0 + n], pos[n0:n0 + n], None if edge_scores is None else edge_scores[e0:e0 + e], margins))
        n0, e0 = n0 + n, e0 + e
    return out


def census(refs):
    """How many graphs of a restated batch are valid / carry each status bit of the distance screen."""
    c = {'valid': sum(r['valid'] for r in refs)}
    for bit, name in M.DISTANCE_STATUS_NAMES.items():
        c[name] = sum(bool(r['status'] & bit) for r in refs)
    return c


# ---- building inputs ----------------------------------------------------------------------------------------------------------
def clear_of_thresholds(cls_placed, k, placed, c, thresholds):
    """100 * distance from the fp32 point c of class k to every placed atom keeps MARGIN_PM, with a reserve, from every threshold."""
    if len(placed) == 0:
        return True
    d100 = 100.0 * np.sqrt(((placed.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1))
    t = thresholds[np.asarray(cls_placed), k].astype(np.float64)
    return np.where(t > 0, np.abs(d100[:, None] - t), np.inf).min() >= 10 * MARGIN_PM


def place_atoms(cls, propose, thresholds, accept, tries=400):
    """fp32 [n, 3]: atom i is propose(i, placed [i, 3]), redrawn until it is clear of the thresholds and accept(i, candidate, placed)
    holds; after `tries` draws only the thresholds count."""
    n = len(cls)
    pos = np.zeros((n, 3), dtype=np.float32)
    for i in range(n):
        for k in range(100000):
            c = np.asarray(propose(i, pos[:i]), dtype=np.float64).astype(np.float32)
            if clear_of_thresholds(cls[:i], cls[i], pos[:i], c, thresholds) and (i == 0 or k >= tries or accept(i, c, pos[:i])):
                break
        pos[i] = c
    return pos


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


GEN_SEED = 20240913
GEN_SIZES = [1, 2, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS]
GEN_GRAPHS = 96
# classes of C, N, O, F and their largest degree in a grown tree of single bonds
TREE_CLASSES, TREE_P, TREE_DEGREE = [1, 2, 3, 4], [0.7, 0.12, 0.12, 0.06], {1: 4, 2: 3, 3: 2, 4: 1}


def tree_graph(rng, n, thresholds, lo=3.0, hi=12.0, clear=1.95):
    """A grown tree: every atom `lo .. hi` pm inside the single-bond threshold of its pair with a parent that has a free valence (for
    C, N, O, F that is above every double-bond threshold), at least `clear` Angstrom from every other atom (their largest single-bond
    threshold is 1.64), so that the bonds are exactly the tree's and all single."""
    cls = rng.choice(TREE_CLASSES, size=n, p=TREE_P)
    cls[0] = 1
    deg = np.zeros(n, dtype=np.int64)
    parent = [0]

    def propose(i, placed):
        if i == 0:
            return np.zeros(3)
        free = [j for j in range(i) if deg[j] < TREE_DEGREE[int(cls[j])]]
        if sum(TREE_DEGREE[int(cls[j])] - deg[j] for j in free) + TREE_DEGREE[int(cls[i])] - 2 <= 0:
            cls[i] = 1                                     # (it would use the last free valence: a carbon, which brings three)
        parent[0] = j = int(rng.choice([j for j in free if j >= i - 3] or free))
        return placed[j].astype(np.float64) + (thresholds[cls[j], cls[i], 0] - rng.uniform(lo, hi)) / 100.0 * unit(rng)

    def accept(i, c, placed):
        d = np.sqrt(((placed.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1))
        d[parent[0]] = np.inf
        if d.min() <= clear:
            return False
        deg[parent[0]] += 1                                # (accepted: the degrees follow the placement)
        deg[i] += 1
        return True

    return cls, place_atoms(cls, propose, thresholds, accept, tries=10 ** 9)


def generate_batch(seed=GEN_SEED, n_graphs=GEN_GRAPHS, margins=None):
    """Ragged batch for the distance screen: grown trees of C / N / O / F with single-bond lengths (valid), the same with a part moved
    far away (disconnected), dense clouds of all eleven elements with contacts from 1.0 Angstrom (over-valent, double and triple
    orders, B and Si), loose clouds; a few atoms of class 11, two graphs all-masked, one graph with a NaN coordinate.  Edge scores:
    logits whose first-half argmax is the distance order on most pairs and another class (4 and 5 included) on the rest; the reversed
    half holds other values.  Returns (node [N, 12], pos [N, 3], edge [E, 6], num_atoms list) as CPU tensors."""
    rng = np.random.default_rng(seed)
    thresholds = M.bond_thresholds(margins)
    sizes = list(GEN_SIZES) + [int(v) for v in rng.integers(3, 36, n_graphs - len(GEN_SIZES))]
    nodes, poss, edges = [], [], []
    for g, n in enumerate(sizes):
        kind = (0, 0, 1, 2, 3)[g % 5] if g >= len(GEN_SIZES) else (0 if n in (16, 63, 65, M.MAX_ATOMS) else 2 if n in (17, 78) else 1)
        if kind in (0, 1):
            cls, pos = tree_graph(rng, n, thresholds)
            if kind == 1 and n > 1:
                pos[n // 2:] += np.float32(40.0)           # the later half far away: no bond crosses (margins hold: far above any threshold)
        else:
            spread = (0.55 if kind == 2 else 2.2) * max(n, 2) ** (1.0 / 3.0)
            cls = rng.choice(11, size=n, p=np.array([3, 50, 12, 12, 4, 3, 3, 5, 3, 3, 2]) / 100.0)
            pos = place_atoms(list(cls), lambda i, pl: rng.normal(0, spread, 3), thresholds,
                              lambda i, c, pl: np.sqrt(((pl.astype(np.float64) - c) ** 2).sum(1)).min() > 1.0)
        assert min_margin_pm(cls, pos, thresholds) >= MARGIN_PM
        ac = np.array(cls, dtype=np.int64)
        if g % 9 == 4 and n > 2:
            ac[rng.integers(0, n, max(1, n // 10))] = 11
        if g in (20, 21):
            ac[:] = 11
        if g == 30:
            pos[n // 2, 1] = np.nan
        h = n * (n - 1) // 2
        et = distance_orders(ac, pos, thresholds).astype(np.int64)
        flip = rng.random(h) < np.where(et > 0, 0.3, 0.01)
        et[flip] = rng.integers(0, 6, int(flip.sum()))
        node = rng.normal(0, 1, (n, 12)).astype(np.float32)
        node[np.arange(n), ac] += 8.0
        edge = rng.normal(0, 1, (2 * h, 6)).astype(np.float32)
        edge[np.arange(2 * h), np.concatenate([et, rng.integers(0, 6, h)])] += 8.0
        nodes.append(node), poss.append(pos), edges.append(edge)
    return (torch.from_numpy(np.concatenate(nodes)), torch.from_numpy(np.concatenate(poss)),
            torch.from_numpy(np.concatenate(edges)), sizes)
