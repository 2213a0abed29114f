"""What the molecule timing tools share (tools/bench_mol_*.py, bench_fingerprints.py, bench_shape.py, bench_shape_align.py): the one
event-timing loop and the one wall-clock loop, the relaunch of a holder's kernel into fresh outputs, the headline sampling run, the
synthetic inputs, and the argument parser and report tail.  A module of plain functions, imported by those tools and their tests
only; importing it puts the repository root on sys.path, so a tool imports it first and the package after it.

Kernel times are HIP events around the launch alone (outputs allocated before), warm, median of repeats with the smallest and the
largest; wall times are a host clock around a call that ends in a device synchronise."""
import argparse
import functools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ligphore_workload  # noqa: E402
from phoregen_amd import molecule as M, shape  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.plan import make_edge_data  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


# ---- timing ---------------------------------------------------------------------------------------------------------------------------

def event_ms(go, repeats, warmup):
    """(median, min, max) of `repeats` event-timed calls of `go` after `warmup` calls.  Nothing but `go` runs between the two events:
    a final-frame kernel takes 30 to 80 us, so host work inside the bracket would show in the number."""
    for _ in range(warmup):
        go()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def same(a, b):
    """torch.equal, with fp32 compared by its bits (an output may hold NaN where nothing was measured)."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def relaunch_ms(holder, names, launch, repeats, warmup):
    """Event-times `launch(out)`, out = fresh arrays shaped like the holder's `names`, and asserts that they come out equal to the
    holder's: a tool's spelling of a `_launch_X` call is checked against the public function that made the holder."""
    out = {k: torch.empty_like(getattr(holder, k)) for k in names}
    t = event_ms(functools.partial(launch, out), repeats, warmup)
    assert all(same(out[k], getattr(holder, k)) for k in names)
    return t


def headline_run(graphs, steps, warm=True, traj=True):
    """The bench's batch sampled with deterministic weights: (model, workload, result, seconds of the sampling call, ms per step).
    warm: five steps first (code objects, plan, packed weights), so that the timed call is a warm one."""
    model = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to('cuda')
    w = ligphore_workload(graphs)
    sample = lambda n, keep: model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], w['num_atoms'],   # noqa: E731
                                                torch.zeros(graphs, 3), rng='device', seed=1, num_steps=n, return_traj=keep)
    if warm:
        sample(5, False)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sample(steps, traj)
    torch.cuda.synchronize()
    t_sample = time.perf_counter() - t0
    return model, w, res, t_sample, t_sample * 1e3 / steps


# ---- arguments and report --------------------------------------------------------------------------------------------------------------

def parser(steps_default=1000, steps_help='reverse steps of the sampled trajectory (frames = steps + 1)'):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=steps_default, help=steps_help)
    ap.add_argument('--graphs', type=int, default=128)
    ap.add_argument('--out', type=str, default=None)
    return ap


def fmt(t):
    return '%.3f (%.3f - %.3f)' % tuple(t[:3])


def report(lines, record, out):
    """Prints the table and the JSON line, writes the table to `out` if given; (text, record)."""
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps(record))
    if out:
        with open(out, 'w') as fh:
            fh.write(text)
    return text, record


# ---- synthetic inputs, in the sampler's layout -----------------------------------------------------------------------------------------

def _result(node, pos, edge, na, dev):
    ei, eb = make_edge_data(na)
    return {'pred': [node.to(dev), pos.to(dev), edge.to(dev)], 'traj': [None, None, None],
            'lig_info': [na.to(dev), torch.repeat_interleave(torch.arange(len(na)), na).to(dev), ei.to(dev), eb.to(dev)]}


def dense_result(graphs, n, dev, seed=0):
    """`graphs` graphs of n atoms with random logits, in the sampler's layout."""
    gen = torch.Generator().manual_seed(seed)
    node, pos = torch.randn(graphs * n, 12, generator=gen), torch.randn(graphs * n, 3, generator=gen)
    node[:, 11] -= 4.0
    edge = torch.randn(graphs * n * (n - 1), 6, generator=gen)
    return _result(node, pos, edge, torch.full((graphs,), n, dtype=torch.long), dev)


def onehot_result(graphs, dev):
    """[(atom classes, {(a, b): bond class})] as one-hot scores in the sampler's layout."""
    nodes, edges, sizes = [], [], []
    for classes, bonds in graphs:
        n = len(classes)
        h = n * (n - 1) // 2
        node = torch.zeros(n, 12)
        node[torch.arange(n), torch.tensor(classes)] = 1.0
        et = torch.zeros(2 * h, dtype=torch.long)
        for (a, b), t in bonds.items():
            r = a * n - a * (a + 1) // 2 + (b - a - 1)
            et[r] = et[h + r] = t
        edge = torch.zeros(2 * h, 6)
        edge[torch.arange(2 * h), et] = 1.0
        nodes.append(node), edges.append(edge), sizes.append(n)
    return _result(torch.cat(nodes), torch.zeros(sum(sizes), 3), torch.cat(edges), torch.tensor(sizes, dtype=torch.long), dev)


def sparse_aromatic_graphs(graphs, n=64, seed=0):
    """Three naphthalene-like ring pairs of C / N per graph, joined to a chain of single bonds that holds the other atoms; the atoms
    are numbered at random."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(graphs):
        p = rng.permutation(n)
        classes, bonds = [1] * n, {}

        def bond(a, b, t):
            bonds[(int(min(p[a], p[b])), int(max(p[a], p[b])))] = t
        for k in range(3):
            o = 10 * k
            for a, b in [(i, (i + 1) % 6) for i in range(6)] + [(0, 6), (6, 7), (7, 8), (8, 9), (1, 9)]:
                bond(o + a, o + b, 4)
            for a in (2, 3, 4, 5, 6, 7, 8, 9):
                if rng.random() < 0.2:
                    classes[p[o + a]] = 2
            bond(o + 3, 30 + k, 1)
        for a in range(30, n - 1):
            bond(a, a + 1, 1)
        out.append((classes, bonds))
    return out


def ladder_graphs(graphs, n):
    r = n // 2
    bonds = {(i, i + 1): 4 for i in range(r - 1)}
    bonds.update({(r + i, r + i + 1): 4 for i in range(r - 1)})
    bonds.update({(i, r + i): 4 for i in range(0, r, 2)})
    return [([1] * n, bonds)] * graphs


def label_chain_graphs(graphs, n, closures=M.SMILES_MAX_LABEL):
    """A chain of n carbons with atom 0 also bonded to atoms 2 .. 2 + closures - 1."""
    bonds = {(i, i + 1): 1 for i in range(n - 1)}
    bonds.update({(0, i): 1 for i in range(2, 2 + closures)})
    return [([1] * n, bonds)] * graphs


def chain_result(n_graphs, n, dev):
    """A sampler-shaped result of n_graphs chains of n atoms, single bonds, N or O in every fourth place: one-hot scores."""
    h = n * (n - 1) // 2
    cls = torch.ones(n, dtype=torch.long)
    cls[3::8], cls[7::8] = 2, 3
    node = torch.zeros(n, 12)
    node[torch.arange(n), cls] = 1.0
    half = torch.zeros(h, dtype=torch.long)
    a = torch.arange(n - 1)
    half[a * n - a * (a + 1) // 2] = 1                                 # the pair (a, a + 1) is the first of row a
    edge = torch.zeros(2 * h, 6)
    edge[torch.arange(2 * h), torch.cat([half, half])] = 1.0
    return _result(node.repeat(n_graphs, 1), torch.randn(n_graphs * n, 3), edge.repeat(n_graphs, 1),
                   torch.full((n_graphs,), n, dtype=torch.long), dev)


def molecule_like(num_atoms, dev, seed=1):
    """A sampler-shaped result with one-hot scores: per graph a random tree of degree <= 4 plus up to three ring closures."""
    rng = np.random.default_rng(seed)
    nodes, edges = [], []
    for n in num_atoms:
        h = n * (n - 1) // 2
        cls = rng.choice([1, 1, 1, 1, 1, 2, 2, 3, 3, 7, 8], n)
        et, degree = np.zeros(h, dtype=np.int64), [0] * n
        row = lambda a, b: a * n - a * (a + 1) // 2 + (b - a - 1)   # noqa: E731
        for v in range(1, n):
            u = int(rng.integers(max(0, v - 6), v))
            while degree[u] >= 4:
                u = int(rng.integers(0, v))
            et[row(u, v)] = int(rng.choice([1, 1, 1, 1, 2, 4]))
            degree[u] += 1
            degree[v] += 1
        for _ in range(3):
            a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False)) if n > 1 else (0, 0)
            if a != b and et[row(a, b)] == 0 and degree[a] < 4 and degree[b] < 4:
                et[row(a, b)] = 1
                degree[a] += 1
                degree[b] += 1
        node = torch.zeros(n, 12)
        node[torch.arange(n), torch.from_numpy(cls)] = 1.0
        edge = torch.zeros(2 * h, 6)
        edge[torch.arange(2 * h), torch.from_numpy(np.concatenate([et, et]))] = 1.0
        nodes.append(node)
        edges.append(edge)
    na = torch.tensor(num_atoms, dtype=torch.long)
    pos = torch.from_numpy(rng.normal(0, 3, (int(na.sum()), 3)).astype(np.float32))
    return _result(torch.cat(nodes), pos, torch.cat(edges), na, dev)


def synthetic_set(n, seed, colour, device):
    """n molecules for phoregen_amd.shape: the bench workload's atom counts, random walks with 1.3 .. 1.6 Angstrom steps around a
    centre within 1 Angstrom of the origin, carbon-heavy mixed elements, with `colour` random feature bytes; (set, atom counts)."""
    g = torch.Generator().manual_seed(seed)
    n_at = (40 + 6 * torch.randn(n, generator=g)).round().clamp(20, 60).long().tolist()
    rng = np.random.default_rng(seed)
    p = np.array([1, 30, 8, 8, 2, 1, 1, 2, 2, 1, 1]) / 57.0
    mols = []
    for k in n_at:
        step = rng.normal(size=(k, 3))
        step *= rng.uniform(1.3, 1.6, size=(k, 1)) / np.linalg.norm(step, axis=1, keepdims=True)
        pos = np.cumsum(step, axis=0)
        m = {'element': [shape.ATOM_TYPES[c] for c in rng.choice(11, size=k, p=p)],
             'atom_pos': (pos - pos.mean(axis=0) + rng.normal(0, 1.0, size=3)).astype(np.float32)}
        if colour:
            m['features'] = {'atom_fp': rng.integers(0, 128, size=k).astype(np.uint8)}
        mols.append(m)
    return shape.from_molecules(mols, device), n_at
