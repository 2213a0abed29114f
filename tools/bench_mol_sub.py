#!/usr/bin/env python3
"""Timing of the substructure search (csrc/mol_sub.hip, phoregen_amd/substructure.py) on the headline batch; writes the table of
profiles/mol_sub_timing.md.

  python tools/bench_mol_sub.py [--steps 1000] [--out FILE.md]

Two batches of the headline shape (128 graphs, the workload's atom counts) against tables of P = 1, 16 and 256 patterns -- (a) the
final prediction of the sampler with the deterministic noise weights, whose graphs are close to cliques, so that every root runs
into the work bound: the worst case; (b) molecule-like graphs made up here (a random tree of degree at most 4 with a few ring
closures per graph, mostly carbon, mostly single bonds), where nothing is cut short.  The tables: the 6-cycle of any atoms alone;
the paths of 2 .. 16 any-atoms and the 6-cycle; those sixteen repeated sixteen times under other names.  Kernel times are HIP events
around the launch alone (table and outputs on the device before), warm, median of repeats; next to them the wall time of
`substructure()` with the screen, the rings and the Kekulé form handed in.  There is no target: the numbers are recorded, not gated."""
import argparse
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
from phoregen_amd import hip, molecule as M, substructure as S  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


def pattern_lists():
    cycle = {'name': 'cycle6', 'atoms': [{}] * 6, 'bonds': [{'a': min(i, (i + 1) % 6), 'b': max(i, (i + 1) % 6)} for i in range(6)]}
    sixteen = [{'name': 'path%d' % n, 'atoms': [{}] * n, 'bonds': [{'a': i, 'b': i + 1} for i in range(n - 1)]} for n in range(2, 17)] + [cycle]
    many = [dict(p, name='%s_%d' % (p['name'], r)) for r in range(16) for p in sixteen]
    return {1: [cycle], 16: sixteen, 256: many}


def molecule_like(num_atoms, dev, seed=1):
    """A sampler-shaped result with one-hot scores: per graph a random tree of degree <= 4 plus up to three ring closures."""
    from phoregen_amd.plan import make_edge_data
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
    ei, eb = make_edge_data(na)
    pos = torch.from_numpy(rng.normal(0, 3, (int(na.sum()), 3)).astype(np.float32))
    return {'pred': [torch.cat(nodes).to(dev), pos.to(dev), torch.cat(edges).to(dev)], 'traj': [None, None, None],
            'lig_info': [na.to(dev), torch.repeat_interleave(torch.arange(len(num_atoms)), na).to(dev), ei.to(dev), eb.to(dev)]}


def kernel_ms(sc, rg, kek, patterns, max_steps, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed launches, after `warmup` launches; and the outputs."""
    dev = sc.cls.device
    F, B = sc.status.shape
    P = len(patterns)
    host = S.pattern_table(patterns)
    table = torch.from_numpy(host).to(dev)
    out = dict(embeddings=torch.empty(F, B, P, dtype=torch.int32, device=dev), anchors=torch.empty(F, B, P, dtype=torch.int32, device=dev),
               atom_mask=torch.empty(F, B, P, 2, dtype=torch.int64, device=dev), first=torch.empty(F, B, P, S.MAX_ATOMS, dtype=torch.int16, device=dev),
               status=torch.empty(F, B, P, dtype=torch.int32, device=dev))
    lib = hip.lib()

    def go():
        S._launch_sub(lib, sc, rg, kek, B, F, max(sc.num_atoms), table, host, P, max_steps, out)
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
    return (statistics.median(ts), min(ts), max(ts)), out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1000, help='reverse steps of the sampler')
    ap.add_argument('--graphs', type=int, default=128)
    ap.add_argument('--max_steps', type=int, default=S.DEFAULT_STEPS)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    dev = 'cuda'
    model = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to(dev)
    w = ligphore_workload(args.graphs)
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], w['num_atoms'], torch.zeros(args.graphs, 3),
                             rng='device', seed=1, num_steps=args.steps)
    torch.cuda.synchronize()
    lines, record = [], {}
    for tag, title, batch in (('a', '(a) the sampler\'s final prediction, noise weights', res),
                              ('b', '(b) molecule-like graphs', molecule_like([int(n) for n in w['num_atoms'].tolist()], dev))):
        sc = M.screen(batch)
        rg, kek = M.rings(batch, screen=sc), M.kekulize(batch, screen=sc)
        lines += ['## ' + title, '',
                  '| patterns | kernel ms, median (min - max) | us per (graph, pattern) | `substructure()` wall ms | rows matched | rows truncated |',
                  '|---|---|---|---|---|---|']
        for P, dicts in pattern_lists().items():
            patterns = [S.Pattern.from_dict(d) for d in dicts]
            k3, out = kernel_ms(sc, rg, kek, patterns, args.max_steps, args.repeats)
            wall = wall_ms(lambda: S.substructure(batch, patterns, screen=sc, rings=rg, kekule=kek, max_steps=args.max_steps), 10)
            matched = int(((out['status'] & S.SUB_MATCHED) != 0).sum())
            truncated = int(((out['status'] & S.SUB_TRUNCATED) != 0).sum())
            lines.append('| %d | %.3f (%.3f - %.3f) | %.3f | %.3f (%.3f - %.3f) | %d of %d | %d |' %
                         ((P,) + k3 + (k3[0] * 1e3 / (args.graphs * P),) + wall + (matched, args.graphs * P, truncated)))
            record['kernel_ms_%s_P%d' % (tag, P)] = k3[0]
        lines += ['', 'The batch: %d graphs, %d atom rows, %d kept atoms, %d bonds, %d valid graphs; max_steps %d.' %
                  (args.graphs, sc.cls.size(1), int(sc.counts[0, :, 0].sum()), int(sc.counts[0, :, 1].sum()), int(sc.valid.sum()), args.max_steps), '']
    lines += ['(a) was sampled with %d reverse steps.' % args.steps]
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps(record))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
