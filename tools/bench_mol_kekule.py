#!/usr/bin/env python3
"""Timing of the Kekulé kernel (csrc/mol_kekule.hip, phoregen_amd/molecule.py) next to the screen kernel on the same inputs and in
the same run; writes the table of profiles/mol_kekule_timing.md.

  python tools/bench_mol_kekule.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) a synthetic batch of sparse
aromatic graphs: 64 atoms each, three fused aromatic ring pairs of C / N joined by single bonds, the rest a chain, (d) the serial
worst case: a ladder of PG_MOL_MAX_ATOMS aromatic carbons per graph, 128 searches of growing trees on one lane.  Kernel times are HIP
events around the launch alone (outputs allocated before), warm, median of repeats, exactly as tools/bench_mol_screen.py takes the
screen's; wall times are a host clock around a call that ends in a device synchronise.  The reverse step the two are held against is
the sampling call of this run divided by its steps.  A record, not a pass/fail."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench import ligphore_workload  # noqa: E402
from bench_mol_screen import kernel_ms, wall_ms  # noqa: E402
from phoregen_amd import hip, molecule as M  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.plan import make_edge_data  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


def kekule_kernel_ms(kk, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_kekule launches over all frames of a Kekule's screen, after `warmup`."""
    sc = kk.screen
    F, B = sc.status.shape
    out = {k: torch.empty_like(getattr(kk, k)) for k in ('status', 'counts', 'kekule_order', 'hcount', 'charge')}
    lib, tables = hip.lib(), M._kekule_table(sc.cls.device)

    def go():
        M._launch_kekule(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), tables, kk.options.allow_charged, out)
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
    assert all(torch.equal(out[k], getattr(kk, k)) for k in out)
    return statistics.median(ts), min(ts), max(ts)


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
    na = torch.tensor(sizes, dtype=torch.long)
    ei, eb = make_edge_data(na)
    N = int(na.sum())
    return {'pred': [torch.cat(nodes).to(dev), torch.zeros(N, 3, device=dev), torch.cat(edges).to(dev)], 'traj': [None, None, None],
            'lig_info': [na.to(dev), torch.repeat_interleave(torch.arange(len(sizes)), na).to(dev), ei.to(dev), eb.to(dev)]}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1000, help='reverse steps of the sampled trajectory (frames = steps + 1)')
    ap.add_argument('--graphs', type=int, default=128)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    dev = 'cuda'
    model = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to(dev)
    w = ligphore_workload(args.graphs)
    sample = lambda steps, traj: model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], w['num_atoms'],   # noqa: E731
                                                    torch.zeros(args.graphs, 3), rng='device', seed=1, num_steps=steps, return_traj=traj)
    sample(5, False)                                                   # warm: code objects, plan, packed weights
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sample(args.steps, True)
    torch.cuda.synchronize()
    t_sample = time.perf_counter() - t0
    step_ms = t_sample * 1e3 / args.steps

    def census(kk):
        c = dict(zip(M.KEKULE_COUNTS, kk.counts.reshape(-1, len(M.KEKULE_COUNTS)).sum(0).tolist()))
        return 'ok %d of %d, aromatic atoms %d, doubled %d' % (int(kk.ok.sum()), kk.ok.numel(), c['aromatic_atoms'], c['doubled'])

    sc = M.screen(res)
    node, pos, edge = res['pred']
    ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50)
    kk = M.kekulize(res, screen=sc)
    kr = kekule_kernel_ms(kk, 50)
    w_kk = wall_ms(lambda: M.kekulize(res, screen=sc), 10)
    w_asm, w_asm_k = wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: M.assemble(res, kekule=M.kekulize(res)), 10)
    flags = {name: int(((kk.status & bit) != 0).sum()) for bit, name in M.KEKULE_NAMES.items()}
    totals = dict(zip(M.KEKULE_COUNTS, kk.counts[0].sum(0).tolist()))
    cen_a = census(kk)

    tn, tp, te = res['traj']
    F = tn.size(0)
    kst = kernel_ms(tn, tp, te, F, (tn.stride(0), te.stride(0), tp.stride(0)), sc, 7, warmup=2)
    sct = M.screen(res, frames='traj')
    kkt = M.kekulize(res, frames='traj', screen=sct)
    krt = kekule_kernel_ms(kkt, 7, warmup=2)
    w_kk_t = wall_ms(lambda: M.kekulize(res, frames='traj', screen=sct), 5)
    cen_b = census(kkt)
    del kkt, sct, res

    rows = []
    for label, graphs in (('(c) sparse aromatic: %d graphs of 64 atoms, 30 aromatic' % args.graphs, sparse_aromatic_graphs(args.graphs)),
                          ('(d) serial worst case: %d ladders of %d aromatic C' % (args.graphs, M.MAX_ATOMS), ladder_graphs(args.graphs, M.MAX_ATOMS))):
        syn = onehot_result(graphs, dev)
        scs = M.screen(syn)
        sn, sp, se = syn['pred']
        kss = kernel_ms(sn, sp, se, 1, (0, 0, 0), scs, 20)
        kks = M.kekulize(syn, screen=scs)
        rows.append((label, kss, kekule_kernel_ms(kks, 20), census(kks)))

    fmt = lambda t: '%.3f (%.3f - %.3f)' % t[:3]   # noqa: E731
    row = '| %s | %s | %s | %.1f x | %s | %s |'
    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_kekule` kernel ms | kekule / screen | census | `kekulize()` wall ms |',
             '|---|---|---|---|---|---|',
             row % ('(a) final frame, %d graphs' % args.graphs, fmt(ks), fmt(kr), kr[0] / ks[0], cen_a, fmt(w_kk)),
             row % ('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), fmt(kst), fmt(krt), krt[0] / kst[0], cen_b, fmt(w_kk_t))]
    lines += [row % (label, fmt(a), fmt(b), b[0] / a[0], c, '-') for label, a, b, c in rows]
    lines += ['',
              '`assemble()` %s ms wall, `assemble(kekule=kekulize(..))` %s ms wall.' % (fmt(w_asm), fmt(w_asm_k)),
              '',
              'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
              'The Kekulé form of the final frame costs %.4f of one step, that of all %d frames %.3f steps.' % (step_ms, args.steps, t_sample, kr[0] / step_ms, F, krt[0] / step_ms),
              '',
              'Final frame, %d graphs (deterministic noise weights, so the molecules are noise): %d pass the screen, %d have a Kekulé structure; '
              'graphs per bit: %s; totals: %s.' % (args.graphs, int(sc.valid.sum()), int(kk.ok.sum()), ', '.join('%s %d' % kv for kv in flags.items()),
                                                   ', '.join('%s %d' % kv for kv in totals.items()))]
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps({'screen_ms_final': ks[0], 'kekule_ms_final': kr[0], 'screen_ms_traj': kst[0], 'kekule_ms_traj': krt[0], 'frames': F,
                      'screen_ms_sparse': rows[0][1][0], 'kekule_ms_sparse': rows[0][2][0], 'screen_ms_ladder': rows[1][1][0],
                      'kekule_ms_ladder': rows[1][2][0], 'step_ms': step_ms}))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
