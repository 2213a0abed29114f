#!/usr/bin/env python3
"""Timing of the ring kernel (csrc/mol_rings.hip, phoregen_amd/molecule.py) next to the screen kernel on the same inputs and in the
same run; writes the table of profiles/mol_rings_timing.md.

  python tools/bench_mol_rings.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) the worst case: graphs of
PG_MOL_MAX_ATOMS atoms with random logits, which bond about two thirds of all pairs, so every lane searches about 85 rings.  Kernel
times are HIP events around the launch alone (outputs allocated before), warm, median of repeats, exactly as
tools/bench_mol_screen.py takes the screen's; wall times are a host clock around a call that ends in a device synchronise.  The
reverse step the two are held against is the sampling call of this run divided by its steps.  A record, not a pass/fail."""
import argparse
import json
import os
import statistics
import sys
import time
from dataclasses import astuple

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


def rings_kernel_ms(rg, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_rings launches over all frames of a Rings' screen, after `warmup`."""
    sc = rg.screen
    F, B = sc.status.shape
    out = {k: torch.empty_like(getattr(rg, k)) for k in ('status', 'counts', 'ring_size', 'atom_ring', 'ring_sys')}
    lib, lim = hip.lib(), astuple(rg.limits)

    def go():
        M._launch_rings(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), lim, out)
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
    assert all(torch.equal(out[k], getattr(rg, k)) for k in out)
    return statistics.median(ts), min(ts), max(ts)


def dense_result(graphs, n, dev, seed=0):
    """`graphs` graphs of n atoms with random logits, in the sampler's layout."""
    gen = torch.Generator().manual_seed(seed)
    node, pos = torch.randn(graphs * n, 12, generator=gen), torch.randn(graphs * n, 3, generator=gen)
    node[:, 11] -= 4.0
    edge = torch.randn(graphs * n * (n - 1), 6, generator=gen)
    na = torch.full((graphs,), n, dtype=torch.long)
    ei, eb = make_edge_data(na)
    return {'pred': [node.to(dev), pos.to(dev), edge.to(dev)], 'traj': [None, None, None],
            'lig_info': [na.to(dev), torch.repeat_interleave(torch.arange(graphs), na).to(dev), ei.to(dev), eb.to(dev)]}


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

    sc = M.screen(res)
    node, pos, edge = res['pred']
    ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50)
    rg = M.rings(res, screen=sc)
    kr = rings_kernel_ms(rg, 50)
    w_rg = wall_ms(lambda: M.rings(res, screen=sc), 10)
    w_asm, w_asm_r = wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: M.assemble(res, rings=M.rings(res)), 10)
    census = {name: int(((rg.status & bit) != 0).sum()) for bit, name in M.RING_NAMES.items()}
    totals = dict(zip(M.RING_COUNTS, rg.counts[0].sum(0).tolist()))

    tn, tp, te = res['traj']
    F = tn.size(0)
    kst = kernel_ms(tn, tp, te, F, (tn.stride(0), te.stride(0), tp.stride(0)), sc, 7, warmup=2)
    sct = M.screen(res, frames='traj')
    rgt = M.rings(res, frames='traj', screen=sct)
    krt = rings_kernel_ms(rgt, 7, warmup=2)
    w_rg_t = wall_ms(lambda: M.rings(res, frames='traj', screen=sct), 5)
    bonds, bonds_t = int(sc.counts[..., 1].sum()), int(sct.counts[..., 1].sum())
    del rgt, sct, res

    dense = dense_result(args.graphs, M.MAX_ATOMS, dev)
    scd = M.screen(dense)
    dn, dp, de = dense['pred']
    ksd = kernel_ms(dn, dp, de, 1, (0, 0, 0), scd, 20)
    rgd = M.rings(dense, screen=scd)
    krd = rings_kernel_ms(rgd, 20)
    bonds_d = int(scd.counts[..., 1].sum())

    fmt = lambda t: '%.3f (%.3f - %.3f)' % t[:3]   # noqa: E731
    row = '| %s | %s | %s | %.1f x | %.3g | %s |'
    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_rings` kernel ms | rings / screen | ring searches (bonds) per call | `rings()` wall ms |',
             '|---|---|---|---|---|---|',
             row % ('(a) final frame, %d graphs' % args.graphs, fmt(ks), fmt(kr), kr[0] / ks[0], bonds, fmt(w_rg)),
             row % ('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), fmt(kst), fmt(krt), krt[0] / kst[0], bonds_t, fmt(w_rg_t)),
             row % ('(c) worst case: %d graphs of %d atoms, random logits (dense)' % (args.graphs, M.MAX_ATOMS), fmt(ksd), fmt(krd), krd[0] / ksd[0], bonds_d, '-'),
             '',
             '`assemble()` %s ms wall, `assemble(rings=rings(..))` %s ms wall.' % (fmt(w_asm), fmt(w_asm_r)),
             '',
             'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
             'The rings of the final frame cost %.4f of one step, those of all %d frames %.3f steps.' % (step_ms, args.steps, t_sample, kr[0] / step_ms, F, krt[0] / step_ms),
             '',
             'Final frame, %d graphs (deterministic noise weights, so the molecules are noise): %d pass the screen, %d the default ring limits; '
             'graphs per bit: %s; totals: %s.' % (args.graphs, int(sc.valid.sum()), int(rg.ok.sum()), ', '.join('%s %d' % kv for kv in census.items()),
                                                  ', '.join('%s %d' % kv for kv in totals.items()))]
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps({'screen_ms_final': ks[0], 'rings_ms_final': kr[0], 'screen_ms_traj': kst[0], 'rings_ms_traj': krt[0], 'frames': F,
                      'screen_ms_dense': ksd[0], 'rings_ms_dense': krd[0], 'step_ms': step_ms}))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
