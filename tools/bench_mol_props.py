#!/usr/bin/env python3
"""Timing of the property kernel (csrc/mol_props.hip, phoregen_amd/properties.py) next to the scaffold kernel on the same batch and in
the same run, for scale; writes the table of profiles/mol_props_timing.md.

  python tools/bench_mol_props.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) molecule-like graphs: 128
chains of PG_MOL_MAX_ATOMS atoms with a hetero atom in every fourth place, all of which have a Kekulé structure, so every atom is
typed against every row it has to pass.  The property kernel does no search: two walks over the pair rows, two passes over each
atom's neighbours and one over the tables' rows.  A graph without a Kekulé structure leaves after staging its inputs, so the share
of such graphs is printed with each case.  Kernel times are HIP events around the launch alone (outputs allocated before), warm,
median of repeats, exactly as tools/bench_mol_scaffold.py takes them; wall times are a host clock around a call that ends in a device
synchronise.  A record, not a pass/fail."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench import ligphore_workload  # noqa: E402
from bench_mol_scaffold import scaffold_kernel_ms  # noqa: E402
from bench_mol_screen import wall_ms  # noqa: E402
from phoregen_amd import hip, molecule as M, properties as P, scaffold as SC  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402

OUTPUTS = ('status', 'counts', 'atom_env', 'atom_row', 'sums', 'weight_milli', 'violated')


def props_kernel_ms(pr, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_props launches over all frames of a Properties' inputs, after `warmup`."""
    sc = pr.screen
    F, B = sc.status.shape
    out = {k: torch.empty_like(getattr(pr, k)) for k in OUTPUTS}
    packed = torch.from_numpy(P.pack_tables(pr.tables)).to(sc.cls.device)
    weights = torch.tensor(P.weight_table(), dtype=torch.int32, device=sc.cls.device)
    rows, pairs = [len(t.rows) for t in pr.tables], pr.limits.pairs(pr.tables)
    lib = hip.lib()

    def go():
        P._launch_props(lib, sc, pr.kekule, pr.rings, B, F, max(sc.num_atoms), packed, rows, weights, pairs, pr.limits.max_violations, out)
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
    assert all(torch.equal(out[k], getattr(pr, k)) for k in OUTPUTS)
    return statistics.median(ts), min(ts), max(ts)


def chain_result(n_graphs, n, dev):
    """A sampler-shaped result of n_graphs chains of n atoms, single bonds, N or O in every fourth place: one-hot scores."""
    from phoregen_amd.plan import make_edge_data
    na = torch.full((n_graphs,), n, dtype=torch.long)
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
    ei, eb = make_edge_data(na)
    return {'pred': [node.repeat(n_graphs, 1).to(dev), torch.randn(n_graphs * n, 3).to(dev), edge.repeat(n_graphs, 1).to(dev)],
            'traj': [None, None, None],
            'lig_info': [na.to(dev), torch.repeat_interleave(torch.arange(n_graphs), na).to(dev), ei.to(dev), eb.to(dev)]}


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
    step_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    limits = P.PropertyLimits.lipinski()
    no_kekule = lambda pr: float((pr.status & P.PROP_NO_KEKULE != 0).float().mean())   # noqa: E731

    sc = M.screen(res)
    kek, rg = M.kekulize(res, screen=sc), M.rings(res, screen=sc)
    pr = P.properties(res, screen=sc, kekule=kek, rings=rg, limits=limits)
    kp = props_kernel_ms(pr, 50)
    ks = scaffold_kernel_ms(SC.scaffolds(sc), 50)
    w_pr = wall_ms(lambda: P.properties(res, screen=sc, kekule=kek, rings=rg, limits=limits), 10)
    w_all = wall_ms(lambda: P.properties(res, limits=limits), 10)
    share = no_kekule(pr)

    sct = M.screen(res, frames='traj')
    F = sct.status.size(0)
    kekt, rgt = M.kekulize(res, frames='traj', screen=sct), M.rings(res, frames='traj', screen=sct)
    prt = P.properties(res, frames='traj', screen=sct, kekule=kekt, rings=rgt, limits=limits)
    kpt = props_kernel_ms(prt, 7, warmup=2)
    kst = scaffold_kernel_ms(SC.scaffolds(sct), 7, warmup=2)
    w_pr_t = wall_ms(lambda: P.properties(res, frames='traj', screen=sct, kekule=kekt, rings=rgt, limits=limits), 5)
    share_t = no_kekule(prt)
    del prt, kekt, rgt, sct, res

    chains = chain_result(args.graphs, M.MAX_ATOMS, dev)
    scc = M.screen(chains)
    prc = P.properties(chains, screen=scc, limits=limits)
    kpc = props_kernel_ms(prc, 20)
    ksc = scaffold_kernel_ms(SC.scaffolds(scc), 20)
    share_c = no_kekule(prc)

    fmt = lambda t: '%.3f (%.3f - %.3f)' % t[:3]   # noqa: E731
    row = '| %s | %s | %s | %.2f x | %.2f | %s |'
    lines = ['| case | `pg_mol_props` kernel ms, median (min - max) | `pg_mol_scaffold` kernel ms | props / scaffold | share of graphs without a Kekulé structure | `properties()` wall ms (screen, Kekulé form and rings handed in) |',
             '|---|---|---|---|---|---|',
             row % ('(a) final frame, %d graphs' % args.graphs, fmt(kp), fmt(ks), kp[0] / ks[0], share, fmt(w_pr)),
             row % ('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), fmt(kpt), fmt(kst), kpt[0] / kst[0], share_t, fmt(w_pr_t)),
             row % ('(c) %d chains of %d atoms, N or O in every fourth place' % (args.graphs, M.MAX_ATOMS), fmt(kpc), fmt(ksc), kpc[0] / ksc[0], share_c, '-'),
             '',
             '(a) `properties(results)` with the screen, the Kekulé form and the rings computed too: %s ms wall.' % fmt(w_all),
             '',
             'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept, host clock around the call).  The '
             'properties of the final frame cost %.4f of one step, those of all %d frames %.3f steps.' % (step_ms, args.steps, kp[0] / step_ms, F, kpt[0] / step_ms),
             '',
             'Tables: %s (%s rows), limits: Lipinski.  Final frame: %d of %d graphs pass; (c): %d of %d pass, %d untyped atoms.'
             % (', '.join(t.name for t in pr.tables), ' + '.join(str(len(t.rows)) for t in pr.tables), int(pr.ok.sum()), args.graphs,
                int(prc.ok.sum()), args.graphs, int(prc.counts[..., hip.PG_PROP_C_UNTYPED].sum()))]
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps({'props_ms_final': kp[0], 'scaffold_ms_final': ks[0], 'props_ms_traj': kpt[0], 'scaffold_ms_traj': kst[0], 'frames': F,
                      'props_ms_chains': kpc[0], 'scaffold_ms_chains': ksc[0], 'step_ms': step_ms}))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
