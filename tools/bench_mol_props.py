#!/usr/bin/env python3
"""Timing of the property kernel (csrc/mol_props.hip, phoregen_amd/properties.py) next to the scaffold kernel on the same batch and in
the same run, for scale; writes the table of profiles/mol_props_timing.md.

  python tools/bench_mol_props.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) molecule-like graphs: 128
chains of PG_MOL_MAX_ATOMS atoms with a hetero atom in every fourth place, all of which have a Kekulé structure, so every atom is
typed against every row it has to pass.  The property kernel does no search: two walks over the pair rows, two passes over each
atom's neighbours and one over the tables' rows.  A graph without a Kekulé structure leaves after staging its inputs, so the share
of such graphs is printed with each case.  Kernel times are HIP events around the launch alone (outputs allocated before), warm,
median of repeats, as tools/mol_bench.py takes them; wall times are a host clock around a call that ends in a device synchronise.
A record, not a pass/fail."""
import torch

from mol_bench import chain_result, fmt, headline_run, parser, relaunch_ms, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_scaffold import scaffold_kernel_ms
from phoregen_amd import hip, molecule as M, properties as P, scaffold as SC

OUTPUTS = ('status', 'counts', 'atom_env', 'atom_row', 'sums', 'weight_milli', 'violated')


def props_kernel_ms(pr, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_props launches over all frames of a Properties' inputs, after `warmup`."""
    sc = pr.screen
    F, B = sc.status.shape
    packed = torch.from_numpy(P.pack_tables(pr.tables)).to(sc.cls.device)
    weights = torch.tensor(P.weight_table(), dtype=torch.int32, device=sc.cls.device)
    rows, pairs = [len(t.rows) for t in pr.tables], pr.limits.pairs(pr.tables)
    lib = hip.lib()
    return relaunch_ms(pr, OUTPUTS, lambda out: P._launch_props(lib, sc, pr.kekule, pr.rings, B, F, max(sc.num_atoms), packed, rows, weights, pairs,
                                                                pr.limits.max_violations, out), repeats, warmup)


def main(argv=None):
    args = parser().parse_args(argv)
    dev = 'cuda'
    _, _, res, _, step_ms = headline_run(args.graphs, args.steps)
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
    return report(lines, {'props_ms_final': kp[0], 'scaffold_ms_final': ks[0], 'props_ms_traj': kpt[0], 'scaffold_ms_traj': kst[0], 'frames': F,
                          'props_ms_chains': kpc[0], 'scaffold_ms_chains': ksc[0], 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
