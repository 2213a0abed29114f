#!/usr/bin/env python3
"""Timing of the scaffold kernel (csrc/mol_scaffold.hip, phoregen_amd/scaffold.py) next to the ring kernel on the same inputs and in
the same run; writes the table of profiles/mol_scaffold_timing.md.

  python tools/bench_mol_scaffold.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) the worst case of the ring
search: graphs of PG_MOL_MAX_ATOMS atoms with random logits, which bond about two thirds of all pairs.  Both kernels run the same
per-bond ring search (csrc/ring_search.h); the scaffold kernel runs it on the bonds of the core only and adds the pruning rounds.
Kernel times are HIP events around the launch alone (outputs allocated before), warm, median of repeats, as tools/mol_bench.py
takes them; wall times are a host clock around a call that ends in a device synchronise.  A record, not a pass/fail."""
import torch

from mol_bench import dense_result, event_ms, fmt, headline_run, parser, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_rings import rings_kernel_ms
from phoregen_amd import hip, molecule as M, scaffold as SC

SCREEN_ARRAYS = ('status', 'counts', 'cls', 'compact', 'valence2', 'comp', 'order')


def scaffold_kernel_ms(sf, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_scaffold launches over all frames of a Scaffolds' source, after `warmup`."""
    sc = sf.source
    F, B = sc.status.shape
    part, counts = torch.empty_like(sf.part), torch.empty_like(sf.counts)
    out = {k: torch.empty_like(getattr(sf.screen, k)) for k in SCREEN_ARRAYS}
    lib = hip.lib()
    t = event_ms(lambda: SC._launch_scaffold(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), sf.options.flags, part, counts,
                                             out), repeats, warmup)
    assert torch.equal(part, sf.part) and torch.equal(counts, sf.counts) and all(torch.equal(out[k], getattr(sf.screen, k)) for k in out)
    return t


def main(argv=None):
    args = parser().parse_args(argv)
    dev = 'cuda'
    _, _, res, _, step_ms = headline_run(args.graphs, args.steps)

    sc = M.screen(res)
    kr = rings_kernel_ms(M.rings(res, screen=sc), 50)
    sf = SC.scaffolds(sc)
    kf = scaffold_kernel_ms(sf, 50)
    kg = scaffold_kernel_ms(SC.scaffolds(sc, SC.ScaffoldOptions(generic=True)), 50)
    w_sf = wall_ms(lambda: SC.scaffolds(sc), 10)
    w_keys = wall_ms(lambda: SC.scaffold_keys(SC.scaffolds(sc)), 10)
    totals = dict(zip(SC.SCAFFOLD_COUNTS, sf.counts[0].sum(0).tolist()))
    distinct = len(set(SC.scaffold_keys(sf).key[0].tolist()))
    core_bonds = int(sf.counts[0, :, 1].sum() - sf.counts[0, :, 4].sum())

    sct = M.screen(res, frames='traj')
    F = sct.status.size(0)
    krt = rings_kernel_ms(M.rings(res, frames='traj', screen=sct), 7, warmup=2)
    sft = SC.scaffolds(sct)
    kft = scaffold_kernel_ms(sft, 7, warmup=2)
    w_sf_t = wall_ms(lambda: SC.scaffolds(sct), 5)
    core_bonds_t = int(sft.counts[..., 1].sum() - sft.counts[..., 4].sum())
    del sft, sct, res

    dense = dense_result(args.graphs, M.MAX_ATOMS, dev)
    scd = M.screen(dense)
    krd = rings_kernel_ms(M.rings(dense, screen=scd), 20)
    sfd = SC.scaffolds(scd)
    kfd = scaffold_kernel_ms(sfd, 20)
    core_bonds_d = int(sfd.counts[..., 1].sum() - sfd.counts[..., 4].sum())

    row = '| %s | %s | %s | %.2f x | %.3g | %s |'
    lines = ['| case | `pg_mol_rings` kernel ms, median (min - max) | `pg_mol_scaffold` kernel ms | scaffold / rings | ring searches (core bonds) per call | `scaffolds()` wall ms |',
             '|---|---|---|---|---|---|',
             row % ('(a) final frame, %d graphs' % args.graphs, fmt(kr), fmt(kf), kf[0] / kr[0], core_bonds, fmt(w_sf)),
             row % ('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), fmt(krt), fmt(kft), kft[0] / krt[0], core_bonds_t, fmt(w_sf_t)),
             row % ('(c) worst case: %d graphs of %d atoms, random logits (dense)' % (args.graphs, M.MAX_ATOMS), fmt(krd), fmt(kfd), kfd[0] / krd[0], core_bonds_d, '-'),
             '',
             '(a) with `generic=True`: %s ms.  `scaffold_keys(scaffolds(..))` %s ms wall.' % (fmt(kg), fmt(w_keys)),
             '',
             'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept, host clock around the call).  The '
             'scaffolds of the final frame cost %.4f of one step, those of all %d frames %.3f steps.' % (step_ms, args.steps, kf[0] / step_ms, F, kft[0] / step_ms),
             '',
             'Final frame, %d graphs (deterministic noise weights, so the molecules are noise): %d have a scaffold, %d distinct scaffold keys; '
             'totals: %s.' % (args.graphs, int((sf.counts[0, :, 0] > 0).sum()), distinct, ', '.join('%s %d' % kv for kv in totals.items()))]
    return report(lines, {'rings_ms_final': kr[0], 'scaffold_ms_final': kf[0], 'rings_ms_traj': krt[0], 'scaffold_ms_traj': kft[0], 'frames': F,
                          'rings_ms_dense': krd[0], 'scaffold_ms_dense': kfd[0], 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
