#!/usr/bin/env python3
"""Timing of the ring kernel (csrc/mol_rings.hip, phoregen_amd/molecule.py) next to the screen kernel on the same inputs and in the
same run; writes the table of profiles/mol_rings_timing.md.

  python tools/bench_mol_rings.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) the worst case: graphs of
PG_MOL_MAX_ATOMS atoms with random logits, which bond about two thirds of all pairs, so every lane searches about 85 rings.  Kernel
times are HIP events around the launch alone (outputs allocated before), warm, median of repeats, as tools/mol_bench.py takes
them; wall times are a host clock around a call that ends in a device synchronise.  The reverse step the two are held against is
the sampling call of this run divided by its steps.  A record, not a pass/fail."""
from dataclasses import astuple

from mol_bench import dense_result, fmt, headline_run, parser, relaunch_ms, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_screen import kernel_ms
from phoregen_amd import hip, molecule as M


def rings_kernel_ms(rg, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_rings launches over all frames of a Rings' screen, after `warmup`."""
    sc = rg.screen
    F, B = sc.status.shape
    lib, lim = hip.lib(), astuple(rg.limits)
    return relaunch_ms(rg, ('status', 'counts', 'ring_size', 'atom_ring', 'ring_sys'),
                       lambda out: M._launch_rings(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), lim, out), repeats, warmup)


def main(argv=None):
    args = parser().parse_args(argv)
    dev = 'cuda'
    _, _, res, t_sample, step_ms = headline_run(args.graphs, args.steps)

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
    return report(lines, {'screen_ms_final': ks[0], 'rings_ms_final': kr[0], 'screen_ms_traj': kst[0], 'rings_ms_traj': krt[0], 'frames': F,
                          'screen_ms_dense': ksd[0], 'rings_ms_dense': krd[0], 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
