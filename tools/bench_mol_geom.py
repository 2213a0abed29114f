#!/usr/bin/env python3
"""Timing of the geometry screen kernel (csrc/mol_geom.hip, phoregen_amd/molecule.py) next to the screen kernel on the same inputs and
in the same run; writes the table of profiles/mol_geom_timing.md.

  python tools/bench_mol_geom.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch; every graph is measured against
its own pharmacophore of the workload.  Kernel times are HIP events around the launch alone (outputs allocated before), warm, median
of repeats, as tools/mol_bench.py takes them; wall times are a host clock around a call that ends in a device synchronise.  The
reverse step the two are held against is the sampling call of this run divided by its steps.  A record, not a pass/fail."""
import torch

from mol_bench import fmt, headline_run, parser, relaunch_ms, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_screen import kernel_ms
from phoregen_amd import hip, molecule as M


def geom_kernel_ms(geo, pos, pos_fs, ppos, pex, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_geom launches over all frames of a Geometry's screen, after `warmup`."""
    sc = geo.screen
    F, B = sc.status.shape
    lib, lim = hip.lib(), tuple(float(getattr(geo.limits, k)) for k in ('bond_min', 'bond_max', 'clash_min', 'ex_clear', 'feat_cut'))
    return relaunch_ms(geo, ('status', 'metrics', 'counts', 'point_dist', 'point_atom'),
                       lambda out: M._launch_geom(lib, pos, pos_fs, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), ppos, pex,
                                                  geo.point_range, geo.point_off, geo.point_dist.size(1), lim, out), repeats, warmup)


def pair_evaluations(geo):
    """Distances one call measures: atom pairs of every graph plus atoms x points, per frame, times the frames."""
    na = geo.screen.num_atoms
    npt = (geo.point_off[1:] - geo.point_off[:-1]).tolist()
    return geo.status.size(0) * sum(n * (n - 1) // 2 + n * p for n, p in zip(na, npt))


def main(argv=None):
    args = parser().parse_args(argv)
    dev = 'cuda'
    model, w, res, t_sample, step_ms = headline_run(args.graphs, args.steps)

    ppos = w['pos_phore'].float().to(dev).contiguous()                 # (centres are zero in this workload)
    pex = (w['h_phore'][:, model.ex_col] == 1).to(torch.uint8).to(dev)
    pb = w['batch_phore']
    geometry = lambda frames, sc=None: M.geometry(res, ppos, pex, point_batch=pb, frames=frames, screen=sc)   # noqa: E731

    sc = M.screen(res)
    node, pos, edge = res['pred']
    ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50)
    geo = geometry('final', sc)
    kg = geom_kernel_ms(geo, pos, 0, ppos, pex, 50)
    w_geo = wall_ms(lambda: geometry('final', sc), 10)
    w_asm, w_asm_g = wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: M.assemble(res, geometry=geometry('final')), 10)
    n_ok, n_valid = int(geo.ok.sum()), int(sc.valid.sum())
    census = {name: int(((geo.status & bit) != 0).sum()) for bit, name in M.GEOM_NAMES.items()}

    tn, tp, te = res['traj']
    F = tn.size(0)
    kst = kernel_ms(tn, tp, te, F, (tn.stride(0), te.stride(0), tp.stride(0)), sc, 7, warmup=2)
    sct = M.screen(res, frames='traj')
    geot = geometry('traj', sct)
    kgt = geom_kernel_ms(geot, tp, tp.stride(0), ppos, pex, 7, warmup=2)
    w_geo_t = wall_ms(lambda: geometry('traj', sct), 5)
    ev, evt = pair_evaluations(geo), pair_evaluations(geot)

    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_geom` kernel ms | geom / screen | distances per call | `geometry()` wall ms |',
             '|---|---|---|---|---|---|',
             '| (a) final frame, %d graphs | %s | %s | %.1f x | %.3g | %s |' % (args.graphs, fmt(ks), fmt(kg), kg[0] / ks[0], ev, fmt(w_geo)),
             '| (b) trajectory, %d frames x %d graphs, ONE launch | %s | %s | %.1f x | %.3g | %s |' % (F, args.graphs, fmt(kst), fmt(kgt), kgt[0] / kst[0], evt, fmt(w_geo_t)),
             '',
             '`assemble()` %s ms wall, `assemble(geometry=geometry(..))` %s ms wall.  (b) measures %.2f distances per nanosecond.' % (fmt(w_asm), fmt(w_asm_g), evt / (kgt[0] * 1e6)),
             '',
             'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
             'The geometry of the final frame costs %.4f of one step, that of all %d frames %.3f steps.' % (step_ms, args.steps, t_sample, kg[0] / step_ms, F, kgt[0] / step_ms),
             '',
             'Final frame, %d graphs, %d points (deterministic noise weights, so the molecules are noise): %d pass the screen, %d the geometry '
             'limits; graphs per bit: %s.' % (args.graphs, ppos.size(0), n_valid, n_ok, ', '.join('%s %d' % (k, v) for k, v in census.items()))]
    return report(lines, {'screen_ms_final': ks[0], 'geom_ms_final': kg[0], 'screen_ms_traj': kst[0], 'geom_ms_traj': kgt[0], 'frames': F,
                          'step_ms': step_ms, 'distances_final': ev, 'distances_traj': evt}, args.out)


if __name__ == '__main__':
    main()
