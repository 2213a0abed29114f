#!/usr/bin/env python3
"""Timing of the hydrogen kernel (csrc/mol_hydrogens.hip) next to the stereo kernel, with which it shares its structure, on the same
inputs and in the same run.

  python tools/bench_mol_hydrogens.py [--steps 10] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its saved trajectory (steps + 1 frames) in ONE launch.  Kernel times are
HIP events around the launch alone (outputs allocated before), warm, median of repeats, as tools/mol_bench.py takes them; the wall
time is a host clock around a call that ends in a device synchronise.  A record, not a pass/fail: the kernel is new, there is
nothing to regress against and no target was set in advance."""
from mol_bench import headline_run, parser, relaunch_ms, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_stereo import stereo_kernel_ms
from phoregen_amd import hip, hydrogens as HY, molecule as M


def hydrogens_kernel_ms(hy, pos, pos_fs, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_hydrogens launches over all frames of a Hydrogens' screen, after `warmup`."""
    sc = hy.screen
    F, B = sc.status.shape
    lib, table = hip.lib(), HY._length_table(hy.options, pos.device)
    return relaunch_ms(hy, ('status', 'counts', 'h_pos', 'h_placed', 'site_shape', 'min_contact'),
                       lambda out: HY._launch_hydrogens(lib, pos, pos_fs, sc, hy.kekule, B, F, max(sc.num_atoms), table, hy.options, out),
                       repeats, warmup)


def main(argv=None):
    args = parser(10).parse_args(argv)
    _, _, res, _, _ = headline_run(args.graphs, args.steps, warm=False)
    rows = []
    for label, frames, reps in (('(a) final frame', 'final', 50), ('(b) trajectory, ONE launch', 'traj', 20)):
        _, pos, _, F, fs = M._frames(res, frames)
        st = M.stereo(res, frames=frames)
        hy = HY.hydrogens(res, frames=frames, screen=st.screen, kekule=st.kekule)
        t_st = stereo_kernel_ms(st, pos, fs[2], reps)
        t_hy = hydrogens_kernel_ms(hy, pos, fs[2], reps)
        wall = wall_ms(lambda: HY.hydrogens(res, frames=frames, screen=st.screen, kekule=st.kekule), 10)
        c = dict(zip(HY.HYD_COUNTS, hy.counts.reshape(-1, len(HY.HYD_COUNTS)).sum(0).tolist()))
        rows.append(('%s, %d frames x %d graphs, %d atom rows' % (label, F, args.graphs, pos.size(-2)), t_st, t_hy, c, wall, int(hy.ok.sum()), hy.ok.numel()))
    fmt = lambda t: '%.4f (%.4f - %.4f)' % t[:3]   # noqa: E731
    lines = ['| case | `pg_mol_stereo` kernel ms, median (min - max) | `pg_mol_hydrogens` kernel ms | hydrogens / stereo | census | `hydrogens()` wall ms |',
             '|---|---|---|---|---|---|']
    lines += ['| %s | %s | %s | %.2f x | %d hydrogens at %d sites (%d generic), %d contacts, %d of %d ok | %s |'
              % (label, fmt(s), fmt(h), h[0] / s[0], c['hydrogens'], c['sites'], c['sites_generic'], c['contacts'], ok, n, fmt(wl))
              for label, s, h, c, wl, ok, n in rows]
    return report(lines, {'stereo_ms_final': rows[0][1][0], 'hydrogens_ms_final': rows[0][2][0], 'stereo_ms_traj': rows[1][1][0],
                          'hydrogens_ms_traj': rows[1][2][0], 'frames': args.steps + 1}, args.out)


if __name__ == '__main__':
    main()
