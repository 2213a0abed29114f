#!/usr/bin/env python3
"""Timing of the stereo kernel (csrc/mol_stereo.hip) and of the isomeric SMILES (pg_mol_smiles_stereo, csrc/mol_smiles.hip) next to
the screen and the plain SMILES kernel on the same inputs and in the same run; writes the table of profiles/mol_stereo_timing.md.

  python tools/bench_mol_stereo.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch.  Kernel times are HIP events
around the launch alone (outputs allocated before), warm, median of repeats, as tools/mol_bench.py takes them; wall times are a
host clock around a call that ends in a device synchronise.  The reverse step they are held against is the sampling call of this run
divided by its steps.  A record, not a pass/fail: the kernels are new, there is nothing to regress against and no target was set in
advance."""
from mol_bench import fmt, headline_run, parser, relaunch_ms, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_screen import kernel_ms
from bench_mol_smiles import smiles_kernel_ms
from phoregen_amd import hip, molecule as M


def stereo_kernel_ms(st, pos, pos_fs, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_stereo launches over all frames of a Stereo's screen, after `warmup`."""
    sc = st.screen
    F, B = sc.status.shape
    lib = hip.lib()
    return relaunch_ms(st, ('status', 'counts', 'atom_parity', 'atom_label', 'bond_stereo', 'bond_label', 'stereo_key'),
                       lambda out: M._launch_stereo(lib, pos, pos_fs, sc, st.kekule, st.rings, st.keys, B, F, max(sc.num_atoms), st.limits, out),
                       repeats, warmup)


def smiles_stereo_kernel_ms(sm, repeats, warmup=3):
    """The same of pg_mol_smiles_stereo for a Smiles written with stereo=."""
    sc = sm.screen
    F, B = sc.status.shape
    lib, table = hip.lib(), M._smiles_table(sc.cls.device)
    return relaunch_ms(sm, ('status', 'counts', 'text', 'length', 'atom_rank', 'stereo_counts'),
                       lambda out: M._launch_smiles(lib, sc, sm.kekule, B, F, max(sc.num_atoms), table, sm.capacity, out, sm.stereo),
                       repeats, warmup)


def main(argv=None):
    args = parser().parse_args(argv)
    _, _, res, t_sample, step_ms = headline_run(args.graphs, args.steps)

    def census(st, sm):
        c = dict(zip(M.STEREO_COUNTS, st.counts.reshape(-1, len(M.STEREO_COUNTS)).sum(0).tolist()))
        s = dict(zip(M.SMILES_STEREO_COUNTS, sm.stereo_counts.reshape(-1, 4).sum(0).tolist()))
        return ('centres %d defined / %d undefined, double bonds %d / %d; texts %d of %d with %d centres and %d double bonds'
                % (c['centres_defined'], c['centres_undefined'], c['bonds_defined'], c['bonds_undefined'], int(sm.ok.sum()), sm.ok.numel(),
                   s['centres'], s['double_bonds']))

    def case(frames, reps, warmup):
        node, pos, edge, F, fs = M._frames(res, frames)
        sc = M.screen(res, frames=frames)
        ks = kernel_ms(node, pos, edge, F, fs, sc, reps, warmup=warmup)
        st = M.stereo(res, frames=frames, screen=sc)
        plain = M.smiles(res, frames=frames, screen=sc, kekule=st.kekule)
        sm = M.smiles(res, frames=frames, stereo=st)
        return (ks, smiles_kernel_ms(plain, reps, warmup=warmup), stereo_kernel_ms(st, pos, fs[2], reps, warmup=warmup),
                smiles_stereo_kernel_ms(sm, reps, warmup=warmup), st, sm)

    a = case('final', 50, 3)
    st = a[4]
    w_st = wall_ms(lambda: M.stereo(res, screen=st.screen, kekule=st.kekule, rings=st.rings, keys=st.keys), 10)
    w_all = wall_ms(lambda: M.stereo(res), 10)
    w_sm = wall_ms(lambda: M.smiles(res, stereo=st), 10)
    flags = {name: int(((st.status & bit) != 0).sum()) for bit, name in M.STEREO_NAMES.items()}
    rows = [('(a) final frame, %d graphs' % args.graphs, *a[:4], census(st, a[5]), w_st)]
    b = case('traj', 7, 2)
    F = b[4].status.size(0)
    stt = b[4]
    w_st_t = wall_ms(lambda: M.stereo(res, frames='traj', screen=stt.screen, kekule=stt.kekule, rings=stt.rings, keys=stt.keys), 5)
    rows.append(('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), *b[:4], census(stt, b[5]), w_st_t))

    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_smiles` kernel ms | `pg_mol_stereo` kernel ms | '
             '`pg_mol_smiles_stereo` kernel ms | stereo / screen | census | `stereo()` wall ms |', '|---|---|---|---|---|---|---|---|']
    lines += ['| %s | %s | %s | %s | %s | %.1f x | %s | %s |' % (label, fmt(k), fmt(p), fmt(s), fmt(i), s[0] / k[0], cen, fmt(wl))
              for label, k, p, s, i, cen, wl in rows]
    lines += ['',
              '`stereo()` with the screen, the Kekulé form, the rings and the keys computed too: %s ms wall; `smiles(stereo=)` %s ms wall.'
              % (fmt(w_all), fmt(w_sm)),
              '',
              'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
              'The stereo of the final frame costs %.4f of one step, that of all %d frames %.3f steps.'
              % (step_ms, args.steps, t_sample, a[2][0] / step_ms, F, b[2][0] / step_ms),
              '',
              'Final frame, %d graphs (deterministic noise weights, so the molecules are noise): graphs per bit: %s.'
              % (args.graphs, ', '.join('%s %d' % kv for kv in flags.items()))]
    return report(lines, {'screen_ms_final': a[0][0], 'smiles_ms_final': a[1][0], 'stereo_ms_final': a[2][0], 'smiles_stereo_ms_final': a[3][0],
                          'screen_ms_traj': b[0][0], 'smiles_ms_traj': b[1][0], 'stereo_ms_traj': b[2][0], 'smiles_stereo_ms_traj': b[3][0],
                          'frames': F, 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
