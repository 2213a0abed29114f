#!/usr/bin/env python3
"""Timing of the identity key kernel (csrc/mol_key.hip, phoregen_amd/molecule.py) next to the screen kernel on the same inputs and
in the same run; writes the table of profiles/mol_key_timing.md.

  python tools/bench_mol_key.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch.  Kernel times are HIP events
around the launch alone (outputs allocated before), warm, median of repeats, as tools/mol_bench.py takes them; wall times are a
host clock around a call that ends in a device synchronise.  The reverse step the two are held against is the sampling call of
this run divided by its steps."""
import torch

from mol_bench import event_ms, fmt, headline_run, parser, report, wall_ms      # first: puts the repository root on sys.path
from bench_mol_screen import kernel_ms
from phoregen_amd import hip, molecule as M


def key_kernel_ms(sc, repeats, warmup=3, colour=True):
    """Median / min / max of `repeats` event-timed pg_mol_key launches over all frames of a Screen, after `warmup` launches; the keys."""
    F, B = sc.status.shape
    key = torch.empty(F, B, dtype=torch.int64, device=sc.cls.device)
    col = torch.empty(F, sc.cls.size(1), dtype=torch.int64, device=sc.cls.device) if colour else None
    lib = hip.lib()
    return event_ms(lambda: M._launch_key(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), key, col), repeats, warmup) + (key,)


def main(argv=None):
    args = parser().parse_args(argv)
    _, _, res, t_sample, step_ms = headline_run(args.graphs, args.steps)

    sc = M.screen(res)
    node, pos, edge = res['pred']
    ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50)
    kk = key_kernel_ms(sc, 50)
    kk0 = key_kernel_ms(sc, 50, colour=False)
    assert torch.equal(kk[3], kk0[3]) and torch.equal(kk[3], M.molecule_keys(sc).key)
    w_keys = wall_ms(lambda: M.molecule_keys(sc), 10)
    w_asm, w_asm_k = wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: M.assemble(res, keys=True), 10)
    n_kept = int((sc.cls >= 0).sum())
    distinct_final = int(M.duplicate_groups(kk[3])[0].numel())

    tn, tp, te = res['traj']
    F = tn.size(0)
    kst = kernel_ms(tn, tp, te, F, (tn.stride(0), te.stride(0), tp.stride(0)), sc, 7, warmup=2)
    sct = M.screen(res, frames='traj')
    kkt = key_kernel_ms(sct, 7, warmup=2)
    w_keys_t = wall_ms(lambda: M.molecule_keys(sct), 5)
    distinct_traj = int(M.duplicate_groups(kkt[3])[0].numel())

    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_key` kernel ms | key / screen | `molecule_keys()` wall ms |',
             '|---|---|---|---|---|',
             '| (a) final frame, %d graphs | %s | %s | %.1f x | %s |' % (args.graphs, fmt(ks), fmt(kk), kk[0] / ks[0], fmt(w_keys)),
             '| (b) trajectory, %d frames x %d graphs, ONE launch | %s | %s | %.1f x | %s |' % (F, args.graphs, fmt(kst), fmt(kkt), kkt[0] / kst[0], fmt(w_keys_t)),
             '',
             '(a) without the colour output (null pointer): %s ms.  `assemble()` %s ms wall, `assemble(keys=True)` %s ms wall.' % (fmt(kk0), fmt(w_asm), fmt(w_asm_k)),
             '',
             'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
             'The key of the final frame costs %.4f of one step, the keys of all %d frames %.3f steps.' % (step_ms, args.steps, t_sample, kk[0] / step_ms, F, kkt[0] / step_ms),
             '',
             'Kept atoms of the final frame: %d of %d rows.  Distinct keys: %d of %d graphs in the final frame, %d of %d (frame, graph) pairs '
             'of the trajectory (deterministic noise weights).' % (n_kept, sc.cls.numel(), distinct_final, args.graphs, distinct_traj, F * args.graphs)]
    return report(lines, {'screen_ms_final': ks[0], 'key_ms_final': kk[0], 'key_ms_final_no_colour': kk0[0], 'screen_ms_traj': kst[0],
                          'key_ms_traj': kkt[0], 'frames': F, 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
