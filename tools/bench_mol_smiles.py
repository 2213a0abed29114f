#!/usr/bin/env python3
"""Timing of the SMILES kernel (csrc/mol_smiles.hip, phoregen_amd/molecule.py) next to the screen and Kekulé kernels on the same inputs
and in the same run; writes the table of profiles/mol_smiles_timing.md.

  python tools/bench_mol_smiles.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) the synthetic batch of sparse
aromatic graphs of tools/mol_bench.py, which all have a Kekulé structure and therefore a text, (d) the longest serial walk: a
chain of PG_MOL_MAX_ATOMS carbons with 99 ring closures open at once per graph.  Kernel times are HIP events around the launch alone
(outputs allocated before), warm, median of repeats, as tools/mol_bench.py takes them; wall times are a host clock around a call
that ends in a device synchronise.  The reverse step they are held against is the sampling call of this run divided by its steps.
A record, not a pass/fail: the kernel is new, there is nothing to regress against."""
from mol_bench import (fmt, headline_run, label_chain_graphs, onehot_result, parser, relaunch_ms, report, sparse_aromatic_graphs,
                       wall_ms)      # first: puts the repository root on sys.path
from bench_mol_kekule import kekule_kernel_ms
from bench_mol_screen import kernel_ms
from phoregen_amd import hip, molecule as M


def smiles_kernel_ms(sm, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_smiles launches over all frames of a Smiles' screen, after `warmup`."""
    sc, kk = sm.screen, sm.kekule
    F, B = sc.status.shape
    lib, table = hip.lib(), M._smiles_table(sc.cls.device)
    return relaunch_ms(sm, ('status', 'counts', 'text', 'length', 'atom_rank'),
                       lambda out: M._launch_smiles(lib, sc, kk, B, F, max(sc.num_atoms), table, sm.capacity, out), repeats, warmup)


def main(argv=None):
    args = parser().parse_args(argv)
    dev = 'cuda'
    _, _, res, t_sample, step_ms = headline_run(args.graphs, args.steps)

    def census(sm):
        c = dict(zip(M.SMILES_COUNTS, sm.counts.reshape(-1, len(M.SMILES_COUNTS)).sum(0).tolist()))
        return 'ok %d of %d, bytes %d, ring closures %d, largest label %d' % (int(sm.ok.sum()), sm.ok.numel(), int(sm.length.sum()),
                                                                             c['ring_closures'], int(sm.counts[..., 6].max()) if sm.ok.numel() else 0)

    def case(result, frames, sc, reps, warmup):
        node, pos, edge, F, fs = M._frames(result, frames)
        ks = kernel_ms(node, pos, edge, F, fs, sc, reps, warmup=warmup)
        kk = M.kekulize(result, frames=frames, screen=sc)
        kr = kekule_kernel_ms(kk, reps, warmup=warmup)
        sm = M.smiles(result, frames=frames, screen=sc, kekule=kk)
        return ks, kr, smiles_kernel_ms(sm, reps, warmup=warmup), sm

    sc = M.screen(res)
    ks, kr, sr, sm = case(res, 'final', sc, 50, 3)
    w_sm = wall_ms(lambda: M.smiles(res, screen=sc, kekule=sm.kekule), 10)
    w_all = wall_ms(lambda: M.smiles(res), 10)
    w_str = wall_ms(lambda: sm.strings(), 10)
    w_asm, w_asm_s = wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: M.assemble(res, smiles=M.smiles(res)), 10)
    flags = {name: int(((sm.status & bit) != 0).sum()) for bit, name in M.SMILES_NAMES.items()}
    cen_a = census(sm)
    rows = [('(a) final frame, %d graphs' % args.graphs, ks, kr, sr, cen_a, w_sm)]

    sct = M.screen(res, frames='traj')
    F = sct.status.size(0)
    kst, krt, srt, smt = case(res, 'traj', sct, 7, 2)
    w_sm_t = wall_ms(lambda: M.smiles(res, frames='traj', screen=sct, kekule=smt.kekule), 5)
    rows.append(('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), kst, krt, srt, census(smt), w_sm_t))
    del smt, sct, res

    for label, graphs in (('(c) sparse aromatic: %d graphs of 64 atoms, 30 aromatic' % args.graphs, sparse_aromatic_graphs(args.graphs)),
                          ('(d) longest walk: %d chains of %d C with %d closures open at once' % (args.graphs, M.MAX_ATOMS, M.SMILES_MAX_LABEL),
                           label_chain_graphs(args.graphs, M.MAX_ATOMS))):
        syn = onehot_result(graphs, dev)
        a, b, c, sms = case(syn, 'final', M.screen(syn), 20, 3)
        rows.append((label, a, b, c, census(sms), None))

    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_kekule` kernel ms | `pg_mol_smiles` kernel ms | smiles / screen | census | `smiles()` wall ms |',
             '|---|---|---|---|---|---|---|']
    lines += ['| %s | %s | %s | %s | %.1f x | %s | %s |' % (label, fmt(a), fmt(b), fmt(c), c[0] / a[0], cen, fmt(wl) if wl else '-')
              for label, a, b, c, cen, wl in rows]
    lines += ['',
              '`smiles()` with the screen and the Kekulé form computed too: %s ms wall; `Smiles.strings()` %s ms wall; `assemble()` %s ms wall, '
              '`assemble(smiles=smiles(..))` %s ms wall.' % (fmt(w_all), fmt(w_str), fmt(w_asm), fmt(w_asm_s)),
              '',
              'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
              'The text of the final frame costs %.4f of one step, that of all %d frames %.3f steps.' % (step_ms, args.steps, t_sample, sr[0] / step_ms, F, srt[0] / step_ms),
              '',
              'Final frame, %d graphs (deterministic noise weights, so the molecules are noise): %d pass the screen, %d have a text; graphs per '
              'bit: %s.' % (args.graphs, int(sc.valid.sum()), int(sm.ok.sum()), ', '.join('%s %d' % kv for kv in flags.items()))]
    return report(lines, {'screen_ms_final': ks[0], 'kekule_ms_final': kr[0], 'smiles_ms_final': sr[0], 'screen_ms_traj': kst[0],
                          'kekule_ms_traj': krt[0], 'smiles_ms_traj': srt[0], 'frames': F, 'smiles_ms_sparse': rows[2][3][0],
                          'smiles_ms_chain': rows[3][3][0], 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
