#!/usr/bin/env python3
"""Timing of the Kekulé kernel (csrc/mol_kekule.hip, phoregen_amd/molecule.py) next to the screen kernel on the same inputs and in
the same run; writes the table of profiles/mol_kekule_timing.md.

  python tools/bench_mol_kekule.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) a synthetic batch of sparse
aromatic graphs: 64 atoms each, three fused aromatic ring pairs of C / N joined by single bonds, the rest a chain, (d) the serial
worst case: a ladder of PG_MOL_MAX_ATOMS aromatic carbons per graph, 128 searches of growing trees on one lane.  Kernel times are HIP
events around the launch alone (outputs allocated before), warm, median of repeats, as tools/mol_bench.py takes them; wall times are
a host clock around a call that ends in a device synchronise.  The reverse step the two are held against is the sampling call of
this run divided by its steps.  A record, not a pass/fail."""
from mol_bench import (fmt, headline_run, ladder_graphs, onehot_result, parser, relaunch_ms, report, sparse_aromatic_graphs,
                       wall_ms)      # first: puts the repository root on sys.path
from bench_mol_screen import kernel_ms
from phoregen_amd import hip, molecule as M


def kekule_kernel_ms(kk, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_kekule launches over all frames of a Kekule's screen, after `warmup`."""
    sc = kk.screen
    F, B = sc.status.shape
    lib, tables = hip.lib(), M._kekule_table(sc.cls.device)
    return relaunch_ms(kk, ('status', 'counts', 'kekule_order', 'hcount', 'charge'),
                       lambda out: M._launch_kekule(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), tables,
                                                    kk.options.allow_charged, out), repeats, warmup)


def main(argv=None):
    args = parser().parse_args(argv)
    dev = 'cuda'
    _, _, res, t_sample, step_ms = headline_run(args.graphs, args.steps)

    def census(kk):
        c = dict(zip(M.KEKULE_COUNTS, kk.counts.reshape(-1, len(M.KEKULE_COUNTS)).sum(0).tolist()))
        return 'ok %d of %d, aromatic atoms %d, doubled %d' % (int(kk.ok.sum()), kk.ok.numel(), c['aromatic_atoms'], c['doubled'])

    sc = M.screen(res)
    node, pos, edge = res['pred']
    ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50)
    kk = M.kekulize(res, screen=sc)
    kr = kekule_kernel_ms(kk, 50)
    w_kk = wall_ms(lambda: M.kekulize(res, screen=sc), 10)
    w_asm, w_asm_k = wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: M.assemble(res, kekule=M.kekulize(res)), 10)
    flags = {name: int(((kk.status & bit) != 0).sum()) for bit, name in M.KEKULE_NAMES.items()}
    totals = dict(zip(M.KEKULE_COUNTS, kk.counts[0].sum(0).tolist()))
    cen_a = census(kk)

    tn, tp, te = res['traj']
    F = tn.size(0)
    kst = kernel_ms(tn, tp, te, F, (tn.stride(0), te.stride(0), tp.stride(0)), sc, 7, warmup=2)
    sct = M.screen(res, frames='traj')
    kkt = M.kekulize(res, frames='traj', screen=sct)
    krt = kekule_kernel_ms(kkt, 7, warmup=2)
    w_kk_t = wall_ms(lambda: M.kekulize(res, frames='traj', screen=sct), 5)
    cen_b = census(kkt)
    del kkt, sct, res

    rows = []
    for label, graphs in (('(c) sparse aromatic: %d graphs of 64 atoms, 30 aromatic' % args.graphs, sparse_aromatic_graphs(args.graphs)),
                          ('(d) serial worst case: %d ladders of %d aromatic C' % (args.graphs, M.MAX_ATOMS), ladder_graphs(args.graphs, M.MAX_ATOMS))):
        syn = onehot_result(graphs, dev)
        scs = M.screen(syn)
        sn, sp, se = syn['pred']
        kss = kernel_ms(sn, sp, se, 1, (0, 0, 0), scs, 20)
        kks = M.kekulize(syn, screen=scs)
        rows.append((label, kss, kekule_kernel_ms(kks, 20), census(kks)))

    row = '| %s | %s | %s | %.1f x | %s | %s |'
    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_kekule` kernel ms | kekule / screen | census | `kekulize()` wall ms |',
             '|---|---|---|---|---|---|',
             row % ('(a) final frame, %d graphs' % args.graphs, fmt(ks), fmt(kr), kr[0] / ks[0], cen_a, fmt(w_kk)),
             row % ('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), fmt(kst), fmt(krt), krt[0] / kst[0], cen_b, fmt(w_kk_t))]
    lines += [row % (label, fmt(a), fmt(b), b[0] / a[0], c, '-') for label, a, b, c in rows]
    lines += ['',
              '`assemble()` %s ms wall, `assemble(kekule=kekulize(..))` %s ms wall.' % (fmt(w_asm), fmt(w_asm_k)),
              '',
              'One reverse step of this batch in this run: %.2f ms (%d steps with the trajectory kept in %.1f s, host clock around the call).  '
              'The Kekulé form of the final frame costs %.4f of one step, that of all %d frames %.3f steps.' % (step_ms, args.steps, t_sample, kr[0] / step_ms, F, krt[0] / step_ms),
              '',
              'Final frame, %d graphs (deterministic noise weights, so the molecules are noise): %d pass the screen, %d have a Kekulé structure; '
              'graphs per bit: %s; totals: %s.' % (args.graphs, int(sc.valid.sum()), int(kk.ok.sum()), ', '.join('%s %d' % kv for kv in flags.items()),
                                                   ', '.join('%s %d' % kv for kv in totals.items()))]
    return report(lines, {'screen_ms_final': ks[0], 'kekule_ms_final': kr[0], 'screen_ms_traj': kst[0], 'kekule_ms_traj': krt[0], 'frames': F,
                          'screen_ms_sparse': rows[0][1][0], 'kekule_ms_sparse': rows[0][2][0], 'screen_ms_ladder': rows[1][1][0],
                          'kekule_ms_ladder': rows[1][2][0], 'step_ms': step_ms}, args.out)


if __name__ == '__main__':
    main()
