#!/usr/bin/env python3
"""Timing of the feature kernel (csrc/mol_feat.hip, phoregen_amd/molecule.py) next to the geometry and the screen kernels on the same
inputs and in the same run; writes the table of profiles/mol_feat_timing.md.

  python tools/bench_mol_feat.py [--steps 50] [--out FILE.md]

(a) final prediction of the 128-graph headline batch with its own pharmacophore points, typed by name, (b) a synthetic batch of sparse
aromatic graphs with something to type: 64 atoms each, three fused aromatic ring pairs of C / N joined by single bonds to a chain of
C / N / O, random coordinates, twelve points per graph on its own atoms.  Kernel times are HIP events around the launch alone (outputs
allocated before), warm, median of repeats, as tools/mol_bench.py takes them; wall times are a host clock around a call that ends
in a device synchronise.  A record, not a pass/fail."""
import numpy as np
import torch

from mol_bench import (fmt, headline_run, onehot_result, parser, relaunch_ms, report, sparse_aromatic_graphs,
                       wall_ms)      # first: puts the repository root on sys.path
from bench_mol_geom import geom_kernel_ms
from bench_mol_screen import kernel_ms
from phoregen_amd import hip, molecule as M
from phoregen_amd.data import PHORETYPES1


def feat_kernel_ms(ft, pos, pos_fs, ppos, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_feat launches over all frames of a Features' screen, after `warmup`."""
    sc = ft.screen
    F, B = sc.status.shape
    lib = hip.lib()
    return relaunch_ms(ft, ('status', 'counts', 'atom_fp', 'point_dist', 'point_atom'),
                       lambda out: M._launch_feat(lib, pos, pos_fs, sc, ft.kekule, ft.rings, B, F, max(sc.num_atoms), ppos, ft.point_kind,
                                                  ft.point_range, ft.point_off, ft.point_dist.size(1), ft.limits, out), repeats, warmup)


def census(ft):
    c = dict(zip(M.FEATURE_COUNTS, ft.counts.reshape(-1, len(M.FEATURE_COUNTS)).sum(0).tolist()))
    return 'ok %d of %d, typed points %d, matched %d, typed atoms %d' % (int(ft.ok.sum()), ft.ok.numel(), c['typed_points'], c['matched'],
                                                                         int((ft.atom_fp != 0).sum()))


def main(argv=None):
    ap = parser(50, 'reverse steps of the sampled batch')
    ap.add_argument('--repeats', type=int, default=50)
    args = ap.parse_args(argv)
    dev = 'cuda'
    _, w, res, _, _ = headline_run(args.graphs, args.steps, warm=False, traj=False)
    rows = []

    def measure(label, res, ppos, kinds, pb):
        pex = (kinds == M.POINT_IGNORED).to(torch.uint8).to(dev)
        sc = M.screen(res)
        node, pos, edge = res['pred']
        ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, args.repeats)
        geo = M.geometry(res, ppos, pex, point_batch=pb, screen=sc)
        kg = geom_kernel_ms(geo, pos, 0, ppos, pex, args.repeats)
        ft = M.features(res, ppos, kinds, point_batch=pb, screen=sc)
        kf = feat_kernel_ms(ft, pos, 0, ppos, args.repeats)
        wf = wall_ms(lambda: M.features(res, ppos, kinds, point_batch=pb, screen=sc, kekule=ft.kekule, rings=ft.rings), 10)
        wall = wall_ms(lambda: M.features(res, ppos, kinds, point_batch=pb, screen=sc), 10)
        rows.append((label, ks, kg, kf, census(ft), wf, wall))

    ppos = w['pos_phore'].float().to(dev).contiguous()                 # (centres are zero in this workload)
    measure('(a) final frame, %d graphs, their %d pharmacophore points' % (args.graphs, ppos.size(0)), res, ppos,
            M.point_kinds_of(w['h_phore'].to(dev), PHORETYPES1), w['batch_phore'])
    rng = np.random.default_rng(0)
    graphs = []
    for classes, bonds in sparse_aromatic_graphs(args.graphs):
        in_ring = {x for (a, b), t in bonds.items() if t == 4 for x in (a, b)}
        graphs.append(([c if i in in_ring else int(rng.choice([1, 1, 2, 3])) for i, c in enumerate(classes)], bonds))
    syn = onehot_result(graphs, dev)
    xyz = torch.from_numpy((rng.random((64 * args.graphs, 3)) * 28.0).astype(np.float32)).to(dev)
    syn['pred'][1] = xyz
    pick = torch.from_numpy(np.concatenate([64 * g + rng.choice(64, 12, replace=False) for g in range(args.graphs)])).to(dev)
    kinds = torch.from_numpy(rng.integers(-2, 7, 12 * args.graphs).astype(np.int8)).to(dev)
    measure('(b) sparse aromatic: %d graphs of 64 atoms, 12 points each on their atoms' % args.graphs, syn, (xyz[pick] + 0.25).contiguous(), kinds,
            torch.repeat_interleave(torch.arange(args.graphs), 12))

    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_geom` kernel ms | `pg_mol_feat` kernel ms | feat / geom | census | '
             '`features()` wall ms, parts handed in | `features()` wall ms, Kekulé form and rings computed |', '|---|---|---|---|---|---|---|---|']
    lines += ['| %s | %s | %s | %s | %.1f x | %s | %s | %s |' % (label, fmt(ks), fmt(kg), fmt(kf), kf[0] / kg[0], cen, fmt(wf), fmt(wall))
              for label, ks, kg, kf, cen, wf, wall in rows]
    return report(lines, {'screen_ms_final': rows[0][1][0], 'geom_ms_final': rows[0][2][0], 'feat_ms_final': rows[0][3][0],
                          'screen_ms_sparse': rows[1][1][0], 'geom_ms_sparse': rows[1][2][0], 'feat_ms_sparse': rows[1][3][0]}, args.out)


if __name__ == '__main__':
    main()
