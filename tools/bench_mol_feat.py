#!/usr/bin/env python3
"""Timing of the feature kernel (csrc/mol_feat.hip, phoregen_amd/molecule.py) next to the geometry and the screen kernels on the same
inputs and in the same run; writes the table of profiles/mol_feat_timing.md.

  python tools/bench_mol_feat.py [--steps 50] [--out FILE.md]

(a) final prediction of the 128-graph headline batch with its own pharmacophore points, typed by name, (b) a synthetic batch of sparse
aromatic graphs with something to type: 64 atoms each, three fused aromatic ring pairs of C / N joined by single bonds to a chain of
C / N / O, random coordinates, twelve points per graph on its own atoms.  Kernel times are HIP events around the launch alone (outputs
allocated before), warm, median of repeats, exactly as tools/bench_mol_geom.py takes the geometry's; wall times are a host clock
around a call that ends in a device synchronise.  A record, not a pass/fail."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench import ligphore_workload  # noqa: E402
from bench_mol_geom import geom_kernel_ms  # noqa: E402
from bench_mol_kekule import onehot_result, sparse_aromatic_graphs  # noqa: E402
from bench_mol_screen import kernel_ms, wall_ms  # noqa: E402
from phoregen_amd import hip, molecule as M  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.data import PHORETYPES1  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


def feat_kernel_ms(ft, pos, pos_fs, ppos, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_feat launches over all frames of a Features' screen, after `warmup`."""
    sc = ft.screen
    F, B = sc.status.shape
    out = {k: torch.empty_like(getattr(ft, k)) for k in ('status', 'counts', 'atom_fp', 'point_dist', 'point_atom')}
    lib = hip.lib()

    def go():
        M._launch_feat(lib, pos, pos_fs, sc, ft.kekule, ft.rings, B, F, max(sc.num_atoms), ppos, ft.point_kind, ft.point_range, ft.point_off,
                       ft.point_dist.size(1), ft.limits, out)
    for _ in range(warmup):
        go()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    assert all(torch.equal(out[k].view(torch.int32) if out[k].dtype == torch.float32 else out[k],
                           getattr(ft, k).view(torch.int32) if out[k].dtype == torch.float32 else getattr(ft, k)) for k in out)
    return statistics.median(ts), min(ts), max(ts)


def census(ft):
    c = dict(zip(M.FEATURE_COUNTS, ft.counts.reshape(-1, len(M.FEATURE_COUNTS)).sum(0).tolist()))
    return 'ok %d of %d, typed points %d, matched %d, typed atoms %d' % (int(ft.ok.sum()), ft.ok.numel(), c['typed_points'], c['matched'],
                                                                         int((ft.atom_fp != 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50, help='reverse steps of the sampled batch')
    ap.add_argument('--graphs', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    dev = 'cuda'
    model = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to(dev)
    w = ligphore_workload(args.graphs)
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], w['num_atoms'], torch.zeros(args.graphs, 3),
                             rng='device', seed=1, num_steps=args.steps, return_traj=False)
    torch.cuda.synchronize()
    rows = []

    def measure(label, res, ppos, kinds, pb):
        pex = (kinds == M.POINT_IGNORED).to(torch.uint8).to(dev)
        sc = M.screen(res)
        node, pos, edge = res['pred']
        ks = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, args.repeats)
        geo = M.geometry(res, ppos, pex, point_batch=pb, screen=sc)
        kg = geom_kernel_ms(geo, pos, 0, ppos, pex, args.repeats)[:3]
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

    fmt = lambda t: '%.3f (%.3f - %.3f)' % t[:3]   # noqa: E731
    lines = ['| case | `pg_mol_screen` kernel ms, median (min - max) | `pg_mol_geom` kernel ms | `pg_mol_feat` kernel ms | feat / geom | census | '
             '`features()` wall ms, parts handed in | `features()` wall ms, Kekulé form and rings computed |', '|---|---|---|---|---|---|---|---|']
    lines += ['| %s | %s | %s | %s | %.1f x | %s | %s | %s |' % (label, fmt(ks), fmt(kg), fmt(kf), kf[0] / kg[0], cen, fmt(wf), fmt(wall))
              for label, ks, kg, kf, cen, wf, wall in rows]
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps({'screen_ms_final': rows[0][1][0], 'geom_ms_final': rows[0][2][0], 'feat_ms_final': rows[0][3][0],
                      'screen_ms_sparse': rows[1][1][0], 'geom_ms_sparse': rows[1][2][0], 'feat_ms_sparse': rows[1][3][0]}))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
