#!/usr/bin/env python3
"""Timing of the hydrogen kernel (csrc/mol_hydrogens.hip) next to the stereo kernel, with which it shares its structure, on the same
inputs and in the same run.

  python tools/bench_mol_hydrogens.py [--steps 10] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its saved trajectory (steps + 1 frames) in ONE launch.  Kernel times are
HIP events around the launch alone (outputs allocated before), warm, median of repeats, exactly as tools/bench_mol_stereo.py takes
its own; the wall time is a host clock around a call that ends in a device synchronise.  A record, not a pass/fail: the kernel is
new, there is nothing to regress against and no target was set in advance."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench import ligphore_workload  # noqa: E402
from bench_mol_screen import wall_ms  # noqa: E402
from bench_mol_stereo import _timed, stereo_kernel_ms  # noqa: E402
from phoregen_amd import hip, hydrogens as HY, molecule as M  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


def hydrogens_kernel_ms(hy, pos, pos_fs, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed pg_mol_hydrogens launches over all frames of a Hydrogens' screen, after `warmup`."""
    sc = hy.screen
    F, B = sc.status.shape
    names = ('status', 'counts', 'h_pos', 'h_placed', 'site_shape', 'min_contact')
    out = {k: torch.empty_like(getattr(hy, k)) for k in names}
    lib, table = hip.lib(), HY._length_table(hy.options, pos.device)
    t = _timed(lambda: HY._launch_hydrogens(lib, pos, pos_fs, sc, hy.kekule, B, F, max(sc.num_atoms), table, hy.options, out), repeats, warmup)
    assert all(torch.equal(out[k].view(torch.uint8), getattr(hy, k).view(torch.uint8)) for k in names)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10, help='reverse steps of the sampled trajectory (frames = steps + 1)')
    ap.add_argument('--graphs', type=int, default=128)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    dev = 'cuda'
    model = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to(dev)
    w = ligphore_workload(args.graphs)
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], w['num_atoms'], torch.zeros(args.graphs, 3),
                             rng='device', seed=1, num_steps=args.steps, return_traj=True)
    torch.cuda.synchronize()
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
    text = '\n'.join(lines) + '\n'
    print(text)
    print(json.dumps({'stereo_ms_final': rows[0][1][0], 'hydrogens_ms_final': rows[0][2][0], 'stereo_ms_traj': rows[1][1][0],
                      'hydrogens_ms_traj': rows[1][2][0], 'frames': args.steps + 1}))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
