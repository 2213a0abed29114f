#!/usr/bin/env python3
"""Cost of fragment-conditioned sampling on the headline batch (bench.py's workload: BASELINE config 3 shape, 128 graphs): the
pipelined sampler loop with and without an 8-atom fragment on every graph, runs alternating, median of 3 each.  Prints one JSON
line with ms/step of both and the relative overhead.

  python tools/bench_fragment.py [--graphs 128] [--steps 50] [--warmup 10] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ligphore_workload  # noqa: E402
from phoregen_amd.config import default_model_config  # noqa: E402
from phoregen_amd.fragment import Fragment  # noqa: E402
from phoregen_amd.models.diffusion import PhoreDiff  # noqa: E402
from phoregen_amd.weights import init_deterministic_  # noqa: E402


def fragment8():
    """a benzene ring with a carboxyl group: 8 heavy atoms, aromatic bonds as class 4"""
    import math
    ring = [[1.39 * math.cos(k * math.pi / 3), 1.39 * math.sin(k * math.pi / 3), 0.0] for k in range(6)]
    pos = ring + [[2.90, 0.0, 0.0], [3.50, 1.05, 0.0]]
    bonds = [(k, (k + 1) % 6, 4) for k in range(6)] + [(0, 6, 1), (6, 7, 2)]
    return Fragment.from_dict({'element': [6] * 7 + [8], 'pos': pos, 'bonds': bonds})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=128)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    dev = 'cuda'
    model = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to(dev)
    work = ligphore_workload(args.graphs, seed=1234)
    B = args.graphs
    frags = [fragment8()] * B
    T = model.num_timesteps

    def run(fragments):
        st = model.begin_sampling(work['h_phore'], work['pos_phore'], work['phore_norm'], work['batch_phore'], work['num_atoms'],
                                  torch.zeros(B, 3), rng='device', seed=0, return_traj=True,
                                  num_steps=args.warmup + args.steps, pipeline=True, fragments=fragments)
        for i in range(args.warmup):
            model.reverse_step(st, i, T - 1 - i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.warmup, args.warmup + args.steps):
            model.reverse_step(st, i, T - 1 - i)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps * 1e3
        model.finish_sampling(st)
        return dt

    times = {'plain': [], 'fragment': []}
    for _ in range(args.repeats):
        times['plain'].append(run(None))
        times['fragment'].append(run(frags))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({'metric': 'sampler ms/step, headline batch, with / without an 8-atom fragment on every graph',
                      'graphs': B, 'n_lig': int(work['num_atoms'].sum()), 'steps': args.steps, 'warmup': args.warmup,
                      'plain_ms_per_step': med['plain'], 'fragment_ms_per_step': med['fragment'],
                      'overhead_pct': 100.0 * (med['fragment'] / med['plain'] - 1.0),
                      'repeats_ms_per_step': times}))


if __name__ == '__main__':
    main()
