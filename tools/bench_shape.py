#!/usr/bin/env python3
"""Times phoregen_amd.shape.similarity and .nearest on two synthetic sets of n molecules each (csrc/shape_sim.hip).

  python tools/bench_shape.py [--sizes 1000 4000] [--repeats 7] [--colour]

Atom counts are the bench workload's, clamp(round(N(40, 6^2)), 20, 60); a molecule is a random walk with 1.3 .. 1.6 Angstrom steps
around a centre drawn within 1 Angstrom of the origin, carbon-heavy mixed elements, random feature bytes.  Every shape is warmed up
once, then timed `repeats` times with device events (one event pair around one call, so a time includes the launch and, for nearest,
the combining launch); the median is reported, with the smallest and largest beside it.  A pair of molecules with n_a and n_b atoms
needs n_a * n_b shape terms, one exponential each, and with --colour as many colour terms again: exponentials/s is that count over
the median time.  One JSON line per (function, size)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phoregen_amd import shape  # noqa: E402


def synthetic_set(n, seed, colour, device):
    g = torch.Generator().manual_seed(seed)
    n_at = (40 + 6 * torch.randn(n, generator=g)).round().clamp(20, 60).long().tolist()
    rng = np.random.default_rng(seed)
    p = np.array([1, 30, 8, 8, 2, 1, 1, 2, 2, 1, 1]) / 57.0
    mols = []
    for k in n_at:
        step = rng.normal(size=(k, 3))
        step *= rng.uniform(1.3, 1.6, size=(k, 1)) / np.linalg.norm(step, axis=1, keepdims=True)
        pos = np.cumsum(step, axis=0)
        m = {'element': [shape.ATOM_TYPES[c] for c in rng.choice(11, size=k, p=p)],
             'atom_pos': (pos - pos.mean(axis=0) + rng.normal(0, 1.0, size=3)).astype(np.float32)}
        if colour:
            m['features'] = {'atom_fp': rng.integers(0, 128, size=k).astype(np.uint8)}
        mols.append(m)
    return shape.from_molecules(mols, device), n_at


def timed(fn, repeats):
    fn()                                                               # warm-up of this shape
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1000, 4000])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--colour', action='store_true', help='sets with feature bytes: the colour overlap is computed too')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_shape: no GPU visible; there is no CPU fallback and nothing to time')
    for n in args.sizes:
        a, na = synthetic_set(n, 1, args.colour, 'cuda')
        b, nb = synthetic_set(n, 2, args.colour, 'cuda')
        terms = sum(na) * sum(nb) * (2 if args.colour else 1)
        for name, fn in (('similarity', lambda: shape.similarity(a, b)), ('nearest', lambda: shape.nearest(a, b, colour_weight=0.5 if args.colour else 0.0))):
            med, lo, hi = timed(fn, args.repeats)
            print(json.dumps({'function': name, 'n_a': n, 'n_b': n, 'colour': args.colour, 'atoms_a': sum(na), 'atoms_b': sum(nb),
                              'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'repeats': args.repeats,
                              'pairs_per_s': n * n / (med * 1e-3), 'exponentials_per_s': terms / (med * 1e-3)}))


if __name__ == '__main__':
    main()
