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

import torch

from mol_bench import event_ms, synthetic_set      # first: puts the repository root on sys.path
from phoregen_amd import shape


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1000, 4000])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--colour', action='store_true', help='sets with feature bytes: the colour overlap is computed too')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_shape: no GPU visible; there is no CPU fallback and nothing to time')
    records = []
    for n in args.sizes:
        a, na = synthetic_set(n, 1, args.colour, 'cuda')
        b, nb = synthetic_set(n, 2, args.colour, 'cuda')
        terms = sum(na) * sum(nb) * (2 if args.colour else 1)
        for name, fn in (('similarity', lambda: shape.similarity(a, b)), ('nearest', lambda: shape.nearest(a, b, colour_weight=0.5 if args.colour else 0.0))):
            med, lo, hi = event_ms(fn, args.repeats, 1)                # one warm-up of this shape
            records.append({'function': name, 'n_a': n, 'n_b': n, 'colour': args.colour, 'atoms_a': sum(na), 'atoms_b': sum(nb),
                            'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'repeats': args.repeats,
                            'pairs_per_s': n * n / (med * 1e-3), 'exponentials_per_s': terms / (med * 1e-3)})
            print(json.dumps(records[-1]))
    return '\n'.join(json.dumps(r) for r in records) + '\n', records


if __name__ == '__main__':
    main()
