#!/usr/bin/env python3
"""Times phoregen_amd.shape.align (csrc/shape_align.hip): 1000 molecules against one reference, and 256 x 256 pairs.

  python tools/bench_shape_align.py [--repeats 7] [--colour] [--starts both]

The molecules are those of tools/bench_shape.py (tools/mol_bench.py's `synthetic_set`: the bench workload's atom counts, 40 on average; random walks).  Every case is warmed up
once, then timed `repeats` times with device events around one `align` call (the two frame launches and the overlay launch); the
median is reported, with the smallest and largest beside it.  Beside the time: the share of the pairs every start wins, the mean
evaluations the winning start used, the mean score, and evaluations/s counted as pairs x enabled starts x the winner's evaluations
(the other starts of a pair use about as many).  One JSON line per case."""
import argparse
import json

import torch

from mol_bench import event_ms, synthetic_set      # first: puts the repository root on sys.path
from phoregen_amd import shape


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--colour', action='store_true', help='sets with feature bytes, colour weight 0.5')
    ap.add_argument('--starts', choices=shape.START_NAMES, default='both')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_shape_align: no GPU visible; there is no CPU fallback and nothing to time')
    options, w = shape.AlignOptions(starts=args.starts), 0.5 if args.colour else 0.0
    n_starts = bin(options.mask()).count('1')
    records = []
    for name, na, nb in (('1000 x 1 reference', 1000, 1), ('256 x 256', 256, 256)):
        a, atoms_a = synthetic_set(na, 1, args.colour, 'cuda')
        b, atoms_b = synthetic_set(nb, 2, args.colour, 'cuda')
        med, lo, hi = event_ms(lambda: shape.align(a, b, colour_weight=w, options=options), args.repeats, 1)
        got = shape.align(a, b, colour_weight=w, options=options)
        wins = torch.bincount(got.start.long().clamp(min=0), minlength=5).double() / got.start.numel()
        steps = got.steps.double().mean().item()
        records.append({'case': name, 'pairs': na * nb, 'colour': args.colour, 'starts': args.starts, 'atoms_a': sum(atoms_a), 'atoms_b': sum(atoms_b),
                        'ms_median': round(med, 4), 'ms_min': round(lo, 4), 'ms_max': round(hi, 4), 'repeats': args.repeats,
                        'pairs_per_s': na * nb / (med * 1e-3), 'evaluations_per_s': na * nb * n_starts * steps / (med * 1e-3),
                        'mean_evaluations': round(steps, 2), 'start_wins': [round(x, 4) for x in wins.tolist()],
                        'mean_score': round(got.score.double().mean().item(), 6)})
        print(json.dumps(records[-1]))
    return '\n'.join(json.dumps(r) for r in records) + '\n', records


if __name__ == '__main__':
    main()
