#!/usr/bin/env python3
"""Timing of the substructure search (csrc/mol_sub.hip, phoregen_amd/substructure.py) on the headline batch; writes the table of
profiles/mol_sub_timing.md.

  python tools/bench_mol_sub.py [--steps 1000] [--out FILE.md]

Two batches of the headline shape (128 graphs, the workload's atom counts) against tables of P = 1, 16 and 256 patterns -- (a) the
final prediction of the sampler with the deterministic noise weights, whose graphs are close to cliques, so that every root runs
into the work bound: the worst case; (b) tools/mol_bench.py's molecule-like graphs (a random tree of degree at most 4 with a few ring
closures per graph, mostly carbon, mostly single bonds), where nothing is cut short.  The tables: the 6-cycle of any atoms alone;
the paths of 2 .. 16 any-atoms and the 6-cycle; those sixteen repeated sixteen times under other names.  Kernel times are HIP events
around the launch alone (table and outputs on the device before), warm, median of repeats; next to them the wall time of
`substructure()` with the screen, the rings and the Kekulé form handed in.  There is no target: the numbers are recorded, not gated."""
import torch

from mol_bench import event_ms, headline_run, molecule_like, parser, report, wall_ms      # first: puts the repository root on sys.path
from phoregen_amd import hip, molecule as M, substructure as S


def pattern_lists():
    cycle = {'name': 'cycle6', 'atoms': [{}] * 6, 'bonds': [{'a': min(i, (i + 1) % 6), 'b': max(i, (i + 1) % 6)} for i in range(6)]}
    sixteen = [{'name': 'path%d' % n, 'atoms': [{}] * n, 'bonds': [{'a': i, 'b': i + 1} for i in range(n - 1)]} for n in range(2, 17)] + [cycle]
    many = [dict(p, name='%s_%d' % (p['name'], r)) for r in range(16) for p in sixteen]
    return {1: [cycle], 16: sixteen, 256: many}


def kernel_ms(sc, rg, kek, patterns, max_steps, repeats, warmup=3):
    """Median / min / max of `repeats` event-timed launches, after `warmup` launches; and the outputs."""
    dev = sc.cls.device
    F, B = sc.status.shape
    P = len(patterns)
    host = S.pattern_table(patterns)
    table = torch.from_numpy(host).to(dev)
    out = dict(embeddings=torch.empty(F, B, P, dtype=torch.int32, device=dev), anchors=torch.empty(F, B, P, dtype=torch.int32, device=dev),
               atom_mask=torch.empty(F, B, P, 2, dtype=torch.int64, device=dev), first=torch.empty(F, B, P, S.MAX_ATOMS, dtype=torch.int16, device=dev),
               status=torch.empty(F, B, P, dtype=torch.int32, device=dev))
    lib = hip.lib()
    return event_ms(lambda: S._launch_sub(lib, sc, rg, kek, B, F, max(sc.num_atoms), table, host, P, max_steps, out), repeats, warmup), out


def main(argv=None):
    ap = parser(steps_help='reverse steps of the sampler')
    ap.add_argument('--max_steps', type=int, default=S.DEFAULT_STEPS)
    ap.add_argument('--repeats', type=int, default=30)
    args = ap.parse_args(argv)
    dev = 'cuda'
    _, w, res, _, _ = headline_run(args.graphs, args.steps, warm=False)      # the trajectory is kept, as sample_batch does by default
    lines, record = [], {}
    for tag, title, batch in (('a', '(a) the sampler\'s final prediction, noise weights', res),
                              ('b', '(b) molecule-like graphs', molecule_like([int(n) for n in w['num_atoms'].tolist()], dev))):
        sc = M.screen(batch)
        rg, kek = M.rings(batch, screen=sc), M.kekulize(batch, screen=sc)
        lines += ['## ' + title, '',
                  '| patterns | kernel ms, median (min - max) | us per (graph, pattern) | `substructure()` wall ms | rows matched | rows truncated |',
                  '|---|---|---|---|---|---|']
        for P, dicts in pattern_lists().items():
            patterns = [S.Pattern.from_dict(d) for d in dicts]
            k3, out = kernel_ms(sc, rg, kek, patterns, args.max_steps, args.repeats)
            wall = wall_ms(lambda: S.substructure(batch, patterns, screen=sc, rings=rg, kekule=kek, max_steps=args.max_steps), 10)
            matched = int(((out['status'] & S.SUB_MATCHED) != 0).sum())
            truncated = int(((out['status'] & S.SUB_TRUNCATED) != 0).sum())
            lines.append('| %d | %.3f (%.3f - %.3f) | %.3f | %.3f (%.3f - %.3f) | %d of %d | %d |' %
                         ((P,) + k3 + (k3[0] * 1e3 / (args.graphs * P),) + wall + (matched, args.graphs * P, truncated)))
            record['kernel_ms_%s_P%d' % (tag, P)] = k3[0]
        lines += ['', 'The batch: %d graphs, %d atom rows, %d kept atoms, %d bonds, %d valid graphs; max_steps %d.' %
                  (args.graphs, sc.cls.size(1), int(sc.counts[0, :, 0].sum()), int(sc.counts[0, :, 1].sum()), int(sc.valid.sum()), args.max_steps), '']
    lines += ['(a) was sampled with %d reverse steps.' % args.steps]
    return report(lines, record, args.out)


if __name__ == '__main__':
    main()
