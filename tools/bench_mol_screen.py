#!/usr/bin/env python3
"""Timing of the molecule screen (csrc/mol_screen.hip, phoregen_amd/molecule.py) on the headline batch; writes the table of
profiles/mol_screen_timing.md.

  python tools/bench_mol_screen.py [--steps 1000] [--out FILE.md]

(a) final prediction of the 128-graph headline batch, (b) its whole saved trajectory in ONE launch, (c) the final prediction
tiled 32 x to 4096 graphs (the atom-count distribution of BASELINE config 4).  Kernel times are HIP events around the launch alone
(outputs allocated before), warm, median of repeats; next to them the wall time of what a caller pays today: `decode_batch` for (a)
and (c), and for (b) a frame-by-frame loop, both as one launch per frame and as `decode_batch` per frame (a few frames timed,
scaled to all).  Next to every kernel time stands the distance bond screen's (pg_mol_screen_dist, csrc/mol_screen_dist.hip;
`screen(bonds='distance')`, without the agreement counts) on the same tensors in the same process, and the ratio of the two medians."""
import torch

from mol_bench import event_ms, fmt, headline_run, parser, report, wall_ms      # first: puts the repository root on sys.path
from phoregen_amd import hip, molecule as M
from phoregen_amd.plan import make_edge_data
from phoregen_amd.utils.sample_utils import decode_batch


def _buffers(F, B, N, E, dev):
    return dict(status=torch.empty(F, B, dtype=torch.int32, device=dev), counts=torch.empty(F, B, 4, dtype=torch.int32, device=dev),
                cls=torch.empty(F, N, dtype=torch.int8, device=dev), compact=torch.empty(F, N, dtype=torch.int16, device=dev),
                valence2=torch.empty(F, N, dtype=torch.uint8, device=dev), comp=torch.empty(F, N, dtype=torch.int16, device=dev),
                order=torch.empty(F, E // 2, dtype=torch.int8, device=dev))


def kernel_ms(node, pos, edge, F, strides, sc, repeats, warmup=3, dist=False):
    """Median / min / max of `repeats` event-timed launches over F frames (strides in elements), after `warmup` launches.
    dist: pg_mol_screen_dist (no edge scores, no agreement counts) instead of pg_mol_screen."""
    B, N, E = len(sc.num_atoms), node.size(-2), edge.size(-2)
    out = _buffers(F, B, N, E, node.device)
    lib = hip.lib()

    thresholds = M._bond_threshold_table(M.BondMargins(), node.device)

    def go():
        if dist:
            M._launch_dist(lib, node, strides[0], pos, strides[2], None, 0, sc.lig_off, sc.bond_off, B, F, N, E, max(sc.num_atoms),
                           thresholds, out, None)
        else:
            M._launch(lib, node, strides[0], edge, strides[1], pos, strides[2], sc.lig_off, sc.bond_off, B, F, N, E, max(sc.num_atoms), out)
    return event_ms(go, repeats, warmup) + (out,)


def traffic_bytes(sc, F):
    """Bytes the kernel must move per call: scores and coordinates read (first half of the bond rows only), outputs written."""
    N, H = sum(sc.num_atoms), sum(n * (n - 1) // 2 for n in sc.num_atoms)
    return F * (N * (48 + 12 + 6) + H * (24 + 1) + len(sc.num_atoms) * 20)


def main(argv=None):
    ap = parser()
    ap.add_argument('--tile', type=int, default=32, help='(c): the final prediction repeated this many times')
    args = ap.parse_args(argv)
    dev = 'cuda'
    _, _, res, t_sample, _ = headline_run(args.graphs, args.steps, warm=False)
    rows = []

    # (a) final prediction
    sc = M.screen(res)
    node, pos, edge = res['pred']
    k = kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50)
    dist_ms = [kernel_ms(node, pos, edge, 1, (0, 0, 0), sc, 50, dist=True)]
    assert torch.equal(dist_ms[0][3]['order'], M.screen(res, bonds='distance').order)
    rows.append(('(a) final frame, %d graphs' % args.graphs, 1, k[:3], traffic_bytes(sc, 1),
                 wall_ms(lambda: M.screen(res), 10), wall_ms(lambda: M.assemble(res), 10), wall_ms(lambda: decode_batch(res), 10)))
    valid_final = int(sc.valid.sum())

    # (b) the whole trajectory in one launch
    tn, tp, te = res['traj']
    F = tn.size(0)
    strides = (tn.stride(0), te.stride(0), tp.stride(0))
    kb = kernel_ms(tn, tp, te, F, strides, sc, 7, warmup=2)
    dist_ms.append(kernel_ms(tn, tp, te, F, strides, sc, 7, warmup=2, dist=True))
    sct = M.screen(res, frames='traj')
    assert torch.equal(sct.status, kb[3]['status']) and torch.equal(sct.order, kb[3]['order'])
    first_valid = [int(v) for v in (sct.valid.int().argmax(0) + F * (~sct.valid.any(0)).int()).tolist()]    # F = never
    # frame by frame, one launch each (what a caller without the frame stride would do); 50 frames timed, scaled
    nf = min(F, 50)
    out1 = _buffers(1, len(sc.num_atoms), node.size(0), edge.size(0), node.device)
    lib = hip.lib()

    def per_frame_launches():
        for f in range(F - nf, F):
            M._launch(lib, tn[f], 0, te[f], 0, tp[f], 0, sc.lig_off, sc.bond_off, len(sc.num_atoms), 1, node.size(0), edge.size(0),
                      max(sc.num_atoms), out1)
    pf = wall_ms(per_frame_launches, 5)
    # frame by frame on the host path of today: decode_batch of a frame; 3 frames timed, scaled
    frames3 = [F - 1, F // 2, 0][:min(3, F)]

    def per_frame_decode():
        for f in frames3:
            decode_batch(dict(res, pred=[tn[f], tp[f], te[f]]))
    pd = wall_ms(per_frame_decode, 3)
    rows.append(('(b) trajectory, %d frames x %d graphs, ONE launch' % (F, args.graphs), F, kb[:3], traffic_bytes(sc, F),
                 wall_ms(lambda: M.screen(res, frames='traj'), 5), None, None))

    # (c) 4096 graphs: the final prediction tiled
    big = {'pred': [t.repeat(args.tile, 1) for t in res['pred']], 'traj': [None, None, None],
           'lig_info': [res['lig_info'][0].repeat(args.tile)] + [None] * 3}
    big['lig_info'][2] = make_edge_data(big['lig_info'][0].cpu())[0].to(dev)
    scc = M.screen(big)
    kc = kernel_ms(*big['pred'], 1, (0, 0, 0), scc, 30)
    dist_ms.append(kernel_ms(*big['pred'], 1, (0, 0, 0), scc, 30, dist=True))
    assert torch.equal(scc.status[0, :args.graphs], sc.status[0])
    rows.append(('(c) final frame, %d graphs' % (args.graphs * args.tile), 1, kc[:3], traffic_bytes(scc, 1),
                 wall_ms(lambda: M.screen(big), 5), wall_ms(lambda: M.assemble(big), 5), wall_ms(lambda: decode_batch(big), 5)))

    dash = lambda t: '-' if t is None else fmt(t)   # noqa: E731
    lines = ['| case | kernel ms, median (min - max) | GB/s of needed traffic | `screen()` wall ms | `assemble()` wall ms | `decode_batch()` wall ms '
             '| `pg_mol_screen_dist` kernel ms | dist / screen |',
             '|---|---|---|---|---|---|---|---|']
    for (name, _, k3, nbytes, ws, wa, wd), d in zip(rows, dist_ms):
        lines.append('| %s | %s | %.0f | %s | %s | %s | %s | %.2f |' % (name, fmt(k3), nbytes / k3[0] / 1e6, fmt(ws), dash(wa), dash(wd), fmt(d),
                                                                     d[0] / k3[0]))
    lines += ['',
              'Trajectory frame by frame instead of one launch (scaled to %d frames): one launch per frame %.1f ms wall (%d frames timed: %.3f ms); '
              '`decode_batch` per frame %.0f ms wall (%d frames timed: %.1f ms).' %
              (F, pf[0] * F / nf, nf, pf[0], pd[0] * F / len(frames3), len(frames3), pd[0]),
              '',
              'Sampling the batch with its trajectory took %.1f s.  Valid graphs of the final prediction (deterministic noise weights): %d of %d; '
              'graphs with a valid frame anywhere in the trajectory: %d.' %
              (t_sample, valid_final, args.graphs, sum(v < F for v in first_valid))]
    return report(lines, {'dist_kernel_ms': [d[0] for d in dist_ms], 'kernel_ms_final': rows[0][2][0], 'kernel_ms_traj': rows[1][2][0],
                          'kernel_ms_4096': rows[2][2][0], 'frames': F, 'per_frame_launch_ms_scaled': pf[0] * F / nf,
                          'per_frame_decode_ms_scaled': pd[0] * F / len(frames3)}, args.out)


if __name__ == '__main__':
    main()
