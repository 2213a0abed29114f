#!/usr/bin/env python3
"""Timing of the fingerprint kernel (csrc/mol_fp.hip) next to the identity key kernel, and of the set kernels (csrc/fp_sim.hip) next
to the same results computed with torch on the same device; writes the table of profiles/mol_fp_timing.md.

  python tools/bench_fingerprints.py [--steps 1000] [--rows 16384] [--job_rows 102400] [--picks 1000] [--out FILE.md]

Kernel times are HIP events around the call alone (outputs allocated before), warm, median of repeats with the range.  (a) pg_mol_fp
and pg_mol_key on the final frame of the 128-graph headline batch and on its whole saved trajectory in one launch; (b) pg_fp_tanimoto
and pg_fp_nearest at rows x rows, pg_fp_nearest at job_rows x job_rows (the config-4 job's set), pg_fp_maxmin for `picks` of job_rows.
The torch yardstick unpacks the bits to fp16, takes the intersections with `matmul` and divides (in row blocks where the matrix would
not fit); pairs/s are held against the popcount form's bound of DESIGN.md 2.9, which is arithmetic, not a measurement."""
import time

import torch

from mol_bench import event_ms, headline_run, parser      # first: puts the repository root on sys.path
from bench_mol_key import key_kernel_ms
from phoregen_amd import hip, molecule as M, similarity as S

BOUND_PAIRS = 39e12 / 128         # lane-operations per second over the 64 v_and_b32 + 64 v_bcnt_u32_b32 of a pair


def fp_kernel_ms(sc, repeats, radius=M.FP_RADIUS):
    F, B = sc.status.shape
    fp = torch.empty(F, B, M.FP_WORDS, dtype=torch.int64, device=sc.cls.device)
    bits = torch.empty(F, B, dtype=torch.int32, device=sc.cls.device)
    lib = hip.lib()
    return event_ms(lambda: M._launch_fp(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms), radius, fp, bits), repeats, 2)


def random_rows(n, seed):
    """Sparse random rows, about 50 bits each (the corpus mean of tests/fp_reference.py), with every 97th row a copy of its neighbour."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    pos = torch.randint(0, M.FP_BITS, (n, 50), generator=g, device='cuda')
    rows = torch.zeros(n, M.FP_WORDS, dtype=torch.int64, device='cuda')
    one = torch.ones((), dtype=torch.int64, device='cuda')
    for k in range(pos.size(1)):
        rows.scatter_(1, (pos[:, k:k + 1] >> 6), rows.gather(1, pos[:, k:k + 1] >> 6) | (one << (pos[:, k:k + 1] & 63)))
    idx = torch.arange(97, n, 97, device='cuda')
    rows[idx] = rows[idx - 1]
    return rows.contiguous()


def unpack(rows):
    """fp16 [n, 2048] of int64 [n, 32]"""
    shifts = torch.arange(64, device=rows.device, dtype=torch.int64)
    return ((rows.unsqueeze(-1) >> shifts) & 1).reshape(rows.size(0), -1).to(torch.float16)


def torch_matrix(xa, xb, pa, pb):
    c = (xa @ xb.T).float()
    u = pa[:, None] + pb[None, :] - c
    return torch.where(u > 0, c / u, torch.ones_like(c))


def torch_nearest(xa, pa, block=8192):
    """Self nearest neighbour with row sums, in row blocks; (sim, index, sum)."""
    n = xa.size(0)
    sim, idx, tot = [], [], []
    for i0 in range(0, n, block):
        s = torch_matrix(xa[i0:i0 + block], xa, pa[i0:i0 + block], pa)
        r = torch.arange(i0, min(i0 + block, n), device=xa.device)
        diag = s[r - i0, r].double()
        tot.append(s.double().sum(1) - diag)
        s[r - i0, r] = -1.0
        m, j = s.max(1)
        sim.append(m), idx.append(j)
    return torch.cat(sim), torch.cat(idx), torch.cat(tot)


def torch_maxmin(xa, pa, k):
    n = xa.size(0)
    m = torch.full((n,), -1.0, device=xa.device)
    picked = torch.zeros(k, dtype=torch.long, device=xa.device)
    p = picked[0]
    for t in range(1, k):
        c = (xa @ xa[p]).float()
        u = pa + pa[p] - c
        m = torch.maximum(m, torch.where(u > 0, c / u, torch.ones_like(c)))
        m[p] = 2.0
        p = torch.argmin(m)
        picked[t] = p
    return picked


def main(argv=None):
    ap = parser()
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--job_rows', type=int, default=102400)
    ap.add_argument('--picks', type=int, default=1000)
    args = ap.parse_args(argv)
    dev = 'cuda'
    record = {}
    lines = ['# Fingerprints and similarity (`pg_mol_fp`, `pg_fp_tanimoto`, `pg_fp_nearest`, `pg_fp_maxmin`): timing', '',
             f'`python tools/bench_fingerprints.py --steps {args.steps} --rows {args.rows} --job_rows {args.job_rows} --picks {args.picks}` on '
             f'{torch.cuda.get_device_name(0)}.  HIP events around the call alone, warm, median (min .. max) of the repeats.  The bound is '
             'arithmetic, not a measurement: 128 lane-operations per pair (64 `v_and_b32`, 64 accumulating `v_bcnt_u32_b32`) against about '
             f'39 T lane-operations/s, {BOUND_PAIRS / 1e12:.2f} T pairs/s.  The torch column is the same result on the same device with the '
             'bits unpacked to fp16, the intersections by `matmul`, then the division.', '']

    # ---- (a) the fingerprint kernel beside the key kernel -------------------------------------------------------------------------
    _, _, res, _, _ = headline_run(args.graphs, args.steps, warm=False)
    lines += [f'## `pg_mol_fp` beside `pg_mol_key` ({args.graphs} graphs, radius {M.FP_RADIUS})', '',
              '| frames | `pg_mol_fp` ms | `pg_mol_key` ms |', '|---|---|---|']
    for frames, reps in (('final', 50), ('traj', 7)):
        sc = M.screen(res, frames=frames)
        f, k = fp_kernel_ms(sc, reps), key_kernel_ms(sc, reps)
        lines.append(f'| {sc.status.size(0)} | {f[0]:.3f} ({f[1]:.3f} .. {f[2]:.3f}) | {k[0]:.3f} ({k[1]:.3f} .. {k[2]:.3f}) |')
        record['fp_ms_' + frames], record['key_ms_' + frames] = f[0], k[0]
    del res, sc
    lines.append('')

    # ---- (b) the set kernels --------------------------------------------------------------------------------------------------------
    lib = hip.lib()
    lines += ['## The set kernels (random rows of about 50 bits)', '', '| call | ms | T pairs/s | of the bound | torch ms |', '|---|---|---|---|---|']

    def row(name, t, pairs, t_torch):
        rate = pairs / (t[0] * 1e-3)
        lines.append(f'| {name} | {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {rate / 1e12:.4f} | {100 * rate / BOUND_PAIRS:.1f} % | '
                     f'{t_torch[0]:.3f} ({t_torch[1]:.3f} .. {t_torch[2]:.3f}) |')
        record[name + ' ms'], record[name + ' torch ms'] = t[0], t_torch[0]

    n = args.rows
    a = random_rows(n, 1)
    xa = unpack(a)
    pa = xa.float().sum(1)
    out = torch.empty(n, n, dtype=torch.float32, device=dev)
    t = event_ms(lambda: hip.check(lib.pg_fp_tanimoto(a.data_ptr(), n, a.data_ptr(), n, out.data_ptr(), hip.stream_ptr())), 7, 2)
    tt = event_ms(lambda: torch_matrix(xa, xa, pa, pa), 7, 2)
    worst = (out - torch_matrix(xa, xa, pa, pa)).abs().max().item()
    row(f'`pg_fp_tanimoto` {n} x {n}', t, n * n, tt)
    near = S.nearest(a)
    t = event_ms(lambda: S.nearest(a), 7, 2)
    tt = event_ms(lambda: torch_nearest(xa, pa), 3, 2)
    ts, ti, tsum = torch_nearest(xa, pa)
    agree = [bool((near.sim == ts).all()), bool((near.index.long() == ti).all()), (near.sum - tsum).abs().max().item()]
    row(f'`pg_fp_nearest` {n} x {n} (self)', t, n * (n - 1), tt)
    del out, xa, pa, a

    n = args.job_rows
    a = random_rows(n, 2)
    xa = unpack(a)
    pa = xa.float().sum(1)
    t = event_ms(lambda: S.nearest(a), 3, warmup=1)
    tt = event_ms(lambda: torch_nearest(xa, pa), 1, warmup=1)
    row(f'`pg_fp_nearest` {n} x {n} (self)', t, n * (n - 1), tt)
    k = min(args.picks, n)
    picks = S.maxmin_pick(a, k)
    t = event_ms(lambda: S.maxmin_pick(a, k), 3, warmup=1)
    tt = event_ms(lambda: torch_maxmin(xa, pa, k), 1, warmup=0)
    same_picks = bool((picks.index.long() == torch_maxmin(xa, pa, k)).all())
    row(f'`pg_fp_maxmin` {k} of {n}', t, (k - 1) * n, tt)
    lines += ['', f'Agreement with the torch yardstick in this run: matrix max |difference| {worst:.3g} (the yardstick divides in fp32 as well), '
              f'nearest similarity equal {agree[0]}, index equal {agree[1]}, row sums max |difference| {agree[2]:.3g}; MaxMin picks equal '
              f'{same_picks} (torch.argmin and torch.max promise no tie rule, so equality is not required of them).', '',
              'No test asserts a time.  The int8 / fp8 matrix-core form on unpacked bits has not been built or measured.', '']
    text = '\n'.join(lines)                                            # this tool's report is a whole document and prints no JSON line
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    return text, record


if __name__ == '__main__':
    t0 = time.time()
    main()
    print(f'({time.time() - t0:.0f} s)')
