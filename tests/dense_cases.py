"""Shapes, inputs and tolerances of the dense kernel tests, shared by the CPU part (tests/test_dense_host.py) and the GPU part
(tests/test_gpu_dense.py).  Everything is seeded torch-CPU data; no model, no device.

Profiles.  `exact`: every operand a small integer stored as fp32 (data, weights and gradients in -4 .. 4, bias, added operands and
prefilled accumulators in -64 .. 64), out_scale a power of two: every product and partial sum is an integer below 2^24, so the fp32
result does not depend on the summation order and must equal the float64 reference bit for bit.  `real`: randn operands, with one
constant row (2.5) and one all-zero row among the data rows.  `mean100`: data rows of mean 100, deviation 1 (LayerNorm's cancellation).

Shapes that depend on the device are functions of the compute-unit count `cu`; the host test evaluates them at NOMINAL_CU.

Tolerances.  Products are held to the derived bound of dense_reference.gemm_bound.  The two figures below cannot be derived; each is
FLOOR_MULT x the largest distance of the fp32 restatement (dense_reference.*_f32) from float64 over the cases, rounded up to one
digit, and tests/test_dense_host.py asserts restatement <= tolerance / FLOOR_MULT.  Neither comes from a kernel."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

NOMINAL_CU = 256
GUARD = 64
BAND_CAP = 0.01                # at most this share of a case's rows may hold a pre-activation inside the LayerNorm tolerance

# (a) absolute error of the shifted softplus on base-2 exp / log (pre-activations of the softplus cases, |v| up to ~60)
TOL_SSP = 7e-6
# (b) error of a LayerNorm(128)+ReLU'd operand: the largest of the errors of x_hat, of ReLU(x_hat gamma + beta) and of the adjoint gX
TOL_LN = {'real': 7e-6, 'mean100': 1.4e-4}


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def draw(profile, shape, g, kind='x'):
    """kind: 'x' data rows, 'w' weights / gradients, 'add' bias, added operands, prefilled accumulators."""
    if profile == 'exact':
        lim = 64 if kind == 'add' else 4
        return torch.randint(-lim, lim + 1, shape, generator=g).float()
    v = torch.randn(shape, generator=g)
    if profile == 'mean100' and kind == 'x':
        v = v + 100.0
    return v


def plant(X, profile):
    """`real`: one constant row and one all-zero row."""
    n = X.shape[0]
    if profile == 'real' and n >= 4:
        X[n // 3] = 2.5
        X[(2 * n) // 3] = 0.0
    return X


def gather_index(M, A, g):
    """[M] int32 in 0 .. A-1 that hits row 0 and row A-1 (as far as M allows)."""
    idx = torch.randint(0, A, (M,), generator=g).int()
    idx[0] = A - 1
    idx[M - 1] = 0 if M > 1 else A - 1
    return idx


# ---- streaming GEMM: the 20 instantiations ----
ADD_ROWS = 301


def stream_variants():
    out = []
    for NW in (4, 8):
        for nadd in (0, 1, 2):
            for kform in ('128', '128+20', '20'):
                out.append(NS(name=f'<{NW},{nadd},{kform}>', NW=NW, N=32 * NW, nadd=nadd, kform=kform, ln=False, ssp=False))
    out.append(NS(name='<4,0,128,LN>', NW=4, N=128, nadd=0, kform='128', ln=True, ssp=False))
    out.append(NS(name='<4,0,128,SSP>', NW=4, N=128, nadd=0, kform='128', ln=False, ssp=True))
    return out


def stream_per_cb(v, cu):
    return (2 if v.NW == 4 else 1) * cu          # N = 32 NW: one column block


def stream_Ms(v, cu):
    """64, 65, 127: the anchored last tile over (almost) all of the first; the tall one: 2.5 per_cb + 1 tiles, so workgroups run three
    tiles (stages 0, 1, 0) or two, the last tile is anchored and the trailing DMA is never consumed."""
    p = stream_per_cb(v, cu)
    return [64, 65, 127, 64 * (2 * p + p // 2) + 37]


def stream_profiles(v):
    return ('real', 'mean100') if v.ln else ('real',) if v.ssp else ('exact', 'real')


@functools.lru_cache(maxsize=4)
def stream_pool(N, M, profile):
    """Operands every instantiation of one (N, M, profile) draws from."""
    g = gen(7, N, M, len(profile))
    p = NS(M=M, N=N)
    p.X = plant(draw(profile, (M, 128), g), profile)
    p.X2 = draw('real' if profile == 'mean100' else profile, (M, 20), g)
    p.X20 = p.X2             # K = 20 alone: the same values as the X operand (which must be 16-byte aligned; X2 need not be)
    p.W = draw(profile, (N, 148), g, 'w')
    p.bias = draw(profile, (N,), g, 'add')
    p.add_idx = draw(profile, (ADD_ROWS, N), g, 'add')
    p.idx1 = gather_index(M, ADD_ROWS, g)
    p.add_own = draw(profile, (M, N), g, 'add')
    p.gamma, p.beta = torch.randn(128, generator=g), torch.randn(128, generator=g)
    return p


def stream_args(v, p):
    """Keyword arguments of dense_reference.gemm (and of the launch) for instantiation v on pool p."""
    a = dict(bias=p.bias)
    if v.kform == '128':
        a.update(X=p.X, W=p.W[:, :128])
    elif v.kform == '128+20':
        a.update(X=p.X, X2=p.X2, W=p.W)
    else:
        a.update(X=p.X20, W=p.W[:, 128:])
    if v.nadd == 1:
        a.update(add1=p.add_idx, idx1=p.idx1)
    elif v.nadd == 2:
        a.update(add1=p.add_own)
    if v.ln:
        a.update(ln=(p.gamma, p.beta), out_scale=0.5)
    if v.ssp:
        a.update(act=1)
    return a


# ---- tiled GEMM: the M x N x K grid, the remaining options drawn per combination (coverage asserted on the host) ----
TILED_M = (1, 127, 128, 129, 300)
TILED_N = (1, 12, 127, 130, 256)
TILED_K = ((128, 0), (18, 0), (18, 5), (128, 20), (130, 3), (7, 0))
BIAS_MODES = ('none', 'aligned', 'off1', 'off3')
ADD_MODES = ('none', 'own', 'idx')


def tiled_cases(K1, K2):
    out = []
    ki = TILED_K.index((K1, K2))
    for mi, M in enumerate(TILED_M):
        for ni, N in enumerate(TILED_N):
            i = (ki * 5 + mi) * 5 + ni
            r = np.random.RandomState(4242 + i)
            c = NS(M=M, N=N, K1=K1, K2=K2, seed=i, act=i % 3, scale=(0.5, 1.0)[(i // 3) % 2], bias=BIAS_MODES[r.randint(4)],
                   add1=ADD_MODES[r.randint(3)], add2=ADD_MODES[r.randint(3)], xoff=(4, 1)[r.randint(2)], woff=(4, 1)[r.randint(2)],
                   yoff=(4, 1)[r.randint(2)], addoff=(4, 1)[r.randint(4) == 0], ln=bool(K1 == 128 and K2 == 0 and r.randint(2)), rows=None)
            if c.ln:
                c.xoff = 4                                  # LayerNorm-on-load asks for 16-byte aligned rows
            out.append(c)
    return out


def tiled_extra():
    """What the grid leaves to chance: the 16-byte epilogue with a bias 1 and 3 floats off a 16-byte boundary, both gathered operands with
    different indices, ReLU, every alignment of the rest fixed to `vector`."""
    out = []
    for i, (M, N, bias, act) in enumerate(((129, 256, 'off1', 2), (129, 12, 'off3', 0), (300, 256, 'off3', 1), (127, 12, 'off1', 2),
                                           (128, 256, 'aligned', 2), (300, 12, 'none', 2))):
        out.append(NS(M=M, N=N, K1=18, K2=5, seed=900 + i, act=act, scale=(0.5, 1.0)[i % 2], bias=bias, add1='idx', add2='idx', xoff=4,
                      woff=4, yoff=4, addoff=4, ln=False, rows=None))
    return out


def rows_cases():
    """Row subsets: M logical rows, a shuffled subset of R rows; with and without LayerNorm-on-load; added operands without an index
    (they follow rows[r]) and with one."""
    out = []
    i = 0
    for ln in (False, True):
        for add1, add2 in (('own', 'own'), ('idx', 'own'), ('own', 'idx'), ('none', 'none')):
            for M, R, N in ((150, 300, 130), (129, 131, 128)):
                out.append(NS(M=M, N=N, K1=128, K2=0 if ln else (20, 0)[i % 2], seed=700 + i, act=(0, 2, 1)[i % 3], scale=(1.0, 0.5)[i % 2],
                              bias=BIAS_MODES[i % 4], add1=add1, add2=add2, xoff=4, woff=(4, 1)[i % 2], yoff=(4, 1)[(i // 2) % 2], addoff=4,
                              ln=ln, rows=R))
                i += 1
    return out


GEMM_ADD_ROWS = 53


def gemm_operands(c, profile):
    """CPU operands of one tiled-kernel case as keyword arguments of dense_reference.gemm."""
    g = gen(11, c.seed, len(profile))
    R = c.rows or c.M
    a = dict(X=plant(draw(profile, (R, c.K1), g), profile), W=draw(profile, (c.N, c.K1 + c.K2), g, 'w'), act=c.act, out_scale=c.scale)
    if c.K2:
        a['X2'] = draw('real' if profile == 'mean100' else profile, (R, c.K2), g)
    if c.bias != 'none':
        a['bias'] = draw(profile, (c.N,), g, 'add')
    if c.ln:
        a['ln'] = (torch.randn(128, generator=g), torch.randn(128, generator=g))
    if c.rows:
        a['rows'] = torch.randperm(R, generator=g)[:c.M].int()
    for k, mode in (('1', c.add1), ('2', c.add2)):
        if mode == 'own':
            a['add' + k] = draw(profile, (R, c.N), g, 'add')
        elif mode == 'idx':
            a['add' + k] = draw(profile, (GEMM_ADD_ROWS, c.N), g, 'add')
            a['idx' + k] = gather_index(c.M, GEMM_ADD_ROWS, g)
    return a


def gemm_profiles(c):
    if c.ln:
        return ('real', 'mean100')
    return ('real',) if c.act == 1 else ('exact', 'real')


# ---- pg_rows_linear ----
RL_K = (1, 63, 64, 65, 128, 200, 256)
RL_NOUT = (1, 7, 16)
RL_M = (1, 63, 64, 65)


def rows_linear_cases(cu):
    out = []
    i = 0
    for K in RL_K:
        for n_out in RL_NOUT:
            for M in RL_M:
                out.append(NS(K=K, n_out=n_out, M=M, seed=i, bias=bool(i % 3), rows=bool((i // 2) % 2), xoff=4, pad=(4, 3)[i % 2] if K != 128 else 4))
                i += 1
    tall = 64 * (8 * cu) + 37                      # K = 128, 16-byte aligned: workgroups of the matrix-pipe kernel take a second tile
    out += [NS(K=128, n_out=7, M=65, seed=500, bias=True, rows=False, xoff=1, pad=3),       # one float off: the wave kernel
            NS(K=128, n_out=16, M=65, seed=501, bias=False, rows=True, xoff=1, pad=3),
            NS(K=128, n_out=6, M=tall, seed=502, bias=True, rows=False, xoff=4, pad=0),     # ldx = 132
            NS(K=128, n_out=16, M=tall, seed=503, bias=False, rows=True, xoff=4, pad=0)]
    return out


def rows_linear_operands(c, profile):
    g = gen(13, c.seed, len(profile))
    R = c.M + 9 if c.rows else c.M
    a = dict(X=plant(draw(profile, (R, c.K), g), profile), W=draw(profile, (c.n_out, c.K), g, 'w'))
    if c.bias:
        a['b'] = draw(profile, (c.n_out,), g, 'add')
    if c.rows:
        a['rows'] = torch.randperm(R, generator=g)[:c.M].int()
    return a


# ---- pg_gemm_wgrad ----
def wgrad_split(M, N, K, cu):
    """`split` as pg_gemm_wgrad computes it."""
    bn, bk = (N + 63) // 64, (K + 63) // 64
    return max(1, min((8 * cu + bn * bk - 1) // (bn * bk), (M + 63) // 64))


def wgrad_cases(cu):
    bn_bk = 4 * 3
    split = (8 * cu + bn_bk - 1) // bn_bk
    M2 = 2 * 64 * split + 37                        # every z-block loops twice, the last chunk is partial
    assert wgrad_split(M2, 256, 148, cu) == split
    shapes = ((1, 1, 1), (63, 64, 64), (65, 130, 148), (200, 118, 12), (M2, 256, 148))
    out = []
    for i, (M, N, K) in enumerate(shapes):
        for j, (gb, yoff, xoff) in enumerate(((True, 4, 4), (False, 1, 4), (True, 4, 1))):
            out.append(NS(M=M, N=N, K=K, seed=10 * i + j, gb=gb, yoff=yoff, xoff=xoff, profiles=('exact', 'real') if M <= 300 else ('exact',)))
    return out


def wgrad_operands(c, profile):
    g = gen(17, c.seed, len(profile))
    a = dict(dY=draw(profile, (c.M, c.N), g, 'w'), X=draw(profile, (c.M, c.K), g), gW0=draw(profile, (c.N, c.K), g, 'add'))
    if c.gb:
        a['gb0'] = draw(profile, (c.N,), g, 'add')
    return a


# ---- pg_ln_relu, pg_ln_relu_bwd ----
def ln_Ms(cu, blocks_per_cu):
    return [1, 3, 4, 5, 1001, 4 * (blocks_per_cu * cu) + 37]


LN_FWD_PROFILES = ('real', 'mean100')
# the adjoint: `real` / `mean100` without constant rows (a zero-variance row multiplies every rounding by rstd = 316, which no tolerance of
# a LayerNorm'd OPERAND speaks for); `beta0`: beta = 0 and planted constant rows, whose pre-activations are exactly 0 -- mask closed, gX = 0
LN_BWD_PROFILES = ('real', 'mean100', 'beta0')


# seeds: chosen so that, at NOMINAL_CU, the rows of every adjoint case with a float64 pre-activation inside the tolerance stay under
# BAND_CAP (counted from the reference alone, tests/test_dense_host.py).  At mean 100 the tolerance is 20 times the `real` one, and
# with beta = 0 the pre-activations x_hat gamma crowd around 0: both sit near the cap in expectation
LN_SALT = {'real': 0, 'mean100': 17, 'beta0': 1}


def ln_operands(M, profile, bwd=False, sparse=False):
    """X, gamma, beta (+ integer gY for the adjoint; sparse: non-zero in 64 rows spread over the range, the last one included)."""
    g = gen(19, M, len(profile), int(bwd), LN_SALT[profile])
    X = draw('mean100' if profile == 'mean100' else 'real', (M, 128), g)
    gamma, beta = torch.randn(128, generator=g), torch.randn(128, generator=g)
    a = NS(X=X, gamma=gamma, beta=beta, planted=torch.zeros(M, dtype=torch.bool), tol=TOL_LN['mean100' if profile == 'mean100' else 'real'])
    if not bwd:
        plant(X, profile)
    if profile == 'beta0':
        a.beta = torch.zeros(128)
        rows = sorted({0, M // 3, (2 * M) // 3, M - 1}) if M >= 4 else [M - 1]
        for k, r in enumerate(rows):
            X[r] = (2.5, 0.0, -3.0, 100.0)[k % 4]
            a.planted[r] = True
    if bwd:
        a.gY = torch.randint(-4, 5, (M, 128), generator=g).float()
        if sparse:
            keep = torch.zeros(M, dtype=torch.bool)
            keep[torch.linspace(0, M - 1, 64).round().long()] = True
            a.gY[~keep] = 0.0
    return a


# ---- pg_attn_fold_wgrad, pg_attn_unfold_bias_grad ----
def fold_ns(cu):
    """1, 5; 4 (cu/2) + 3: the unrolled segment u = 1 is in range for three waves only; 16 (cu/2) 2 + 5: the outer loop runs twice
    and its second pass is ragged."""
    b = cu // 2
    return [1, 5, 4 * b + 3, 16 * b * 2 + 5]


def fold_operands(n, with_ids, profile):
    g = gen(23, n, int(with_ids), len(profile))
    R = n + 41 if with_ids else n
    a = NS(X=draw(profile, (R, 128), g), T=draw(profile, (R, 2048), g, 'w'), g0=draw(profile, (128 * 128,), g, 'add'), ids=None)
    if with_ids:
        a.ids = torch.randperm(R, generator=g)[:n].int()
    return a


def unfold_ns(cu):
    return [1, 5, 4 * (4 * cu) * 2 + 3]


def unfold_operands(n, with_ids, profile='exact'):
    g = gen(29, n, int(with_ids), len(profile))
    R = n + 41 if with_ids else n
    a = NS(gout=draw(profile, (R, 128), g, 'w'), swn=draw(profile, (R, 16), g), b2v=draw(profile, (128,), g, 'w'),
           gb0=draw(profile, (128,), g, 'add'), ids=None)
    if with_ids:
        a.ids = torch.randperm(R, generator=g)[:n].int()
    return a


# ---- pg_bond_rows_sum ----
def bond_batches(cu):
    """(ligand sizes, pharmacophore sizes, ncol): more than 4 x 8 cu ligand atoms at 8 columns (the atom loop repeats); the small ragged
    batch of tests/test_gpu_training.py at 260 columns (the column loop repeats)."""
    need = 4 * 8 * cu + 5
    sizes, cyc, k = [], (27, 1, 28, 33, 2, 29), 0
    while sum(sizes) < need:
        sizes.append(cyc[k % len(cyc)])
        k += 1
    return [(sizes, [3 + (i % 5) for i in range(len(sizes))], 8), ([5, 1, 17, 33, 2, 16], [4, 9, 3, 12, 7, 5], 260)]
