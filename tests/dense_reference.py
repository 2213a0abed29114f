"""float64 restatements of the dense kernels (phoregen_amd/csrc/gemm.hip, gemm_stream.hip, train_ops.hip), one output element at a
time, and the error bound each fp32 kernel is asked to meet.

TEST INFRASTRUCTURE: torch tensor algebra only, nothing of the product.  Every function widens the fp32 operands it is given to float64
and works on whatever device they live on (the tall streaming cases are evaluated on the GPU, everything else on the host), so the
result is the exact answer to the question the kernel is asked.  The `*_f32` functions restate the two expressions whose fp32 error
cannot be derived -- the shifted softplus and LayerNorm+ReLU with its adjoint -- in numpy fp32 (sums by numpy's fp32 reduction: eight running sums
combined by a tree, the shape of the kernels' own lane-then-shuffle sums); they
measure what fp32 rounding of the expression itself costs (tests/test_dense_host.py) and never see a kernel.

Bounds.  A product of K terms plus bias and added operands, summed in any order in fp32 with every operation rounded to within one
whole ulp (2^-23 relative) of its result: at most K + 3 roundings of partial sums none of which exceeds S = sum_k |x_k||w_k| + |bias|
+ |add1| + |add2| by more than the error itself, so |Y - ref| <= |out_scale| (K + 4) 2^-23 S.  The bound owes nothing to the order
of summation or to the rounding mode of the matrix pipe."""
import numpy as np
import torch

U = 2.0 ** -23                       # one whole fp32 ulp, relative
LN_EPS = 1e-5
LN2 = 0.6931471805599453
f64 = torch.float64


def _d(t):
    return None if t is None else t.to(f64)


def _l(t):
    return None if t is None else t.long()


# ---- forward pieces ----
def layer_norm_hat(X):
    """(x_hat, rstd) of LayerNorm over the last dimension (biased variance, eps 1e-5) in float64."""
    X = _d(X)
    mu = X.mean(-1, keepdim=True)
    d = X - mu
    rs = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + LN_EPS)
    return d * rs, rs


def ln_relu(X, gamma, beta):
    h, _ = layer_norm_hat(X)
    return torch.clamp(h * _d(gamma) + _d(beta), min=0.0)


def ssp(v):
    """Shifted softplus of models/common.py:58-64: softplus(v) - ln 2 (float64: no threshold needed below 700)."""
    v = _d(v)
    return torch.clamp(v, min=0.0) + torch.log1p(torch.exp(-v.abs())) - LN2


def gemm(X, W, X2=None, bias=None, ln=None, add1=None, idx1=None, add2=None, idx2=None, act=0, out_scale=1.0, rows=None):
    """pg_gemm as include/phoregen_hip.h states it, for the logical rows r = 0 .. M-1 (the caller places row r at Y row rows[r]).
    Returns (Y, S, Wln): the float64 result, S = sum_k |x_k||w_k| + |bias| + |add1| + |add2| of every element, and
    Wln[n] = sum_{k < K1} |W[n,k]| when the X rows went through LayerNorm+ReLU (the weight of that operand's error), else None."""
    W = _d(W)
    r = _l(rows)
    A = _d(X) if r is None else _d(X)[r]
    wln = None
    if ln is not None:
        A = ln_relu(A, ln[0], ln[1])
        wln = W[:, :A.shape[1]].abs().sum(1)
    if X2 is not None:
        A = torch.cat([A, _d(X2) if r is None else _d(X2)[r]], 1)
    assert A.shape[1] == W.shape[1]
    pre = A @ W.T
    S = A.abs() @ W.abs().T
    M = A.shape[0]
    own = torch.arange(M, device=A.device) if r is None else r
    if bias is not None:
        pre = pre + _d(bias)
        S = S + _d(bias).abs()
    for add, idx in ((add1, idx1), (add2, idx2)):
        if add is not None:
            g = _d(add)[own if idx is None else _l(idx)]
            pre = pre + g
            S = S + g.abs()
    y = ssp(pre) if act == 1 else torch.clamp(pre, min=0.0) if act == 2 else pre
    return y * out_scale, S, wln


def gemm_bound(S, K, out_scale=1.0, wln=None, delta=0.0, tol_act=0.0):
    """Per-element bound of pg_gemm: the derived product bound, plus delta * sum_k |w_k| for a LayerNorm+ReLU'd operand known to
    delta, plus the absolute error of the softplus evaluation.  ReLU and the softplus are 1-Lipschitz: the bound of the
    pre-activation carries over."""
    b = (K + 4) * U * S
    if wln is not None:
        b = b + delta * wln
    return abs(out_scale) * (b + tol_act)


def rows_linear(X, W, b=None, rows=None):
    """pg_rows_linear: Y[r] = X[rows[r]] W^T + b (row r of Y, not rows[r]).  Returns (Y, S)."""
    A = _d(X) if rows is None else _d(X)[_l(rows)]
    Y, S = A @ _d(W).T, A.abs() @ _d(W).abs().T
    if b is not None:
        Y, S = Y + _d(b), S + _d(b).abs()
    return Y, S


# ---- adjoints ----
def gemm_wgrad(dY, X, gW0=None, gb0=None):
    """pg_gemm_wgrad: gW[n,k] (+=) sum_r dY[r,n] X[r,k], gb[n] (+=) sum_r dY[r,n].  Returns (gW, gb, S_W, S_b)."""
    dY, X = _d(dY), _d(X)
    gW, SW = dY.T @ X, dY.abs().T @ X.abs()
    gb, Sb = dY.sum(0), dY.abs().sum(0)
    if gW0 is not None:
        gW, SW = gW + _d(gW0), SW + _d(gW0).abs()
    if gb0 is not None:
        gb, Sb = gb + _d(gb0), Sb + _d(gb0).abs()
    return gW, gb, SW, Sb


def ln_relu_bwd(X, gamma, beta, gY, band=0.0):
    """Adjoint of Y = ReLU(LN(X) gamma + beta).  Returns a dict: gX under the reference's own mask (pre > 0), gX_alt under the mask
    that also opens (pre <= 0) or closes (pre > 0) every element whose |pre| < band, ggamma / gbeta over the elements outside the
    band, the absolute sums S_gamma / S_beta of those terms, the widening W_gamma / W_beta = sum of |gY h| / |gY| over the in-band
    elements, `band_rows` (bool per row) and `pre`."""
    h, rs = layer_norm_hat(X)
    ga, gY = _d(gamma), _d(gY)
    pre = h * ga + _d(beta)
    inband = (pre.abs() < band) & (pre != 0)          # (a pre-activation of exactly 0 is planted, and decided: `> 0.f` is false)
    out = dict(pre=pre, h=h, band_rows=inband.any(1), inband=inband)

    def gx(mask):
        a = gY * mask * ga
        return rs * (a - a.mean(-1, keepdim=True) - h * (a * h).mean(-1, keepdim=True))

    m = (pre > 0).to(f64)
    out['gX'] = gx(m)
    out['gX_alt'] = gx(torch.where(inband, 1.0 - m, m))
    keep = m * (~inband)
    out['ggamma'], out['gbeta'] = (gY * h * keep).sum(0), (gY * keep).sum(0)
    out['S_gamma'], out['S_beta'] = (gY * h * keep).abs().sum(0), (gY * keep).abs().sum(0)
    out['W_gamma'], out['W_beta'] = (gY * h * inband).abs().sum(0), (gY * inband).abs().sum(0)
    return out


def fold_slots():
    """(column of X, column of T) behind every element of the flat gW2_l of pg_attn_fold_wgrad, as documented in train_ops.hip:
    gW2_l[((2i + half) * 64 + lane) * 4 + j] = sum_s X[s, 8 (lane & 15) + 4 half + j] * T[s, 64 i + lane], i = 0 .. 31."""
    i, half, lane, j = torch.meshgrid(torch.arange(32), torch.arange(2), torch.arange(64), torch.arange(4), indexing='ij')
    return (8 * (lane & 15) + 4 * half + j).reshape(-1), (64 * i + lane).reshape(-1)


def fold_wgrad(X, T, ids=None, g0=None):
    """pg_attn_fold_wgrad over the rows `ids` (all rows if None) as an einsum over the documented layout.  Returns (gW2_l, S)."""
    X, T = _d(X), _d(T)
    if ids is not None:
        X, T = X[_l(ids)], T[_l(ids)]
    n = X.shape[0]
    Xg = X.reshape(n, 16, 2, 4)                                 # [s, m, half, j]
    Tg = T.reshape(n, 32, 4, 16)                                # [s, i, g, m]  (lane = 16 g + m)
    g = torch.einsum('smhj,sigm->ihgmj', Xg, Tg).reshape(-1)
    S = torch.einsum('smhj,sigm->ihgmj', Xg.abs(), Tg.abs()).reshape(-1)
    if g0 is not None:
        g, S = g + _d(g0).reshape(-1), S + _d(g0).reshape(-1).abs()
    return g, S


def unfold_bias_grad(gout, swn, b2v, ids=None, gb0=None):
    """pg_attn_unfold_bias_grad: gswn[s, h] = sum_d gout[s, 8h+d] b2v[8h+d] on the rows `ids`; gb2v[c] (+=) sum_s gout[s, c] swn[s, c >> 3].
    Returns (rows, gswn[rows], gb2v, S_swn, S_b)."""
    gout, swn, b2v = _d(gout), _d(swn), _d(b2v)
    rows = torch.arange(gout.shape[0]) if ids is None else _l(ids)
    g = gout[rows]
    p = g * b2v
    gswn, Ss = p.reshape(-1, 16, 8).sum(-1), p.abs().reshape(-1, 16, 8).sum(-1)
    t = g * swn[rows].repeat_interleave(8, 1)
    gb, Sb = t.sum(0), t.abs().sum(0)
    if gb0 is not None:
        gb, Sb = gb + _d(gb0), Sb + _d(gb0).abs()
    return rows, gswn, gb, Ss, Sb


def bond_rows_sum(Y, index, n_ctx):
    """pg_bond_rows_sum: out[index[e]] += Y[e] (index = bond_src or bond_dst, context rows)."""
    Y = _d(Y)
    return torch.zeros(n_ctx, Y.shape[1], dtype=f64, device=Y.device).index_add_(0, _l(index), Y)


# ---- fp32 restatements (numpy) ----
f32 = np.float32


def _sum32(a):
    return np.sum(a, axis=-1, keepdims=True, dtype=f32)


def ssp_f32(v):
    """The kernels' form: log(1 + e^v) through base-2 exponential and logarithm, threshold 20, minus ln 2."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(over='ignore'):                      # e^v = inf above v = 88: that branch is not taken
        e = np.exp2(v * f32(1.4426950408889634)).astype(f32)
    sp = np.where(v > f32(20.0), v, np.log2(f32(1.0) + e).astype(f32) * f32(LN2))
    return (sp - f32(LN2)).astype(f32)


def ln_hat_f32(X):
    X = np.asarray(X, dtype=f32)
    mu = _sum32(X) * f32(1.0 / 128.0)
    d = X - mu
    rs = f32(1.0) / np.sqrt(_sum32(d * d) * f32(1.0 / 128.0) + f32(LN_EPS))
    return d * rs, rs


def ln_relu_f32(X, gamma, beta):
    h, _ = ln_hat_f32(X)
    return np.maximum(h * np.asarray(gamma, f32) + np.asarray(beta, f32), f32(0.0))


def ln_relu_bwd_gx_f32(X, gamma, gY, mask):
    """gX in fp32 under a GIVEN mask (the reference's: the restatement measures rounding, not mask flips)."""
    h, rs = ln_hat_f32(X)
    a = np.asarray(gY, f32) * np.asarray(mask, f32) * np.asarray(gamma, f32)
    m1 = _sum32(a) * f32(1.0 / 128.0)
    m2 = _sum32(a * h) * f32(1.0 / 128.0)
    return rs * (a - m1 - h * m2)
