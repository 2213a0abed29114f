"""The contract of pg_seg_attn, pg_attn_fold_query and pg_attn_unfold_value (include/phoregen_hip.h) restated in plain torch.

One function per mode family, written from the header and the row rules of csrc/seg_common.h: for every segment the list of its rows,
per row the factored first layer, the folded LayerNorm (no mean subtraction: the packed first layer is centred), the logits, an exact
base-2 softmax over the valid rows and the gated sums.  No tiles, no lanes, no running maximum; segments that share a row count are
evaluated together as [segments, rows, 128] arrays.  `dtype` is torch.float64 for the reference and torch.float32 for the
restatement whose distance from it is the rounding floor of the formula on the test inputs (tests/test_seg_attn_host.py).

All matrices are in their plain form: U [n, 128 (c), 16 (h)], S [n, 128, 16], W2k / W2v [128 (8h+d), 128 (c)], W2xv [16, 128],
Wf [128, F]; tests stage them for the kernels through packing.lane_fixed_* and lane_fixed_u below.

Beside every output the functions return its per-element SCALE: the same contraction with every term replaced by its magnitude, a
ReLU output z = relu(hidden + b' sigma) counted as |hidden| + |b'| sigma (that, not z, is what a rounding error of z is relative to:
an element whose rows all sit at the kink is as uncertain as its pre-activations).  Errors are judged as |error| / scale.

Everything is plain differentiable torch: tests/seg_attn_grad_cases.py runs it under autograd for the adjoint tests, and takes the
LayerNorm+ReLU pre-activations h + b' sigma of every row through `pre` (`_report`) to keep its inputs off the ReLU kink.

`variant` names one deliberate mistake (VARIANTS); tests/test_seg_attn_host.py shows that every one of them lies far outside the
tolerances, i.e. that the tolerances would catch it in a kernel."""
import math
from types import SimpleNamespace as NS

import torch

SMEAR_OFF = (0., 1., 1.25, 1.5, 1.75, 2., 2.25, 2.5, 2.75, 3., 3.5, 4., 4.5, 5., 5.5, 6., 7., 8., 9., 10.)
ANG_FREQ = (1., 2., 3., 0.5, 1. / 3.)
KNN_NODE, KNN_POS, BOND_NODE, BOND_POS, TRIPLET, PHORE = range(6)

VARIANTS = ('drop_last_row', 'skip_row_16', 'gate_in_denominator', 'normals_swapped', 'target_not_excluded', 'bias_on_empty',
            'natural_base', 'mean_subtracted', 'smear_offset_shifted')


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def lane_fixed_u(U):
    """[n, 128 (c), 16 (h)] -> the kernels' [n][32][64]: element [4 tau + r][lane = (g, h)] = U[16 tau + 4 g + r][h]."""
    n = U.shape[0]
    return U.reshape(n, 8, 4, 4, 16).permute(0, 1, 3, 2, 4).reshape(n, 32, 64).contiguous()     # [tau, g, r, h] -> [tau, r, g, h]


def plain_u(Ul):
    """Inverse of lane_fixed_u."""
    n = Ul.shape[0]
    return Ul.reshape(n, 8, 4, 4, 16).permute(0, 1, 3, 2, 4).reshape(n, 128, 16).contiguous()   # [tau, r, g, h] -> [tau, g, r, h]


# ---- the three small pieces ----------------------------------------------------------------------------------------------------
def fold_query(q, W2k, dtype=torch.float64):
    """U[s][c][h] = sum_d q[s, 8h+d] * W2k[8h+d, c]; returns (U, scale)."""
    q, W = q.to(dtype).reshape(-1, 16, 8), W2k.to(dtype).reshape(16, 8, 128)
    return torch.einsum('shd,hdc->sch', q, W), torch.einsum('shd,hdc->sch', q.abs(), W.abs())


def unfold_value(S, swn, W2v, b2v, dtype=torch.float64, S_scale=None):
    """out[s, 8h+d] = sum_c W2v[8h+d, c] * S[s][c][h] + b2v[8h+d] * swn[s][h] (swn / b2v None: no bias term); (out, scale)."""
    S, W = S.to(dtype), W2v.to(dtype).reshape(16, 8, 128)
    Sa = S.abs() if S_scale is None else S_scale.to(dtype)
    out, sc = torch.einsum('hdc,sch->shd', W, S), torch.einsum('hdc,sch->shd', W.abs(), Sa)
    if swn is not None and b2v is not None:
        b = b2v.to(dtype).reshape(16, 8)
        out = out + b[None] * swn.to(dtype)[:, :, None]
        sc = sc + b.abs()[None] * swn.to(dtype).abs()[:, :, None]
    return out.reshape(-1, 128), sc.reshape(-1, 128)


def pre_activation(h, bp):
    """The LayerNorm+ReLU pre-activation h + b' sigma, its scale |h| + |b'| sigma, and sigma."""
    var = (h * h).mean(-1) + 1e-5
    sigma = var.sqrt()
    return h + bp * sigma[..., None], h.abs() + bp.abs() * sigma[..., None], sigma


def _ln_relu(h, bp, variant):
    if variant == 'mean_subtracted':
        h = h - h.mean(-1, keepdim=True)
    pre, scale, sigma = pre_activation(h, bp)
    return torch.relu(pre), 1.0 / sigma, scale


def _report(pre, seg, crow, valid, hk, hv, bk, bv):
    """pre (a list or a callable, or None) receives one entry per group of segments: the pre-activations of both MLP paths [segments,
    rows, 128], their scales, the segments' ids (rows of Cdst), the rows of Csrc every row reads and the rows that take part."""
    if pre is not None:
        with torch.no_grad():
            (pk, sk, gk), (pv, sv, gv) = pre_activation(hk, bk), pre_activation(hv, bv)
            (pre if callable(pre) else pre.append)(NS(seg=seg, crow=crow, valid=valid, pre=dict(k=pk, v=pv), scale=dict(k=sk, v=sv),
                                                      sigma=dict(k=gk, v=gv)))


def _attend(hk, valid, gate, U, bk, variant):
    """hk [S, R, 128], valid [S, R], gate [S, R], U [S, 128, 16] -> softmax weights x gate [S, R, 16] and the logits with their scale."""
    zk, rk, zka = _ln_relu(hk, bk, variant)
    logit = rk[..., None] * torch.einsum('src,sch->srh', zk, U)
    logit_scale = rk[..., None] * torch.einsum('src,sch->srh', zka, U.abs())
    valid = valid.clone()
    if variant == 'drop_last_row':
        last = (valid.long() * torch.arange(1, valid.shape[1] + 1, device=valid.device)).argmax(1)
        any_ = valid.any(1)
        valid[torch.nonzero(any_)[:, 0], last[any_]] = False
    if variant == 'skip_row_16' and valid.shape[1] > 16:
        valid[:, 16] = False
    v3 = valid[..., None]
    mx = torch.where(v3, logit, torch.full_like(logit, -math.inf)).amax(1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    d = torch.where(v3, logit - mx, torch.zeros_like(logit))
    e = torch.where(v3, torch.exp(d) if variant == 'natural_base' else torch.exp2(d), torch.zeros_like(d))
    if variant == 'gate_in_denominator':
        e = e * gate[..., None]
    den = e.sum(1, keepdim=True)
    alpha = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
    aw = alpha if variant == 'gate_in_denominator' else alpha * gate[..., None]
    return NS(aw=aw, logit=logit, logit_scale=logit_scale, valid=valid, has=valid.any(1))


def _node_finish(a, hv, bv, variant):
    """S[s][c][h] = sum_row alpha gate rstd_v z_v, swn[s][h] = sum_row alpha gate."""
    zv, rv, zva = _ln_relu(hv, bv, variant)
    S = torch.einsum('srh,sr,src->sch', a.aw, rv, zv)
    S_scale = torch.einsum('srh,sr,src->sch', a.aw, rv, zva)
    return S, S_scale, a.aw.sum(1)


def _pos_finish(a, hx, bx, W2xv, b2xv, rel, variant):
    """v[row, h] = rstd (z . W2xv[h, :]) + b2xv[h];  dx = mean_h sum_row alpha gate v (x_dst - x_src)."""
    zx, rx, zxa = _ln_relu(hx, bx, variant)
    v = rx[..., None] * (zx @ W2xv.T) + b2xv
    v_scale = rx[..., None] * (zxa @ W2xv.abs().T) + b2xv.abs()
    dx = torch.einsum('srh,srh,srd->sd', a.aw, v, rel) / 16.0
    dx_scale = torch.einsum('srh,srh,srd->sd', a.aw, v_scale, rel.abs()) / 16.0
    return dx, dx_scale, v, v_scale


def _smear(d, variant):
    off = list(SMEAR_OFF)
    if variant == 'smear_offset_shifted':
        off[5] = off[6]
    t = d[..., None] - torch.tensor(off, dtype=d.dtype, device=d.device)
    return torch.exp(-0.5 * t * t)


# ---- node-target modes (knn / bond / phore) ------------------------------------------------------------------------------------
def _cast(c, names, dtype):
    return NS(**{k: (getattr(c, k).to(dtype) if getattr(c, k, None) is not None else None) for k in names})


def node_attn(c, t, mode, ids, Wf_k=None, Wf_v=None, dtype=torch.float64, variant='', U=None, pre=None):
    """One sub-layer over the target nodes `ids` (ctx ids, any order).  c: the case's tensors (tests/seg_attn_cases.py), t: its
    topology (long tensors).  U None: folded from c.q and c.W2k.  Returns per listed target (rows in the order of ids):
    U, S, swn, out (node-update modes), dx (position modes, WITHOUT the accumulate term), the training record and the scales."""
    pos, knn = mode in (KNN_POS, BOND_POS), mode in (KNN_NODE, KNN_POS)
    f = _cast(c, ('x', 'nrm', 'ew', 'Csrc_k', 'Csrc_v', 'Cdst_k', 'Cdst_v', 'bk', 'bv', 'q', 'W2k', 'W2v', 'b2v', 'W2xv', 'b2xv', 'efeat'),
              dtype)
    ids = ids.long()
    n_ids = ids.numel()
    dev = ids.device
    if U is None:
        U_all, U_scale = fold_query(f.q[ids], f.W2k, dtype)
    else:
        U_all, U_scale = U.to(dtype), U.to(dtype).abs()
    Wf_k = Wf_k.to(device=dev, dtype=dtype) if Wf_k is not None else None
    Wf_v = Wf_v.to(device=dev, dtype=dtype) if Wf_v is not None else None
    if knn:
        groups = [(torch.arange(n_ids, device=dev), c.knn_k)]
    else:
        gr = t.ctx_graph[ids]
        groups = [(torch.nonzero(gr == g)[:, 0], int(t.g_nph[g] if mode == PHORE else t.g_nlig[g])) for g in torch.unique(gr).tolist()]
    R_max = max([r for _, r in groups] + [1])
    res = NS(U=U_all, U_scale=U_scale, rows=torch.zeros(n_ids, dtype=torch.long, device=dev),
             valid=torch.zeros(n_ids, R_max, dtype=torch.bool, device=dev))
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)
    if pos:
        res.dx, res.dx_scale = z(n_ids, 3), z(n_ids, 3)
        res.logit, res.logit_scale, res.v, res.v_scale = z(n_ids, R_max, 16), z(n_ids, R_max, 16), z(n_ids, R_max, 16), z(n_ids, R_max, 16)
    else:
        res.S, res.S_scale, res.swn, res.aw = z(n_ids, 128, 16), z(n_ids, 128, 16), z(n_ids, 16), z(n_ids, R_max, 16)
    for sel, R in groups:
        seg = ids[sel]
        S_ = seg.numel()
        k = torch.arange(R, device=dev)[None, :].expand(S_, R)
        gate = torch.ones(S_, R, dtype=dtype, device=dev)
        if knn:
            valid = k < t_deg(c, seg)[:, None]
            src = torch.where(valid, c.nbr.long()[seg], torch.zeros_like(k))
            csrc = src
            gate = f.ew[seg]
        elif mode == PHORE:
            g = t.ctx_graph[seg]
            first = t.g_ctx_off[g]
            valid = torch.ones(S_, R, dtype=torch.bool, device=dev)
            src = first[:, None] + k
            csrc = src
        else:
            g = t.ctx_graph[seg]
            lig0 = t.g_ctx_off[g] + t.g_nph[g]
            li = seg - lig0
            valid = k != li[:, None]
            src = lig0[:, None] + k
            csrc = t.eid[t.g_eid_off[g][:, None] + k * R + li[:, None]]
            if variant == 'target_not_excluded':
                valid = torch.ones_like(valid)
        use = (valid & (csrc >= 0))[..., None]                       # (the diagonal of eid is -1: such a row has no first-layer row)
        crow = csrc.clamp_min(0)
        hk = torch.where(use, f.Csrc_k[crow], z(1)) + f.Cdst_k[seg][:, None, :]
        hv = torch.where(use, f.Csrc_v[crow], z(1)) + f.Cdst_v[seg][:, None, :]
        rel = f.x[seg][:, None, :] - f.x[src] if f.x is not None else None
        if knn:
            d = rel.norm(dim=-1)
            lig = t.ctx_is_lig[src].to(dtype)
            sm = _smear(d, variant)
            ns, nd = f.nrm[src], f.nrm[seg][:, None, :].expand(S_, R, 3)
            if variant == 'normals_swapped':
                ns, nd = nd, ns
            feat = torch.cat([sm * lig[..., None], sm * (1 - lig)[..., None], (ns * nd).sum(-1, keepdim=True),
                              -(ns * rel).sum(-1, keepdim=True), -(nd * rel).sum(-1, keepdim=True), lig[..., None],
                              (1 - lig)[..., None], z(S_, R, 3)], -1)
            hk, hv = hk + feat @ Wf_k.T, hv + feat @ Wf_v.T
        elif mode == PHORE:
            if f.efeat is not None:
                d = f.efeat[c.efeat_off.long()[g][:, None] + k * R + (seg - first)[:, None]]
            else:
                d = rel.norm(dim=-1)
            hk, hv = hk + d[..., None] * Wf_k[:, 0], hv + d[..., None] * Wf_v[:, 0]
        _report(pre, seg, crow, valid, hk, hv, f.bk, f.bv)
        a = _attend(hk, valid, gate, U_all[sel], f.bk, variant)
        res.rows[sel] = R
        res.valid[sel, :R] = a.valid
        if pos:
            res.dx[sel], res.dx_scale[sel], v, v_scale = _pos_finish(a, hv, f.bv, f.W2xv, f.b2xv, rel, variant)
            res.logit[sel, :R], res.logit_scale[sel, :R], res.v[sel, :R], res.v_scale[sel, :R] = a.logit, a.logit_scale, v, v_scale
        else:
            res.S[sel], res.S_scale[sel], res.swn[sel] = _node_finish(a, hv, f.bv, variant)
            res.aw[sel, :R] = a.aw
    if not pos and f.W2v is not None:
        res.out, res.out_scale = unfold_value(res.S, res.swn, f.W2v, f.b2v, dtype, res.S_scale)
    return res


def t_deg(c, seg):
    return c.deg.long()[seg]


# ---- triplet ---------------------------------------------------------------------------------------------------------------------
def triplet(c, t, dtype=torch.float64, variant='', staged=True, U=None, pre=None):
    """Every bond edge j -> i of the batch (rows of the results = internal bond ids).  staged: Cdst_k / Cdst_v given explicitly and the
    query folded from q; else Cdst = G . Wg2.  Returns U, S, swn (the training form's outputs), out = resid + W2v . S + b2v [not empty],
    aw [n_bond, max_nlig, 16] (softmax weights by ATOM k, zero for i and j) and the scales."""
    f = _cast(c, ('x', 'Csrc_k', 'Csrc_v', 'Cdst_k', 'Cdst_v', 'G', 'Wg2_k', 'Wg2_v', 'bk', 'bv', 'q', 'W2k', 'W2v', 'b2v', 'resid',
                  'Wf_k', 'Wf_v'), dtype)
    nb, dev = t.bond_src.numel(), t.bond_src.device
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)
    if U is None:
        U, U_scale = fold_query(f.q, f.W2k, dtype)
    else:
        U, U_scale = U.to(dtype), U.to(dtype).abs()
    if staged:
        Ck, Cv = f.Cdst_k, f.Cdst_v
    else:
        Ck, Cv = f.G @ f.Wg2_k, f.G @ f.Wg2_v
    nmax = int(t.g_nlig.max())
    res = NS(U=U, U_scale=U_scale, S=z(nb, 128, 16), S_scale=z(nb, 128, 16), swn=z(nb, 16), aw=z(nb, nmax, 16),
             has=torch.zeros(nb, dtype=torch.bool, device=dev))
    fr = torch.tensor(ANG_FREQ, dtype=dtype, device=dev)
    for g in range(t.g_nlig.numel()):
        n = int(t.g_nlig[g])
        if n < 2:
            continue
        lig0 = int(t.g_ctx_off[g] + t.g_nph[g])
        eid = t.eid[int(t.g_eid_off[g]):int(t.g_eid_off[g]) + n * n].reshape(n, n)       # [src, dst]
        xg = f.x[lig0:lig0 + n]
        for j in range(n):
            i = torch.tensor([a for a in range(n) if a != j], device=dev)
            seg = eid[j, i]                                           # edges j -> i
            k = torch.arange(n, device=dev)[None, :].expand(n - 1, n)
            valid = (k != i[:, None]) & (k != j)
            csrc = eid[:, j][None, :].expand(n - 1, n)                # edges k -> j
            use = (valid & (csrc >= 0))[..., None]
            crow = csrc.clamp_min(0)
            u = (xg[j] - xg[i])[:, None, :]
            v = xg[None, :, :] - xg[i][:, None, :]
            theta = torch.atan2(torch.linalg.cross(u.expand_as(v), v).norm(dim=-1), (u * v).sum(-1))
            ang = theta[..., None] * fr
            feat = torch.cat([theta[..., None], torch.sin(ang), torch.cos(ang), z(n - 1, n, 1)], -1)
            hk = torch.where(use, f.Csrc_k[crow], z(1)) + Ck[seg][:, None, :] + feat @ f.Wf_k.T
            hv = torch.where(use, f.Csrc_v[crow], z(1)) + Cv[seg][:, None, :] + feat @ f.Wf_v.T
            _report(pre, seg, crow, valid, hk, hv, f.bk, f.bv)
            a = _attend(hk, valid, torch.ones(n - 1, n, dtype=dtype, device=dev), U[seg], f.bk, variant)
            res.S[seg], res.S_scale[seg], res.swn[seg] = _node_finish(a, hv, f.bv, variant)
            res.aw[seg, :n] = a.aw
            res.has[seg] = a.has
    has = torch.ones_like(res.has) if variant == 'bias_on_empty' else res.has
    upd, upd_scale = unfold_value(res.S, has.to(dtype)[:, None].expand(nb, 16), f.W2v, f.b2v, dtype, res.S_scale)
    res.out, res.out_scale = f.resid + upd, f.resid.abs() + upd_scale
    return res
