"""Inputs, float64 autograd reference and comparison of the segment-attention ADJOINT tests (tests/test_seg_attn_grad_host.py on the
CPU, tests/test_gpu_seg_attn_bwd.py on the GPU).

A gradient case is a forward case of tests/seg_attn_cases.py made differentiable in a well-conditioned place:

  * `place`: the ligand coordinates are redrawn greedily so that no two atoms are closer than MIN_DIST and no angle of three atoms
    has a sine below MIN_SIN (the forward cases plant collinear atoms and a 1e-3 distance on purpose; there float64 and float32
    autograd disagree on gx by more than the gradient's own size).  The triplet cases recompute G and the Cdst rows from the new
    positions on tri_case's grid, so Cdst stays smear(d_ji) . Wg2 of the segment's own edge;
  * `off_kink`: the gradient is discontinuous where a LayerNorm+ReLU pre-activation h + b' sigma is zero.  Every pre-activation of a
    row that takes part, on both MLP paths, is moved to at least KINK_MARGIN x its scale |h| + |b'| sigma from zero by changing one
    addend of its channel.  This is a condition on the inputs: no element is ever left out of a comparison;
  * `grads`: the inputs are leaves, tests/seg_attn_reference.py runs forward, S / swn (or dx) are contracted with the case's fixed
    cotangents and torch.autograd gives the gradients -- in float64 the reference, in float32 the restatement whose distance from it
    is the rounding floor.

Comparison (`scales`, `kind_ratios`): |got - ref| <= TOL_GRAD[kind] x scale.  Row tensors (gU, gCdst, gCsrc, gx, gnrm, gew) are judged
per row -- one node, one bond or one segment -- against the largest |ref| of that row, the summed parameter gradients (gWf, gb, gW2xv,
gb2xv) against the largest |ref| of the tensor; scale 0 means exactly zero.  TOL_GRAD is FLOOR_MULT x the float32 restatement's largest
ratio over all gradient cases, measured on the CPU and recorded in profiles/seg_attn_bwd_parity.md; none of it comes from a kernel.

Layouts.  packing.lane_fixed_feat ([128, F] -> [F/4][8][64], F a multiple of 4) and packing.lane_fixed_xv ([16, 128] -> [32][64])
are gathers WITHOUT duplicates and without padding: permutations of the matrix's elements (tests/test_seg_attn_grad_host.py checks
it).  A kernel's gWf / gW2xv is therefore compared with the same map applied to the reference gradient; what is padding is the
feature COLUMNS no feature feeds (knn 45..47, triplet 11, pharmacophore 1..3), whose gradient must be exactly zero -- the
reference's is, so the comparison at scale 0 asks for it.  U goes in through sr.lane_fixed_u and gU comes back through sr.plain_u."""
import functools
from types import SimpleNamespace as NS

import torch

import seg_attn_cases as sc
import seg_attn_reference as sr
from helpers import FLOOR_MULT

f64, f32 = torch.float64, torch.float32
MIN_DIST, MIN_SIN = 0.4, 0.02

# 100 x the largest |pre_32 - pre_64| / kink_scale of the float32 restatement over all gradient cases (measured on the CPU: 8.2e-7,
# profiles/seg_attn_bwd_parity.md), rounded up to one digit
PRE_FLOOR = 8.2e-7
KINK_MARGIN = 9e-5
KINK_ROUNDS = 8

# FLOOR_MULT x the float32 autograd restatement's largest ratio over all gradient cases, rounded up to one digit (profiles/seg_attn_bwd_parity.md)
TOL_GRAD = dict(gU=1e-5, gCdst=3e-5, gCsrc=5e-5, gx=4e-5, gnrm=3e-5, gew=3e-5, gWf=3e-6, gb=3e-6, gW2xv=2e-6, gb2xv=2e-6)
EPS32 = 2.0 ** -24
ROW_KINDS = ('gU', 'gCdst', 'gCsrc', 'gx', 'gnrm', 'gew')
KIND_OF = dict(gU='gU', gCdst_k='gCdst', gCdst_v='gCdst', gCsrc_k='gCsrc', gCsrc_v='gCsrc', gx='gx', gnrm='gnrm', gew='gew', gWf_k='gWf',
               gWf_v='gWf', gbk='gb', gbv='gb', gW2xv='gW2xv', gb2xv='gb2xv')

TRI_GRAD_SIZES = dict(g18=sc.TRI_SIZES['small'], g33=((2, 1), (3, 2), (4, 1), (17, 2), (18, 1), (19, 1), (32, 1), (33, 1)), b64=((64, 1), (3, 1)),
                      b65=((64, 1), (65, 1), (3, 1)))


# ---- positions -------------------------------------------------------------------------------------------------------------------
def _min_sin(p, P):
    """Smallest sine of an angle the point p forms with two of the points P, at any of the three vertices (P [m, 3], m >= 2)."""
    D = P - p                                                                  # p -> a
    m = P.shape[0]
    off = ~torch.eye(m, dtype=torch.bool)
    at_p = torch.linalg.cross(D[:, None, :].expand(m, m, 3), D[None, :, :].expand(m, m, 3)).norm(dim=-1) / (D.norm(dim=-1)[:, None] * D.norm(dim=-1)[None, :])
    E = P[None, :, :] - P[:, None, :]                                          # a -> b
    at_a = torch.linalg.cross((-D)[:, None, :].expand(m, m, 3), E).norm(dim=-1) / (D.norm(dim=-1)[:, None] * E.norm(dim=-1).clamp_min(1e-300))
    return float(torch.minimum(at_p[off].min(), at_a[off].min()))


def place(n, gen, others=None, spread=1.8):
    """[n, 3] float32 positions chosen greedily: a candidate (normal, `spread` wide) is kept only if it is at least MIN_DIST from every
    placed atom (and from every row of `others`: the graph's pharmacophore nodes) and every angle it forms with two placed atoms,
    at any of the three vertices, has a sine of at least MIN_SIN.  Judged in float64 on the float32 values."""
    pts = torch.zeros(0, 3, dtype=f64)
    others = torch.zeros(0, 3, dtype=f64) if others is None else others.double()
    draws = 0
    while pts.shape[0] < n:
        draws += 1
        assert draws < 200 * n + 1000, 'place: no room left'
        p = (torch.randn(3, generator=gen) * spread).float().double()
        near = torch.cat([pts, others])
        if near.shape[0] and float((near - p).norm(dim=-1).min()) < MIN_DIST:
            continue
        if pts.shape[0] >= 2 and _min_sin(p, pts) < MIN_SIN:
            continue
        pts = torch.cat([pts, p[None]])
    return pts.float()


def geometry_bounds(x):
    """(smallest distance, smallest sine of an angle of three atoms) of one ligand's positions [n, 3], in float64."""
    x = x.double()
    n = x.shape[0]
    if n < 2:
        return float('inf'), float('inf')
    E = x[None, :, :] - x[:, None, :]                                          # [a, b] = a -> b
    d = E.norm(dim=-1)
    dmin = float(d[~torch.eye(n, dtype=torch.bool)].min())
    if n < 3:
        return dmin, float('inf')
    cr = torch.linalg.cross(E[:, :, None, :].expand(n, n, n, 3), E[:, None, :, :].expand(n, n, n, 3)).norm(dim=-1)   # vertex a, arms b and c
    s = cr / (d[:, :, None] * d[:, None, :]).clamp_min(1e-300)
    i = torch.arange(n)
    ok = (i[:, None, None] != i[None, :, None]) & (i[:, None, None] != i[None, None, :]) & (i[None, :, None] != i[None, None, :])
    return dmin, float(s[ok].min())


def _replace_ligands(c, t, g):
    x = c.x.clone()
    for gi in range(t.g_nlig.numel()):
        n, p0, l0 = int(t.g_nlig[gi]), int(t.g_ctx_off[gi]), int(t.g_ctx_off[gi] + t.g_nph[gi])
        x[l0:l0 + n] = place(n, g, others=x[p0:l0])
    return x


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _cot(g, n, pos):
    return dict(gdx=torch.randn(n, 3, generator=g)) if pos else dict(gS=torch.randn(n, 128, 16, generator=g), gswn=torch.randn(n, 16, generator=g))


def _finish(c, g, well):
    """Fixed random cotangents per target list (both of the node update and of the position update), then the kink condition."""
    n = lambda ids: c.n_bond if ids is None else ids.numel()
    c.cot = [dict(**_cot(g, n(l.ids), False), **(_cot(g, n(l.ids), True) if c.pos_mode is not None else {})) for l in c.lists]
    c.kink_rounds = off_kink(c, KINK_MARGIN) if well else None
    return c


def _clone(c, **kw):
    d = NS(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(c).items()})
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def topo(c):
    return sc.topo_of(sc.make_plan(c.sizes))


@functools.lru_cache(maxsize=None)
def knn_grad_case(name, well=True):
    """well False: the forward case as it is (degenerate geometry, nothing moved off the kink): its gradients need only be finite.  mixed: the ligand targets and the pharmacophore targets as two lists, each with its own Wf (what a sub-layer of the model
    launches); grouped, k48: the forward case's shuffled list."""
    fwd = dict(mixed=lambda: sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS), grouped=lambda: sc.knn_case('grouped', sc.KNN_SIZES, 32, sc.DEGS, grouped=True, seed=5),
               k48=lambda: sc.knn_case('k48', sc.KNN48_SIZES, 48, sc.DEGS48, seed=10))[name]()
    c = _clone(fwd, kind='knn', node_mode=sr.KNN_NODE, pos_mode=sr.KNN_POS)
    t, g = topo(c), sc._gen(100 + len(name))
    if well:
        c.x = _replace_ligands(c, t, g)
    if name == 'mixed':
        lig = t.ctx_is_lig[c.ids.long()].bool()
        c.lists = [NS(label='lig', ids=c.ids[lig], Wf_k=c.Wf[0][0].clone(), Wf_v=c.Wf[0][1].clone()),
                   NS(label='phore', ids=c.ids[~lig], Wf_k=c.Wf[1][0].clone(), Wf_v=c.Wf[1][1].clone())]
    else:
        c.lists = [NS(label='all', ids=c.ids, Wf_k=c.Wf[0][0].clone(), Wf_v=c.Wf[0][1].clone())]
    return _finish(c, g, well)


@functools.lru_cache(maxsize=None)
def bond_grad_case(name, well=True):
    c = _clone(sc.bond_case(name), kind='bond', node_mode=sr.BOND_NODE, pos_mode=sr.BOND_POS)
    t, g = topo(c), sc._gen(200 + len(name))
    if well:
        c.x = _replace_ligands(c, t, g)
    c.lists = [NS(label='lig', ids=c.ids, Wf_k=None, Wf_v=None)]
    return _finish(c, g, well)


@functools.lru_cache(maxsize=None)
def tri_grad_case(name, well=True):
    c = _clone(sc.tri_case(name, sizes=TRI_GRAD_SIZES[name]), kind='tri', node_mode=sr.TRIPLET, pos_mode=None)
    t, g = topo(c), sc._gen(300 + len(name))
    c.n_bond = t.n_bond
    if well:
        c.x = _replace_ligands(c, t, g)
        d = (c.x[t.bond_dst] - c.x[t.bond_src]).norm(dim=-1)
        c.G = sc._grid(torch.exp(-0.5 * (d[:, None] - torch.tensor(sr.SMEAR_OFF)) ** 2), 64)
        c.Cdst_k, c.Cdst_v = (c.G.double() @ c.Wg2_k.double()).float(), (c.G.double() @ c.Wg2_v.double()).float()
    c.Csrc_k, c.Csrc_v = c.Csrc[:, :128], c.Csrc[:, 128:]                    # (views of the clone: one [n_bond, 256] tensor)
    c.lists = [NS(label='edges', ids=None, Wf_k=c.Wf_k, Wf_v=c.Wf_v)]
    _finish(c, g, well)
    assert bool((c.Cdst_k.double() == c.G.double() @ c.Wg2_k.double()).all()) and bool((c.Cdst_v.double() == c.G.double() @ c.Wg2_v.double()).all())
    return c


@functools.lru_cache(maxsize=None)
def phore_grad_case(explicit, well=True):
    c = _clone(sc.phore_case(explicit), kind='phore', node_mode=sr.PHORE, pos_mode=None)
    c.lists = [NS(label='phore', ids=c.ids, Wf_k=c.Wf_k, Wf_v=c.Wf_v)]
    return _finish(c, sc._gen(400 + int(explicit)), well)


SMALL_CASES = (('knn', 'mixed'), ('knn', 'grouped'), ('knn', 'k48'), ('bond', 't2'), ('bond', 't3'), ('tri', 'g33'), ('phore', False), ('phore', True))
LARGE_CASES = (('bond', 't5'), ('bond', 'generic'), ('tri', 'b64'), ('tri', 'b65'))          # more than 34 atoms: the GPU tests and the measurement


DEGENERATE_CASES = (('knn', 'mixed'), ('bond', 't2'), ('tri', 'g18'), ('phore', False))     # the forward cases, for the finiteness check


def grad_case(kind, name, well=True):
    return dict(knn=knn_grad_case, bond=bond_grad_case, tri=tri_grad_case, phore=phore_grad_case)[kind](name, well)


def case_id(kn):
    return f'{kn[0]}_{kn[1]}'.replace('True', 'efeat').replace('False', 'distance')


def modes_of(c):
    return (c.node_mode,) if c.pos_mode is None else (c.node_mode, c.pos_mode)


# ---- the reference under autograd ------------------------------------------------------------------------------------------------
LEAVES = ('x', 'nrm', 'ew', 'Csrc_k', 'Csrc_v', 'Cdst_k', 'Cdst_v', 'bk', 'bv', 'W2xv', 'b2xv')


def _run(c, t, mode, li, dtype, variant='', device=None, pre=None, leaves=False):
    """The reference on list `li` of the case: (result, {name: leaf})."""
    dev = device or 'cpu'
    d = NS(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(c).items()})
    L = c.lists[li]
    leaf = {}

    def mk(v):
        v = v.to(dev).to(dtype).detach().clone()
        return v.requires_grad_(True) if leaves else v
    for k in LEAVES:
        if getattr(c, k, None) is not None:
            leaf[k] = mk(getattr(c, k))
            setattr(d, k, leaf[k])
    for k in ('Wf_k', 'Wf_v'):
        if getattr(L, k) is not None:
            leaf[k] = mk(getattr(L, k))
    ids = None if L.ids is None else L.ids.to(dev)
    q = c.q if ids is None else c.q[L.ids.long()]
    U, _ = sr.fold_query(q, c.W2k)
    assert torch.equal(U.float().double(), U)                    # (the cases' fold is exact in fp32: one U for every dtype)
    leaf['U'] = mk(U)
    if mode == sr.TRIPLET:
        d.Wf_k, d.Wf_v = leaf['Wf_k'], leaf['Wf_v']
        res = sr.triplet(d, t, dtype, variant, U=leaf['U'], pre=pre)
    else:
        res = sr.node_attn(d, t, mode, ids, leaf.get('Wf_k'), leaf.get('Wf_v'), dtype, variant, U=leaf['U'], pre=pre)
    return res, leaf


def grads(c, mode, dtype=f64, li=0, variant='', device=None, t=None):
    """{name: gradient} of sum(S gS) + sum(swn gswn) (node update, triplet, pharmacophore) or sum(dx gdx) (position update) on list
    `li` of the case.  gU rows are the listed targets in list order (plain layout), gCdst / gx / gnrm / gew rows context nodes (triplet:
    gCdst rows bond edges), gCsrc rows as Csrc; '_rows': the rows of gCdst the rows of gU belong to.  An input the mode does not read has
    gradient zero."""
    t = t or sc.topo_of(sc.make_plan(c.sizes), device)
    res, leaf = _run(c, t, mode, li, dtype, variant, device, leaves=True)
    cot = {k: v.to(res.U.device).to(dtype) for k, v in c.cot[li].items()}
    if mode in (sr.KNN_POS, sr.BOND_POS):
        loss = (res.dx * cot['gdx']).sum()
    else:
        loss = (res.S * cot['gS']).sum() + (res.swn * cot['gswn']).sum()
    names = list(leaf)
    gs = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
    out = {'g' + k: (torch.zeros_like(leaf[k]) if g is None else g) for k, g in zip(names, gs)}
    L = c.lists[li]
    out['_rows'] = torch.arange(out['gU'].shape[0], device=out['gU'].device) if L.ids is None else L.ids.long().to(out['gU'].device)
    return out


def scales(ref):
    """{name: per-element scale} of a float64 gradient dict.  Row tensors: the largest |ref| of the element's row, where a row is what
    the product's tensors hold -- one segment's [128, 16] block of gU, one 256-wide k | v row of Ydst / Ysrc (gCdst_k and gCdst_v, gCsrc_k
    and gCsrc_v are its halves and share one scale), one node's 3 coordinates or k gates.  A segment's gU is held against at least
    rho x the scale of its gCdst row, rho = the median of that ratio over the segments of the launch: the adjoints that are fed by the
    forward's record form d logit as a DIFFERENCE of two separately rounded sums of the size of the value path's terms, so the key
    path's error does not shrink with the key path's gradient, which is exactly zero for a segment with one row
    (profiles/seg_attn_bwd_parity.md).  Summed parameter gradients: the tensor's largest |ref|."""
    rowmax = lambda t: t.double().abs().reshape(t.shape[0], -1).amax(1)
    like = lambda m, t: m.reshape(-1, *([1] * (t.dim() - 1))).expand_as(t)
    out = {}
    for name, r in ref.items():
        if name.startswith('_') or name in out:
            continue
        if name[:-2] in ('gCdst', 'gCsrc'):
            k, v = ref[name[:-2] + '_k'], ref[name[:-2] + '_v']
            m = torch.maximum(rowmax(k), rowmax(v))
            out[name[:-2] + '_k'], out[name[:-2] + '_v'] = like(m, k), like(m, v)
        elif name == 'gU':
            m, c = rowmax(r), torch.maximum(rowmax(ref['gCdst_k']), rowmax(ref['gCdst_v']))[ref['_rows']]
            both = (m > 0) & (c > 0)
            rho = (m[both] / c[both]).median() if bool(both.any()) else m.new_zeros(())
            out[name] = like(torch.maximum(m, rho * c), r)
        elif KIND_OF[name] in ROW_KINDS:
            out[name] = like(rowmax(r), r)
        else:
            out[name] = r.double().abs().max().expand_as(r) if r.numel() else r.double()
    return out


def n_terms(c, li, t=None):
    """The rows (segment, source) that take part on list `li`: the terms of every summed parameter gradient of the launch."""
    t = t or topo(c)
    if c.kind == 'tri':
        n = t.g_nlig
        return int((n * (n - 1) * (n - 2)).sum())
    ids = c.lists[li].ids.long()
    g = t.ctx_graph.cpu()[ids]
    if c.kind == 'knn':
        return int(c.deg.long()[ids].sum())
    return int((t.g_nlig.cpu()[g] - 1).sum()) if c.kind == 'bond' else int(t.g_nph.cpu()[g].sum())


def tol_of(kind, chain=0):
    """The bound of a gradient kind.  A summed parameter gradient of a kernel that adds `chain` terms into ONE fp32 accumulator one after
    the other carries the rounding of the partial sums on top: with terms of random sign the partial sum after i terms is of the size
    sqrt(i) x rms, every addition rounds it by up to EPS32 of that, the roundings add up to EPS32 x rms x sqrt(chain^2 / 2), and the sum
    itself is of the size sqrt(chain) x rms: EPS32 x sqrt(chain / 2) relative to the result.  float32 autograd does not show it (torch
    sums pairwise).  chain = terms of the launch / persistent workgroups asked for (profiles/seg_attn_bwd_parity.md)."""
    return TOL_GRAD[kind] + (0.0 if kind in ROW_KINDS else EPS32 * (chain / 2.0) ** 0.5)


def kind_ratios(got, ref):
    """{kind: largest |got - ref| / scale} over the tensors of two gradient dicts (ref: float64, owner of the scales)."""
    out, sca = {}, scales(ref)
    for name, scale in sca.items():
        out[KIND_OF[name]] = max(out.get(KIND_OF[name], 0.0), sc.ratio(got[name], ref[name], scale))
    return out


# ---- the kink --------------------------------------------------------------------------------------------------------------------
def pre_activations(c, t=None, dtype=f64):
    """[(list index, entry)] of sr._report over every target list of the case (both modes of a case share their pre-activations)."""
    t = t or topo(c)
    out = []
    for li in range(len(c.lists)):
        pre = []
        _run(c, t, c.node_mode, li, dtype, pre=pre)
        out += [(li, e) for e in pre]
    return out


def kink_scale(e, path):
    """What a pre-activation's distance from zero is judged against: its scale |h| + |b'| sigma, but at least the row's sigma.  The
    addends of a channel (Csrc, Cdst, the feature terms) are of the size of sigma, and so is their rounding error; where they cancel,
    |h| + |b'| sigma alone is far smaller than what the error is relative to (profiles/seg_attn_bwd_parity.md)."""
    return torch.maximum(e.scale[path], e.sigma[path][..., None])


def near_kink(c, margin, t=None):
    """Pre-activations of rows that take part with |pre| < margin x scale: [(path, Csrc row, Cdst row, channel, pre, scale)]."""
    bad = []

    def look(e):
        for path in 'kv':
            scale = kink_scale(e, path)
            m = (e.pre[path].abs() < margin * scale) & e.valid[..., None]
            for s, r, ch in torch.nonzero(m).tolist():
                bad.append((path, int(e.crow[s, r]), int(e.seg[s]), ch, float(e.pre[path][s, r, ch]), float(scale[s, r, ch])))
    t = t or topo(c)
    for li in range(len(c.lists)):
        _run(c, t, c.node_mode, li, f64, pre=look)
    return bad


def off_kink(c, margin, rounds=KINK_ROUNDS):
    """Moves every pre-activation nearer to zero than margin x scale away from it by 4 x margin x scale, through one addend of its
    channel: the Csrc row in the bond and triplet cases, the Cdst row in the knn and pharmacophore cases (the triplet's Cdst stays
    G . Wg2; q and W2k stay on their grid).  Returns the number of rounds that changed something; more than `rounds` is an error."""
    t = topo(c)
    way = {}                # an addend keeps the direction of its first move: two pre-activations that share it cannot push it to and fro
    for rnd in range(rounds + 1):
        bad = near_kink(c, margin, t)
        if not bad:
            return rnd
        assert rnd < rounds, f'off_kink: {len(bad)} pre-activations still within {margin:g} of the kink after {rounds} rounds'
        for path, crow, drow, ch, p, s in bad:
            tensor, row = (getattr(c, 'Csrc_' + path), crow) if c.kind in ('bond', 'tri') else (getattr(c, 'Cdst_' + path), drow)
            sign = way.setdefault((path, row, ch), 1.0 if p >= 0 else -1.0)
            tensor[row, ch] += sign * 4.0 * margin * s
