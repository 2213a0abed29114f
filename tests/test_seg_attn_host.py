"""CPU side of the segment-attention tests: what makes tests/seg_attn_reference.py trustworthy and the tolerances of
tests/seg_attn_cases.py honest, with no kernel in sight.

  * invariances of the reference a transliteration error would break (slot order, softmax shift, rigid motions, fused = fold ->
    attend -> unfold, staged = generic triplet, layout round trips);
  * floors: the same code in float32 stays within TOL / MARGIN of float64 on every case and output kind, so every bound the kernels are
    asked to meet is at least MARGIN times what fp32 rounding of the contract itself costs on these inputs;
  * sharpness: every deliberate mistake of seg_attn_reference.VARIANTS lies at least 10 x outside the tolerance on some case.
Each figure is printed (pytest -s) before it is asserted; profiles/seg_attn_parity.md records them."""
import math
from types import SimpleNamespace as NS

import pytest
import torch

import seg_attn_cases as sc
import seg_attn_reference as sr

F64_EQ = 1e-11          # two float64 evaluations of one expression, relative to the element's scale
f64, f32 = torch.float64, torch.float32


def _topo(c):
    return sc.topo_of(sc.make_plan(c.sizes))


def _knn(c, mode, dtype=f64, variant='', lst=0, ids=None):
    return sr.node_attn(c, _topo(c), mode, c.ids if ids is None else ids, c.Wf[lst][0], c.Wf[lst][1], dtype, variant)


def _copy(c, **kw):
    d = NS(**vars(c))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _close(a, b, scale, what):
    r = sc.ratio(a, b, scale)
    print(f'seg-attn reference invariance {what:58s} {r:.3e}')
    assert r <= F64_EQ, (what, r)


def _rotation():
    a, b = 0.7, -1.1
    Rz = torch.tensor([[math.cos(a), -math.sin(a), 0.], [math.sin(a), math.cos(a), 0.], [0., 0., 1.]], dtype=f64)
    Rx = torch.tensor([[1., 0., 0.], [0., math.cos(b), -math.sin(b)], [0., math.sin(b), math.cos(b)]], dtype=f64)
    return Rz @ Rx


# ---- invariances -----------------------------------------------------------------------------------------------------------------
def test_lane_fixed_layouts_round_trip():
    from phoregen_amd import packing
    U = torch.randn(5, 128, 16, dtype=f64)
    Ul = sr.lane_fixed_u(U)
    assert torch.equal(sr.plain_u(Ul), U)
    # the same layout as a [16, 128] matrix per segment takes through packing.lane_fixed_xv
    assert torch.equal(Ul, packing.lane_fixed_xv(U.transpose(1, 2).contiguous()))
    lane = torch.arange(64)
    g, m = lane >> 4, lane & 15
    for i in (0, 7, 31):
        assert torch.equal(Ul[:, i, :], U[:, 16 * (i >> 2) + 4 * g + (i & 3), m])
    W = torch.randn(128, 48, dtype=f64)
    Wl = packing.lane_fixed_feat(W)
    for st, tq in ((0, 0), (10, 3), (11, 7)):
        assert torch.equal(Wl[st, tq], W[16 * tq + m, 4 * st + g])
    W2 = torch.randn(128, 128, dtype=f64)
    W2l = packing.lane_fixed_w2(W2)                       # [64][64][4]: n = 4 i + j -> tau = n >> 5, r = (n >> 3) & 3, d = n & 7
    for n in (0, 9, 100, 255):
        assert torch.equal(W2l[n >> 2, :, n & 3], W2[8 * m + (n & 7), 16 * (n >> 5) + 4 * g + ((n >> 3) & 3)])


def test_knn_slot_order_is_free():
    c = sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS)
    g = torch.Generator().manual_seed(3)
    nbr, ew = c.nbr.clone(), c.ew.clone()
    for v in range(nbr.shape[0]):
        d = int(c.deg[v])
        p = torch.randperm(d, generator=g)
        nbr[v, :d], ew[v, :d] = c.nbr[v, :d][p], c.ew[v, :d][p]
    d = _copy(c, nbr=nbr, ew=ew)
    a, b = _knn(c, sr.KNN_NODE), _knn(d, sr.KNN_NODE)
    _close(b.S, a.S, a.S_scale, 'knn node S under a slot permutation')
    _close(b.out, a.out, a.out_scale, 'knn node out under a slot permutation')
    a, b = _knn(c, sr.KNN_POS), _knn(d, sr.KNN_POS)
    _close(b.dx, a.dx, a.dx_scale, 'knn pos dx under a slot permutation')


def test_softmax_shift_is_free():
    """A constant per head added to all logits of a segment, through U.  Key channel 0 is made the same for every row (no first-layer
    rows, no features, b' = 0.75: z rstd = 0.75 there), so U[0, h] += s_h / 0.75 adds s_h to every logit of head h."""
    c = sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS)
    t = _topo(c)
    Ck, Cd, bk = c.Csrc_k.clone(), c.Cdst_k.clone(), c.bk.clone()
    Wk = c.Wf[0][0].clone()
    Ck[:, 0], Cd[:, 0], Wk[0, :], bk[0] = 0.0, 0.0, 0.0, 0.75
    d = _copy(c, Csrc_k=Ck, Cdst_k=Cd, bk=bk)
    U, _ = sr.fold_query(c.q[c.ids.long()], c.W2k)
    U2 = U.clone()
    U2[:, 0, :] += torch.randn(c.ids.numel(), 16, dtype=f64) * 4.0 / 0.75
    for mode in (sr.KNN_NODE, sr.KNN_POS):
        a = sr.node_attn(d, t, mode, c.ids, Wk, c.Wf[0][1], U=U)
        b = sr.node_attn(d, t, mode, c.ids, Wk, c.Wf[0][1], U=U2)
        if mode == sr.KNN_NODE:
            _close(b.S, a.S, a.S_scale * 1e3, 'knn node S under a per-head logit shift')
            _close(b.swn, a.swn, a.swn * 1e3, 'knn node swn under a per-head logit shift')
        else:
            assert float((b.logit - a.logit)[a.valid].abs().max()) > 1.0          # the logits did move
            _close(b.dx, a.dx, a.dx_scale * 1e3, 'knn pos dx under a per-head logit shift')


def test_rigid_motion():
    R, sh = _rotation(), torch.tensor([0.3, -2.0, 1.1], dtype=f64)
    c = sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS)
    d = _copy(c, x=c.x.double() @ R.T + sh, nrm=c.nrm.double() @ R.T)
    a, b = _knn(c, sr.KNN_NODE), _knn(d, sr.KNN_NODE)
    _close(b.S, a.S, a.S_scale * 1e3, 'knn node S under a rigid motion')
    a, b = _knn(c, sr.KNN_POS), _knn(d, sr.KNN_POS)
    _close(b.dx, a.dx @ R.T, a.dx_scale.norm(dim=-1, keepdim=True).expand(-1, 3) * 1e3, 'knn pos dx rotates')
    c = sc.tri_case('small')
    t = _topo(c)
    d = _copy(c, x=c.x.double() @ R.T + sh)
    a, b = sr.triplet(c, t), sr.triplet(d, t)
    # (theta near 0 / pi amplifies the rotation's rounding by 1 / sin(theta): collinear atoms are 1e-8 apart in angle)
    _close(b.out, a.out, a.out_scale * 1e5, 'triplet out under a rigid motion')


@pytest.mark.parametrize('mode', (sr.KNN_NODE, sr.BOND_NODE))
def test_fused_is_fold_attend_unfold(mode):
    c = sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS) if mode == sr.KNN_NODE else sc.bond_case('t2')
    t = _topo(c)
    wf = c.Wf[0] if mode == sr.KNN_NODE else (None, None)
    fused = sr.node_attn(c, t, mode, c.ids, *wf)
    U, _ = sr.fold_query(c.q[c.ids.long()], c.W2k)
    assert torch.equal(U.float().double(), U)                       # the cases' fold is exact in fp32 (seg_attn_cases._common)
    plain = sr.node_attn(c, t, mode, c.ids, *wf, U=U)
    out, _ = sr.unfold_value(plain.S, plain.swn, c.W2v, c.b2v)
    _close(out, fused.out, fused.out_scale, f'mode {mode}: fused out = unfold(attend(fold))')
    # the fold against its definition, element by element
    s, cc, h = 3, 77, 5
    assert abs(float(U[s, cc, h]) - sum(float(c.q[c.ids[s], 8 * h + dd]) * float(c.W2k[8 * h + dd, cc]) for dd in range(8))) < 1e-12
    o = sum(float(c.W2v[8 * h + 2, k]) * float(plain.S[s, k, h]) for k in range(128)) + float(c.b2v[8 * h + 2]) * float(plain.swn[s, h])
    assert abs(float(out[s, 8 * h + 2]) - o) < 1e-12


def test_staged_and_generic_triplet_contracts_agree():
    c = sc.tri_case('small')
    t = _topo(c)
    a, b = sr.triplet(c, t, staged=True), sr.triplet(c, t, staged=False)
    _close(b.out, a.out, a.out_scale, 'triplet: Cdst rows = G . Wg2')
    empty = ~a.has
    assert bool(empty.any()) and bool((a.out[empty] == c.resid.double()[empty]).all())     # 2-atom ligand: no row, no bias
    assert bool((a.swn[a.has] - 1).abs().max() < 1e-12)


# ---- floors ----------------------------------------------------------------------------------------------------------------------
def _node_cases():
    for c in sc.knn_cases():
        yield f'knn {c.name}', c, (sr.KNN_NODE, sr.KNN_POS), c.Wf[0]
    for name in sc.BOND_SIZES:
        yield f'bond {name}', sc.bond_case(name), (sr.BOND_NODE, sr.BOND_POS), (None, None)
    for e in (False, True):
        c = sc.phore_case(e)
        yield c.name, c, (sr.PHORE,), (c.Wf_k, c.Wf_v)


_FLOOR = {}


def _floor(kind, case, r):
    tol = sc.TOL[kind]
    _FLOOR[kind] = max(_FLOOR.get(kind, 0.0), r)
    print(f'seg-attn fp32-restatement {kind:8s} {case:28s} {r:.3e}   (tolerance {tol:.1e}, 1 / {sc.MARGIN:g} of it {tol / sc.MARGIN:.1e})')
    assert r <= tol / sc.MARGIN, (kind, case, r)


@pytest.mark.parametrize('item', list(_node_cases()), ids=lambda i: i[0].replace(' ', '_'))
def test_float32_restatement_node_modes(item):
    name, c, modes, wf = item
    t = _topo(c)
    for mode in modes:
        a, b = sr.node_attn(c, t, mode, c.ids, *wf, dtype=f32), sr.node_attn(c, t, mode, c.ids, *wf)
        kinds = sc.POS_KINDS if mode in (sr.KNN_POS, sr.BOND_POS) else [k for k in sc.NODE_KINDS if k[0] != 'U']
        for kind, r in sc.ratios(a, b, kinds).items():
            _floor(kind, f'{name} mode {mode}', r)


@pytest.mark.parametrize('name', list(sc.TRI_SIZES))
def test_float32_restatement_triplet(name):
    c = sc.tri_case(name)
    t = _topo(c)
    a, b = sr.triplet(c, t, f32), sr.triplet(c, t)
    for kind, r in sc.ratios(a, b, [k for k in sc.TRI_KINDS if k[0] != 'U']).items():
        _floor(kind, f'triplet {name}', r)


@pytest.mark.parametrize('n', sc.FOLD_NS)
def test_float32_restatement_fold_unfold(n):
    c = sc.fold_case(n)
    (a, _), (b, s) = sr.fold_query(c.q, c.W2k, f32), sr.fold_query(c.q, c.W2k)
    _floor('U', f'fold n={n}', sc.ratio(a, b, s))
    (a, _), (b, s) = sr.unfold_value(c.S, c.swn, c.W2v, c.b2v, f32), sr.unfold_value(c.S, c.swn, c.W2v, c.b2v)
    _floor('out', f'unfold n={n}', sc.ratio(a, b, s))


# ---- sharpness -------------------------------------------------------------------------------------------------------------------
# output kinds every mistake must move by at least 10 x the tolerance on some case, and the cases it is looked for in
_NODE, _POS = ('S', 'swn', 'out', 'alpha'), ('dx',)
SHARP = {
    'drop_last_row': dict(knn=_NODE + _POS, bond=('S', 'out', 'alpha', 'dx'), tri=('S', 'tri_out', 'alpha')),
    'skip_row_16': dict(knn=_NODE + _POS, bond=('S', 'out', 'alpha', 'dx'), tri=('S', 'tri_out', 'alpha')),
    'gate_in_denominator': dict(knn=_NODE + _POS),
    'normals_swapped': dict(knn=_NODE + _POS + ('logit', 'v')),
    'target_not_excluded': dict(bond=('S', 'out', 'alpha', 'dx')),
    'bias_on_empty': dict(tri=('tri_out',)),
    'natural_base': dict(knn=_NODE + _POS, bond=('S', 'out', 'alpha', 'dx'), tri=('S', 'tri_out', 'alpha'), phore=('S', 'out', 'alpha')),
    'mean_subtracted': dict(knn=_NODE + _POS + ('logit', 'v'), bond=('S', 'out', 'alpha', 'dx', 'logit', 'v'), tri=('S', 'tri_out', 'alpha'),
                            phore=('S', 'out', 'alpha')),
    'smear_offset_shifted': dict(knn=_NODE + _POS + ('logit', 'v')),
}


def _family(fam, variant):
    """{kind: largest distance of the mistaken reference from the true one over the family's cases}."""
    worst = {}

    def take(r):
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    if fam == 'knn':
        for c in (sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS), sc.knn_case('k48', sc.KNN48_SIZES, 48, sc.DEGS48, seed=10)):
            for mode, kinds in ((sr.KNN_NODE, sc.NODE_KINDS[1:]), (sr.KNN_POS, sc.POS_KINDS)):
                take(sc.ratios(_knn(c, mode, variant=variant), _knn(c, mode), kinds))
    elif fam == 'bond':
        for name in ('t2', 't3'):
            c = sc.bond_case(name)
            t = _topo(c)
            for mode, kinds in ((sr.BOND_NODE, sc.NODE_KINDS[1:]), (sr.BOND_POS, sc.POS_KINDS)):
                take(sc.ratios(sr.node_attn(c, t, mode, c.ids, variant=variant), sr.node_attn(c, t, mode, c.ids), kinds))
    elif fam == 'tri':
        c = sc.tri_case('t3')
        t = _topo(c)
        take(sc.ratios(sr.triplet(c, t, variant=variant), sr.triplet(c, t), sc.TRI_KINDS[1:]))
    else:
        c = sc.phore_case(False)
        t = _topo(c)
        take(sc.ratios(sr.node_attn(c, t, sr.PHORE, c.ids, c.Wf_k, c.Wf_v, variant=variant), sr.node_attn(c, t, sr.PHORE, c.ids, c.Wf_k, c.Wf_v),
                       sc.NODE_KINDS[1:]))
    return worst


@pytest.mark.parametrize('variant', sr.VARIANTS)
def test_every_mistake_is_far_outside_the_tolerance(variant):
    assert set(SHARP) == set(sr.VARIANTS)
    for fam, kinds in SHARP[variant].items():
        worst = _family(fam, variant)
        for kind in kinds:
            tol = sc.TOL[kind]
            print(f'seg-attn mistake {variant:22s} {fam:5s} {kind:8s} {worst[kind]:.3e}   ({worst[kind] / tol:.1e} x the tolerance {tol:.1e})')
            assert worst[kind] >= 10 * tol, (variant, fam, kind, worst[kind])


def test_tolerances_are_margin_times_a_measured_floor():
    """TOL is a one-digit round-up: nothing in it is looser than ten times the margin over the floor the tests above measured (run
    after them in file order; alone it checks the table's shape only)."""
    assert sc.MARGIN >= 3.0 and set(sc.TOL) == {'U', 'S', 'swn', 'out', 'dx', 'tri_out', 'alpha', 'logit', 'v'}
    for kind, worst in _FLOOR.items():
        assert worst <= sc.TOL[kind] / sc.MARGIN
