"""CPU side of the segment-attention adjoint tests: what makes the gradient cases of tests/seg_attn_grad_cases.py well conditioned
and their tolerances honest, with no kernel in sight.

  * every gradient case is clear of the ReLU kink by KINK_MARGIN and its ligands meet `place`'s bounds;
  * floors: float32 autograd through tests/seg_attn_reference.py stays within TOL_GRAD / FLOOR_MULT of float64 autograd for every
    gradient kind, and its pre-activations within KINK_MARGIN / 100 of float64's;
  * sharpness: every deliberate mistake of seg_attn_reference.VARIANTS that applies to a mode moves at least one gradient kind by
    more than 100 x TOL_GRAD;
  * the lane-fixed feature and value-weight layouts are permutations, so a kernel's gradient is compared through the same map.
Only the cases with ligands of at most 34 atoms run here; the larger ones were measured once (profiles/seg_attn_bwd_parity.md) and run
on the GPU.  Each figure is printed (pytest -s) before it is asserted."""
import functools

import pytest
import torch

import seg_attn_cases as sc
import seg_attn_grad_cases as gc
import seg_attn_reference as sr

f64, f32 = gc.f64, gc.f32


@functools.lru_cache(maxsize=None)
def _ref(kind, name, mode, li):
    return gc.grads(gc.grad_case(kind, name), mode, f64, li)


def test_lane_fixed_weight_layouts_are_permutations():
    from phoregen_amd import packing
    for F in (4, 12, 48):
        W = torch.arange(128 * F, dtype=f64).reshape(128, F)
        assert torch.equal(torch.sort(packing.lane_fixed_feat(W).reshape(-1)).values, W.reshape(-1)), F
    W = torch.arange(16 * 128, dtype=f64).reshape(16, 128)
    assert torch.equal(torch.sort(packing.lane_fixed_xv(W).reshape(-1)).values, W.reshape(-1))
    U = torch.arange(3 * 2048, dtype=f64).reshape(3, 128, 16)
    assert torch.equal(torch.sort(sr.lane_fixed_u(U).reshape(-1)).values, U.reshape(-1))


def test_place_meets_its_bounds():
    g = sc._gen(1)
    for n in (1, 2, 3, 34):
        d, s = gc.geometry_bounds(gc.place(n, g))
        assert d >= gc.MIN_DIST and s >= gc.MIN_SIN, (n, d, s)
    # ... and the bounds see what the forward cases plant
    d, s = gc.geometry_bounds(torch.tensor([[0., 0, 0], [1e-3, 0, 0], [1, 1, 0]]))
    assert d < 2e-3
    d, s = gc.geometry_bounds(torch.tensor([[0., 0, 0], [1, 0, 0], [2, 1e-3, 0]]))
    assert s < 2e-3


@pytest.mark.parametrize('kn', gc.SMALL_CASES, ids=gc.case_id)
def test_gradient_cases_are_off_the_kink_and_well_placed(kn):
    c = gc.grad_case(*kn)
    t = gc.topo(c)
    assert c.kink_rounds <= gc.KINK_ROUNDS
    assert gc.near_kink(c, gc.KINK_MARGIN, t) == []
    print(f'seg-attn gradient case {gc.case_id(kn):16s} off the kink after {c.kink_rounds} round(s)')
    if c.kind != 'phore':
        for gi in range(t.g_nlig.numel()):
            n, l0 = int(t.g_nlig[gi]), int(t.g_ctx_off[gi] + t.g_nph[gi])
            d, s = gc.geometry_bounds(c.x[l0:l0 + n])
            assert d >= gc.MIN_DIST and s >= gc.MIN_SIN, (gi, n, d, s)
    if c.kind == 'tri':
        fwd = sc.tri_case(kn[1], sizes=gc.TRI_GRAD_SIZES[kn[1]])
        assert torch.equal(c.q, fwd.q) and torch.equal(c.W2k, fwd.W2k)                     # the grid of the query fold is untouched
        assert bool((c.Cdst_k.double() == c.G.double() @ c.Wg2_k.double()).all()) and bool((c.Cdst_v.double() == c.G.double() @ c.Wg2_v.double()).all())
        assert torch.equal(c.Csrc[:, :128], c.Csrc_k) and torch.equal(c.Csrc[:, 128:], c.Csrc_v)


_FLOOR = {}


@pytest.mark.parametrize('kn', gc.SMALL_CASES, ids=gc.case_id)
def test_float32_autograd_restatement(kn):
    c = gc.grad_case(*kn)
    t = gc.topo(c)
    for li in range(len(c.lists)):
        a, b = [], []
        gc._run(c, t, c.node_mode, li, f64, pre=a)
        gc._run(c, t, c.node_mode, li, f32, pre=b)
        worst = 0.0
        for ea, eb in zip(a, b):
            for path in 'kv':
                r = ((eb.pre[path].double() - ea.pre[path]).abs() / gc.kink_scale(ea, path))[ea.valid[..., None].expand_as(ea.pre[path])]
                worst = max(worst, float(r.max()) if r.numel() else 0.0)
        print(f'seg-attn fp32 pre-activation   {gc.case_id(kn):16s} list {li}  {worst:.3e}   (KINK_MARGIN / 100 = {gc.KINK_MARGIN / 100:.1e})')
        assert worst <= gc.KINK_MARGIN / 100
        for mode in gc.modes_of(c):
            for kind, r in gc.kind_ratios(gc.grads(c, mode, f32, li, t=t), _ref(*kn, mode, li)).items():
                tol = gc.TOL_GRAD[kind]
                _FLOOR[kind] = max(_FLOOR.get(kind, 0.0), r)
                print(f'seg-attn fp32 autograd         {gc.case_id(kn):16s} list {li} mode {mode} {kind:6s} {r:.3e}   (tolerance {tol:.0e}, 1 / {gc.FLOOR_MULT:g} of it {tol / gc.FLOOR_MULT:.1e})')
                assert r <= tol / gc.FLOOR_MULT, (kind, kn, mode, r)


# the mistakes that apply to a mode (gate_in_denominator: only the knn modes have a gate; bias_on_empty changes `out` alone, which no
# adjoint differentiates) and the case each is looked for in
MISTAKES = {
    ('knn', 'mixed'): ('drop_last_row', 'skip_row_16', 'gate_in_denominator', 'normals_swapped', 'natural_base', 'mean_subtracted', 'smear_offset_shifted'),
    ('bond', 't2'): ('drop_last_row', 'skip_row_16', 'target_not_excluded', 'natural_base', 'mean_subtracted'),
    ('tri', 'g18'): ('drop_last_row', 'skip_row_16', 'natural_base', 'mean_subtracted'),
    ('phore', False): ('drop_last_row', 'skip_row_16', 'natural_base', 'mean_subtracted'),
}
SEPARATION = 100.0


@pytest.mark.parametrize('kn', list(MISTAKES), ids=gc.case_id)
def test_every_mistake_moves_a_gradient_far_outside_the_tolerance(kn):
    assert {v for vs in MISTAKES.values() for v in vs} == set(sr.VARIANTS) - {'bias_on_empty'}
    c = gc.grad_case(*kn)
    t = gc.topo(c)
    for mode in gc.modes_of(c):
        for variant in MISTAKES[kn]:
            moved = {k: r / gc.TOL_GRAD[k] for k, r in gc.kind_ratios(gc.grads(c, mode, f64, 0, variant, t=t), _ref(*kn, mode, 0)).items()}
            best = max(moved, key=moved.get)
            print(f'seg-attn gradient mistake {variant:22s} {gc.case_id(kn):12s} mode {mode}  {best:6s} moves by {moved[best]:.1e} x its tolerance; '
                  f'kinds beyond {SEPARATION:g} x: {sorted(k for k, v in moved.items() if v > SEPARATION)}')
            assert moved[best] > SEPARATION, (variant, kn, mode, moved)


def test_tolerances_are_floor_mult_times_a_measured_floor():
    """(Run after the floors above in file order; alone it checks the table's shape only.)"""
    assert gc.FLOOR_MULT >= 3.0 and set(gc.TOL_GRAD) == set(gc.KIND_OF.values())
    assert gc.KINK_MARGIN >= 100 * gc.PRE_FLOOR
    for kind, worst in _FLOOR.items():
        assert worst <= gc.TOL_GRAD[kind] / gc.FLOOR_MULT
