"""-m gpu: the segment-attention ADJOINT kernels (csrc/seg_attn_bwd.hip, csrc/triplet_bwd2.hip) element by element against float64
autograd through tests/seg_attn_reference.py, on the gradient cases of tests/seg_attn_grad_cases.py.

Every check is one forward plus one backward of training.seg_core -- the product's own single-sub-layer entry, with the product's
own allocation of the record, the row buffer and the two-pass scratch; no PgSegAttn / PgSegAttnGrad is filled here.  `cfg` is built as
TrainForward._attention and TrainForward.denoise build it.  Every form of a case (options.override) is held against the SAME
float64 gradients, never against another form, and training.form_log says which form ran.

Staging: Ydst / Ysrc are column slices of wider NaN-filled tensors (the adjoint's ld_cdst / ld_csrc / ld_gcdst handling; the triplet's
Ysrc is the one contiguous [n_bond, 256] tensor the staged forward requires), U is [n, 2048] with NaN in the rows outside the target
list, and so are the cotangents.  Checked per launch: every gradient kind of the mode within TOL_GRAD of the reference (where the
reference is exactly zero -- rows of gCdst / gew outside the target list, gx / gnrm of nodes no segment touches, feature columns
nothing feeds -- the kernel's must be exactly zero), and all of it finite.  gU rows outside the target list are NOT looked at:
SegCoreFn leaves them unwritten (torch.empty) and FoldFn's adjoint reads the listed rows only.
Each ratio is printed beside its bound (pytest -s) before it is asserted; profiles/seg_attn_bwd_parity.md records them."""
import functools

import pytest
import torch

import seg_attn_cases as sc
import seg_attn_grad_cases as gc
import seg_attn_reference as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
MODE_NAMES = ('knn node', 'knn pos', 'bond node', 'bond pos', 'triplet', 'phore')


@functools.lru_cache(maxsize=None)
def _setup(kind, name, well=True):
    c = gc.grad_case(kind, name, well)
    plan = sc.make_plan(c.sizes, DEV)
    return c, plan, sc.topo_of(plan)


@functools.lru_cache(maxsize=None)
def _ref(kind, name, mode, li):
    """float64 autograd on the device, once per (case, mode, list)."""
    c, plan, t = _setup(kind, name)
    return gc.grads(c, mode, gc.f64, li, device=DEV, t=t)


def _wide(a, b):
    """[R, 128] | [R, 128] as the column slice 4:260 of one NaN leaf [R, 268] (16-byte aligned rows, row stride 268)."""
    buf = torch.full((a.shape[0], 268), NAN, device=DEV)
    buf[:, 4:132], buf[:, 132:260] = a.to(DEV), b.to(DEV)
    buf.requires_grad_(True)
    return buf, buf[:, 4:260]


def _leaf(t):
    return None if t is None else t.to(DEV).float().contiguous().detach().clone().requires_grad_(True)


def _launch(c, plan, mode, li, **opts):
    """One forward and one backward of training.seg_core under `opts`: ({name: kernel gradient in the reference's layout}, raw leaf
    gradients for the zero checks, the (direction, form name) the launch logged)."""
    from phoregen_amd import hip, options, packing, training
    L = c.lists[li]
    tri, pos, knn = mode == sr.TRIPLET, mode in (sr.KNN_POS, sr.BOND_POS), mode in (sr.KNN_NODE, sr.KNN_POS)
    n_rows = plan.n_bond if tri else plan.n_ctx
    ids = None if tri else L.ids.to(torch.int32).to(DEV).contiguous()
    listed = torch.arange(n_rows, device=DEV) if tri else L.ids.long().to(DEV)
    U, _ = sr.fold_query(c.q if tri else c.q[L.ids.long()], c.W2k)
    U_l = torch.full((n_rows, 2048), NAN, device=DEV)
    U_l[listed] = sr.lane_fixed_u(U.float()).reshape(-1, 2048).to(DEV)
    U_l.requires_grad_(True)
    dst_buf, Ydst = _wide(c.Cdst_k, c.Cdst_v)
    if tri:
        src_buf = _leaf(c.Csrc)
        Ysrc = src_buf
    else:
        src_buf, Ysrc = _wide(c.Csrc_k, c.Csrc_v)
    x, nrm, ew = _leaf(c.x), _leaf(c.nrm) if knn else None, _leaf(c.ew) if knn else None
    Wf_k = None if L.Wf_k is None else _leaf(packing.lane_fixed_feat(L.Wf_k.to(DEV)))
    Wf_v = None if L.Wf_v is None else _leaf(packing.lane_fixed_feat(L.Wf_v.to(DEV)))
    bk, bv = _leaf(c.bk), _leaf(c.bv)
    W2xv_l, b2xv = (_leaf(packing.lane_fixed_xv(c.W2xv.to(DEV))), _leaf(c.b2xv)) if pos else (None, None)
    max_lig = int(plan.num_atoms.max())
    if tri:
        cfg = dict(mode=mode, n_seg=plan.n_bond, seg_ids=None, k=32, topo=plan.topo_ref, plan=plan, n_out_rows=plan.n_bond, max_rows=max_lig,
                   need_gx=True,
                   tri_fwd=dict(q=c.q.to(DEV).contiguous(), W2k_l=packing.lane_fixed_w2(c.W2k.to(DEV)).contiguous(),
                                W2v_l=packing.lane_fixed_w2(c.W2v.to(DEV)).contiguous(), b2v=c.b2v.to(DEV), Wg2_k=c.Wg2_k.to(DEV).contiguous(),
                                Wg2_v=c.Wg2_v.to(DEV).contiguous(), G=c.G.to(DEV).contiguous(), seg_ids=plan.tri_order, seg_chunks=plan.tri_chunks,
                                tri_iters=plan.tri_iters, n_tri_iters=plan.n_tri_iters, tri_counter=plan.tri_counter))
    else:
        cfg = dict(mode=mode, n_seg=ids.numel(), seg_ids=ids, k=c.knn_k if knn else 32, topo=plan.topo_ref,
                   nbr=c.nbr.to(DEV).contiguous() if knn else None, deg=c.deg.to(DEV).contiguous() if knn else None, n_out_rows=plan.n_ctx,
                   max_rows=c.knn_k if knn else int(plan.g_nph.max()) if mode == sr.PHORE else max_lig, need_gx=mode != sr.PHORE)
    kw = dict(Wf_k=Wf_k, Wf_v=Wf_v, bk=bk, bv=bv)
    cot = c.cot[li]
    full = lambda v, w: torch.full((n_rows, w), NAN, device=DEV).index_copy(0, listed, v.to(DEV).reshape(-1, w))
    training.form_log = log = []
    try:
        with options.override(**opts):
            training.zero_pool.begin_step()
            if pos:
                dx = training.seg_core(cfg, Ydst, Ysrc, U_l, x, nrm, ew, W2xv_l=W2xv_l, b2xv=b2xv, **kw)
                torch.autograd.backward([dx], [full(cot['gdx'], 3)])
            else:
                S, swn = training.seg_core(cfg, Ydst, Ysrc, U_l, x, nrm, ew, **kw)
                torch.autograd.backward([S, swn], [full(sr.lane_fixed_u(cot['gS']), 2048), full(cot['gswn'], 16)])
    finally:
        training.form_log = None
    torch.cuda.synchronize()
    assert all(m == mode for _, m, _ in log)
    raw = dict(dst=dst_buf.grad, src=src_buf.grad, U=U_l.grad)
    g = dict(gU=sr.plain_u(U_l.grad[listed].reshape(-1, 32, 64)), gCdst_k=dst_buf.grad[:, 4:132], gCdst_v=dst_buf.grad[:, 132:260], gbk=bk.grad, gbv=bv.grad)
    g['gCsrc_k'], g['gCsrc_v'] = (src_buf.grad[:, :128], src_buf.grad[:, 128:]) if tri else (src_buf.grad[:, 4:132], src_buf.grad[:, 132:260])
    if mode != sr.PHORE:
        g['gx'] = x.grad
    else:
        assert x.grad is None                                            # need_gx = False: no coordinate gradient is formed
    if knn:
        g['gnrm'], g['gew'] = nrm.grad, ew.grad
    if Wf_k is not None:
        g['gWf_k'], g['gWf_v'] = Wf_k.grad, Wf_v.grad
    if pos:
        g['gW2xv'], g['gb2xv'] = W2xv_l.grad, b2xv.grad
    return g, raw, [(d, n) for d, _, n in log], listed


_STATS = {}


def _check(kn, mode, li, want_form, finite_only=False, well=True, **opts):
    """want_form: (family, with the forward's record or not, substrings the form name must hold)."""
    from phoregen_amd import packing
    c, plan, t = _setup(*kn, well)
    g, raw, log, listed = _launch(c, plan, mode, li, **opts)
    ran = [n for d, n in log if d == 'adjoint']
    assert len(ran) == 1, log
    family, record, *parts = want_form
    label = f'{MODE_NAMES[mode]:9s} {gc.case_id(kn):12s} {c.lists[li].label:5s} {ran[0]:40s} {",".join(f"{k}={v}" for k, v in opts.items()) or "default"}'
    form_ok = ran[0].split('/')[0] == family and ('/rec' in ran[0]) == record and all(p in ran[0] for p in parts)
    for name, got in g.items():
        assert got is not None and bool(torch.isfinite(got).all()), (label, name, 'a gradient is missing or not finite')
    for k in ('dst', 'src'):
        assert bool(torch.isfinite(raw[k]).all()), (label, k)
    if finite_only:
        print(f'seg-attn adjoint {label}  finite on the degenerate geometry')
        assert form_ok, (label, want_form, log)
        return
    ref = _ref(*kn, mode, li)
    # columns of the wide staging tensors outside the slices take no gradient
    assert not bool(raw['dst'][:, :4].any()) and not bool(raw['dst'][:, 260:].any())
    out = torch.ones(raw['dst'].shape[0], dtype=torch.bool, device=DEV)
    out[listed] = False
    assert not bool(raw['dst'][out].any()), (label, 'gCdst of a row outside the target list is not zero')
    if 'gew' in g:
        assert not bool(g['gew'][out].any()), (label, 'gew of a row outside the target list is not zero')
    worst, scales = {}, gc.scales(ref)
    for name, got in g.items():
        want, scale = ref[name], scales[name]
        if name in ('gWf_k', 'gWf_v'):                                   # (a permutation, and one scale for the whole tensor)
            want, scale = packing.lane_fixed_feat(want), packing.lane_fixed_feat(scale)
        elif name == 'gW2xv':
            want, scale = packing.lane_fixed_xv(want), packing.lane_fixed_xv(scale)
        kind = gc.KIND_OF[name]
        worst[kind] = max(worst.get(kind, 0.0), sc.ratio(got, want, scale))
    # terms one accumulator of a summed parameter gradient takes one after the other: at least those of the launch over the persistent
    # workgroups asked for (the launch may run fewer)
    chain = -(-gc.n_terms(c, li) // int(opts.get('tri_bwd_grid' if mode == sr.TRIPLET and 'tri_bwd_grid' in opts else 'bwd_grid', 256)))
    tol = {k: gc.tol_of(k, chain) for k in worst}
    line = '  '.join(f'{k} {r / tol[k]:.3f}' for k, r in worst.items())
    print(f'seg-attn adjoint {label}  chain {chain:6d}  ratio / bound: {line}')
    for k, r in worst.items():
        st = _STATS.setdefault((MODE_NAMES[mode], ran[0], k), [0, 0.0, 0.0])
        st[0], st[1], st[2] = st[0] + 1, max(st[1], r), max(st[2], r / tol[k])
    assert form_ok, (label, want_form, log)
    bad = {k: (r, tol[k]) for k, r in worst.items() if not r <= tol[k]}
    assert not bad, (label, bad)


ONE, ONE_REC, TWO = ('bwd_one_wave', False), ('bwd_one_wave', True), ('bwd_two_pass', True)


@pytest.mark.parametrize('name', ('mixed', 'grouped', 'k48'))
def test_knn_adjoints_against_float64_autograd(name):
    """k = 32: the two-pass form, the one-wave form fed by the forward's record and the one without a record (the position update's
    one-wave form recomputes its logits: it reads no record either way); bwd_grid = 2: a workgroup walks many segments.  k = 48 is
    beyond PG_SEG_KNN_MAX_K: no record, whatever is asked for.  mixed: the ligand and the pharmacophore list, each with its own Wf."""
    kn = ('knn', name)
    c, _, _ = _setup(*kn)
    for mode in gc.modes_of(c):
        pos = mode == sr.KNN_POS
        for li in range(len(c.lists)):
            if name == 'k48':
                _check(kn, mode, li, ONE)
                _check(kn, mode, li, ONE, bwd_split='none')
                continue
            _check(kn, mode, li, TWO, bwd_split='all')
            _check(kn, mode, li, ONE if pos else ONE_REC, bwd_split='none')
            _check(kn, mode, li, ONE, tri_onepass=False)
        if name == 'mixed':
            _check(kn, mode, 0, TWO, bwd_grid=2)


@pytest.mark.parametrize('name', ('t2', 't3', 't5', 'generic'))
def test_bond_adjoints_against_float64_autograd(name):
    """1 ... 32 atoms with tails of 1, 15 and 16 rows (t2), 3 and 5 row tiles (t3, t5), and 81 atoms, beyond the record's limit."""
    kn = ('bond', name)
    c, _, _ = _setup(*kn)
    for mode in gc.modes_of(c):
        pos = mode == sr.BOND_POS
        with_record = ONE if (pos or name == 'generic') else ONE_REC
        _check(kn, mode, 0, with_record)
        _check(kn, mode, 0, ONE, tri_onepass=False)
        if name == 't2':
            _check(kn, mode, 0, with_record, bwd_grid=2)


CHANNEL = 'bwd_channel_split'


@pytest.mark.parametrize('name', ('g18', 'g33', 'b64', 'b65'))
def test_triplet_adjoints_against_float64_autograd(name):
    """g33 straddles PG_SEG_BWD_TRI_FORM2_ATOMS: tri_bwd_form = 2 makes both of its launches (g18: the 8-wave launch alone); b64 / b65 lie
    on either side of PG_SEG_BWD_TRI_MAX_ATOMS and run under the default options."""
    from phoregen_amd import hip
    kn = ('tri', name)
    m = sr.TRIPLET
    if name == 'g18':
        _check(kn, m, 0, (CHANNEL, False, '/512'))
    elif name == 'g33':
        _check(kn, m, 0, (CHANNEL, False, '/512+', '/256'), tri_bwd_form=2)
        _check(kn, m, 0, (CHANNEL, False, '/256'), tri_bwd_form=1)
        _check(kn, m, 0, TWO, tri_bwd_form=0, bwd_split='all')
        _check(kn, m, 0, ONE_REC, tri_bwd_form=0, bwd_split='none')
        _check(kn, m, 0, ONE, tri_bwd_form=0, tri_onepass=False)
        _check(kn, m, 0, (CHANNEL, False, '/512+'), tri_bwd_grid=2)
        _check(kn, m, 0, (CHANNEL, False, '/512+'), bwd_atom_sort=False)
        _check(kn, m, 0, TWO, tri_bwd_form=0, bwd_atom_sort=False)
    elif name == 'b64':
        assert hip.PG_SEG_BWD_TRI_MAX_ATOMS == 64
        _check(kn, m, 0, (CHANNEL, False, '/512+', '/256'))
    else:
        _check(kn, m, 0, ('bwd_one_wave', True, '/128'))


@pytest.mark.parametrize('onepass', (True, False), ids=('record', 'generic'))
def test_phore_adjoint_against_float64_autograd(onepass):
    """PHORE_SIZES, distances from x (training.seg_core has no explicit edge feature: tests/test_gpu_seg_attn.py holds the forward's);
    need_gx = False."""
    _check(('phore', False), sr.PHORE, 0, ONE_REC if onepass else ONE, ph_onepass=onepass)


@pytest.mark.parametrize('kn', gc.DEGENERATE_CASES, ids=gc.case_id)
def test_gradients_are_finite_on_degenerate_geometry(kn):
    """The forward cases as they are -- atoms 1e-3 apart, collinear triples, pre-activations at the kink -- under the default form:
    float64 and float32 autograd disagree there, so no value is compared; every gradient must be finite."""
    c, _, _ = _setup(*kn, False)
    want = dict(knn=TWO, bond=None, tri=(CHANNEL, False), phore=ONE_REC)[kn[0]]
    for mode in gc.modes_of(c):
        for li in range(len(c.lists)):
            _check(kn, mode, li, want or (ONE if mode == sr.BOND_POS else ONE_REC), finite_only=True, well=False)


def test_summary_of_the_run():
    """Per mode, adjoint form and gradient kind: checks and the largest ratio / bound (the table of profiles/seg_attn_bwd_parity.md)."""
    for (mode, form, kind), (n, r, rb) in sorted(_STATS.items()):
        print(f'seg-attn adjoint summary {mode:9s} {form:40s} {kind:6s} checks {n:3d}   largest ratio {r:.3e}   largest ratio / bound {rb:.3f}')
        assert rb <= 1.0
