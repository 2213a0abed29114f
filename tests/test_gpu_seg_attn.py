"""-m gpu: the forward segment-attention kernels (csrc/seg_attn.hip, node_attn.hip, triplet2.hip) through the C ABI, one launch per
check, element by element against the float64 restatement of the contract in tests/seg_attn_reference.py on the inputs of
tests/seg_attn_cases.py.

Every form of a case (plain two-pass, fused, fused + tiled, generic one-pass, training record; staged / split / generic / 8-wave
triplet) is held against the SAME reference output, never against another form.  First-layer rows are column slices of wider NaN
tensors, every output is NaN-prefilled with guard rows behind it: targets that are not listed and the guards must still be NaN
afterwards, every listed target finite.  Each error is printed with its bound (pytest -s) before it is asserted;
profiles/seg_attn_parity.md records them."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import pytest
import torch

import seg_attn_cases as sc
import seg_attn_reference as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
OK, ERR_ARG = 0, 1
G = sc.GUARD


def _lib():
    from phoregen_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=4)
def _plan(sizes):
    plan = sc.make_plan(sizes, DEV)
    return plan, sc.topo_of(plan)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _pair(a, b):
    """Two [R, 128] tensors as the column slices 4:132 and 136:264 of one NaN tensor (both 16-byte aligned, one row stride)."""
    buf = _nan(a.shape[0], 268)
    buf[:, 4:132], buf[:, 136:264] = a.to(DEV), b.to(DEV)
    return buf, buf[:, 4:132], buf[:, 136:264]


def _stage(c, contiguous_src=False):
    """The case's tensors on the device; the first-layer rows inside NaN tensors (the staged triplet kernel needs [n_bond, 256])."""
    d = NS(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in vars(c).items()})
    if contiguous_src:
        d.Csrc = c.Csrc.to(DEV).contiguous()
        d.Csrc_k, d.Csrc_v = d.Csrc[:, :128], d.Csrc[:, 128:]
    else:
        d._src_buf, d.Csrc_k, d.Csrc_v = _pair(c.Csrc_k, c.Csrc_v)
    d._dst_buf, d.Cdst_k, d.Cdst_v = _pair(c.Cdst_k, c.Cdst_v)
    return d


_STATS = {}


def _check(kind, form, case, got, ref, scale, mask=None):
    """|got - ref| <= TOL[kind] x scale for every element (of mask); printed before it is asserted."""
    if mask is not None:
        got, ref, scale = got[mask], ref[mask], scale[mask]
    assert bool(torch.isfinite(got).all()), (kind, form, case, 'an element was not written')
    tol = sc.TOL[kind]
    err = (got.double() - ref).abs()
    bound = tol * scale.double()
    e = float(err.max()) if err.numel() else 0.0
    r = sc.ratio(got, ref, scale) / tol
    st = _STATS.setdefault((form, kind), [0, 0.0, 0.0])
    st[0], st[1], st[2] = st[0] + 1, max(st[1], e), max(st[2], r)
    print(f'seg-attn kernel {form:28s} {kind:8s} {case:34s} {e:.3e}   (largest error / bound {r:.3f})')
    assert bool((err <= bound).all()), (kind, form, case, e, r)


def _untouched(buf, rows):
    """Every row of buf but `rows` is still NaN."""
    keep = torch.ones(buf.shape[0], dtype=torch.bool, device=DEV)
    keep[rows.long()] = False
    assert bool(torch.isnan(buf[keep]).all()), 'a row outside the target list (or a guard row) was written'


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(topo_ref, p, force=0, runs=None):
    """runs: (family, row tiles, threads, composite parts, floats per row of the record) the case's label promises; the library's own
    answer (pg_seg_attn_form) is held against it before the launch."""
    hip, lib, s = _lib()
    old = lib.pg_debug_force_generic_seg(force)
    try:
        if runs is not None:
            f = hip.seg_form(topo_ref, p)
            assert (hip.FORM_NAMES[f.family], f.tiles, f.threads, f.compose, f.record_floats) == runs, (hip.form_name(f), runs)
        rc = lib.pg_seg_attn(topo_ref, C.byref(p), s)
    finally:
        lib.pg_debug_force_generic_seg(old)
    torch.cuda.synchronize()
    return rc, lib.pg_last_error()


# ---- node-target modes -----------------------------------------------------------------------------------------------------------
def _node_args(d, mode, lists, n_ctx, form, accumulate=0, alpha=False, pos_tiled=0, alpha_rows=0, U=None):
    """PgSegAttn of one launch, filled field by field, and its NaN-prefilled outputs.  lists: [(ids, (Wf_k, Wf_v))] (one or two)."""
    from phoregen_amd import packing
    hip, _, _ = _lib()
    pos, knn = mode in (sr.KNN_POS, sr.BOND_POS), mode in (sr.KNN_NODE, sr.KNN_POS)
    p, keep = hip.PgSegAttn(), []
    hold = lambda t: (keep.append(t), t.data_ptr())[1]
    p.mode = mode
    ids32 = [l[0].to(torch.int32).to(DEV).contiguous() for l in lists]
    p.n_seg, p.seg_ids = ids32[0].numel(), hold(ids32[0])
    if len(lists) == 2:
        p.n_seg2, p.seg_ids2 = ids32[1].numel(), hold(ids32[1])
    p.x, p.nrm = _ptr(d.x), _ptr(d.nrm)
    if knn:
        p.nbr, p.deg, p.ew, p.knn_k = hold(d.nbr.contiguous()), hold(d.deg.contiguous()), hold(d.ew.contiguous()), d.knn_k
    p.Csrc_k, p.Csrc_v, p.ld_csrc = d.Csrc_k.data_ptr(), d.Csrc_v.data_ptr(), d.Csrc_k.stride(0)
    p.Cdst_k, p.Cdst_v, p.ld_cdst = d.Cdst_k.data_ptr(), d.Cdst_v.data_ptr(), d.Cdst_k.stride(0)
    for i, (_, wf) in enumerate(lists):
        if wf[0] is not None:
            lk, lv = packing.lane_fixed_feat(wf[0].to(DEV)).contiguous(), packing.lane_fixed_feat(wf[1].to(DEV)).contiguous()
            setattr(p, ('Wf_k', 'Wf_k2')[i], hold(lk))
            setattr(p, ('Wf_v', 'Wf_v2')[i], hold(lv))
    p.ln_gk = p.ln_bk = hold(d.bk.contiguous())                      # (the kernels read b' only; packing passes it for gamma too)
    p.ln_gv = p.ln_bv = hold(d.bv.contiguous())
    o = NS(keep=keep, S=None, swn=None, out=None, dx=None, alpha=None, U=None)
    all_ids = torch.cat(ids32).long()
    o.U = _nan(n_ctx + G, 32, 64)
    if form == 'plain':
        o.U[all_ids] = sr.lane_fixed_u(U.float())
    else:
        p.q, p.W2k_l = hold(d.q.contiguous()), hold(packing.lane_fixed_w2(d.W2k).contiguous())
    p.U = o.U.data_ptr()
    if pos:
        p.W2xv_l, p.b2xv = hold(packing.lane_fixed_xv(d.W2xv).contiguous()), hold(d.b2xv.contiguous())
        o.dx = _nan(n_ctx + G, 3)
        if accumulate:
            o.dx[all_ids] = d.dx0[all_ids]
        p.dx, p.accumulate_dx, p.pos_tiled = o.dx.data_ptr(), accumulate, pos_tiled
    else:
        o.S, o.swn = _nan(n_ctx + G, 32, 64), _nan(n_ctx + G, 16)
        p.S, p.swn = o.S.data_ptr(), o.swn.data_ptr()
        if form != 'plain':
            o.out = _nan(n_ctx + G, 128)
            p.W2v_l, p.b2v, p.out = hold(packing.lane_fixed_w2(d.W2v).contiguous()), hold(d.b2v.contiguous()), o.out.data_ptr()
    if alpha:
        o.alpha = _nan(n_ctx + G, alpha_rows, 32 if pos else 16)
        p.alpha, p.alpha_rows = o.alpha.data_ptr(), alpha_rows
    if getattr(d, 'efeat', None) is not None:
        p.efeat, p.efeat_off = hold(d.efeat.contiguous()), hold(d.efeat_off.contiguous())
    return p, o


def _node_form(case, plan, d, mode, lists, refs, form, force=0, tiles=0, tiled=0, **kw):
    """One launch of one form over one or two target lists, every output against the lists' references.  tiles: the row-tile instance
    of the node kernels that holds the case (0: none does, or force: the generic kernel); tiled: the tiled position form's, where
    pos_tiled is asked for and the form holds the case.  The label says what runs, and the library is asked whether it does."""
    from phoregen_amd import hip
    pos = mode in (sr.KNN_POS, sr.BOND_POS)
    n_ctx = plan.n_ctx
    U = torch.cat([r.U for r in refs]) if form == 'plain' else None
    p, o = _node_args(d, mode, lists, n_ctx, form, U=U, **kw)
    generic = bool(force & 1) or not tiles
    record = 0 if not kw.get('alpha') or (generic and mode != sr.PHORE) else 32 if pos else 16
    if generic:
        runs = ('generic', 0, 256, (hip.PG_FORM_FOLD_UNFOLD if form == 'fused' else 0) | (hip.PG_FORM_TWO_LISTS if len(lists) == 2 else 0), record)
    elif tiled:
        runs = ('pos_tiled', tiled, 768, 0, 0)
    elif form == 'fused':
        runs = ('node_fused', tiles, 768, 0, record)
    else:
        runs = ('node_two_pass', tiles, 256, hip.PG_FORM_TWO_LISTS if len(lists) == 2 else 0, record)
    rc, msg = _call(plan.topo_ref, p, force, runs)
    assert rc == OK, (rc, msg)
    name = f'{("knn", "knn", "bond", "bond", "triplet", "phore")[mode]} {("node", "pos")[pos]} {form}' + \
        (' generic' if generic and mode != sr.PHORE else '') + (' tiled' if tiled and not generic else '') + (' 2 lists' if len(lists) == 2 else '') + \
        (' record' if kw.get('alpha') else '')
    ids = torch.cat([l[0] for l in lists]).long().to(DEV)
    ref = NS(**{k: torch.cat([getattr(r, k) for r in refs]) for k in vars(refs[0]) if torch.is_tensor(getattr(refs[0], k))
                and getattr(refs[0], k).dim() > 0 and k not in ('valid', 'aw', 'logit', 'logit_scale', 'v', 'v_scale')})
    if pos:
        _untouched(o.dx, ids)
        want, scale = ref.dx, ref.dx_scale
        if kw.get('accumulate'):
            want, scale = want + d.dx0[ids].double(), scale + d.dx0[ids].double().abs()
        _check('dx', name, case, o.dx[ids], want, scale)
    elif o.out is not None:
        _untouched(o.out, ids)
        _check('out', name, case, o.out[ids], ref.out, ref.out_scale)
    else:
        _untouched(o.S, ids)
        _untouched(o.swn, ids)
        _check('S', name, case, sr.plain_u(o.S[ids]), ref.S, ref.S_scale)
        _check('swn', name, case, o.swn[ids], ref.swn, ref.swn)
    if form == 'plain':
        keep = torch.ones(n_ctx + G, dtype=torch.bool, device=DEV)
        keep[ids] = False
        assert bool(torch.isnan(o.U[keep]).all())
    if kw.get('alpha'):
        _untouched(o.alpha, ids)
        r = refs[0]
        R = r.valid.shape[1]
        if pos:
            got = o.alpha[ids][:, :R]
            _check('logit', name, case, got[..., :16], r.logit, r.logit_scale, r.valid[..., None].expand_as(r.logit))
            _check('v', name, case, got[..., 16:], r.v, r.v_scale, r.valid[..., None].expand_as(r.v))
            masked = got[..., :16][~r.valid[..., None].expand_as(r.logit)]
            masked = masked[~torch.isnan(masked)]
            assert bool((masked <= -0.5e30).all()), 'a row outside the segment carries a logit'
        else:
            got = o.alpha[ids][:, :R]
            if mode == sr.PHORE:                                     # rows past the graph's nodes are not part of the record
                got = torch.where(r.valid[..., None].expand_as(got), got, torch.zeros_like(got))
            _check('alpha', name, case, got, r.aw, r.aw)
    return o


def _node_refs(c, t, d, mode, lists):
    return [sr.node_attn(d, t, mode, ids.to(DEV), wf[0], wf[1]) for ids, wf in lists]


@pytest.mark.parametrize('idx', range(7), ids=('mixed', 'grouped', 'all_lig', 'all_phore', 'centred', 'rounds2', 'k48'))
def test_knn_modes_against_float64(idx):
    c = sc.knn_cases(_cu())[idx]
    plan, t = _plan(c.sizes)
    d = _stage(c)
    two_pass = c.knn_k <= 32
    if c.name == 'rounds2':
        assert c.ids.numel() > 12 * _cu()                            # a second round of the persistent fused kernel
    for mode in (sr.KNN_NODE, sr.KNN_POS):
        pos = mode == sr.KNN_POS
        lists = [(c.ids, c.Wf[0])]
        refs = _node_refs(c, t, d, mode, lists)
        run = functools.partial(_node_form, c.name, plan, d, mode, lists, refs, tiles=2 if two_pass else 0)
        run('plain', **(dict(accumulate=1) if pos else {}))
        run('fused')
        if pos:
            run('fused', pos_tiled=1, accumulate=1, tiled=2 if two_pass else 0)
        if c.name != 'rounds2':
            run('plain', force=1)
            run('fused', force=1, **(dict(accumulate=1) if pos else {}))
            if two_pass:
                run('plain', alpha=True, alpha_rows=c.knn_k)
                run('fused', alpha=True, alpha_rows=c.knn_k)
        if c.name in ('mixed', 'k48'):
            for split, (a, b) in c.splits.items():
                lists2 = [(a, c.Wf[0]), (b, c.Wf[1])]
                refs2 = _node_refs(c, t, d, mode, lists2)
                _node_form(f'{c.name} {split}', plan, d, mode, lists2, refs2, 'fused', tiles=2 if two_pass else 0)
                _node_form(f'{c.name} {split}', plan, d, mode, lists2, refs2, 'fused', force=1)


@pytest.mark.parametrize('name', list(sc.BOND_SIZES))
def test_bond_modes_against_float64(name):
    """MAXT 3 (t2, t3), 4 and 5 of the two-pass kernels, the tiled position form with 2, 3 and 4 tiles and its fallback at 5, and the
    one-pass kernel above 80 atoms."""
    c = sc.bond_case(name)
    plan, t = _plan(c.sizes)
    d = _stage(c)
    rows = plan.topo.max_nlig
    for mode in (sr.BOND_NODE, sr.BOND_POS):
        pos = mode == sr.BOND_POS
        lists = [(c.ids, (None, None))]
        refs = _node_refs(c, t, d, mode, lists)
        run = functools.partial(_node_form, c.name, plan, d, mode, lists, refs, tiles=dict(t2=3, t3=3, t4=4, t5=5, generic=0)[name])
        run('plain')
        run('fused', **(dict(accumulate=1) if pos else {}))
        if pos:
            run('fused', pos_tiled=1, tiled=dict(t2=2, t3=3, t4=4, t5=0, generic=0)[name])
        if name in ('t2', 't4', 'generic'):
            run('plain', force=1, **(dict(accumulate=1) if pos else {}))
            run('fused', force=1)
        if name != 'generic':
            run('plain', alpha=True, alpha_rows=rows)


@pytest.mark.parametrize('explicit', (False, True), ids=('distance', 'efeat'))
def test_phore_mode_against_float64(explicit):
    c = sc.phore_case(explicit)
    plan, t = _plan(c.sizes)
    d = _stage(c)
    lists = [(c.ids, (c.Wf_k, c.Wf_v))]
    refs = _node_refs(c, t, d, sr.PHORE, lists)
    _node_form(c.name, plan, d, sr.PHORE, lists, refs, 'plain')
    _node_form(c.name, plan, d, sr.PHORE, lists, refs, 'plain', alpha=True, alpha_rows=int(max(p for _, p in c.sizes)))


# ---- triplet ---------------------------------------------------------------------------------------------------------------------
def _tri_args(plan, d, queue=None, train=False, alpha=False, seg_ids=None, tri_grid=0, given_cdst=True):
    """queue: (tri_iters, n_tri_iters, tri_max_nlig, tri_counter) or None (the generic kernel)."""
    from phoregen_amd import packing
    hip, _, _ = _lib()
    nb = plan.n_bond
    p, keep = hip.PgSegAttn(), []
    hold = lambda t: (keep.append(t), t.data_ptr())[1]
    p.mode = sr.TRIPLET
    if seg_ids is not None:
        s32 = seg_ids.to(torch.int32).to(DEV).contiguous()
        p.n_seg, p.seg_ids = s32.numel(), hold(s32)
    else:
        p.n_seg = nb
    p.x = d.x.data_ptr()
    p.Csrc_k, p.Csrc_v, p.ld_csrc = d.Csrc_k.data_ptr(), d.Csrc_v.data_ptr(), d.Csrc_k.stride(0)
    if given_cdst:
        p.Cdst_k, p.Cdst_v, p.ld_cdst = d.Cdst_k.data_ptr(), d.Cdst_v.data_ptr(), d.Cdst_k.stride(0)
    p.G, p.Wg2_k, p.Wg2_v = hold(d.G.contiguous()), hold(d.Wg2_k.contiguous()), hold(d.Wg2_v.contiguous())
    p.Wf_k, p.Wf_v = hold(packing.lane_fixed_feat(d.Wf_k).contiguous()), hold(packing.lane_fixed_feat(d.Wf_v).contiguous())
    p.ln_gk = p.ln_bk = hold(d.bk.contiguous())
    p.ln_gv = p.ln_bv = hold(d.bv.contiguous())
    p.q, p.W2k_l = hold(d.q.contiguous()), hold(packing.lane_fixed_w2(d.W2k).contiguous())
    p.W2v_l, p.b2v = hold(packing.lane_fixed_w2(d.W2v).contiguous()), hold(d.b2v.contiguous())
    o = NS(keep=keep, S=None, swn=None, out=None, alpha=None, counter=None)
    if train:
        o.S, o.swn = _nan(nb + G, 32, 64), _nan(nb + G, 16)
        p.S, p.swn = o.S.data_ptr(), o.swn.data_ptr()
        U, _ = sr.fold_query(d.q, d.W2k)
        p.U = hold(sr.lane_fixed_u(U.float()))
        if alpha:
            o.alpha = _nan(nb + G, plan.topo.max_nlig, 16)
            p.alpha, p.alpha_rows = o.alpha.data_ptr(), plan.topo.max_nlig
    else:
        o.out = _nan(nb + G, 128)
        p.resid, p.out = hold(d.resid.contiguous()), o.out.data_ptr()
    if queue is not None:
        iters, n_it, max_n, counter = queue
        assert not bool(counter.any())
        p.tri_iters, p.n_tri_iters, p.tri_counter, p.tri_max_nlig, p.tri_grid = iters.data_ptr(), n_it, counter.data_ptr(), max_n, tri_grid
        o.counter = counter
    return p, o


def _tri_launch(plan, p, o, runs, force=0):
    """runs: (family, row tiles, threads) the launch's label promises."""
    rc, msg = _call(plan.topo_ref, p, force, runs + (0, 16 if o.alpha is not None and runs[0] != 'generic' else 0))
    assert rc == OK, (rc, msg)
    if o.counter is not None:
        assert not bool(o.counter.any()), 'tri_counter is not zero after the launch'


def _tri_check(form, case, o, ref, rows):
    rows = rows.long().to(DEV)
    if o.out is not None:
        _untouched(o.out, rows)
        _check('tri_out', form, case, o.out[rows], ref.out[rows], ref.out_scale[rows])
    else:
        _untouched(o.S, rows)
        _untouched(o.swn, rows)
        _check('S', form, case, sr.plain_u(o.S[rows]), ref.S[rows], ref.S_scale[rows])
        _check('swn', form, case, o.swn[rows], ref.swn[rows], ref.swn[rows])
    if o.alpha is not None:
        _untouched(o.alpha, rows)
        # rows [segment][atom k][head]: the atoms of the segment's ligand are written, the rest of a shorter ligand's block is not
        n_of = ref.n_of[rows]
        k = torch.arange(o.alpha.shape[1], device=DEV)[None, :] < n_of[:, None]
        m = k[..., None].expand(-1, -1, 16)
        assert bool(torch.isnan(o.alpha[rows][~m]).all())
        _check('alpha', form, case, o.alpha[rows], ref.aw[rows], ref.aw[rows], m)


@functools.lru_cache(maxsize=2)
def _tri_ref(name):
    c = sc.tri_case(name)
    plan, t = _plan(c.sizes)
    d = _stage(c, contiguous_src=True)
    ref = sr.triplet(d, t)
    ref.n_of = t.g_nlig[t.ctx_graph[t.bond_src]]
    return c, plan, t, d, ref


@pytest.mark.parametrize('name', ('t3', 't4', 't5'))
def test_staged_triplet_against_float64(name):
    """The staged kernel's 3-, 4- and 5-tile instances on 12 and 8 waves, with the plan's queue (tri_grid 0 and 3), the two tri_split
    queues as two launches, and the training S-form with its record."""
    c, plan, t, d, ref = _tri_ref(name)
    every = torch.arange(plan.n_bond)
    assert plan.n_tri_iters > 0
    queue = (plan.tri_iters, plan.n_tri_iters, 0, plan.tri_counter)
    tiles = dict(t3=3, t4=4, t5=5)[name]
    for grid in (0, 3):
        p, o = _tri_args(plan, d, queue, tri_grid=grid)
        _tri_launch(plan, p, o, ('tri_staged', tiles, 768))
        _tri_check(f'triplet staged grid={grid}', name, o, ref, every)
    p, o = _tri_args(plan, d, queue)
    _tri_launch(plan, p, o, ('tri_staged', tiles, 512), force=4)
    _tri_check('triplet staged 8 waves', name, o, ref, every)
    p, o = _tri_args(plan, d, queue, train=True, alpha=True)
    _tri_launch(plan, p, o, ('tri_staged_train', tiles, 768))
    _tri_check('triplet staged S-form', name, o, ref, every)
    assert plan.tri_split is not None or name == 't3'
    if plan.tri_split is not None:
        small_n = plan.tri_split['small'][2]
        is_small = (ref.n_of <= small_n).cpu()
        p, o = _tri_args(plan, d, plan.tri_split['small'])
        _tri_launch(plan, p, o, ('tri_staged', 3, 768))                                   # (the point of the split: the 3-tile instance)
        _tri_check('triplet staged split small', name, o, ref, every[is_small])       # the other queue's segments are still NaN
        p.tri_iters, p.n_tri_iters, p.tri_max_nlig, p.tri_counter = plan.tri_split['big'][0].data_ptr(), plan.tri_split['big'][1], \
            plan.tri_split['big'][2], plan.tri_split['big'][3].data_ptr()
        o.counter = plan.tri_split['big'][3]
        _tri_launch(plan, p, o, ('tri_staged', tiles, 768))
        _tri_check('triplet staged split both', name, o, ref, every)


@pytest.mark.parametrize('name', ('small', 'generic'))
def test_generic_triplet_against_float64(name):
    """No queue: the one-pass kernel, Cdst from G . Wg2, a shuffled strict subset of the edges; above 81 atoms the plan has no queue."""
    c, plan, t, d, ref = _tri_ref(name)
    if name == 'generic':
        assert plan.n_tri_iters == 0
    g = torch.Generator().manual_seed(5)
    ids = torch.randperm(plan.n_bond, generator=g)[:plan.n_bond - 5]
    p, o = _tri_args(plan, d, None, seg_ids=ids, given_cdst=False)
    _tri_launch(plan, p, o, ('generic', 0, 256))
    _tri_check('triplet generic', name, o, ref, ids)
    p, o = _tri_args(plan, d, None, train=True, seg_ids=ids)
    _tri_launch(plan, p, o, ('generic', 0, 256))
    _tri_check('triplet generic S-form', name, o, ref, ids)


# ---- fold / unfold on their own ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sc.FOLD_NS)
def test_fold_and_unfold_against_float64(n):
    from phoregen_amd import packing
    hip, lib, s = _lib()
    c = sc.fold_case(n)
    rows = c.q.shape[0]
    W2k_l, W2v_l = packing.lane_fixed_w2(c.W2k.to(DEV)).contiguous(), packing.lane_fixed_w2(c.W2v.to(DEV)).contiguous()
    Uref, Uscale = sr.fold_query(c.q.to(DEV), c.W2k.to(DEV))
    S, swn, b2v = c.S.to(DEV), c.swn.to(DEV).contiguous(), c.b2v.to(DEV)
    Sl = sr.lane_fixed_u(S)
    for with_ids in (True, False):
        ids = c.ids.to(DEV) if with_ids else None
        listed = c.ids.long().to(DEV) if with_ids else torch.arange(n, device=DEV)
        qbuf = _nan(rows, 140)                                          # ldq = 140 > 128, 16-byte aligned rows
        qbuf[:, 4:132] = c.q.to(DEV)
        U = _nan(rows + G, 32, 64)
        assert lib.pg_attn_fold_query(qbuf[:, 4:132].data_ptr(), 140, W2k_l.data_ptr(), n, _ptr(ids), U.data_ptr(), s) == OK
        torch.cuda.synchronize()
        _untouched(U, listed)
        _check('U', 'fold_query', f'n={n} ids={with_ids}', sr.plain_u(U[listed]), Uref[listed], Uscale[listed])
        for bias in (True, False):
            obuf = _nan(rows + G, 136)                                  # ldo = 136 > 128
            out = obuf[:, 4:132]
            assert lib.pg_attn_unfold_value(Sl.data_ptr(), swn.data_ptr() if bias else None, W2v_l.data_ptr(),
                                            b2v.data_ptr() if bias else None, n, _ptr(ids), out.data_ptr(), 136, s) == OK
            torch.cuda.synchronize()
            _untouched(obuf, listed)
            assert bool(torch.isnan(obuf[:, :4]).all()) and bool(torch.isnan(obuf[:, 132:]).all())
            ref, scale = sr.unfold_value(S, swn if bias else None, c.W2v.to(DEV), b2v if bias else None)
            _check('out', 'unfold_value', f'n={n} ids={with_ids} bias={bias}', out[listed], ref[listed], scale[listed])


# ---- refusals that happen before anything is launched ----------------------------------------------------------------------------
def test_arguments_refused_before_the_launch():
    hip, lib, s = _lib()
    c = sc.knn_case('mixed', sc.KNN_SIZES, 32, sc.DEGS)
    plan, t = _plan(c.sizes)
    d = _stage(c)
    lists = [(c.ids, c.Wf[0])]
    U, _ = sr.fold_query(d.q[c.ids.long().to(DEV)], d.W2k)
    # a feature table that is not 16-byte aligned
    p, o = _node_args(d, sr.KNN_NODE, lists, plan.n_ctx, 'plain', U=U)
    from phoregen_amd import packing
    odd = torch.zeros(12 * 8 * 64 + 4, device=DEV)
    odd[1:1 + 6144] = packing.lane_fixed_feat(c.Wf[0][0].to(DEV)).reshape(-1)
    p.Wf_k = odd.data_ptr() + 4
    rc, msg = _call(plan.topo_ref, p)
    assert rc == ERR_ARG and b'aligned' in msg, (rc, msg)
    assert bool(torch.isnan(o.S).all()) and bool(torch.isnan(o.swn).all())
    # a second target list outside the knn modes
    cb = sc.bond_case('t2')
    planb, _ = _plan(cb.sizes)
    db = _stage(cb)
    Ub, _ = sr.fold_query(db.q[cb.ids.long().to(DEV)], db.W2k)
    p, o = _node_args(db, sr.BOND_NODE, [(cb.ids, (None, None))], planb.n_ctx, 'plain', U=Ub)
    two = cb.ids[:2].to(torch.int32).to(DEV)
    p.n_seg2, p.seg_ids2 = 2, two.data_ptr()
    rc, msg = _call(planb.topo_ref, p)
    assert rc == ERR_ARG and b'second target list' in msg, (rc, msg)
    assert bool(torch.isnan(o.S).all())
    # the fused request without U scratch where the one-pass kernel has to run
    p, o = _node_args(d, sr.KNN_NODE, lists, plan.n_ctx, 'fused')
    p.U = None
    rc, msg = _call(plan.topo_ref, p, force=1)
    assert rc == ERR_ARG and b'scratch' in msg, (rc, msg)
    assert bool(torch.isnan(o.out).all())


def test_summary_of_the_run():
    """Per kernel form and output kind: checks, largest error, largest error / bound (the table of profiles/seg_attn_parity.md)."""
    for (form, kind), (n, e, r) in sorted(_STATS.items()):
        print(f'seg-attn summary {form:34s} {kind:8s} checks {n:3d}   largest error {e:.3e}   largest error / bound {r:.3f}')
        assert r <= 1.0
