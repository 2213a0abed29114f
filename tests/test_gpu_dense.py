"""-m gpu: the dense kernels (csrc/gemm.hip, gemm_stream.hip, train_ops.hip) through the C ABI, one launch per check, element by
element against the float64 restatements of tests/dense_reference.py on the inputs of tests/dense_cases.py.

`exact` inputs (small integers) must come out bit for bit: that every row, every k and every gathered operand is taken exactly once
has no tolerance.  `real` inputs meet a per-element bound computed from the reference alone.  Every operand is a column slice of a
wider tensor whose other columns are NaN, every output a slice of a NaN buffer with guard columns on both sides and 64 guard rows
behind it; the guards must stay NaN.  Shapes that decide whether a grid-stride loop repeats follow the device's compute-unit count.
Each error is printed with its bound (pytest -s) before it is asserted; profiles/dense_parity.md records them."""
import ctypes as C

import pytest
import torch

import dense_cases as dc
import dense_reference as dref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
OK, ERR_ARG = 0, 1


def _lib():
    from phoregen_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _width(n):
    return -(-n // 4) * 4


def _emb(t, left=4, right=3, guard=0):
    """A CPU [R, C] tensor as columns left .. left+C of a wider NaN tensor on the device (row stride a multiple of 4 floats, so the
    slice is 16-byte aligned exactly when `left` is a multiple of 4).  Returns (buffer, view)."""
    R, Cn = t.shape
    buf = torch.full((R + guard, _width(left + Cn + right)), NAN, device=DEV)
    v = buf[:R, left:left + Cn]
    v.copy_(t)
    return buf, v


def _emb1(t, left=4):
    buf = torch.full((left + t.numel() + 4,), NAN, device=DEV)
    v = buf[left:left + t.numel()]
    v.copy_(t)
    return buf, v


def _out(R, Cn, left=4, right=3):
    buf = torch.full((R + dc.GUARD, _width(left + Cn + right)), NAN, device=DEV)
    return buf, buf[:R, left:left + Cn]


def _guards_nan(buf, view):
    """Everything of buf outside view is still NaN."""
    keep = torch.ones_like(buf, dtype=torch.bool)
    off = (view.data_ptr() - buf.data_ptr()) // 4
    if buf.dim() == 1:
        keep[off:off + view.numel()] = False
    else:
        r0, c0 = divmod(off, buf.stride(0))
        keep[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    assert bool(torch.isnan(buf[keep]).all()), 'written outside the output'


def _ptr(t):
    return None if t is None else t.data_ptr()


def _check_exact(kind, case, got, ref):
    assert bool(torch.isfinite(got).all()), (kind, case, 'an element was not written')
    r32 = ref.to(torch.float32)
    assert bool((r32.double() == ref).all())                                   # the reference is an fp32 number
    bad = int((got != r32).sum())
    print(f'dense kernel {kind:26s} {case:58s} exact: {bad} of {got.numel()} elements differ')
    assert torch.equal(got, r32), (kind, case, bad, torch.nonzero(got != r32)[:6].tolist())


def _check_bound(kind, case, got, ref, bound):
    assert bool(torch.isfinite(got).all()), (kind, case, 'an element was not written')
    bound = torch.broadcast_to(torch.as_tensor(bound, dtype=torch.float64, device=got.device), ref.shape)
    err = (got.double() - ref).abs()
    ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0
    e, b = (float(err.max()), float(bound.max())) if err.numel() else (0.0, 0.0)
    print(f'dense kernel {kind:26s} {case:58s} {e:.3e}   (bound up to {b:.3e}, largest error / bound {ratio:.3f})')
    assert bool((err <= bound).all()), (kind, case, e, ratio)


# ---- pg_gemm ----
def _stage_gemm(a, c=None):
    """The reference's keyword arguments (CPU) as device tensors laid out for the launch: slices of wider NaN tensors."""
    off = lambda k, d=4: getattr(c, k, d) if c is not None else d
    d = {}
    for k, v in a.items():
        if k in ('X', 'X2'):
            d[k] = _emb(v, off('xoff') if k == 'X' else 2, 3)[1]
        elif k == 'W':
            d[k] = _emb(v, off('woff'), 5)[1]
        elif k in ('add1', 'add2'):
            d[k] = _emb(v, off('addoff'), 1)[1]
        elif k == 'bias':
            d[k] = _emb1(v, {'aligned': 4, 'off1': 1, 'off3': 3}[off('bias', 'aligned')])[1]
        elif k == 'ln':
            d[k] = (v[0].to(DEV), v[1].to(DEV))
        elif torch.is_tensor(v):
            d[k] = v.to(DEV)
        else:
            d[k] = v
    return d


def _run_gemm(d, streaming, yoff=4, y_rows=None):
    """One pg_gemm on staged operands d.  Returns the [y_rows or M, N] output view after the guard check."""
    hip, lib, s = _lib()
    X, W = d['X'], d['W']
    M = d['rows'].numel() if d.get('rows') is not None else X.shape[0]
    N = W.shape[0]
    g = hip.PgGemm()
    g.X, g.ldx, g.K1 = X.data_ptr(), X.stride(0), X.shape[1]
    if d.get('X2') is not None:
        g.X2, g.ldx2, g.K2 = d['X2'].data_ptr(), d['X2'].stride(0), d['X2'].shape[1]
    g.W, g.ldw, g.bias = W.data_ptr(), W.stride(0), _ptr(d.get('bias'))
    if d.get('ln') is not None:
        g.ln_gamma, g.ln_beta = d['ln'][0].data_ptr(), d['ln'][1].data_ptr()
    for k in ('1', '2'):
        add, idx = d.get('add' + k), d.get('idx' + k)
        if add is not None:
            setattr(g, 'add' + k, add.data_ptr())
            setattr(g, 'ld_add' + k, add.stride(0))
            setattr(g, 'idx' + k, _ptr(idx))
            if idx is not None:
                g.add_rows = add.shape[0]
    g.out_scale, g.act = d.get('out_scale', 1.0), d.get('act', 0)
    buf, Y = _out(y_rows or M, N, yoff)
    g.Y, g.ldy, g.M, g.N, g.rows = Y.data_ptr(), Y.stride(0), M, N, _ptr(d.get('rows'))
    old = lib.pg_debug_gemm_streaming(1 if streaming else 0)
    try:
        rc = lib.pg_gemm(C.byref(g), s)
    finally:
        lib.pg_debug_gemm_streaming(old)
    assert rc == OK, (rc, lib.pg_last_error())
    torch.cuda.synchronize()
    _guards_nan(buf, Y)
    return Y


def _gemm_bound(d, S, wln, profile):
    K = d['W'].shape[1]
    return dref.gemm_bound(S, K, d.get('out_scale', 1.0), wln, dc.TOL_LN.get(profile, 0.0) if wln is not None else 0.0,
                           dc.TOL_SSP if d.get('act', 0) == 1 else 0.0)


_POOLS = {}


def _stream_pool(N, M, profile):
    """The staged pool of one (N, M, profile); at most two tall ones are kept on the device."""
    key = (N, M, profile)
    if key not in _POOLS:
        if M > 1000:
            for k in [k for k in _POOLS if k[1] > 1000][:-1]:
                del _POOLS[k]
        p = dc.stream_pool(N, M, profile)
        q = dc.NS(M=M, N=N, idx1=p.idx1.to(DEV), gamma=p.gamma.to(DEV), beta=p.beta.to(DEV))
        q.X, q.X2, q.X20, q.W = _emb(p.X, 4, 8)[1], _emb(p.X2, 2, 2)[1], _emb(p.X2, 4, 4)[1], _emb(p.W, 4, 4)[1]
        q.bias, q.add_idx, q.add_own = _emb1(p.bias, 4)[1], _emb(p.add_idx, 4, 4)[1], _emb(p.add_own, 4, 4)[1]
        _POOLS[key] = q
    return _POOLS[key]


@pytest.mark.parametrize('v', dc.stream_variants(), ids=lambda v: v.name)
def test_streaming_gemm_against_float64(v):
    """Every instantiation of gemm_stream_kernel at M = 64, 65, 127 and at 2.5 per_cb + 1 tiles (stages 0, 1, 0 in one workgroup)."""
    cu = _cu()
    for M in dc.stream_Ms(v, cu):
        tiles = -(-M // 64)
        per_cb = min(dc.stream_per_cb(v, cu), tiles)
        for profile in dc.stream_profiles(v):
            d = dc.stream_args(v, _stream_pool(v.N, M, profile))
            ref, S, wln = dref.gemm(**d)
            case = f'{v.name} M={M} ({tiles} tiles, {-(-tiles // per_cb)} per workgroup) {profile}'
            Y = _run_gemm(d, True, yoff=(4, 1)[M % 2])
            if profile == 'exact':
                _check_exact('gemm streaming', case, Y, ref)
                _check_exact('gemm tiled', case, _run_gemm(d, False, yoff=(4, 1)[M % 2]), ref)
            else:
                _check_bound('gemm streaming', case, Y, ref, _gemm_bound(d, S, wln, profile))


def _tiled_case(c):
    for profile in dc.gemm_profiles(c):
        a = dc.gemm_operands(c, profile)
        d = _stage_gemm(a, c)
        ref, S, wln = dref.gemm(**d)
        case = (f'M={c.M} N={c.N} K={c.K1}+{c.K2} act={c.act} s={c.scale} bias={c.bias} add={c.add1}/{c.add2} '
                f'off={c.xoff}{c.woff}{c.yoff}{c.addoff}{" ln" if c.ln else ""}{" rows" if c.rows else ""} {profile}')
        Yall = _run_gemm(d, False, yoff=c.yoff, y_rows=c.rows)
        if c.rows:
            r = d['rows'].long()
            rest = torch.ones(c.rows, dtype=torch.bool, device=DEV)
            rest[r] = False
            assert bool(torch.isnan(Yall[rest]).all()), 'a row outside the subset was written'
            Y = Yall[r]
        else:
            Y = Yall
        if profile == 'exact':
            _check_exact('gemm tiled', case, Y, ref)
        else:
            _check_bound('gemm tiled ln' if c.ln else 'gemm tiled ssp' if c.act == 1 else 'gemm tiled', case, Y, ref,
                         _gemm_bound(d, S, wln, profile))


@pytest.mark.parametrize('K1,K2', dc.TILED_K)
def test_tiled_gemm_against_float64(K1, K2):
    for c in dc.tiled_cases(K1, K2):
        _tiled_case(c)


def test_tiled_gemm_unaligned_bias_and_two_gathered_operands():
    for c in dc.tiled_extra():
        _tiled_case(c)


def test_tiled_gemm_row_subsets():
    for c in dc.rows_cases():
        _tiled_case(c)


def _gemm_raw(X, W, streaming, ln=None, K1=None, K2=0, X2=None, M=None):
    """pg_gemm on a bare struct, for the calls that must return before any launch.  Returns (status, the whole NaN-filled buffer)."""
    hip, lib, s = _lib()
    g = hip.PgGemm()
    g.X, g.ldx, g.K1, g.K2 = X.data_ptr(), X.stride(0), X.shape[1] if K1 is None else K1, K2
    if X2 is not None:
        g.X2, g.ldx2 = X2.data_ptr(), X2.stride(0)
    g.W, g.ldw = W.data_ptr(), W.stride(0)
    if ln is not None:
        g.ln_gamma, g.ln_beta = _ptr(ln[0]), _ptr(ln[1])
    buf, Y = _out(X.shape[0], W.shape[0])
    g.out_scale, g.Y, g.ldy, g.M, g.N = 1.0, Y.data_ptr(), Y.stride(0), X.shape[0] if M is None else M, W.shape[0]
    old = lib.pg_debug_gemm_streaming(1 if streaming else 0)
    try:
        rc = lib.pg_gemm(C.byref(g), s)
    finally:
        lib.pg_debug_gemm_streaming(old)
    torch.cuda.synchronize()
    return rc, buf


def test_gemm_refusals_and_empty_batch():
    """PG_ERR_ARG before any launch, M = 0 is PG_OK: either way nothing is written."""
    hip, lib, s = _lib()
    X, X2, W = torch.randn(70, 128, device=DEV), torch.randn(70, 4, device=DEV), torch.randn(128, 132, device=DEV)
    ga, be = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    for streaming in (False, True):
        for kw, word in ((dict(K2=4), b'X2'),                                   # K2 > 0 without X2
                         (dict(ln=(ga, be), K1=124), b'LayerNorm'),             # LayerNorm with K1 != 128
                         (dict(ln=(ga, be), K2=4, X2=X2), b'LayerNorm'),        # LayerNorm with K2 != 0
                         (dict(ln=(ga, None)), b'ln_beta')):                    # LayerNorm without its beta
            rc, buf = _gemm_raw(X, W, streaming, **kw)
            assert rc == ERR_ARG and lib.pg_last_error().startswith(b'pg_gemm:') and word in lib.pg_last_error(), (kw, lib.pg_last_error())
            assert bool(torch.isnan(buf).all())
        rc, buf = _gemm_raw(X, W, streaming, M=0)
        assert rc == OK and bool(torch.isnan(buf).all())
        rc, buf = _gemm_raw(X, W, streaming, ln=(ga, be))                       # (the same struct, accepted)
        assert rc == OK and bool(torch.isfinite(buf[:70, 4:132]).all())


# ---- pg_rows_linear ----
def test_rows_linear_against_float64():
    hip, lib, s = _lib()
    for c in dc.rows_linear_cases(_cu()):
        for profile in ('exact', 'real'):
            a = dc.rows_linear_operands(c, profile)
            X = _emb(a['X'], c.xoff, c.pad)[1]
            W = a['W'].to(DEV)
            b = a['b'].to(DEV) if 'b' in a else None
            rows = a['rows'].to(DEV) if 'rows' in a else None
            buf, Y = _out(c.M, c.n_out, 1, 2)
            hip.check(lib.pg_rows_linear(X.data_ptr(), X.stride(0), c.K, W.data_ptr(), _ptr(b), c.n_out, c.M, _ptr(rows), Y.data_ptr(),
                                         Y.stride(0), s), 'pg_rows_linear')
            torch.cuda.synchronize()
            _guards_nan(buf, Y)
            ref, S = dref.rows_linear(X, W, b, rows)
            case = f'K={c.K} n_out={c.n_out} M={c.M} ldx={X.stride(0)} xoff={c.xoff} b={c.bias} rows={c.rows} {profile}'
            if profile == 'exact':
                _check_exact('rows_linear', case, Y, ref)
            else:
                _check_bound('rows_linear', case, Y, ref, dref.gemm_bound(S, c.K))


def test_rows_linear_refusals():
    hip, lib, s = _lib()
    X, W = torch.zeros(4, 260, device=DEV), torch.zeros(17, 260, device=DEV)
    buf, Y = _out(4, 17)
    for K, n_out in ((128, 17), (257, 4), (0, 4), (128, 0)):
        assert lib.pg_rows_linear(X.data_ptr(), 260, K, W.data_ptr(), None, n_out, 4, None, Y.data_ptr(), Y.stride(0), s) == ERR_ARG
        assert lib.pg_last_error().startswith(b'pg_rows_linear:')
    assert lib.pg_rows_linear(X.data_ptr(), 260, 128, W.data_ptr(), None, 4, 0, None, Y.data_ptr(), Y.stride(0), s) == OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ---- pg_gemm_wgrad ----
def test_gemm_wgrad_against_float64():
    hip, lib, s = _lib()
    cu = _cu()
    for c in dc.wgrad_cases(cu):
        for profile in c.profiles:
            a = dc.wgrad_operands(c, profile)
            dY, X = _emb(a['dY'], c.yoff, 3)[1], _emb(a['X'], c.xoff, 2)[1]
            wbuf, gW = _emb(a['gW0'], 4, 3, guard=dc.GUARD)
            bbuf, gb = _emb1(a['gb0']) if c.gb else (None, None)
            hip.check(lib.pg_gemm_wgrad(dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), c.M, c.N, c.K, gW.data_ptr(), gW.stride(0),
                                        _ptr(gb), s), 'pg_gemm_wgrad')
            torch.cuda.synchronize()
            _guards_nan(wbuf, gW)
            rW, rb, SW, Sb = dref.gemm_wgrad(dY, X, a['gW0'].to(DEV), a['gb0'].to(DEV) if c.gb else None)
            case = (f'M={c.M} N={c.N} K={c.K} split={dc.wgrad_split(c.M, c.N, c.K, cu)} ld={dY.stride(0)}/{X.stride(0)}/{gW.stride(0)} '
                    f'off={c.yoff}{c.xoff} gb={c.gb} {profile}')
            if profile == 'exact':
                _check_exact('wgrad gW', case, gW, rW)
            else:
                _check_bound('wgrad gW', case, gW, rW, dref.gemm_bound(SW, c.M))
            if c.gb:
                _guards_nan(bbuf, gb)
                if profile == 'exact':
                    _check_exact('wgrad gb', case, gb, rb)
                else:
                    _check_bound('wgrad gb', case, gb, rb, dref.gemm_bound(Sb, c.M))


# ---- pg_ln_relu, pg_ln_relu_bwd ----
@pytest.mark.parametrize('profile', dc.LN_FWD_PROFILES)
def test_ln_relu_against_float64(profile):
    hip, lib, s = _lib()
    for M in dc.ln_Ms(_cu(), 8):
        a = dc.ln_operands(M, profile)
        X, ga, be = _emb(a.X, 1, 2)[1], a.gamma.to(DEV), a.beta.to(DEV)
        buf, Y = _out(M, 128, 3, 2)
        hip.check(lib.pg_ln_relu(X.data_ptr(), X.stride(0), ga.data_ptr(), be.data_ptr(), M, Y.data_ptr(), Y.stride(0), s), 'pg_ln_relu')
        torch.cuda.synchronize()
        _guards_nan(buf, Y)
        _check_bound('ln_relu', f'M={M} {profile}', Y, dref.ln_relu(X, ga, be), a.tol)


@pytest.mark.parametrize('profile', dc.LN_BWD_PROFILES)
def test_ln_relu_bwd_against_float64(profile):
    hip, lib, s = _lib()
    Ms = dc.ln_Ms(_cu(), 4)
    for M, sparse in [(M, False) for M in Ms] + [(Ms[-1], True)]:
        a = dc.ln_operands(M, profile, bwd=True, sparse=sparse)
        X, gY, ga, be = _emb(a.X, 1, 2)[1], _emb(a.gY, 2, 3)[1], a.gamma.to(DEV), a.beta.to(DEV)
        buf, gX = _out(M, 128, 3, 2)
        gbuf, gg = _emb1(torch.zeros(128))
        bbuf, gb = _emb1(torch.zeros(128), 3)
        hip.check(lib.pg_ln_relu_bwd(X.data_ptr(), X.stride(0), ga.data_ptr(), be.data_ptr(), gY.data_ptr(), gY.stride(0), M, gX.data_ptr(),
                                     gX.stride(0), gg.data_ptr(), gb.data_ptr(), s), 'pg_ln_relu_bwd')
        torch.cuda.synchronize()
        for b_, v_ in ((buf, gX), (gbuf, gg), (bbuf, gb)):
            _guards_nan(b_, v_)
        r = dref.ln_relu_bwd(X, ga, be, gY, band=a.tol)
        case = f'M={M}{" sparse gY" if sparse else ""} {profile}'
        planted = a.planted.to(DEV)
        assert not bool((r['band_rows'] & planted).any())
        # the mask at a pre-activation of exactly 0: closed, outright
        assert bool((r['pre'][planted] == 0).all()) and bool((gX[planted] == 0).all()), case
        # gX: the reference's mask; a row with a pre-activation inside the band may take the other mask there
        assert bool(torch.isfinite(gX).all())
        e1, e2 = (gX.double() - r['gX']).abs().amax(1), (gX.double() - r['gX_alt']).abs().amax(1)
        err = torch.where(r['band_rows'], torch.minimum(e1, e2), e1)
        print(f'dense kernel {"ln_relu_bwd gX":26s} {case:58s} {float(err.max()):.3e}   (tolerance {a.tol:.1e}, '
              f'{int(r["band_rows"].sum())} band rows)')
        assert bool((err <= a.tol).all()), (case, float(err.max()))
        # gbeta: integers under the mask -- bit for bit, widened by exactly the in-band terms
        dbeta = (gb.double() - r['gbeta']).abs()
        print(f'dense kernel {"ln_relu_bwd gbeta":26s} {case:58s} exact: {int((dbeta > 0).sum())} of 128 differ '
              f'(in-band widening up to {float(r["W_beta"].max()):.1f})')
        assert bool((dbeta <= r['W_beta']).all()), (case, dbeta.max())
        nnz = int((gY != 0).any(1).sum())
        bound = (nnz + 4) * dref.U * r['S_gamma'] + a.tol * r['S_beta'] + r['W_gamma']
        _check_bound('ln_relu_bwd ggamma', case, gg, r['ggamma'], bound)


# ---- pg_attn_fold_wgrad, pg_attn_unfold_bias_grad ----
def test_fold_wgrad_against_float64():
    hip, lib, s = _lib()
    ns = dc.fold_ns(_cu())
    for n, with_ids, profile in [(n, w, 'exact') for n in ns for w in (False, True)] + [(61, True, 'real'), (5, False, 'real')]:
        a = dc.fold_operands(n, with_ids, profile)
        X, T = _emb(a.X, 4, 4)[1], a.T.to(DEV)
        ids = a.ids.to(DEV) if with_ids else None
        buf, gW = _emb1(a.g0, 8)
        hip.check(lib.pg_attn_fold_wgrad(X.data_ptr(), X.stride(0), T.data_ptr(), n, _ptr(ids), gW.data_ptr(), s), 'pg_attn_fold_wgrad')
        torch.cuda.synchronize()
        _guards_nan(buf, gW)
        ref, S = dref.fold_wgrad(X, T, ids, a.g0.to(DEV))
        case = f'n={n} ids={with_ids} {profile}'
        if profile == 'exact':
            _check_exact('fold_wgrad', case, gW, ref)
        else:
            _check_bound('fold_wgrad', case, gW, ref, dref.gemm_bound(S, n))


def test_unfold_bias_grad_against_float64():
    hip, lib, s = _lib()
    for n in dc.unfold_ns(_cu()):
        for with_ids in (False, True):
            a = dc.unfold_operands(n, with_ids)
            gout, swn, b2v = _emb(a.gout, 1, 2)[1], a.swn.to(DEV), a.b2v.to(DEV)
            ids = a.ids.to(DEV) if with_ids else None
            R = a.gout.shape[0]
            sbuf = torch.full((R + dc.GUARD, 16), NAN, device=DEV)
            bbuf, gb = _emb1(a.gb0, 2)
            hip.check(lib.pg_attn_unfold_bias_grad(gout.data_ptr(), gout.stride(0), swn.data_ptr(), b2v.data_ptr(), n, _ptr(ids),
                                                   sbuf.data_ptr(), gb.data_ptr(), s), 'pg_attn_unfold_bias_grad')
            torch.cuda.synchronize()
            _guards_nan(bbuf, gb)
            rows, rs, rb, _, _ = dref.unfold_bias_grad(gout, swn, b2v, ids, a.gb0.to(DEV))
            rows = rows.to(DEV)
            rest = torch.ones(R + dc.GUARD, dtype=torch.bool, device=DEV)
            rest[rows] = False
            assert bool(torch.isnan(sbuf[rest]).all()), 'a gswn row outside ids was written'
            case = f'n={n} ids={with_ids} ldg={gout.stride(0)} exact'
            _check_exact('unfold_bias_grad gswn', case, sbuf[rows], rs)
            _check_exact('unfold_bias_grad gb2v', case, gb, rb)


# ---- pg_bond_rows_sum ----
def test_bond_rows_sum_against_float64():
    from phoregen_amd.plan import BatchPlan, make_edge_data
    hip, lib, s = _lib()
    dev = torch.device(DEV)
    for sizes, nph, ncol in dc.bond_batches(_cu()):
        na, nph = torch.tensor(sizes), torch.tensor(nph)
        ei, be = make_edge_data(na)
        B = na.numel()
        plan = BatchPlan(torch.repeat_interleave(torch.arange(B), na), torch.repeat_interleave(torch.arange(B), nph), ei, be, B, dev)
        Y = _emb(dc.draw('exact', (plan.n_bond, ncol), dc.gen(31, ncol)), 4, 4)[1]
        lig = plan.lig2ctx_long
        for by_src, idx in ((1, plan.bond_src), (0, plan.bond_dst)):
            buf, out = _out(plan.n_ctx, ncol, 4, 4)
            hip.check(lib.pg_bond_rows_sum(plan.topo_ref, Y.data_ptr(), Y.stride(0), ncol, by_src, out.data_ptr(), out.stride(0), s),
                      'pg_bond_rows_sum')
            torch.cuda.synchronize()
            _guards_nan(buf, out)
            rest = torch.ones(plan.n_ctx, dtype=torch.bool, device=DEV)
            rest[lig] = False
            assert bool(torch.isnan(out[rest]).all()), 'a pharmacophore row was written'
            ref = dref.bond_rows_sum(Y, idx, plan.n_ctx)
            _check_exact('bond_rows_sum', f'{int(na.sum())} atoms, {plan.n_bond} bond rows, ncol={ncol} by_src={by_src}', out[lig], ref[lig])
