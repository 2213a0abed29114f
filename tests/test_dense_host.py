"""CPU part of the dense kernel tests.  The float64 restatements of tests/dense_reference.py are held equal to torch.nn.functional
(linear, layer_norm, relu, softplus) and to autograd in float64 on the inputs the GPU tests use (tests/dense_cases.py); every `exact`
case is shown, from its operands alone, to keep every partial sum an integer below 2^24; the fp32 restatements of the two expressions
without a derived bound stay within tolerance / FLOOR_MULT of float64; the share of rows whose ReLU mask the tolerance cannot pin is
at most 1 %; the option draws of the tiled grid cover what they are meant to.  Each figure is printed (pytest -s) before it is
asserted; profiles/dense_parity.md records them.

Last, the refusals of pg_gemm and pg_rows_linear that return before any launch, through the library without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_cases as dc
import dense_reference as dref
from helpers import FLOOR_MULT

F64_EQ = 1e-11          # two float64 evaluations of one expression, relative to the largest value
CU = dc.NOMINAL_CU
d64 = lambda t: t.double()


def _close(a, b):
    scale = max(float(b.abs().max()) if b.numel() else 0.0, 1.0)
    assert float((a - b).abs().max() if b.numel() else 0.0) <= F64_EQ * scale


def _all_gemm_cases():
    for K1, K2 in dc.TILED_K:
        yield from dc.tiled_cases(K1, K2)
    yield from dc.tiled_extra()
    yield from dc.rows_cases()


# ---- the restatements are torch's functions ----
def _torch_gemm(a):
    X = d64(a['X'])
    r = a['rows'].long() if 'rows' in a else torch.arange(X.shape[0])
    A = X[r]
    if 'ln' in a:
        A = F.relu(F.layer_norm(A, (A.shape[1],), d64(a['ln'][0]), d64(a['ln'][1]), 1e-5))
    if 'X2' in a:
        A = torch.cat([A, d64(a['X2'])[r]], 1)
    y = F.linear(A, d64(a['W']), d64(a['bias']) if 'bias' in a else None)
    for k in ('1', '2'):
        if 'add' + k in a:
            y = y + d64(a['add' + k])[a['idx' + k].long() if 'idx' + k in a else r]
    y = F.softplus(y, threshold=100.0) - np.log(2.0) if a['act'] == 1 else F.relu(y) if a['act'] == 2 else y
    return y * a['out_scale']


def test_gemm_restatement_equals_torch_functional():
    n = 0
    for c in _all_gemm_cases():
        for profile in dc.gemm_profiles(c):
            a = dc.gemm_operands(c, profile)
            _close(dref.gemm(**a)[0], _torch_gemm(a))
            n += 1
    for v in dc.stream_variants():
        for profile in dc.stream_profiles(v):
            a = dc.stream_args(v, dc.stream_pool(v.N, 127, profile))
            _close(dref.gemm(**a)[0], _torch_gemm(dict(dict(act=0, out_scale=1.0), **a)))
            n += 1
    print(f'dense restatement: pg_gemm equal to torch.nn.functional on {n} cases')
    x = torch.linspace(-60, 60, 4001, dtype=torch.float64)
    _close(dref.ssp(x), F.softplus(x, threshold=100.0) - np.log(2.0))       # (the default threshold of 20 is itself an approximation: e^-20)


def test_rows_linear_restatement_equals_torch_functional():
    for c in dc.rows_linear_cases(2):
        a = dc.rows_linear_operands(c, 'real')
        X = d64(a['X'])[a['rows'].long()] if 'rows' in a else d64(a['X'])
        _close(dref.rows_linear(**a)[0], F.linear(X, d64(a['W']), d64(a['b']) if 'b' in a else None))


def test_adjoint_restatements_equal_autograd():
    # pg_gemm_wgrad
    for c in dc.wgrad_cases(2):
        a = dc.wgrad_operands(c, 'real')
        W, b = torch.zeros(c.N, c.K, dtype=torch.float64, requires_grad=True), torch.zeros(c.N, dtype=torch.float64, requires_grad=True)
        (F.linear(d64(a['X']), W, b) * d64(a['dY'])).sum().backward()
        gW, gb, _, _ = dref.gemm_wgrad(a['dY'], a['X'], a['gW0'], a.get('gb0'))
        _close(gW, W.grad + d64(a['gW0']))
        _close(gb, b.grad + (d64(a['gb0']) if c.gb else 0.0))
    # pg_ln_relu, pg_ln_relu_bwd
    for profile in dc.LN_BWD_PROFILES:
        for M in (1, 5, 1001):
            a = dc.ln_operands(M, profile, bwd=True)
            X, ga, be = (d64(t).requires_grad_() for t in (a.X, a.gamma, a.beta))
            y = F.relu(F.layer_norm(X, (128,), ga, be, 1e-5))
            _close(dref.ln_relu(a.X, a.gamma, a.beta), y.detach())
            (y * d64(a.gY)).sum().backward()
            r = dref.ln_relu_bwd(a.X, a.gamma, a.beta, a.gY)
            _close(r['gX'], X.grad)
            _close(r['ggamma'], ga.grad)
            _close(r['gbeta'], be.grad)
            assert torch.equal(r['gX'], r['gX_alt']) and not bool(r['band_rows'].any())       # band 0: one mask
    # pg_attn_fold_wgrad: the einsum against a gather over the documented slots
    xc, tc = dref.fold_slots()
    for n, with_ids in ((5, False), (61, True)):
        a = dc.fold_operands(n, with_ids, 'real')
        rows = a.ids.long() if with_ids else torch.arange(n)
        _close(dref.fold_wgrad(a.X, a.T, a.ids, a.g0)[0], (d64(a.X)[rows][:, xc] * d64(a.T)[rows][:, tc]).sum(0) + d64(a.g0))
    # pg_attn_unfold_bias_grad: out[s, c] = ... + b2v[c] swn[s, c >> 3]
    a = dc.unfold_operands(5, True, 'real')
    sw, b2 = d64(a.swn).requires_grad_(), d64(a.b2v).requires_grad_()
    mask = torch.zeros(a.gout.shape[0], 1, dtype=torch.float64)
    mask[a.ids.long()] = 1.0
    (b2 * sw.repeat_interleave(8, 1) * mask * d64(a.gout)).sum().backward()
    rows, gs, gb, _, _ = dref.unfold_bias_grad(a.gout, a.swn, a.b2v, a.ids, a.gb0)
    _close(gs, sw.grad[rows])
    _close(gb, b2.grad + d64(a.gb0))


# ---- `exact` cases stay exact: an upper bound of sum |terms| over every output element, from the operands alone ----
def _assert_exact(name, total):
    total = float(total)
    print(f'dense exact precondition {name:64s} sum |terms| <= {total:.0f}  (2^24 = {2 ** 24})')
    assert total < 2 ** 24 and total == int(total)


def _amax(t):
    assert bool((t == t.round()).all())                   # integers
    return float(t.abs().max()) if t.numel() else 0.0


def test_exact_cases_keep_every_partial_sum_below_2_24():
    for c in _all_gemm_cases():
        if 'exact' in dc.gemm_profiles(c):
            a = dc.gemm_operands(c, 'exact')
            for t in (a['X'], a['W'], a.get('X2'), a.get('bias'), a.get('add1'), a.get('add2')):
                t is None or _amax(t)
            S = dref.gemm(**a)[1]                         # per element: sum_k |x||w| + |bias| + |add1| + |add2|
            assert a['out_scale'] in (0.5, 1.0) and a['act'] in (0, 2)
            _assert_exact(f'gemm M={c.M} N={c.N} K={c.K1}+{c.K2} seed {c.seed}', S.max())
    for v in dc.stream_variants():
        if 'exact' in dc.stream_profiles(v):
            for M in dc.stream_Ms(v, CU):
                a = dc.stream_args(v, dc.stream_pool(v.N, M, 'exact'))
                K = a['W'].shape[1]
                xm = max(_amax(a['X']), _amax(a['X2']) if 'X2' in a else 0.0)
                tot = K * xm * _amax(a['W']) + _amax(a['bias']) + (_amax(a['add1']) if 'add1' in a else 0.0)
                _assert_exact(f'gemm streaming {v.name} M={M}', tot)
    for c in dc.rows_linear_cases(CU):
        a = dc.rows_linear_operands(c, 'exact')
        _assert_exact(f'rows_linear K={c.K} n_out={c.n_out} M={c.M}', c.K * _amax(a['X']) * _amax(a['W']) + (_amax(a['b']) if c.bias else 0))
    for c in dc.wgrad_cases(CU):
        a = dc.wgrad_operands(c, 'exact')
        _assert_exact(f'wgrad M={c.M} N={c.N} K={c.K}', c.M * _amax(a['dY']) * max(_amax(a['X']), 1.0) + max(_amax(a['gW0']), _amax(a.get('gb0', a['gW0']))))
    for M in dc.ln_Ms(CU, 4):
        a = dc.ln_operands(M, 'real', bwd=True)
        _assert_exact(f'ln_relu_bwd gbeta M={M}', M * _amax(a.gY))
    for n in dc.fold_ns(CU):
        a = dc.fold_operands(n, True, 'exact')
        _assert_exact(f'fold_wgrad n={n}', n * _amax(a.X) * _amax(a.T) + _amax(a.g0))
    for n in dc.unfold_ns(CU):
        a = dc.unfold_operands(n, True)
        _assert_exact(f'unfold_bias_grad n={n}', max(8 * _amax(a.gout) * _amax(a.b2v), n * _amax(a.gout) * _amax(a.swn) + _amax(a.gb0)))
    for sizes, _, ncol in dc.bond_batches(CU):
        assert sum(sizes) > (4 * 8 * CU if ncol == 8 else 0) and max(sizes) <= 128
        _assert_exact(f'bond_rows_sum {sum(sizes)} atoms ncol={ncol}', (max(sizes) - 1) * 4)


# ---- the two measured tolerances: FLOOR_MULT x the fp32 restatement's own error ----
def _report(kind, case, err, tol):
    print(f'dense fp32-restatement {kind:20s} {case:36s} {err:.3e}   (tolerance {tol:.1e}, a third of it {tol / FLOOR_MULT:.1e})')
    assert err <= tol / FLOOR_MULT, (kind, case, err)


def _err(a32, b64):
    return float(np.abs(np.asarray(a32, dtype=np.float64) - b64.numpy()).max()) if b64.numel() else 0.0


def test_fp32_floor_of_the_shifted_softplus():
    worst, n = 0.0, 0
    pres = [torch.linspace(-60, 60, 20001)]
    for c in _all_gemm_cases():
        if c.act == 1 and not c.ln:
            a = dc.gemm_operands(c, 'real')
            pres.append((dref.gemm(**dict(a, act=0))[0] / a['out_scale']).float().reshape(-1))
    pres.append(dref.gemm(**dict(dc.stream_args(dc.stream_variants()[-1], dc.stream_pool(128, 127, 'real')), act=0))[0].float().reshape(-1))
    for v in pres:
        worst, n = max(worst, _err(dref.ssp_f32(v.numpy()), dref.ssp(v))), n + v.numel()
    _report('shifted softplus', f'{n} pre-activations', worst, dc.TOL_SSP)


@pytest.mark.parametrize('profile', dc.LN_BWD_PROFILES)
def test_fp32_floor_of_layernorm_relu_and_its_adjoint(profile):
    tol = dc.TOL_LN['mean100' if profile == 'mean100' else 'real']
    sets = [dc.ln_operands(M, profile, bwd=True, sparse=sp) for M in dc.ln_Ms(CU, 4) for sp in (False, True)]
    if profile != 'beta0':
        sets += [dc.ln_operands(M, profile) for M in dc.ln_Ms(CU, 8)]
        p = dc.stream_pool(128, 127, profile)
        sets.append(dc.NS(X=p.X, gamma=p.gamma, beta=p.beta))
        p = dc.stream_pool(128, dc.stream_Ms(dc.stream_variants()[-2], CU)[-1], profile)
        sets.append(dc.NS(X=p.X, gamma=p.gamma, beta=p.beta))
        for c in _all_gemm_cases():
            if c.ln:
                a = dc.gemm_operands(c, profile)
                sets.append(dc.NS(X=a['X'], gamma=a['ln'][0], beta=a['ln'][1]))
    e_hat = e_y = e_gx = 0.0
    for a in sets:
        X = a.X.numpy()
        e_hat = max(e_hat, _err(dref.ln_hat_f32(X)[0], dref.layer_norm_hat(a.X)[0]))
        e_y = max(e_y, _err(dref.ln_relu_f32(X, a.gamma.numpy(), a.beta.numpy()), dref.ln_relu(a.X, a.gamma, a.beta)))
        if hasattr(a, 'gY'):
            r = dref.ln_relu_bwd(a.X, a.gamma, a.beta, a.gY)
            e_gx = max(e_gx, _err(dref.ln_relu_bwd_gx_f32(X, a.gamma.numpy(), a.gY.numpy(), (r['pre'] > 0).numpy()), r['gX']))
    _report('layernorm x_hat', f'{profile}, {len(sets)} operand sets', e_hat, tol)
    _report('layernorm+relu', f'{profile}, {len(sets)} operand sets', e_y, tol)
    _report('layernorm+relu gX', f'{profile}', e_gx, tol)


# ---- the ReLU mask band ----
@pytest.mark.parametrize('profile', dc.LN_BWD_PROFILES)
def test_relu_band_share_is_at_most_one_percent(profile):
    for M in dc.ln_Ms(CU, 4):
        a = dc.ln_operands(M, profile, bwd=True)
        r = dref.ln_relu_bwd(a.X, a.gamma, a.beta, a.gY, band=a.tol)
        n = int(r['band_rows'].sum())
        print(f'dense relu band {profile:8s} M={M:5d}: {n} rows hold a pre-activation within {a.tol:.0e} of 0 ({100.0 * n / M:.2f} %), '
              f'{int(a.planted.sum())} planted rows at exactly 0')
        assert n <= dc.BAND_CAP * M
        assert int(r['inband'].sum(1).max()) <= 1                        # one element per row at most: "either mask" is two candidates
        assert not bool((r['band_rows'] & a.planted).any()) and bool((r['pre'][a.planted] == 0).all())
        assert bool((r['gX'][a.planted] == 0).all())
        assert (profile == 'beta0') == bool(a.planted.any())


# ---- the tiled grid's option draws cover what the issue lists ----
def test_tiled_grid_covers_every_option():
    cs = [c for k in dc.TILED_K for c in dc.tiled_cases(*k)]
    assert len(cs) == 150 and {(c.M, c.N, c.K1, c.K2) for c in cs} == {(M, N, *k) for M in dc.TILED_M for N in dc.TILED_N for k in dc.TILED_K}
    for key, vals in (('act', (0, 1, 2)), ('scale', (0.5, 1.0)), ('bias', dc.BIAS_MODES), ('add1', dc.ADD_MODES), ('add2', dc.ADD_MODES),
                      ('xoff', (4, 1)), ('woff', (4, 1)), ('yoff', (4, 1)), ('addoff', (4, 1)), ('ln', (False, True))):
        for K in dc.TILED_K:
            seen = {getattr(c, key) for c in dc.tiled_cases(*K)}
            assert seen == set(vals) or (key == 'ln' and K != (128, 0) and seen == {False}), (key, K, seen)
    assert any(c.add1 == 'idx' and c.add2 == 'idx' for c in cs) and any(c.act == 2 and c.add2 == 'idx' for c in cs)
    # the 16-byte epilogue (N % 4 == 0, Y and the added operands aligned) with a bias 1 and 3 floats off a 16-byte boundary
    vec = [c for c in dc.tiled_extra() if c.N % 4 == 0 and c.yoff == 4 and c.addoff == 4]
    assert {c.bias for c in vec} >= {'off1', 'off3', 'aligned', 'none'}
    rc = dc.rows_cases()
    assert {(c.ln, c.add1, c.add2) for c in rc} >= {(ln, a, b) for ln in (False, True) for a, b in (('own', 'own'), ('idx', 'own'), ('own', 'idx'))}
    # gathered indices reach both ends of the operand, and idx2 differs from idx1
    a = dc.gemm_operands(dc.tiled_extra()[0], 'exact')
    assert int(a['idx1'].min()) == 0 and int(a['idx1'].max()) == dc.GEMM_ADD_ROWS - 1 and not torch.equal(a['idx1'], a['idx2'])
    p = dc.stream_pool(128, 64, 'exact')
    assert int(p.idx1.min()) == 0 and int(p.idx1.max()) == dc.ADD_ROWS - 1


def test_device_dependent_shapes_make_every_loop_repeat():
    for cu in (256, 64, 32):                                                  # a whole device and two partitions
        for v in dc.stream_variants():
            M, p = dc.stream_Ms(v, cu)[-1], dc.stream_per_cb(v, cu)
            tiles = -(-M // 64)
            assert tiles == 2 * p + p // 2 + 1 and M % 64 == 37              # three tiles for some workgroups, two for the rest, anchored
        assert dc.ln_Ms(cu, 8)[-1] > 4 * 8 * cu and dc.ln_Ms(cu, 4)[-1] > 4 * 4 * cu
        b = cu // 2
        n1, n2 = dc.fold_ns(cu)[2:]
        assert 4 * b < n1 < 4 * b + 4 and n2 == 2 * 16 * b + 5               # u = 1 in range for three waves; two whole passes and a ragged one
        assert dc.unfold_ns(cu)[-1] > 2 * 4 * (4 * cu)
        c = dc.wgrad_cases(cu)[-1]
        assert -(-c.M // 64) == 2 * dc.wgrad_split(c.M, c.N, c.K, cu) + 1
        assert dc.rows_linear_cases(cu)[-1].M > 64 * 8 * cu


# ---- refusals that return before any launch ----
def test_gemm_and_rows_linear_refuse_before_any_launch():
    """No GPU is needed: PG_ERR_ARG (or PG_OK for an empty batch) comes back without touching the runtime."""
    from phoregen_amd import hip
    lib = hip.load_library()
    OK, ERR_ARG = 0, 1
    dummy = (C.c_int * 4)()
    p = C.addressof(dummy)                                # a non-NULL pointer that nothing may dereference

    def gemm(**kw):
        g = hip.PgGemm()
        g.X, g.ldx, g.K1, g.W, g.ldw, g.Y, g.ldy, g.M, g.N, g.out_scale = p, 128, 128, p, 128, p, 128, 70, 128, 1.0
        for k, v in kw.items():
            setattr(g, k, v)
        return lib.pg_gemm(C.byref(g), None)

    assert gemm(M=0) == OK and gemm(M=0, ln_gamma=p, ln_beta=p) == OK
    assert gemm(K2=4) == ERR_ARG and b'X2' in lib.pg_last_error()
    assert gemm(ln_gamma=p, ln_beta=p, K1=124) == ERR_ARG and b'LayerNorm' in lib.pg_last_error()
    assert gemm(ln_gamma=p, ln_beta=p, K2=4, X2=p, ldx2=4) == ERR_ARG and b'LayerNorm' in lib.pg_last_error()
    assert gemm(ln_gamma=p) == ERR_ARG and lib.pg_last_error() == b'pg_gemm: ln_gamma without ln_beta'
    assert gemm(ln_gamma=p, K1=124) == ERR_ARG and gemm(N=0) == ERR_ARG and gemm(M=-1) == ERR_ARG
    rl = lambda K, n_out, M=4: lib.pg_rows_linear(p, 260, K, p, None, n_out, M, None, p, 16, None)
    assert rl(128, 17) == ERR_ARG and rl(257, 4) == ERR_ARG and lib.pg_last_error().startswith(b'pg_rows_linear:')
    assert rl(128, 16, 0) == OK and rl(256, 1, 0) == OK
