"""-m gpu: the transition-step kernels (csrc/posterior.hip) through the C ABI, element by element against the float64 restatement of
tests/posterior_reference.py on the inputs of tests/posterior_cases.py -- seven graphs of 1 .. 260 rows at t = 0, 1, 2, 500, 998, 999,
three input profiles, the three Philox counter layouts, every entry point.

The noise is predicted bit for bit (oracle/philox_ref.py), so a sampled class is compared with THE class the reference samples and a
noised coordinate with THE coordinate, not with a distribution.  Float outputs meet the absolute tolerances of posterior_cases.py,
which are three times the fp32 rounding of the formula itself (tests/test_posterior_host.py) and owe nothing to the kernels.  A class
is exact unless the row's float64 top-two score margin is below TIE_BAND; then it must be one of the classes within the band of the
best score (at most 1 % of the rows of a case, asserted on the host).  Copies, one-hots, t = 0 rows with supplied noise, free rows next
to fixed ones and a graph run alone are compared bit for bit.  Every output buffer carries 64 NaN rows behind it that must stay NaN.
Each error is printed (pytest -s) before it is asserted; profiles/posterior_parity.md records them."""
import numpy as np
import pytest
import torch

import posterior_cases as pc
import posterior_reference as pref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
f64 = np.float64


def _lib():
    from phoregen_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


_TABLES = {}


def _tab(name):
    if name not in _TABLES:
        _TABLES[name] = tuple(_dev(a) for a in pc.tables()[name])
    return _TABLES[name]


def _out(n, width):
    return torch.full((n + GUARD, width), float('nan'), device=DEV)


def _take(buf, n):
    """The n rows a kernel owns, after checking that it wrote all of them and nothing behind them."""
    a = buf.cpu().numpy()
    assert np.isnan(a[n:]).all(), 'written past the last row'
    assert np.isfinite(a[:n]).all()
    return a[:n]


def _check(kind, case, out, ref, tol):
    err = float(np.abs(out.astype(f64) - ref).max()) if out.size else 0.0
    print(f'posterior kernel {kind:22s} {case:44s} {err:.3e}   (tolerance {tol:.1e})')
    assert err <= tol, (kind, case, err)


def _check_classes(case, onehot, scores, rows=None):
    """Exactly one 1 per row; the class is the reference's unless the reference's own margin is inside the tie band."""
    assert ((onehot == 0) | (onehot == 1)).all() and (onehot.sum(-1) == 1).all(), case
    cls = onehot.argmax(-1)
    top = scores.max(-1)
    mine = scores[np.arange(cls.size), cls]
    bad = np.nonzero(mine < top - pc.TIE_BAND)[0]
    assert bad.size == 0, (case, (bad if rows is None else rows[bad])[:8], cls[bad[:8]], scores.argmax(-1)[bad[:8]])
    return cls


# ---- the categorical kernel ----
def _rng(K):
    return pc.NODE_RNG if K == 12 else pc.EDGE_RNG


def _run_cat(K, lay, logits, log_vt, form, uniform=None, traj=True, frag_cls=None):
    """One launch of pg_posterior_categorical(_frag): (log_vt_out, onehot_out) as numpy."""
    hip, lib, s = _lib()
    n = lay.n
    row0, key = pc.counter_args(lay, 'flat' if form == 'supplied' else form)
    d = [_dev(a) for a in (logits, log_vt, lay.row_graph, lay.time, uniform if form == 'supplied' else None, row0, key, frag_cls)]
    qm, qt = _tab(K)
    lo, oh, tj = _out(n, K), _out(n, K), (_out(n, K) if traj else None)
    args = (_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), qm.data_ptr(), qt.data_ptr(), n, K, _ptr(d[4]), pc.SEED, _rng(K)['stream_id'],
            _rng(K)['step'], _ptr(d[5]), _ptr(d[6]), lo.data_ptr(), oh.data_ptr(), _ptr(tj))
    if frag_cls is None:
        hip.check(lib.pg_posterior_categorical(*args, s), 'categorical')
    else:
        hip.check(lib.pg_posterior_categorical_frag(*args, _ptr(d[7]), pc.FRAG_STREAMS[K], s), 'categorical_frag')
    torch.cuda.synchronize()
    lo, oh = _take(lo, n), _take(oh, n)
    if traj:
        assert np.array_equal(_take(tj, n), oh)
    return lo, oh


def _ref_cat(c, form):
    qm, qt = pc.tables()[c.K]
    lay = c.lay
    lp = pref.categorical_log_posterior(c.logits, c.log_vt, lay.time, lay.row_graph, qm, qt)
    if form == 'supplied':
        u = c.uniform
    else:
        row0, key = pc.counter_args(lay, form)
        u = pref.uniforms(lay.n, c.K, pc.SEED, _rng(c.K)['stream_id'], _rng(c.K)['step'], lay.row_graph, row0, key)
    return lp, pref.gumbel_scores(lp, u)[0]


@pytest.mark.parametrize('form', pc.FORMS + ('supplied',))
@pytest.mark.parametrize('profile', pc.PROFILES)
@pytest.mark.parametrize('K', [12, 6])
def test_categorical_against_float64(K, profile, form):
    c = pc.cat_case(K, profile)
    case = f'K={K} {profile} {form}'
    lo, oh = _run_cat(K, c.lay, c.logits, c.log_vt, form, c.uniform, traj=form != 'indexed')
    lp, scores = _ref_cat(c, form)
    _check('log posterior', case, lo, lp, pc.TOL_LOG)
    cls = _check_classes(case, oh, scores)
    if profile == 'ties' and form == 'supplied':
        assert (cls[c.all_equal] == 0).all()                                   # every score of the row is one number: the first
        assert np.array_equal(cls[c.pair], c.pair_ab[:, 0])                     # two bit-equal leaders: the lower index


@pytest.mark.parametrize('batch', ['single_row', 'single_graph'])
@pytest.mark.parametrize('K', [12, 6])
def test_categorical_small_batches(K, batch):
    c = pc.cat_case(K, 'benign', batch)
    for form in ('keyed', 'supplied'):
        lo, oh = _run_cat(K, c.lay, c.logits, c.log_vt, form, c.uniform)
        lp, scores = _ref_cat(c, form)
        _check('log posterior', f'K={K} {batch} {form}', lo, lp, pc.TOL_LOG)
        _check_classes(f'K={K} {batch} {form}', oh, scores)


# ---- the position kernel ----
def _run_pos(c, lay, rng, form='flat', eps=None, grad=None, center=None, traj=False, ctx=None, frag=None, rows=slice(None)):
    """One launch of pg_posterior_position[_ctx][_frag] on rows `rows` of case c laid out as `lay`.  ctx: None, 'separate' or 'alias'.
    Returns dict(x_prev, traj, x0_out, ctx_next) as numpy."""
    hip, lib, s = _lib()
    n = lay.n
    row0, key = pc.counter_args(lay, form)
    keep = [_dev(a) for a in (c.x_t[rows], lay.row_graph, lay.time, grad, eps, row0, key, center)]
    x_t, rg, tt, d_grad, d_eps, d_row0, d_key, d_center = keep
    c0, cx, sd = _tab('pos')
    x_prev, tj = _out(n, 3), (_out(n, 3) if traj else None)
    mid = (_ptr(rg), _ptr(tt), c0.data_ptr(), cx.data_ptr(), sd.data_ptr(), _ptr(d_grad), _ptr(d_eps), pc.SEED, rng['stream_id'],
           rng['step'], n, _ptr(d_row0), _ptr(d_key), _ptr(d_center), x_prev.data_ptr(), _ptr(tj))
    tail = ()
    if frag is not None:
        sa, sb = _tab('frag')
        keep += [_dev(frag.cls12[rows]), _dev(frag.x0f[rows])]
        tail = (keep[-2].data_ptr(), keep[-1].data_ptr(), sa.data_ptr(), sb.data_ptr(), pc.FRAG_STREAMS['pos'])
    out = {}
    if ctx is None:
        x0 = _dev(c.x0[rows])
        fn = lib.pg_posterior_position_frag if frag is not None else lib.pg_posterior_position
        hip.check(fn(x_t.data_ptr(), x0.data_ptr(), *mid, *tail, s), 'position')
    else:
        assert rows == slice(None)
        x0_ctx, l2c = _out(c.n_ctx, 3), _dev(c.lig2ctx)
        x0_ctx[:c.n_ctx] = _dev(c.x0_ctx)
        nxt = x0_ctx
        if ctx == 'separate':
            nxt = _out(c.n_ctx, 3)
            nxt[:c.n_ctx] = _dev(c.next_fill)
        x0_out = _out(n, 3)
        fn = lib.pg_posterior_position_ctx_frag if frag is not None else lib.pg_posterior_position_ctx
        hip.check(fn(x_t.data_ptr(), x0_ctx.data_ptr(), l2c.data_ptr(), *mid, nxt.data_ptr(), x0_out.data_ptr(), *tail, s), 'position_ctx')
        torch.cuda.synchronize()
        out['x0_out'], out['ctx_next'] = _take(x0_out, n), _take(nxt, c.n_ctx)
        if ctx == 'separate':
            assert np.array_equal(_take(x0_ctx, c.n_ctx), c.x0_ctx)             # the buffer read is left alone
    torch.cuda.synchronize()
    out['x_prev'], out['traj'] = _take(x_prev, n), (_take(tj, n) if traj else None)
    return out


def _ref_pos(c, rng, form, eps, grad, center, ctx_fill=None):
    lay = c.lay
    c0, cx, sd = pc.tables()['pos']
    row0, key = pc.counter_args(lay, form)
    u = None if eps is not None else pref.position_uniforms(lay.n, pc.SEED, rng['stream_id'], rng['step'], lay.row_graph, row0, key)
    if ctx_fill is None:
        return pref.position_posterior(c.x_t, c.x0, lay.time, lay.row_graph, c0, cx, sd, grad=grad, eps=eps, u=u, center=center)
    return pref.position_posterior(c.x_t, c.x0_ctx, lay.time, lay.row_graph, c0, cx, sd, grad=grad, eps=eps, u=u, lig2ctx=c.lig2ctx,
                                   x_ctx_next=ctx_fill, center=center)


POS_VARIANTS = [  # noise, grad, center, traj
    ('eps', False, False, False), ('eps', True, True, True), ('flat', True, False, True), ('indexed', False, True, True),
    ('keyed', True, True, True), ('keyed', False, False, False)]


@pytest.mark.parametrize('noise,grad,center,traj', POS_VARIANTS)
@pytest.mark.parametrize('batch', list(pc.BATCHES))
def test_position_against_float64(batch, noise, grad, center, traj):
    c = pc.pos_case(batch)
    lay = c.lay
    eps, form = (c.eps, 'flat') if noise == 'eps' else (None, noise)
    grad, center = (c.grad if grad else None), (c.center if center else None)
    rng = pc.POS_RNG[0]
    out = _run_pos(c, lay, rng, form, eps, grad, center, traj)
    ref = _ref_pos(c, rng, form, eps, grad, center)
    tol = pc.TOL_POS_EPS if noise == 'eps' else pc.TOL_POS_DEVICE
    case = f'{batch} {noise} grad={grad is not None} center={center is not None}'
    _check('position', case, out['x_prev'], ref['x_prev'], tol)
    if traj:
        _check('position traj', case, out['traj'], ref['traj'], tol)
        # traj is x_prev + center in fp32, from the x_prev that was written
        shift = c.center[lay.row_graph] if center is not None else np.float32(0.0)
        assert np.array_equal(out['traj'], out['x_prev'] + shift)
    # t = 0: the mean and nothing else -- the same bits with other noise
    tb = lay.time[lay.row_graph]
    if (tb == 0).any():
        other = _run_pos(c, lay, pc.POS_RNG[1], 'flat', None, grad, center, False)
        assert np.array_equal(other['x_prev'][tb == 0], out['x_prev'][tb == 0])
        assert not np.array_equal(other['x_prev'][tb > 0], out['x_prev'][tb > 0])


@pytest.mark.parametrize('ctx', ['separate', 'alias'])
@pytest.mark.parametrize('noise,grad,center,traj', POS_VARIANTS[1:5])
def test_position_ctx_against_float64(noise, grad, center, traj, ctx):
    c = pc.pos_case()
    lay = c.lay
    eps, form = (c.eps, 'flat') if noise == 'eps' else (None, noise)
    grad, center = (c.grad if grad else None), (c.center if center else None)
    rng = pc.POS_RNG[1]
    out = _run_pos(c, lay, rng, form, eps, grad, center, traj, ctx=ctx)
    fill = c.next_fill if ctx == 'separate' else c.x0_ctx
    ref = _ref_pos(c, rng, form, eps, grad, center, ctx_fill=fill)
    tol = pc.TOL_POS_EPS if noise == 'eps' else pc.TOL_POS_DEVICE
    case = f'ctx {ctx} {noise} grad={grad is not None} center={center is not None}'
    _check('position', case, out['x_prev'], ref['x_prev'], tol)
    _check('position traj', case, out['traj'], ref['traj'], tol)
    assert np.array_equal(out['x0_out'], c.x0)                                   # the gathered x0
    assert np.array_equal(out['ctx_next'][c.lig2ctx], out['x_prev'])             # ligand slots: the new positions
    assert np.array_equal(out['ctx_next'][~c.is_lig], fill[~c.is_lig])           # every other row: untouched
    # the row map changes where x0 is read and nothing else: the plain entry point on the gathered x0 gives the same bits
    plain = _run_pos(c, lay, rng, form, eps, grad, center, traj)
    assert np.array_equal(plain['x_prev'], out['x_prev']) and np.array_equal(plain['traj'], out['traj'])


# ---- a graph's noise depends on its key and its own rows only ----
def test_keyed_graph_alone_reproduces_its_rows_of_the_batch():
    lay = pc.layout()
    rows, alone = pc.graph_alone(lay, pc.ALONE)
    assert rows.start < 256 < rows.stop                                          # a block boundary of the batch run falls inside
    for K in (12, 6):
        c = pc.cat_case(K, 'benign')
        lo, oh = _run_cat(K, lay, c.logits, c.log_vt, 'keyed')
        lo1, oh1 = _run_cat(K, alone, c.logits[rows], c.log_vt[rows], 'keyed')
        assert np.array_equal(lo1, lo[rows]) and np.array_equal(oh1, oh[rows])
        # ... and on the key: graph numbers instead of keys draw other classes for it
        oh2 = _run_cat(K, alone, c.logits[rows], c.log_vt[rows], 'indexed')[1]
        assert not np.array_equal(oh2, oh1)
    c = pc.pos_case()
    fr = pc.frag_case('third')
    for frag in (None, fr):
        full = _run_pos(c, lay, pc.POS_RNG[0], 'keyed', None, c.grad, None, False, frag=frag)
        part = _run_pos(c, alone, pc.POS_RNG[0], 'keyed', None, c.grad[rows], None, False, frag=frag, rows=rows)
        assert np.array_equal(part['x_prev'], full['x_prev'][rows])


# ---- the fragment forms ----
def _frag_ref_inputs(lay, fr, K, form):
    rows = np.nonzero(fr.fixed)[0]
    lvl_all = lay.time[lay.row_graph] - 1
    step = np.maximum(lvl_all, 0)
    row0, key = pc.counter_args(lay, form)
    u = None if K is None else pref.uniforms(lay.n, K, pc.SEED, pc.FRAG_STREAMS[K], step, lay.row_graph, row0, key)[rows]
    u1, u2 = pref.position_uniforms(lay.n, pc.SEED, pc.FRAG_STREAMS['pos'], step, lay.row_graph, row0, key)
    return rows, lvl_all[rows], u, pref.box_muller(u1[rows], u2[rows])


@pytest.mark.parametrize('form', pc.FORMS)
@pytest.mark.parametrize('K', [12, 6])
def test_categorical_frag_against_plain_and_float64(K, form):
    c = pc.cat_case(K, 'benign')
    lay = c.lay
    plain = _run_cat(K, lay, c.logits, c.log_vt, form)
    free = _run_cat(K, lay, c.logits, c.log_vt, form, frag_cls=getattr(pc.frag_case('none'), f'cls{K}'))
    assert np.array_equal(free[0], plain[0]) and np.array_equal(free[1], plain[1])        # nothing fixed: the plain kernel's bits
    sup = _run_cat(K, lay, c.logits, c.log_vt, 'supplied', c.uniform)
    for mask in ('third', 'whole'):
        fr = pc.frag_case(mask)
        v0_all = getattr(fr, f'cls{K}')
        lo, oh = _run_cat(K, lay, c.logits, c.log_vt, form, frag_cls=v0_all)
        assert np.array_equal(lo[~fr.fixed], plain[0][~fr.fixed]) and np.array_equal(oh[~fr.fixed], plain[1][~fr.fixed])
        rows, lvl, u, _ = _frag_ref_inputs(lay, fr, K, form)
        ref = pref.fragment_row(v0_all[rows], lvl, K, pc.tables()[K][0], u)
        case = f'K={K} {mask} {form}'
        _check('fragment log', case, lo[rows], ref['log'], pc.TOL_LOG)
        cls = _check_classes(case, oh[rows], ref['scores'], rows)
        done = lvl < 0                                                                     # after step 0: the fragment itself
        if done.any():
            assert np.array_equal(cls[done], v0_all[rows][done])
            assert np.array_equal(lo[rows][done], np.where(oh[rows][done] == 1, np.float32(0.0), np.float32(pref.LOG_FLOOR)))
        if form == 'flat':      # the replacement does not read the caller's uniforms: free rows as the plain run, fixed rows as above
            lo_s, oh_s = _run_cat(K, lay, c.logits, c.log_vt, 'supplied', c.uniform, frag_cls=v0_all)
            assert np.array_equal(lo_s[~fr.fixed], sup[0][~fr.fixed]) and np.array_equal(oh_s[~fr.fixed], sup[1][~fr.fixed])
            assert np.array_equal(lo_s[fr.fixed], lo[fr.fixed]) and np.array_equal(oh_s[fr.fixed], oh[fr.fixed])


@pytest.mark.parametrize('form', pc.FORMS)
@pytest.mark.parametrize('ctx', [None, 'alias'])
def test_position_frag_against_plain_and_float64(ctx, form):
    c = pc.pos_case()
    lay = c.lay
    rng = pc.POS_RNG[0]
    sa, sb = pc.tables()['frag']
    run = lambda frag: _run_pos(c, lay, rng, form, None, c.grad, c.center, True, ctx=ctx, frag=frag)
    plain = run(None)
    free = run(pc.frag_case('none'))
    for k in plain:
        assert plain[k] is None or np.array_equal(free[k], plain[k]), k                    # nothing fixed: the plain kernel's bits
    for mask in ('third', 'whole'):
        fr = pc.frag_case(mask)
        out = run(fr)
        assert np.array_equal(out['x_prev'][~fr.fixed], plain['x_prev'][~fr.fixed])
        assert np.array_equal(out['traj'][~fr.fixed], plain['traj'][~fr.fixed])
        rows, lvl, _, e = _frag_ref_inputs(lay, fr, None, form)
        ref = pref.fragment_row(fr.cls12[rows], lvl, x0f=fr.x0f[rows], sqrt_ab=sa, sqrt_1mab=sb, e=e)
        case = f'{"ctx" if ctx else "plain"} {mask} {form}'
        _check('fragment coordinates', case, out['x_prev'][rows], ref['x'], pc.TOL_FRAG_POS)
        _check('fragment traj', case, out['traj'][rows], ref['x'] + c.center.astype(f64)[lay.row_graph[rows]], pc.TOL_FRAG_POS)
        done = lvl < 0
        if done.any():
            assert np.array_equal(out['x_prev'][rows][done], fr.x0f[rows][done])           # after step 0: the fragment, bit for bit
        if ctx:
            assert np.array_equal(out['x0_out'], c.x0)
            assert np.array_equal(out['ctx_next'][c.lig2ctx], out['x_prev'])                # the replaced value reaches the next step
            assert np.array_equal(out['ctx_next'][~c.is_lig], c.x0_ctx[~c.is_lig])
