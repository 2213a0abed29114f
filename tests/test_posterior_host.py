"""CPU part of the transition-step kernel tests: the float64 restatements of tests/posterior_reference.py are held equal to the
oracle's q_v_posterior / gumbel_argmax / pos_prev_from_recon evaluated in float64 on the very inputs the GPU tests use
(tests/posterior_cases.py) and to the committed g_posterior fixture; the same restatements evaluated in fp32 stay below
tolerance / FLOOR_MULT of the float64 result, so every bound the kernels are asked to meet is at least three times what fp32
rounding of the formula itself costs on these inputs; and the share of rows whose sampled class the tolerance cannot pin is at most
1 % in every case.  Each figure is printed (pytest -s) before it is asserted; profiles/posterior_parity.md records them.

Last, the refusals of the seven entry points that return before any launch, through the library without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import posterior_cases as pc
import posterior_reference as pref
from helpers import FLOOR_MULT, golden, rel_err
from oracle import phoregen_oracle as po

F64_EQ = 1e-12         # two float64 evaluations of one formula (summation order of the K-term products, logsumexp)
f32, f64 = np.float32, np.float64


def _report(kind, case, err, tol):
    print(f'posterior fp32-reference {kind:20s} {case:32s} {err:.3e}   (tolerance {tol:.1e})')
    assert err <= tol / FLOOR_MULT, (kind, case, err)


def _abs_err(a, b):
    return float(np.abs(np.asarray(a, dtype=f64) - np.asarray(b, dtype=f64)).max())


def _log_post(c, dtype=f64):
    qm, qt = pc.tables()[c.K]
    return pref.categorical_log_posterior(c.logits, c.log_vt, c.lay.time, c.lay.row_graph, qm, qt, dtype)


def _cat_uniforms(c, form):
    if form == 'supplied':
        return c.uniform
    rng = pc.NODE_RNG if c.K == 12 else pc.EDGE_RNG
    row0, key = pc.counter_args(c.lay, form)
    return pref.uniforms(c.lay.n, c.K, pc.SEED, rng['stream_id'], rng['step'], c.lay.row_graph, row0, key)


def _cat_cases():
    for K in (12, 6):
        for profile in pc.PROFILES:
            yield pc.cat_case(K, profile)
        for batch in ('single_row', 'single_graph'):
            yield pc.cat_case(K, 'benign', batch)


# ---- the restatements are the oracle's functions ----
@pytest.mark.parametrize('K', [12, 6])
@pytest.mark.parametrize('profile', pc.PROFILES)
def test_categorical_restatement_equals_oracle(profile, K):
    c = pc.cat_case(K, profile)
    lp = _log_post(c)
    tt, batch = torch.from_numpy(c.lay.time), torch.from_numpy(c.lay.row_graph).long()
    lv0 = torch.log_softmax(torch.from_numpy(c.logits).double(), -1)
    ref = po.q_v_posterior(pc.torch_tables(K), lv0, torch.from_numpy(c.log_vt).double(), tt, batch).numpy()
    assert ref.dtype == f64 and np.isfinite(lp).all() and rel_err(lp, ref) <= F64_EQ
    tb = c.lay.time[c.lay.row_graph]
    assert np.array_equal(lp[tb == 0], pref.log_softmax(c.logits)[tb == 0])
    if profile == 'peaked':                              # the case reaches the floor of both logs
        assert lp.min() < -60
    v, cls, margin = pref.gumbel_scores(lp, c.uniform)
    oracle_cls = po.gumbel_argmax(torch.from_numpy(lp), torch.from_numpy(c.uniform).double()).numpy()
    decided = margin > 0                                 # (an exact tie: the first maximum, which torch's argmax does not promise)
    assert np.array_equal(cls[decided], oracle_cls[decided])
    assert (v[np.arange(c.lay.n), cls] == v.max(-1)).all() and (margin >= 0).all()


def test_ties_case_holds_what_it_claims():
    for K in (12, 6):
        c = pc.cat_case(K, 'ties')
        lp = _log_post(c)
        v, cls, margin = pref.gumbel_scores(lp, c.uniform)
        tb = c.lay.time[c.lay.row_graph]
        assert c.all_equal.size >= 100 and (tb[c.all_equal] == 0).all()
        assert (v[c.all_equal] == v[c.all_equal, :1]).all() and (cls[c.all_equal] == 0).all()
        a, b = c.pair_ab[:, 0], c.pair_ab[:, 1]
        assert set(tb[c.pair].tolist()) == set(c.lay.time.tolist()) and (a < b).all()
        assert (c.logits[c.pair, a] == c.logits[c.pair, b]).all() and (c.uniform[c.pair, a] == c.uniform[c.pair, b]).all()
        late = tb[c.pair] > 0                                # (at t = 0 the carried state is not read)
        assert (c.log_vt[c.pair, a] == c.log_vt[c.pair, b])[late].all()
        rest = v[c.pair].copy()
        rest[np.arange(c.pair.size), a] = rest[np.arange(c.pair.size), b] = -np.inf
        assert (np.abs(v[c.pair, a] - v[c.pair, b]) < 1e-9).all() and (v[c.pair, a] - rest.max(-1) > 0.99).all()
        # on the rows at t > 0 the fp32 evaluation ties EXACTLY (one-term products): so does any fp32 evaluation, in any order
        v32 = pref.gumbel_scores(_log_post(c, f32), c.uniform, f32)[0]
        assert (v32[c.pair, a] == v32[c.pair, b]).all()


def test_position_restatement_equals_oracle():
    for batch in pc.BATCHES:
        c = pc.pos_case(batch)
        lay = c.lay
        c0, cx, sd = pc.tables()['pos']
        tab = dict(coef_x0=torch.from_numpy(c0).double(), coef_xt=torch.from_numpy(cx).double(), std=torch.from_numpy(sd).double())
        d = lambda a: torch.from_numpy(a).double()
        tt, bt = torch.from_numpy(lay.time), torch.from_numpy(lay.row_graph).long()
        for grad in (None, c.grad):
            out = pref.position_posterior(c.x_t, c.x0_ctx, lay.time, lay.row_graph, c0, cx, sd, grad=grad, eps=c.eps,
                                          lig2ctx=c.lig2ctx, x_ctx_next=c.next_fill, center=c.center)
            ref = po.pos_prev_from_recon(tab, d(c.x_t), d(c.x0), tt, bt, d(c.eps), 0. if grad is None else d(grad)).numpy()
            assert rel_err(out['x_prev'], ref) <= F64_EQ
            plain = pref.position_posterior(c.x_t, c.x0, lay.time, lay.row_graph, c0, cx, sd, grad=grad, eps=c.eps)
            assert np.array_equal(plain['x_prev'], out['x_prev']) and np.array_equal(plain['traj'], plain['x_prev'])
            assert np.array_equal(out['x0_out'], c.x0)
            assert np.array_equal(out['x_ctx_next'][c.lig2ctx], out['x_prev'])
            assert np.array_equal(out['x_ctx_next'][~c.is_lig], c.next_fill[~c.is_lig].astype(f64))
            assert np.array_equal(out['traj'], out['x_prev'] + c.center.astype(f64)[lay.row_graph])
            tb = lay.time[lay.row_graph]
            assert np.array_equal(out['x_prev'][tb == 0], out['mu'][tb == 0])


def test_restatements_reproduce_the_posterior_fixture():
    g = golden('g_posterior')
    sizes = np.bincount(g['batch'])
    assert np.array_equal(g['batch'], np.repeat(np.arange(sizes.size), sizes))
    for tag, K in (('node', 12), ('edge', 6)):
        qm, qt = pc.tables()[K]
        lp = pref.categorical_log_posterior(g[f'{tag}_log_v0'], g[f'{tag}_log_vt'], g['t'], g['batch'], qm, qt)
        assert _abs_err(lp, g[f'{tag}_post']) <= 2e-6, tag          # (the fixture is the reference's own fp32 evaluation)
        assert np.array_equal(pref.gumbel_scores(g[f'{tag}_post'], g[f'{tag}_u'])[1], g[f'{tag}_sample'])
    c0, cx, sd = pc.tables()['pos']
    out = pref.position_posterior(g['pos_xt'], g['pos_x0'], g['t'], g['batch'], c0, cx, sd, eps=g['pos_eps'])
    assert _abs_err(out['x_prev'], g['pos_prev']) <= 1e-6


def test_counter_forms_are_what_the_kernels_enumerate():
    """The three counter forms differ, agree where they must, and put step and stream in counter words 2 and 3."""
    lay = pc.layout()
    n, K = lay.n, 12
    flat = pref.uniforms(n, K, pc.SEED, 0, 999)
    idx = pref.uniforms(n, K, pc.SEED, 0, 999, lay.row_graph, lay.row0, None)
    key = pref.uniforms(n, K, pc.SEED, 0, 999, lay.row_graph, lay.row0, lay.keys)
    assert flat.dtype == f32 and flat.min() >= 0 and flat.max() < 1
    assert np.array_equal(flat[:1], idx[:1]) and not np.array_equal(flat[1:], idx[1:])       # graph 0: key 0, row0 0
    g2 = lay.row_graph == 2                                                                    # key 0: graph 0 of a flat run
    assert np.array_equal(key[g2], flat[:g2.sum()]) and not np.array_equal(key[~g2], idx[~g2])
    # element e -> counter e >> 2, word e & 3: the first four elements are the four words of counter 0
    w = pr_words([0, 0, 999, 0])
    assert np.array_equal(flat.reshape(-1)[:4], w) and np.array_equal(flat.reshape(-1)[4:8], pr_words([1, 0, 999, 0]))
    assert np.array_equal(key[lay.row0[1], :4], pr_words([0, 2 ** 31 - 1, 999, 0]))
    assert not np.array_equal(pref.uniforms(n, K, pc.SEED, 0, 3), flat) and not np.array_equal(pref.uniforms(n, K, pc.SEED, 2, 999), flat)
    assert not np.array_equal(pref.uniforms(n, K, pc.SEED & 0xFFFFFFFF, 0, 999), flat)        # the upper seed word
    u1, u2 = pref.position_uniforms(n, pc.SEED, 2, 999, lay.row_graph, lay.row0, lay.keys)
    r = int(lay.row0[1])
    w = pr_words([4, 2 ** 31 - 1, 999, 2])                                                    # graph 1, row 1, coordinate 1
    assert u1[r + 1, 1] == f32(1) - w[0] and u2[r + 1, 1] == w[1] and u1.min() > 0 and u1.max() <= 1
    w = pr_words([3 * r + 4, 0, 999, 2])
    f1, f2 = pref.position_uniforms(n, pc.SEED, 2, 999)
    assert f1[r + 1, 1] == f32(1) - w[0] and f2[r + 1, 1] == w[1]


def pr_words(ctr):
    from oracle import philox_ref as pr
    return pr.uniform24(pr.philox4x32([ctr], [[pc.SEED & 0xFFFFFFFF, pc.SEED >> 32]]))[0]


# ---- what fp32 rounding of the formulas costs: the floor under every tolerance ----
def test_fp32_floor_of_the_log_posterior():
    for c in _cat_cases():
        _report('log posterior', f'K={c.K} {c.profile} {c.lay.name}', _abs_err(_log_post(c, f32), _log_post(c)), pc.TOL_LOG)


def test_fp32_floor_of_the_gumbel_term():
    worst = 0.0
    for c in _cat_cases():
        for form in pc.FORMS + ('supplied',):
            u = _cat_uniforms(c, form)
            worst = max(worst, _abs_err(pref.gumbel_noise(u, f32), pref.gumbel_noise(u)))
    edge = np.array([0.0, 2.0 ** -24, 1.0 - 2.0 ** -24], dtype=f32)          # both ends of what the generator can give
    worst = max(worst, _abs_err(pref.gumbel_noise(edge, f32), pref.gumbel_noise(edge)))
    print(f'posterior fp32-reference {"gumbel term":20s} {"all cases, all counter forms":32s} {worst:.3e}   (constant {pc.GUMBEL_FLOOR:.1e})')
    assert worst <= pc.GUMBEL_FLOOR
    assert pc.TIE_BAND == pc.TOL_LOG + FLOOR_MULT * pc.GUMBEL_FLOOR


def _pos_variants(c):
    lay = c.lay
    yield 'eps', dict(eps=c.eps), pc.TOL_POS_EPS
    for form in pc.FORMS:
        for rng in pc.POS_RNG:
            row0, key = pc.counter_args(lay, form)
            u = pref.position_uniforms(lay.n, pc.SEED, rng['stream_id'], rng['step'], lay.row_graph, row0, key)
            yield f'{form} step {rng["step"]}', dict(u=u), pc.TOL_POS_DEVICE


def test_fp32_floor_of_the_position_posterior():
    c0, cx, sd = pc.tables()['pos']
    for batch in pc.BATCHES:
        c = pc.pos_case(batch)
        for name, noise, tol in _pos_variants(c):
            for grad in (None, c.grad):
                run = lambda dt: pref.position_posterior(c.x_t, c.x0, c.lay.time, c.lay.row_graph, c0, cx, sd, grad=grad, center=c.center,
                                                         dtype=dt, **noise)
                a, b = run(f32), run(f64)
                kind = 'position, eps given' if 'eps' in noise else 'position, device draw'
                err = max(_abs_err(a['x_prev'], b['x_prev']), _abs_err(a['traj'], b['traj']))
                _report(kind, f'{batch} {name} grad={grad is not None}', err, tol)


def _frag_draws(K, mask, form, batch='batch'):
    """Inputs of the fragment reference on the fixed rows of a case: rows, v0, lvl, the uniforms of the fragment streams."""
    lay, fr = pc.layout(batch), pc.frag_case(mask, batch)
    rows = np.nonzero(fr.fixed)[0]
    lvl_all = lay.time[lay.row_graph] - 1
    row0, key = pc.counter_args(lay, form)
    step = np.maximum(lvl_all, 0)
    out = dict(rows=rows, lvl=lvl_all[rows], x0f=fr.x0f[rows])
    if K is not None:
        out['v0'] = getattr(fr, f'cls{K}')[rows]
        out['u'] = pref.uniforms(lay.n, K, pc.SEED, pc.FRAG_STREAMS[K], step, lay.row_graph, row0, key)[rows]
    u1, u2 = pref.position_uniforms(lay.n, pc.SEED, pc.FRAG_STREAMS['pos'], step, lay.row_graph, row0, key)
    out['u_pos'] = (u1[rows], u2[rows])
    return out


def test_fp32_floor_of_the_fragment_replacement():
    sa, sb = pc.tables()['frag']
    for mask in ('third', 'whole'):
        for form in pc.FORMS:
            for K in (12, 6):
                d = _frag_draws(K, mask, form)
                run = lambda dt: pref.fragment_row(d['v0'], d['lvl'], K, pc.tables()[K][0], d['u'], d['x0f'], sa, sb,
                                                   pref.box_muller(*d['u_pos'], dtype=dt), dtype=dt)
                a, b = run(f32), run(f64)
                _report('fragment log', f'K={K} {mask} {form}', _abs_err(a['log'], b['log']), pc.TOL_LOG)
                if K == 12:
                    _report('fragment coordinates', f'{mask} {form}', _abs_err(a['x'], b['x']), pc.TOL_FRAG_POS)
                    frag = d['lvl'] < 0
                    assert np.array_equal(b['x'][frag], d['x0f'][frag].astype(f64))
                if mask == 'third':
                    frag = d['lvl'] < 0
                    assert frag.sum() > 50 and (b['cls'][frag] == d['v0'][frag]).all()
                    assert set(np.unique(b['log'][frag]).tolist()) == {0.0, pref.LOG_FLOOR}


# ---- the tie band ----
def _share(case, margin):
    share = float((margin < pc.TIE_BAND).mean())
    print(f'posterior tie band {pc.TIE_BAND:.1e}: {case:44s} {int((margin < pc.TIE_BAND).sum()):3d} of {margin.size:3d} rows = {100 * share:.2f} %')
    return share


def test_tie_band_share_is_at_most_one_percent():
    """From the reference alone: the share of rows whose float64 top-two score margin is below the band -- rows whose class the
    log-posterior tolerance cannot pin.  `ties` plants such rows on purpose and is reported only."""
    for c in _cat_cases():
        lp = _log_post(c)
        for form in pc.FORMS + ('supplied',):
            share = _share(f'K={c.K} {c.profile} {c.lay.name} {form}', pref.gumbel_scores(lp, _cat_uniforms(c, form))[2])
            assert c.profile == 'ties' or share <= pc.TIE_SHARE_CAP
    for mask in ('third', 'whole'):
        for form in pc.FORMS:
            for K in (12, 6):
                d = _frag_draws(K, mask, form)
                m = pref.fragment_row(d['v0'], d['lvl'], K, pc.tables()[K][0], d['u'])['margin']
                assert _share(f'fragment K={K} {mask} {form}', m) <= pc.TIE_SHARE_CAP


# ---- refusals that return before any launch ----
def test_entry_points_refuse_before_any_launch():
    """No GPU is needed: an empty batch returns PG_OK, a bad K or a missing required table PG_ERR_ARG, both without touching the
    runtime; pg_last_error() names the entry point."""
    from phoregen_amd import hip
    lib = hip.load_library()
    OK, ERR_ARG = 0, 1
    dummy = (C.c_int * 4)()
    p = C.addressof(dummy)                                # a non-NULL pointer that nothing may dereference
    N = None

    def cat(n, K, frag=()):
        fn = lib.pg_posterior_categorical_frag if frag else lib.pg_posterior_categorical
        return fn(N, N, N, N, N, N, n, K, N, 1, 0, 0, N, N, N, N, N, *frag, N)

    def pos(n, ctx=None, frag=None):
        head = (N, *ctx[:2]) if ctx else (N, N)
        tail = (N, N) + ((N, N) if ctx else ()) + (tuple(frag) if frag else ())
        fn = getattr(lib, 'pg_posterior_position' + ('_ctx' if ctx else '') + ('_frag' if frag else ''))
        return fn(*head, N, N, N, N, N, N, N, 1, 0, 0, n, N, N, N, *tail, N)

    # empty batches
    assert cat(0, 12) == OK and cat(0, 6, (N, 3)) == OK
    assert pos(0) == OK and pos(0, ctx=(N, N)) == OK and pos(0, frag=(N, N, N, N, 5)) == OK
    assert pos(0, ctx=(N, N), frag=(N, N, N, N, 5)) == OK
    assert lib.pg_fragment_noise(3, 1, 0, 0, *[N] * 12, 3, 4, 5, *[N] * 6) == OK
    # K other than 12 or 6
    assert cat(1, 5) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_categorical:') and b'5' in lib.pg_last_error()
    assert cat(1, 5, (p, 3)) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_categorical_frag:')
    assert cat(1, 12, (N, 3)) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_categorical_frag: frag_cls')
    # the context forms need both the buffer and the row map
    for ctx in ((N, p), (p, N)):
        assert pos(1, ctx=ctx) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_position_ctx:')
        assert pos(1, ctx=ctx, frag=(p, p, p, p, 5)) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_position_ctx_frag:')
    # the fragment forms need the class table, the coordinates and both scale tables
    for missing in range(4):
        frag = [p, p, p, p, 5]
        frag[missing] = N
        assert pos(1, frag=frag) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_position_frag:')
        assert pos(1, ctx=(p, p), frag=frag) == ERR_ARG and lib.pg_last_error().startswith(b'pg_posterior_position_ctx_frag:')


# ---- the keyword wrappers of phoregen_amd/posterior.py: which entry point each call reaches (no GPU: nothing is launched) ----
_T = torch.zeros(4, dtype=torch.int32)                  # a tensor whose (host) address nothing may dereference
_CAT = dict(logits=None, log_vt_in=None, row_graph=None, time_step=None, q_mats=None, q_onestep_T=None, seed=1, stream_id=0, step=0,
            graph_row0=None, graph_key=None, log_vt_out=None, onehot_out=None, stream=None)
_POS = dict(x_t=None, x0=None, row_graph=None, time_step=None, coef_x0=None, coef_xt=None, std=None, seed=1, stream_id=2, step=0,
            graph_row0=None, graph_key=None, x_prev=None, stream=None)
_CTX = dict(lig2ctx=_T, x_ctx_next=_T, x0_out=_T)
_FRAG = dict(frag_cls=_T, x0f=_T, sqrt_ab=_T, sqrt_1mab=_T, frag_stream_id=5)
_NOISE = dict(level=3, seed=1, node_cls=None, edge_cls=None, x0f=None, lig_graph=None, bond_graph=None, g_lig_off=None, g_bond_off=None,
              graph_key=None, q_node=None, q_edge=None, sqrt_ab=None, sqrt_1mab=None, node_stream_id=3, edge_stream_id=4, pos_stream_id=5,
              stream=None)


def _refused(prefix, fn, **kw):
    with pytest.raises(RuntimeError) as e:
        fn(**kw)
    assert f': {prefix}: ' in str(e.value), str(e.value)


def test_wrappers_return_on_zero_rows_for_every_entry_point():
    from phoregen_amd import hip, posterior
    posterior.categorical(n_rows=0, K=12, **_CAT)
    posterior.categorical(n_rows=0, K=6, frag_cls=_T, frag_stream_id=3, **_CAT)
    for ctx in ({}, _CTX):
        for frag in ({}, _FRAG):
            posterior.position(n_rows=0, **_POS, **ctx, **frag)
    posterior.fragment_noise(n_lig=0, n_bond=0, **_NOISE)
    posterior.guidance_grad(topo=C.byref(hip.PgTopo()), x_lig=None, h_edge_prev=None, lig_graph=None, g_lig_off=None, atom_prox=True,
                            min_d=1.2, max_d=2.8, center_prox=False, phore_center=None, mean_over_graphs=0, cnt_ws=None, mean_ws=None,
                            grad=None, stream=None)


def test_wrappers_pick_the_entry_point_from_what_they_are_given():
    """Inputs the library refuses before it launches anything; its error text names the entry point that was reached."""
    from phoregen_amd import posterior
    _refused('pg_posterior_categorical', posterior.categorical, n_rows=1, K=5, **_CAT)
    _refused('pg_posterior_categorical_frag', posterior.categorical, n_rows=1, K=5, frag_cls=_T, frag_stream_id=3, **_CAT)
    for table in ('frag_cls', 'x0f', 'sqrt_ab', 'sqrt_1mab'):
        frag = dict(_FRAG, **{table: None})
        _refused('pg_posterior_position_frag', posterior.position, n_rows=1, **_POS, **frag)
        _refused('pg_posterior_position_ctx_frag', posterior.position, n_rows=1, **dict(_POS, x0=_T), **_CTX, **frag)
    _refused('pg_posterior_position_ctx', posterior.position, n_rows=1, **_POS, **_CTX)                       # x0 missing
    _refused('pg_posterior_position_ctx_frag', posterior.position, n_rows=1, **_POS, **_CTX, **_FRAG)
    _refused('pg_posterior_position_ctx', posterior.position, n_rows=1, **dict(_POS, x0=_T), x_ctx_next=_T)   # lig2ctx missing
    _refused('pg_fragment_noise', posterior.fragment_noise, n_lig=1, n_bond=0, **_NOISE)


@pytest.mark.parametrize('T', [4, 1000])
def test_step_check(T):
    from phoregen_amd.models.diffusion import check_step
    check_step(0, T), check_step(T - 1, T), check_step(np.int64(T - 1), T)
    for bad in (-1, T, 0.5, float(T - 1), None, '0', True):
        with pytest.raises(ValueError):
            check_step(bad, T)
