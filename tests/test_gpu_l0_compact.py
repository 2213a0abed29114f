"""-m gpu: layer 0's bond-row products over the 16 embedding inputs of a bond row (options.l0_compact).

  * pg_embed_bond_e16: e16 is exact (the input rows in internal order, and the very floats of h_bond[:, 118:128]); h_bond against float64
    with the bound of the graph-ops parity test (helpers.TOL), and bit for bit against an fp32 restatement of the one-thread-per-element
    formula (v = fma(h_k, W[c,k], v) in k order from v = 0) on the linear columns; with and without e16 the same h_bond.
  * pg_gemm with K = 16 and K = 16 + 20 (both operands in registers, csrc/gemm_stream.hip): M = 64 (one tile), 72 (the last tile anchored at
    M - 64), 200; N = 128 and 256; with and without a gathered operand; M = 6 goes to the tiled kernel (pg_gemm_is_streaming is asked for
    every launch: 1 from 64 rows up, 0 below).  `exact` operands bit for bit,
    `real` operands under the per-element bound of tests/dense_cases.py, (K + 4) 2^-23 (sum |x||w| + |bias| + |add1|); operands and
    outputs are slices of NaN buffers whose guards must stay NaN.
  * Engine: P, CsB2 and qhid of layer 0 as the engine's own builders launch them, with l0_compact on and off, each against ONE float64
    reference of the uncomposed expression (float64 embedding of the inputs . W^T + gathered rows).  Bounds, with
    T = sum_k |h_k| sum_j |W[c,j]||W_edge[j,k]| + sum_t |ts_t||W[c,118+t]| (+ sum_g |G_g||W[c,128+g]| for P) and A = |gathered row|:
      off: h_bond0 is a 6-term fp32 sum (error <= 6 * 2^-24 of its absolute sum), then a K-term product ((K + 4) 2^-23, dense_cases):
           (K + 4 + 3) 2^-23 (T + A), K = 128 or 148;
      on:  the composed weight is rounded once (2^-24 of its absolute sum, tests/test_l0_compact_host.py), then a K-term product:
           (K + 4 + 1) 2^-23 (T + A), K = 16 or 36.
    Batches: ligands of 2, 5 and 9 atoms (94 bond rows: the streaming kernel, one tile and the anchored one) and ligands of 3 and 4 atoms
    (18 bond rows: the tiled kernel)."""
import ctypes as C

import pytest
import torch

import dense_cases as dc
import dense_reference as dref
import graph_ops_cases as gc
import graph_ops_reference as gr
import test_gpu_dense as tgd
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U23 = 2.0 ** -23


def _lib():
    from phoregen_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


# ---- pg_embed_bond_e16 ----
def _embed_inputs(na, nph, t, seed=5):
    g = torch.Generator().manual_seed(seed)
    plan, _, _ = gc.make_plan(na, nph, DEV)
    E = plan.n_bond
    soft = torch.softmax(torch.randn(E, 6, generator=g), -1)
    hot = torch.nn.functional.one_hot(torch.randint(0, 6, (E,), generator=g), 6).float()
    h_edge = torch.where((torch.arange(E) % 2 == 0)[:, None], hot, soft)
    return plan, gc.topo_arrays(plan), h_edge, torch.tensor(t, dtype=torch.int64)


def test_embed_bond_e16_is_exact_and_h_bond_follows_the_per_element_formula():
    from phoregen_amd.weights import make_tensor
    hip, lib, s = _lib()
    plan, tp, h_edge, t = _embed_inputs([2, 5, 9], [3, 1, 4], [17, 500, 983])
    E = plan.n_bond
    assert E == 94 and not plan.edge_identity
    W_edge = make_tensor('edge_embedder.weight', (118, 6), 0)
    off, coeff = gr.time_tables(dtype=torch.float32)
    d = [x.to(DEV) for x in (h_edge, t, W_edge, off, coeff)]

    def run(with_e16):
        hb = torch.full((E * 128 + 64,), float('nan'), device=DEV)
        e16 = torch.full((E * 16 + 64,), float('nan'), device=DEV)
        args = (plan.topo_ref, d[0].data_ptr(), plan.bond_graph.data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                hb.data_ptr())
        hip.check(lib.pg_embed_bond_e16(*args, e16.data_ptr(), s) if with_e16 else lib.pg_embed_bond(*args, s))
        torch.cuda.synchronize()
        hb, e16 = hb.cpu(), e16.cpu()
        assert bool(torch.isnan(hb[E * 128:]).all()) and bool(torch.isnan(e16[E * 16:]).all())
        return hb[:E * 128].reshape(E, 128), e16[:E * 16].reshape(E, 16)
    hb, e16 = run(True)
    hb_plain, e16_plain = run(False)
    assert bool(torch.isnan(e16_plain).all())
    assert torch.equal(hb, hb_plain)                                         # (one kernel: the optional output changes nothing else)
    # the linear columns bit for bit: the chain of fused multiply-adds a thread per element evaluated, restated in float64 with one
    # rounding to fp32 per step (a product of two fp32 numbers plus an fp32 number is exact in float64 up to double rounding, which the
    # comparison below would show as a differing element)
    hr, v = h_edge[tp.edge_ref].double(), torch.zeros(E, 118, dtype=torch.float64)
    for k in range(6):
        v = (hr[:, k:k + 1] * W_edge[:, k].double()[None, :] + v).float().double()
    differ = int((hb[:, :118].double() != v).sum())
    print(f'l0_compact pg_embed_bond_e16 linear columns: {differ} of {E * 118} elements differ from the fused-multiply-add chain')
    assert differ == 0
    assert torch.equal(e16[:, :6], h_edge[tp.edge_ref])                      # the input rows in internal order
    assert torch.equal(e16[:, 6:], hb[:, 118:])                              # the very floats of the time columns
    ref = gr.embed_bond(h_edge, tp.edge_ref, t, tp.bond_graph, W_edge, off, coeff)
    err = rel_err(hb, ref)
    print(f'l0_compact pg_embed_bond_e16 h_bond {err:.3e} (bound {TOL:.1e})')
    assert err <= TOL
    ts = gr.time_smear(t, off.double(), coeff.double())
    assert rel_err(e16[:, 6:], ts[tp.bond_graph]) <= TOL


def test_embed_bond_e16_refuses_unaligned_outputs():
    hip, lib, s = _lib()
    plan, tp, h_edge, t = _embed_inputs([3, 4], [2, 2], [5, 6])
    z = torch.zeros(plan.n_bond * 128 + 8, device=DEV)
    rc = lib.pg_embed_bond_e16(plan.topo_ref, z.data_ptr(), plan.bond_graph.data_ptr(), t.to(DEV).data_ptr(), z.data_ptr(), z.data_ptr(),
                               z.data_ptr(), z.data_ptr(), z.data_ptr() + 4, s)
    assert rc == 1 and lib.pg_last_error().startswith(b'pg_embed_bond')


# ---- pg_gemm, K = 16 and K = 16 + 20 ----
@pytest.fixture(scope='module')
def gemm_pool():
    """Operands of every case, drawn once per profile: M = 200 rows (smaller cases take the leading rows)."""
    out = {}
    for profile in ('exact', 'real'):
        g = dc.gen(23, len(profile))
        out[profile] = dict(X=dc.plant(dc.draw(profile, (200, 16), g), profile), X2=dc.draw(profile, (200, 20), g),
                            W=dc.draw(profile, (256, 36), g, 'w'), bias=dc.draw(profile, (256,), g, 'add'),
                            add=dc.draw(profile, (dc.GEMM_ADD_ROWS, 256), g, 'add'), idx=dc.gather_index(200, dc.GEMM_ADD_ROWS, g))
    return out


def _gemm_args(pool, M, N, K, gather):
    a = dict(X=pool['X'][:M], W=pool['W'][:N, :K].contiguous(), bias=pool['bias'][:N].contiguous())
    if K == 36:
        a['X2'] = pool['X2'][:M]
    if gather:
        idx = pool['idx'][:M].clone()
        idx[M - 1] = 0
        a.update(add1=pool['add'][:, :N].contiguous(), idx1=idx)
    return a


class _AskingLib:
    """The library with pg_gemm preceded by the question which kernel the call takes."""

    def __init__(self, lib):
        self._lib, self.asked = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def pg_gemm(self, g, s):
        self.asked.append(self._lib.pg_gemm_is_streaming(g))
        return self._lib.pg_gemm(g, s)


@pytest.mark.parametrize('gather', [False, True], ids=['plain', 'gathered'])
@pytest.mark.parametrize('K', [16, 36])
@pytest.mark.parametrize('N', [128, 256])
@pytest.mark.parametrize('M', [64, 72, 200, 6])
def test_register_operand_gemm_against_float64(gemm_pool, M, N, K, gather, monkeypatch):
    hip, lib, s = _lib()
    asking = _AskingLib(lib)
    monkeypatch.setattr(tgd, '_lib', lambda: (hip, asking, s))
    for profile in ('exact', 'real'):
        d = tgd._stage_gemm(_gemm_args(gemm_pool[profile], M, N, K, gather))
        assert d['X'].data_ptr() % 16 == 0 and d['X'].stride(0) % 4 == 0
        ref, S, _ = dref.gemm(**d)
        case = f'M={M} N={N} K={K} {"gathered" if gather else "plain"} {profile}'
        Y = tgd._run_gemm(d, True)
        if profile == 'exact':
            tgd._check_exact('gemm l0 registers' if M >= 64 else 'gemm l0 tiled', case, Y, ref)
        else:
            tgd._check_bound('gemm l0 registers' if M >= 64 else 'gemm l0 tiled', case, Y, ref, dref.gemm_bound(S, K))
    assert asking.asked == [1 if M >= 64 else 0] * 2, asking.asked


# ---- the engine's layer-0 products ----
@pytest.fixture(scope='module')
def model():
    from phoregen_amd.config import default_model_config
    from phoregen_amd.models.diffusion import PhoreDiff
    from phoregen_amd.weights import init_deterministic_
    return init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).eval().to(DEV)


def _layer0_products(model, plan, h_edge, t, Y1, G, compact):
    from phoregen_amd import options
    from phoregen_amd.engine import Engine
    with options.override(l0_compact=compact, streams=False):
        eng = Engine(model.packed(), plan, knn_k=model.denoiser.k)
    assert eng.l0_compact == compact
    w, L0 = eng.ws, eng.pack.layers[0]
    w.in_h_edge.copy_(h_edge)
    w.in_t.copy_(t)
    w.Y1.copy_(Y1)
    w.G.copy_(G)
    for b in (w.P, w.CsB2, w.qhid):
        b.fill_(float('nan'))
    prog = []
    eng._embed_bond(prog, w.in_t)
    eng._triplet_rows(prog, L0, w.hb[0], w.Y1, True, l0=True)
    eng._bond_node_rows(prog, L0, w.hb[0], w.Y1, l0=True)
    eng._triplet_queries(prog, L0, w.hb[0], w.Y1, l0=True)
    gemms = [a[0]._obj for fn, a, _ in prog if fn.__name__ == 'pg_gemm']
    assert [(g.K1, g.K2) for g in gemms[:3]] == ([(16, 20), (16, 0), (16, 0)] if compact else [(128, 20), (128, 0), (128, 0)])
    eng._run(prog)
    torch.cuda.synchronize()
    return w.P.double().cpu(), w.CsB2.double().cpu(), w.qhid.double().cpu(), w.hb[0].cpu()


@pytest.mark.parametrize('na,nph,t', [([2, 5, 9], [3, 1, 4], [17, 500, 983]), ([3, 4], [2, 3], [250, 760])], ids=['E94', 'E18'])
def test_engine_layer0_products_on_and_off_against_float64(model, na, nph, t):
    plan, tp, h_edge, t = _embed_inputs(na, nph, t, seed=9)
    E, n = plan.n_bond, plan.n_ctx
    assert (E >= 64) == (len(na) == 3)
    g = torch.Generator().manual_seed(31)
    Y1, G = torch.randn(n, 1920, generator=g), torch.rand(E, 20, generator=g)
    on = _layer0_products(model, plan, h_edge, t, Y1, G, True)
    off = _layer0_products(model, plan, h_edge, t, Y1, G, False)
    assert torch.equal(on[3], off[3])                                        # h_bond0 itself does not depend on the switch
    pk = model.packed()
    L0, We = pk.layers[0], pk.W_edge_emb.double().cpu()
    h = h_edge[tp.edge_ref].double()
    ts = on[3][:, 118:].double()                                             # the smearing values as the device wrote them (exact in e16)
    src, dst = torch.as_tensor(tp.bond_src), torch.as_tensor(tp.bond_dst)
    hb64, hb_abs = torch.cat([h @ We.T, ts], 1), torch.cat([h.abs() @ We.abs().T, ts.abs()], 1)
    Y1d, Gd = Y1.double(), G.double()
    cases = (('P', 0, L0.TB.W_hbg, Y1d[src, 10 * 128:12 * 128], True), ('CsB2', 1, L0.NB.W_hb, Y1d[src, 7 * 128:9 * 128], False),
             ('qhid', 2, L0.TB.W_q_hb, Y1d[dst, 14 * 128:15 * 128], False))
    for name, i, W, add, with_g in cases:
        W = W.double().cpu()
        ref = hb64 @ W[:, :128].T + add
        T = hb_abs @ W[:, :128].abs().T + add.abs()
        if with_g:
            ref, T = ref + Gd @ W[:, 128:].T, T + Gd.abs() @ W[:, 128:].abs().T
        for tag, got, K, extra in (('on', on[i], 36 if with_g else 16, 1), ('off', off[i], 148 if with_g else 128, 3)):
            assert bool(torch.isfinite(got).all()), (name, tag)
            err, bound = (got - ref).abs(), (K + 4 + extra) * U23 * T
            ratio = float((err / bound.clamp_min(1e-300)).max())
            print(f'l0_compact engine E={E:3d} {name:5s} {tag:3s} largest error {float(err.max()):.3e}, largest error / bound {ratio:.3f}')
            assert bool((err <= bound).all()), (name, tag, ratio)
