"""-m gpu: every graph-side kernel (csrc/graph_ops.hip, the guidance kernels of csrc/posterior.hip) through the C ABI against the
float64 restatement of its own formula (tests/graph_ops_reference.py, held equal to the oracle in tests/test_graph_ops_host.py), on
the batches of tests/graph_ops_cases.py: exact distance ties, graphs at the 512-node limit, k other than 32, time steps at the clamp,
graphs without a bond.

Integer outputs and pure copies are exact; float outputs meet the forward bound of SURVEY.md 8c (helpers.TOL) per output tensor per
case.  Every output buffer is pre-filled with a sentinel: rows the contract writes must all be overwritten, rows it does not write
must keep it.  Buffers the kernels index by neighbour id carry guard rows in front and behind (NaN), so that a kernel reading a slot it
must not read shows as a wrong number.  Each error is printed (pytest -s) before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_ops_cases as gc
import graph_ops_reference as gr
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT, ISENT = -7777.0, -7777


def _lib():
    from phoregen_amd import hip
    return hip, hip.lib(), hip.stream_ptr()


def _check(entry, case, out, ref):
    out = out.detach().cpu()
    assert torch.isfinite(out).all(), (entry, case)
    err = rel_err(out, ref)
    print(f'graph_ops kernel {entry:16s} {case:28s} {err:.3e}')
    assert err <= TOL, (entry, case, err)


def _guarded(x, front=1, back=64):
    """x on the device inside a larger allocation whose other rows are NaN: a read of row -1 or of rows n .. n + 63 stays inside the
    allocation and poisons the result instead of leaving the buffer."""
    buf = torch.full((front + x.shape[0] + back,) + tuple(x.shape[1:]), float('nan'), device=DEV)
    buf[front:front + x.shape[0]] = x.to(DEV)
    return buf, buf[front:front + x.shape[0]]


def _topo_without_edge_ref(plan):
    from phoregen_amd import hip
    t = hip.PgTopo.from_buffer_copy(plan.topo)
    t.edge_ref = None
    return t


# ---- pg_knn_ctx ----
def _run_knn(c):
    hip, lib, s = _lib()
    n, k = c.plan.n_ctx, c.k
    nbr = torch.full((n * k + 64,), ISENT, dtype=torch.int32, device=DEV)
    deg = torch.full((n + 64,), ISENT, dtype=torch.int32, device=DEV)
    _, x = _guarded(c.x)
    hip.check(lib.pg_knn_ctx(c.plan.topo_ref, x.data_ptr(), k, nbr.data_ptr(), deg.data_ptr(), s))
    torch.cuda.synchronize()
    nbr, deg = nbr.cpu(), deg.cpu()
    assert (nbr[n * k:] == ISENT).all() and (deg[n:] == ISENT).all()
    return nbr[:n * k].reshape(n, k).numpy().astype(np.int64), deg[:n].numpy().astype(np.int64)


@pytest.mark.parametrize('k', gc.KNN_KS)
def test_knn_lattice_lists_are_exact(k):
    """Lattice coordinates (d2 exact in fp32, ties everywhere, repeated points, wholly coincident graphs), graphs of 1, 2, k, k + 1,
    63, 64, 65, 128, 129, 511 and 512 nodes: ascending d2, ties by ascending index, self excluded, -1 past deg = min(k, count - 1)."""
    c = gc.knn_case(k, 'lattice', DEV)
    nbr, deg = _run_knn(c)
    ref_nbr, ref_deg = gr.knn_lists(c.x, gr.graph_ranges(c.topo.g_off), k)
    assert (deg == ref_deg).all()
    bad = np.nonzero((nbr != ref_nbr).any(1))[0]
    assert bad.size == 0, (bad[:5], nbr[bad[:2]], ref_nbr[bad[:2]])


@pytest.mark.parametrize('k', gc.KNN_KS)
def test_knn_gaussian_lists_are_ordered_and_nearest(k):
    """Gaussian coordinates, nothing excluded: the list is strictly ascending in the key (fp32 d2 = (dx^2 + dy^2) + dz^2 without
    contraction, then index), holds exactly deg distinct in-graph nodes other than the centre, and in float64 is the deg nearest up
    to the rounding of one fp32 d2 (4 ulp of the node's largest d2)."""
    c = gc.knn_case(k, 'gauss', DEV)
    nbr, deg = _run_knn(c)
    for first, count in gr.graph_ranges(c.topo.g_off):
        dg = min(k, count - 1)
        d32 = gr.dist2(c.x, first, count, torch.float32).numpy()
        d64 = gr.dist2(c.x, first, count).numpy()
        for i in range(count):
            row = nbr[first + i]
            assert deg[first + i] == dg and (row[dg:] == -1).all()
            loc = row[:dg] - first
            assert ((loc >= 0) & (loc < count) & (loc != i)).all() and np.unique(loc).size == dg, (first, i)
            key = [(d32[i, j], j) for j in loc.tolist()]
            assert all(a < b for a, b in zip(key[:-1], key[1:])), (first, i)
            if 0 < dg < count - 1:
                slack = 4.0 * float(np.spacing(np.float32(d32[i].max())))
                rest = np.setdiff1d(np.arange(count), np.append(loc, i))
                kth = np.sort(np.delete(d64[i], i))[dg - 1]
                assert d64[i, loc].max() <= kth + slack and d64[i, rest].min() >= d64[i, loc[-1]] - slack, (first, i)


def test_knn_refusals_come_before_any_launch():
    hip, lib, s = _lib()
    c = gc.knn_case(3, 'lattice', DEV)
    big, _, _ = gc.make_plan([13, 2], [500, 1], DEV)                 # 513 context nodes in one graph
    n = max(c.plan.n_ctx, big.n_ctx)
    x = torch.zeros(n, 3, device=DEV)
    nbr = torch.full((n * 65,), ISENT, dtype=torch.int32, device=DEV)
    deg = torch.full((n,), ISENT, dtype=torch.int32, device=DEV)
    for plan, k, word in ((c.plan, 0, b'[1, 64]'), (c.plan, 65, b'[1, 64]'), (big, 32, b'at most 512')):
        assert lib.pg_knn_ctx(plan.topo_ref, x.data_ptr(), k, nbr.data_ptr(), deg.data_ptr(), s) != 0
        assert word in lib.pg_last_error(), lib.pg_last_error()
    torch.cuda.synchronize()
    assert (nbr == ISENT).all() and (deg == ISENT).all()


# ---- pg_lig_nn3 / pg_lig_normals ----
def test_lig_nn3_and_normals_on_the_lattice():
    """Ligands of 1, 2, 3, 4, 64, 65 and 128 atoms, a pharmacophore node on or right beside every atom (never picked): nn3 exact, ligand
    rows of nrm = float64 mean of those positions - x within 1 ulp of the largest term, pharmacophore rows = phore_norm exactly."""
    hip, lib, s = _lib()
    c = gc.normals_case(DEV)
    tp, plan = c.topo, c.plan
    n = plan.n_ctx
    _, x = _guarded(c.x)
    nn3 = torch.full((plan.n_lig * 3 + 64,), ISENT, dtype=torch.int32, device=DEV)
    hip.check(lib.pg_lig_nn3(plan.topo_ref, x.data_ptr(), nn3.data_ptr(), s))
    nrm = torch.full((n * 3 + 64,), SENT, device=DEV)
    pn = c.phore_norm.to(DEV)
    hip.check(lib.pg_lig_normals(plan.topo_ref, x.data_ptr(), pn.data_ptr(), plan.phore2ctx.data_ptr(), nrm.data_ptr(), s))
    torch.cuda.synchronize()
    nn3, nrm = nn3.cpu(), nrm.cpu()
    assert (nn3[plan.n_lig * 3:] == ISENT).all() and (nrm[n * 3:] == SENT).all()
    nn3, nrm = nn3[:plan.n_lig * 3].reshape(-1, 3).numpy().astype(np.int64), nrm[:n * 3].reshape(n, 3)
    ref_nn3 = gr.lig_nn3(c.x, gr.ligand_ranges(tp.g_off, tp.g_nph, tp.g_nlig), tp.lig2ctx)
    assert (nn3 == ref_nn3).all(), np.nonzero((nn3 != ref_nn3).any(1))[0][:5]
    assert (nn3[0] == -1).all() and tp.is_lig[nn3[nn3 >= 0]].all()
    ref = gr.lig_normals(c.x, ref_nn3, tp.lig2ctx, c.phore_norm, tp.phore2ctx)
    assert torch.equal(nrm[tp.phore2ctx], c.phore_norm)
    assert torch.equal(nrm[tp.lig2ctx[0]], -c.x[tp.lig2ctx[0]])          # 1-atom ligand: mean of nothing is 0
    x64 = c.x.double()
    largest = torch.maximum(torch.maximum((ref + x64).abs(), x64.abs()), ref.abs())[tp.lig2ctx]
    ulp = torch.as_tensor(np.spacing(largest.numpy().astype(np.float32)).astype(np.float64))
    assert ((nrm.double() - ref)[tp.lig2ctx].abs() <= ulp).all()
    _check('pg_lig_normals', 'lattice', nrm, ref)


# ---- pg_edge_gate ----
@pytest.mark.parametrize('profile', ['default', 'gamma_signed', 'trained_like'])
@pytest.mark.parametrize('k', gc.GATE_KS)
def test_edge_gate_against_float64(k, profile):
    """sigmoid(W2 . ReLU(LN(W1 . smear(d) + b1)) + b2) from the unpacked state dict, nbr / deg from the reference kNN; degrees 0, 1, 15,
    16, 17, 31, distances 0 and far beyond the last Gaussian.  Slots from deg to k are exactly 0, nothing is written at or beyond k, and
    what nbr holds past deg is never read (a second run with ids past the last node there gives the same bits)."""
    from phoregen_amd.packing import pack_gate
    hip, lib, s = _lib()
    c = gc.gate_case(k, DEV)
    n = c.plan.n_ctx
    sd = gc.gate_weights(profile)
    W = [sd['denoiser.edge_pred_layer.net.' + w] for w in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias')]
    g = {key: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for key, v in pack_gate(sd).items()}
    ref_nbr, ref_deg = gr.knn_lists(c.x, gr.graph_ranges(c.topo.g_off), k)
    ref = gr.edge_gate(c.x, ref_nbr, ref_deg, *W)
    _, x = _guarded(c.x)
    deg = torch.as_tensor(ref_deg, dtype=torch.int32).to(DEV)
    past = np.arange(k)[None, :] >= ref_deg[:, None]
    garbage = ref_nbr.copy()
    garbage[past] = (n + np.arange(n * k).reshape(n, k) % 64)[past]            # ids past the last node (guard rows of x: NaN)
    outs = []
    for ids in (ref_nbr, garbage):
        nbr = torch.full((n * k + 64,), -1, dtype=torch.int32, device=DEV)          # (guard slots behind the last node's list too)
        nbr[:n * k] = torch.as_tensor(ids, dtype=torch.int32).reshape(-1).to(DEV)
        ew = torch.full((n * k + 64,), SENT, device=DEV)
        hip.check(lib.pg_edge_gate(c.plan.topo_ref, x.data_ptr(), nbr.data_ptr(), deg.data_ptr(), k, g['W0'].data_ptr(),
                                   g['b0'].data_ptr(), g['g'].data_ptr(), g['b'].data_ptr(), g['W3'].data_ptr(), C.c_float(g['b3']),
                                   ew.data_ptr(), s))
        torch.cuda.synchronize()
        ew = ew.cpu()
        assert (ew[n * k:] == SENT).all()
        outs.append(ew[:n * k].reshape(n, k))
    assert (outs[0][torch.as_tensor(past)] == 0).all()
    _check('pg_edge_gate', f'{profile} k={k}', outs[0], ref)
    assert torch.equal(outs[0], outs[1])


# ---- pg_bond_smear / pg_apply_dx ----
def test_bond_smear_and_apply_dx_against_float64():
    hip, lib, s = _lib()
    for i, c in enumerate(gc.geom_cases(DEV)):
        tp, plan = c.topo, c.plan
        n, E = plan.n_ctx, plan.n_bond
        x, dx1, dx2 = c.x.to(DEV), c.dx1.to(DEV), c.dx2.to(DEV)
        x_new = torch.full((n * 3 + 64,), SENT, device=DEV)
        hip.check(lib.pg_apply_dx(plan.topo_ref, x.data_ptr(), dx1.data_ptr(), dx2.data_ptr(), x_new.data_ptr(), s))
        G = torch.full((E * 20 + 64,), SENT, device=DEV)
        hip.check(lib.pg_bond_smear(plan.topo_ref, x.data_ptr(), G.data_ptr(), s))
        torch.cuda.synchronize()
        x_new, G = x_new.cpu(), G.cpu()
        assert (x_new[n * 3:] == SENT).all() and (G[E * 20:] == SENT).all()
        x_new, G = x_new[:n * 3].reshape(n, 3), G[:E * 20].reshape(E, 20)
        assert torch.equal(x_new[tp.is_lig == 0], c.x[tp.is_lig == 0])
        _check('pg_apply_dx', f'batch {i}', x_new, gr.apply_dx(c.x, c.dx1, c.dx2, tp.is_lig))
        if E:
            _check('pg_bond_smear', f'batch {i}', G, gr.bond_smear(c.x, tp.bond_src, tp.bond_dst))


# ---- pg_embed_ctx / pg_embed_bond ----
def test_embeddings_against_float64():
    """Time steps 0, 1, 499, 999, 1000 and -- beyond the clamp -- 5000 and -3; one-hot and soft rows; both halves of pg_embed_ctx alone;
    pg_embed_bond through edge_ref and, on pre-permuted rows, without it."""
    hip, lib, s = _lib()
    c = gc.embed_case(DEV)
    tp, plan = c.topo, c.plan
    n, E = plan.n_ctx, plan.n_bond
    off, coeff = gr.time_tables(dtype=torch.float32)                  # the tables as the model holds them
    d = {k: getattr(c, k).to(DEV) for k in ('h_node', 'pos', 'time_step', 'W_node', 'W_edge', 'h_phore_emb', 'pos_phore', 'h_edge')}
    off_d, coeff_d = off.to(DEV), coeff.to(DEV)
    ref_h, ref_x = gr.embed_ctx(c.h_node, c.pos, c.time_step, tp.lig_graph, tp.lig2ctx, c.W_node, off, coeff, c.h_phore_emb,
                                c.pos_phore, tp.phore2ctx)
    ts = gr.time_smear(c.time_step, off.double(), coeff.double())

    def run(want_h, want_x):
        h = torch.full((n * 128 + 64,), SENT, device=DEV)
        x = torch.full((n * 3 + 64,), SENT, device=DEV)
        hip.check(lib.pg_embed_ctx(plan.topo_ref, d['h_node'].data_ptr(), d['pos'].data_ptr(), d['time_step'].data_ptr(),
                                   d['W_node'].data_ptr(), off_d.data_ptr(), coeff_d.data_ptr(), d['h_phore_emb'].data_ptr(),
                                   d['pos_phore'].data_ptr(), plan.phore2ctx.data_ptr(), h.data_ptr() if want_h else None,
                                   x.data_ptr() if want_x else None, s))
        torch.cuda.synchronize()
        return h.cpu(), x.cpu()
    for want_h, want_x in ((True, True), (True, False), (False, True)):
        h, x = run(want_h, want_x)
        assert (h[n * 128:] == SENT).all() and (x[n * 3:] == SENT).all()
        h, x = h[:n * 128].reshape(n, 128), x[:n * 3].reshape(n, 3)
        if want_h:
            _check('pg_embed_ctx', f'h_ctx (x_ctx {"too" if want_x else "NULL"})', h, ref_h)
            _check('pg_embed_ctx', 'time columns', h[tp.lig2ctx][:, 118:], ts[tp.lig_graph])
            assert torch.equal(h[tp.phore2ctx], c.h_phore_emb)
        else:
            assert (h == SENT).all()
        if want_x:
            assert torch.equal(x.double(), ref_x)
        else:
            assert (x == SENT).all()
    # bond rows
    ref_hb = gr.embed_bond(c.h_edge, tp.edge_ref, c.time_step, tp.bond_graph, c.W_edge, off, coeff)
    assert not plan.edge_identity
    outs = []
    pre = c.h_edge[tp.edge_ref].contiguous().to(DEV)
    for topo, rows in ((plan.topo, d['h_edge']), (_topo_without_edge_ref(plan), pre)):
        hb = torch.full((E * 128 + 64,), SENT, device=DEV)
        hip.check(lib.pg_embed_bond(C.byref(topo), rows.data_ptr(), plan.bond_graph.data_ptr(), d['time_step'].data_ptr(),
                                    d['W_edge'].data_ptr(), off_d.data_ptr(), coeff_d.data_ptr(), hb.data_ptr(), s))
        torch.cuda.synchronize()
        hb = hb.cpu()
        assert (hb[E * 128:] == SENT).all()
        outs.append(hb[:E * 128].reshape(E, 128))
    _check('pg_embed_bond', 'h_bond', outs[0], ref_hb)
    _check('pg_embed_bond', 'time columns', outs[0][:, 118:], ts[tp.bond_graph])
    assert torch.equal(outs[0], outs[1])


# ---- pg_atom_count ----
def test_atom_count_against_float64():
    """Graphs without a pharmacophore node, with EX nodes only, with 1, 64, 65 and 300 nodes; logits at +-40."""
    hip, lib, s = _lib()
    c = gc.count_case()
    B = c.n_graphs
    cl, cu = torch.full((B + 64,), SENT, device=DEV), torch.full((B + 64,), SENT, device=DEV)
    s_all, s_l, is_ex, pg = c.s_all.to(DEV), c.s_l.to(DEV), c.is_ex.to(DEV), c.phore_graph.to(torch.int32).to(DEV)
    hip.check(lib.pg_atom_count(s_all.data_ptr(), s_l.data_ptr(), is_ex.data_ptr(), pg.data_ptr(), pg.numel(), B, cl.data_ptr(),
                                cu.data_ptr(), s))
    torch.cuda.synchronize()
    cl, cu = cl.cpu(), cu.cpu()
    assert (cl[B:] == SENT).all() and (cu[B:] == SENT).all()
    ref_l, ref_u = gr.atom_count(c.s_all, c.s_l, c.is_ex, c.phore_graph, B)
    _check('pg_atom_count', 'count_l', cl[:B], ref_l)
    _check('pg_atom_count', 'count_u', cu[:B], ref_u)
    assert cl[0] == 0 and cu[0] == 0 and cl[1] == 0 and cl[6] == 0 and cu[6] == 0


# ---- pg_guidance_grad ----
@pytest.mark.parametrize('mean_over', [0, 11])
@pytest.mark.parametrize('atom,center', gc.GUIDANCE_MODES)
def test_guidance_grad_against_float64(atom, center, mean_over):
    """A 1-atom ligand, a graph whose bond rows are all class 0, rows where class 0 ties the maximum, pairs whose two directions
    disagree, bond lengths exactly min_d and max_d, the divisor defaulted (0) and larger than the batch, both edge_ref forms."""
    hip, lib, s = _lib()
    c = gc.guidance_case(DEV)
    tp, plan = c.topo, c.plan
    N, B = plan.n_lig, mean_over or c.B
    ref = gr.guidance_grad(c.x, tp.lig_graph, c.h_edge, c.edge_index, c.batch_edge, B, c.B, atom, gc.MIN_D, gc.MAX_D, center,
                           c.phore_center)
    x, pc = c.x.to(DEV), c.phore_center.to(DEV)
    assert not plan.edge_identity
    outs = []
    for topo, rows in ((plan.topo, c.h_edge.to(DEV)), (_topo_without_edge_ref(plan), c.h_edge[tp.edge_ref].contiguous().to(DEV))):
        grad = torch.full((N * 3 + 64,), SENT, device=DEV)
        cnt, mean = torch.full((c.B,), SENT, device=DEV), torch.full((c.B * 3,), SENT, device=DEV)
        hip.check(lib.pg_guidance_grad(C.byref(topo), x.data_ptr(), rows.data_ptr(), plan.lig_graph.data_ptr(), plan.g_lig_off.data_ptr(),
                                       atom, gc.MIN_D, gc.MAX_D, center, pc.data_ptr(), mean_over, cnt.data_ptr(), mean.data_ptr(),
                                       grad.data_ptr(), s))
        torch.cuda.synchronize()
        grad = grad.cpu()
        assert (grad[N * 3:] == SENT).all()
        outs.append(grad[:N * 3].reshape(N, 3))
        assert float(cnt[1]) == 0.0                                   # the graph whose rows are all class 0
    _check('pg_guidance_grad', f'atom={atom} center={center} B={B}', outs[0], ref)
    assert torch.equal(outs[0], outs[1])
    if not center:
        assert (outs[0][:c.off[2]] == 0).all()                        # the 1-atom ligand and the bond-less graph: no force, no NaN
