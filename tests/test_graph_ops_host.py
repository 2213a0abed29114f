"""CPU part of the graph-side kernel tests: the float64 restatements of tests/graph_ops_reference.py are held equal to the oracle's
functions evaluated in float64 on the very batches the GPU tests use (tests/graph_ops_cases.py), and the same restatements
evaluated in fp32 stay below TOL / FLOOR_MULT of the float64 result -- the bound the kernels are asked to meet is then at least
three times what fp32 rounding of the formula itself costs on these inputs.  Each figure is printed (pytest -s) before it is
asserted; profiles/graph_ops_parity.md records them."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_ops_cases as gc
import graph_ops_reference as gr
from helpers import FLOOR_MULT, TOL, rel_err
from oracle import phoregen_oracle as po

F64_EQ = 1e-12         # two float64 evaluations of one formula (summation order, layer_norm's own variance pass)
REF_BOUND = TOL / FLOOR_MULT


class f64_default:
    """The oracle builds its constant tables at torch's default dtype: float64 for the duration."""

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *a):
        torch.set_default_dtype(self.old)


def _report(entry, case, err):
    print(f'graph_ops fp32-reference {entry:16s} {case:24s} {err:.3e}')
    assert err <= REF_BOUND, (entry, case, err)


def _oracle_lists(x, k, batch, n):
    """po.knn_graph as per-centre lists in edge order.  It takes the k + 1 nearest INCLUDING the centre and drops the centre: where
    k + 1 coincident points of lower index precede the centre it keeps k + 1 neighbours; the first k are the list either way."""
    src, dst = po.knn_graph(x, k, batch)
    lists = [[] for _ in range(n)]
    for s, d in zip(src.tolist(), dst.tolist()):
        lists[d].append(s)
    return lists


def _assert_lists_equal(nbr, deg, lists, k):
    for i, ref in enumerate(lists):
        d = int(deg[i])
        assert d <= len(ref) <= d + 1 and nbr[i, :d].tolist() == ref[:d] and (nbr[i, d:] == -1).all(), i
        assert len(ref) == d or d == k


# ---- zero-size batches: every graph-side wrapper returns before it launches ----
def test_zero_size_batches_return_before_any_launch():
    """A zeroed PgTopo (no graph, no node, every pointer NULL): the wrappers return PG_OK without touching the runtime -- on a machine
    without a GPU a launch of zero workgroups would come back as an error."""
    from phoregen_amd import hip
    lib = hip.load_library()
    t = C.byref(hip.PgTopo())
    assert lib.pg_knn_ctx(t, None, 32, None, None, None) == 0
    assert lib.pg_edge_gate(t, None, None, None, 32, None, None, None, None, None, C.c_float(0.0), None, None) == 0
    assert lib.pg_apply_dx(t, None, None, None, None, None) == 0
    assert lib.pg_lig_normals(t, None, None, None, None, None) == 0
    # their siblings already did
    assert lib.pg_lig_nn3(t, None, None, None) == 0 and lib.pg_bond_smear(t, None, None, None) == 0
    assert lib.pg_embed_ctx(t, *[None] * 12) == 0 and lib.pg_embed_bond(t, *[None] * 8) == 0
    assert lib.pg_knn_group_by_kind(t, 32, None, None, None, None) == 0
    # the argument checks still come first
    assert lib.pg_knn_ctx(t, None, 0, None, None, None) != 0 and b'[1, 64]' in lib.pg_last_error()


# ---- kNN ----
@pytest.mark.parametrize('coords', ['lattice', 'gauss'])
@pytest.mark.parametrize('k', gc.KNN_KS)
def test_knn_restatement_equals_oracle(k, coords):
    c = gc.knn_case(k, coords, 'cpu')
    nbr, deg = gr.knn_lists(c.x, gr.graph_ranges(c.topo.g_off), k)
    sizes = np.diff(c.topo.g_off)
    assert (deg == np.minimum(k, sizes - 1)[c.topo.ctx_graph]).all()
    _assert_lists_equal(nbr, deg, _oracle_lists(c.x.double(), k, torch.as_tensor(c.topo.ctx_graph), c.plan.n_ctx), k)
    if coords == 'lattice':
        # the lattice claim: fp32 sees the same d2, so the fp32 restatement gives the same lists, and ties are plenty
        nbr32, deg32 = gr.knn_lists(c.x, gr.graph_ranges(c.topo.g_off), k, torch.float32)
        assert (nbr32 == nbr).all() and (deg32 == deg).all()
        first, count = gr.graph_ranges(c.topo.g_off)[-2 if c.sizes[-1] == 3 else -1]
        d2 = gr.dist2(c.x, first, count).numpy()
        assert count == 512 and np.mean([np.unique(r).size for r in d2]) < 0.8 * count


# ---- direction vectors ----
def test_normals_restatement_equals_oracle():
    c = gc.normals_case('cpu')
    tp = c.topo
    lig_ranges = gr.ligand_ranges(tp.g_off, tp.g_nph, tp.g_nlig)
    nn3 = gr.lig_nn3(c.x, lig_ranges, tp.lig2ctx)
    mask = torch.as_tensor(tp.is_lig).bool()
    batch = torch.as_tensor(tp.ctx_graph)
    x64 = c.x.double()
    lists = _oracle_lists(x64[mask], 3, batch[mask], c.plan.n_lig)          # ligand-local ids
    l2c = tp.lig2ctx
    for a, ref in enumerate(lists):
        want = [int(l2c[j]) for j in ref] + [-1] * (3 - len(ref))
        assert nn3[a].tolist() == want, a
    assert (nn3[:1] == -1).all() and (nn3[1:3, 1:] == -1).all()              # the 1- and 2-atom ligands
    # pharmacophore nodes lie nearer than any atom and are never picked
    assert all(mask[j] for j in nn3.reshape(-1).tolist() if j >= 0)
    other = (batch[mask][:, None] == batch[mask][None, :]) & ~torch.eye(c.plan.n_lig, dtype=torch.bool)
    d_at = torch.cdist(x64[mask], x64[mask]) + 1e9 * (~other)
    d_ph = torch.cdist(x64[mask], x64[~mask])
    same = batch[mask][:, None] == batch[~mask][None, :]
    assert ((d_ph + 1e9 * (~same)).min(1).values < d_at.min(1).values).all() and float(d_at.min()) >= 1.0
    # the oracle's direction feature of a pair (pharmacophore node with a unit normal e_i, ligand atom a) is component i of a's vector
    pn = c.phore_norm.double().clone()
    pn[:3] = torch.eye(3, dtype=torch.float64)
    p2c = torch.as_tensor(tp.phore2ctx)
    nrm = gr.lig_normals(c.x, nn3, l2c, pn, tp.phore2ctx)
    lig_rows = torch.as_tensor(l2c)
    o = po.Oracle({}, dtype=torch.float64)
    comp = [o.direction_feat(x64, pn, p2c[i].expand(lig_rows.numel()), lig_rows, mask, batch)[:, 0] for i in range(3)]
    assert torch.equal(torch.stack(comp, 1), nrm[lig_rows])
    assert torch.equal(nrm[p2c], pn)
    assert torch.equal(nrm[l2c[0]], -x64[l2c[0]])                            # 1-atom ligand: mean of nothing is 0
    nrm32 = gr.lig_normals(c.x, nn3, l2c, c.phore_norm, tp.phore2ctx, torch.float32)
    _report('pg_lig_normals', 'lattice', rel_err(nrm32, gr.lig_normals(c.x, nn3, l2c, c.phore_norm, tp.phore2ctx)))


# ---- edge gate ----
@pytest.mark.parametrize('profile', ['default', 'gamma_signed', 'trained_like'])
@pytest.mark.parametrize('k', gc.GATE_KS)
def test_gate_restatement_equals_oracle(k, profile):
    c = gc.gate_case(k, 'cpu')
    sd = gc.gate_weights(profile)
    W = [sd['denoiser.edge_pred_layer.net.' + s] for s in ('0.weight', '0.bias', '1.weight', '1.bias', '3.weight', '3.bias')]
    nbr, deg = gr.knn_lists(c.x, gr.graph_ranges(c.topo.g_off), k)
    assert set(deg.tolist()) >= {d for d in (0, 1, 15, 16, 17, 31) if d <= k}
    ew = gr.edge_gate(c.x, nbr, deg, *W)
    valid = torch.as_tensor(np.arange(k)[None, :] < deg[:, None])
    dst, slot = valid.nonzero(as_tuple=True)
    src = torch.as_tensor(nbr)[dst, slot]
    x64 = c.x.double()
    dist = (x64[dst] - x64[src]).norm(dim=-1)
    assert (dist == 0).any() and (dist > 12).any() and (dist > 30).any()
    with f64_default():
        ref = torch.sigmoid(po.Oracle(sd, dtype=torch.float64).mlp('denoiser.edge_pred_layer', po.gaussian_smearing(dist))).reshape(-1)
    assert rel_err(ew[dst, slot], ref) <= F64_EQ
    assert (ew[~valid] == 0).all()
    _report('pg_edge_gate', f'{profile} k={k}', rel_err(gr.edge_gate(c.x, nbr, deg, *W, dtype=torch.float32), ew))


# ---- bond smearing, coordinate update ----
def test_geom_restatements_equal_oracle():
    for i, c in enumerate(gc.geom_cases('cpu')):
        tp = c.topo
        G = gr.bond_smear(c.x, tp.bond_src, tp.bond_dst)
        x64 = c.x.double()
        with f64_default():
            ref = po.gaussian_smearing((x64[tp.bond_dst] - x64[tp.bond_src]).pow(2).sum(-1).sqrt())       # Oracle.bond_update's distance
        assert G.shape == (c.plan.n_bond, 20) and (c.plan.n_bond == 0 or rel_err(G, ref) <= F64_EQ)
        mask = torch.as_tensor(tp.is_lig).double()
        xn = gr.apply_dx(c.x, c.dx1, c.dx2, tp.is_lig)
        assert torch.equal(xn, x64 + (c.dx1.double() + c.dx2.double()) * mask[:, None])                    # Oracle.attention_layer's last line
        if c.plan.n_bond:
            _report('pg_bond_smear', f'batch {i}', rel_err(gr.bond_smear(c.x, tp.bond_src, tp.bond_dst, torch.float32), G))
        _report('pg_apply_dx', f'batch {i}', rel_err(gr.apply_dx(c.x, c.dx1, c.dx2, tp.is_lig, torch.float32), xn))


def test_plan_bond_rows_are_the_callers_rows_through_edge_ref():
    """The topology the restatements are handed: internal bond row e is the caller's row edge_ref[e], its ends in context order."""
    for c in (gc.embed_case('cpu'), gc.guidance_case('cpu')):
        plan, tp = c.plan, c.topo
        ei = plan.edge_index.numpy()
        assert sorted(tp.edge_ref.tolist()) == list(range(plan.n_bond))
        assert (tp.bond_src == tp.lig2ctx[ei[0][tp.edge_ref]]).all() and (tp.bond_dst == tp.lig2ctx[ei[1][tp.edge_ref]]).all()
        assert (tp.bond_graph == plan.batch_edge.numpy()[tp.edge_ref]).all()
        assert not plan.edge_identity


# ---- embeddings ----
def test_embed_restatements_equal_oracle():
    c = gc.embed_case('cpu')
    tp, plan = c.topo, c.plan
    off, coeff = gr.time_tables()
    with f64_default():
        assert torch.equal(gr.time_smear(c.time_step, off, coeff), po.time_smearing(c.time_step.double()))
        o = po.Oracle({'node_embedder.weight': c.W_node, 'edge_embedder.weight': c.W_edge}, dtype=torch.float64)
        bn, bp = plan.batch_node, torch.as_tensor(tp.ctx_graph[tp.phore2ctx])
        h_node = torch.cat([o.lin('node_embedder', c.h_node.double()), po.time_smearing(c.time_step[bn].double())], -1)
        h_all, pos_all, _, mask_l, p_idx, l_idx = po.compose_context(c.h_phore_emb.double(), h_node, c.pos_phore.double(),
                                                                     c.pos.double(), bp, bn)
        h_bond = torch.cat([o.lin('edge_embedder', c.h_edge.double()), po.time_smearing(c.time_step[plan.batch_edge].double())], -1)
    assert torch.equal(l_idx, torch.as_tensor(tp.lig2ctx)) and torch.equal(p_idx, torch.as_tensor(tp.phore2ctx))
    args = (c.h_node, c.pos, c.time_step, tp.lig_graph, tp.lig2ctx, c.W_node, off, coeff, c.h_phore_emb, c.pos_phore, tp.phore2ctx)
    h_ctx, x_ctx = gr.embed_ctx(*args)
    assert rel_err(h_ctx, h_all) <= F64_EQ and torch.equal(x_ctx, pos_all)
    assert torch.equal(h_ctx[:, 118:][mask_l], h_node[:, 118:])              # columns 118..127: time_smearing of the row's graph
    hb = gr.embed_bond(c.h_edge, tp.edge_ref, c.time_step, tp.bond_graph, c.W_edge, off, coeff)
    assert rel_err(hb, h_bond[tp.edge_ref]) <= F64_EQ
    # pre-permuted rows without the indirection: the same rows
    assert torch.equal(gr.embed_bond(c.h_edge[tp.edge_ref], None, c.time_step, tp.bond_graph, c.W_edge, off, coeff), hb)
    # the clamp: 5000 embeds as 1000, -3 as 0
    ts = gr.time_smear(c.time_step, off, coeff)
    assert torch.equal(ts[5], ts[4]) and torch.equal(ts[6], ts[0])
    # fp32: the tables as the model holds them (fp32 linspace), the formula in fp32
    off32, coeff32 = gr.time_tables(dtype=torch.float32)
    h32, x32 = gr.embed_ctx(*args[:6], off32, coeff32, *args[8:], dtype=torch.float32)
    _report('pg_embed_ctx', 'h_ctx', rel_err(h32, h_ctx))
    _report('pg_embed_ctx', 'h_ctx time columns', rel_err(h32[:, 118:][mask_l], h_ctx[:, 118:][mask_l]))
    assert torch.equal(x32.double(), x_ctx)
    _report('pg_embed_bond', 'h_bond', rel_err(gr.embed_bond(c.h_edge, tp.edge_ref, c.time_step, tp.bond_graph, c.W_edge, off32, coeff32,
                                                             torch.float32), hb))


# ---- atom-count heads ----
def test_atom_count_restatement_equals_oracle_pooling():
    """Oracle.atom_count with heads that pass a logit through (ReLU(s) - ReLU(-s) = s exactly), so that only its pooling acts."""
    c = gc.count_case()
    cl, cu = gr.atom_count(c.s_all, c.s_l, c.is_ex, c.phore_graph, c.n_graphs)
    pm = torch.tensor([[1.0], [-1.0]])
    sd = {'atom_mlp.0.weight': pm * torch.tensor([[1.0, 0.0]]), 'atom_mlp_1.0.weight': pm * torch.tensor([[0.0, 1.0]]),
          'atom_mlp.2.weight': pm.T.clone(), 'atom_mlp_1.2.weight': pm.T.clone()}
    h_phore = torch.zeros(c.phore_graph.numel(), 13)
    h_phore[:, 12] = c.is_ex.float()
    ol, ou = po.Oracle(sd, dtype=torch.float64).atom_count(torch.stack([c.s_all, c.s_l], 1).double(), c.phore_graph, h_phore, c.n_graphs)
    assert rel_err(cl, ol.reshape(-1)) <= F64_EQ and rel_err(cu, ou.reshape(-1)) <= F64_EQ
    assert cl[0] == 0 and cu[0] == 0 and cl[1] == 0 and cu[1] > 0 and cl[6] == 0            # no node; EX nodes only
    assert float(c.s_all.max()) == 40 and float(c.s_l.min()) == -40
    cl32, cu32 = gr.atom_count(c.s_all, c.s_l, c.is_ex, c.phore_graph, c.n_graphs, torch.float32)
    _report('pg_atom_count', 'count_l', rel_err(cl32, cl))
    _report('pg_atom_count', 'count_u', rel_err(cu32, cu))


# ---- guidance ----
@pytest.mark.parametrize('mean_over', [0, 11])
@pytest.mark.parametrize('atom,center', gc.GUIDANCE_MODES)
def test_guidance_restatement_equals_oracle(atom, center, mean_over):
    c = gc.guidance_case('cpu')
    tp = c.topo
    B = mean_over or c.B
    assert mean_over == 0 or mean_over > c.B
    g = gr.guidance_grad(c.x, tp.lig_graph, c.h_edge, c.edge_index, c.batch_edge, B, c.B, atom, gc.MIN_D, gc.MAX_D, center,
                         c.phore_center)
    opts = [dict(type='atom_prox', min_d=gc.MIN_D, max_d=gc.MAX_D)] * atom + [dict(type='center_prox')] * center
    pc = torch.cat([c.phore_center.double(), torch.zeros(B - c.B, 3, dtype=torch.float64)])
    ref = po.guidance_grad(opts, c.x.double(), c.plan.batch_node, c.h_edge.double(), c.edge_index, c.batch_edge, B, pc)
    # (the oracle forms 1 / (cnt B) in fp32 whatever the dtype of x: equal to fp32 rounding of that one factor)
    assert rel_err(g, ref) <= (2.0 ** -23 if atom else F64_EQ)
    assert torch.isfinite(g).all()
    # the same rows in the internal bond order
    g_int = gr.guidance_grad(c.x, tp.lig_graph, c.h_edge[tp.edge_ref], c.edge_index[:, tp.edge_ref], c.batch_edge[tp.edge_ref], B, c.B,
                             atom, gc.MIN_D, gc.MAX_D, center, c.phore_center)
    assert rel_err(g_int, g) <= F64_EQ
    g32 = gr.guidance_grad(c.x, tp.lig_graph, c.h_edge, c.edge_index, c.batch_edge, B, c.B, atom, gc.MIN_D, gc.MAX_D, center,
                           c.phore_center, torch.float32)
    _report('pg_guidance_grad', f'atom={atom} center={center} B={B}', rel_err(g32, g))


def test_guidance_case_holds_what_it_claims():
    c = gc.guidance_case('cpu')
    am = gr.first_argmax(c.h_edge)
    assert torch.equal(torch.as_tensor(am), c.h_edge.argmax(-1))             # torch's argmax is the first maximum too
    be, ei, off = c.batch_edge.numpy(), c.edge_index.numpy(), c.off
    assert (am[be == 1] == 0).all() and c.na[0] == 1
    h = c.h_edge.numpy()
    tie = (h[:, 1:].max(1) == h[:, 0]) & (be == 3)
    assert tie.sum() >= 10 and (am[tie] == 0).all()
    rev = {(int(s), int(d)): int(a) for s, d, a in zip(ei[0], ei[1], am)}
    assert sum((rev[(d, s)] > 0) != (a > 0) for (s, d), a in rev.items()) >= 10        # the two directions of a pair disagree
    x = c.x.double()
    ln = (x[ei[0]] - x[ei[1]]).norm(dim=-1)
    bonded = torch.as_tensor(am > 0)
    assert ((ln == gc.MIN_D) & bonded).sum() >= 2 and ((ln == gc.MAX_D) & bonded).sum() >= 2
    assert float(ln.min()) >= 0.25
    assert ((ln < gc.MIN_D) & bonded).any() and ((ln > gc.MAX_D) & bonded).any()
