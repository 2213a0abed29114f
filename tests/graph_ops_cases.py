"""The ragged batches of the graph-side kernel tests, shared by the CPU part (tests/test_graph_ops_host.py: restatement against
oracle, fp32 restatement against float64) and the GPU part (tests/test_gpu_graph_ops.py: kernel against restatement).  Every batch
is a BatchPlan on the device asked for plus plain CPU tensors; all inputs are drawn from seeded generators."""
from types import SimpleNamespace

import numpy as np
import torch

KNN_KS = (1, 3, 32, 33, 64)
GATE_KS = (3, 16, 17, 32)
TIME_STEPS = (0, 1, 499, 999, 1000, 5000, -3)          # the last two beyond the clamp [0, 1000]
MIN_D, MAX_D = 1.25, 2.5                                # both are lengths of lattice vectors: (0.75, 1, 0), (1.5, 2, 0)


def make_plan(na, nph, device):
    from phoregen_amd.plan import BatchPlan, make_edge_data
    na, nph = torch.as_tensor(na), torch.as_tensor(nph)
    ei, be = make_edge_data(na)
    B = na.numel()
    plan = BatchPlan(torch.repeat_interleave(torch.arange(B), na), torch.repeat_interleave(torch.arange(B), nph), ei, be, B, device)
    return plan, ei, be


def topo_arrays(plan):
    """The plan's index arrays on the CPU (numpy int64): the topology the restatements are given."""
    c = lambda v: v.cpu().numpy().astype(np.int64)
    return SimpleNamespace(g_off=c(plan.g_ctx_off), g_nph=c(plan.g_nph), g_nlig=c(plan.g_nlig), lig2ctx=c(plan.lig2ctx),
                           phore2ctx=c(plan.phore2ctx), bond_src=c(plan.bond_src), bond_dst=c(plan.bond_dst),
                           bond_graph=c(plan.bond_graph), lig_graph=c(plan.lig_graph), edge_ref=c(plan.edge_ref),
                           is_lig=c(plan.ctx_is_lig), ctx_graph=c(plan.ctx_graph))


def lattice(shape, g, lo=-32, hi=32):
    """Multiples of 0.25 in [lo / 4, hi / 4]: differences, squares and three-term sums of squares are exact in fp32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float() * 0.25


def distinct_lattice(n, g, lo, hi, step=1):
    """n DISTINCT lattice points with coordinates step * [lo, hi] quarter units."""
    side = hi - lo + 1
    assert side ** 3 >= n
    flat = torch.randperm(side ** 3, generator=g)[:n]
    p = torch.stack([flat // (side * side), (flat // side) % side, flat % side], 1) + lo
    return p.float() * (0.25 * step)


# ---- pg_knn_ctx ----
def knn_sizes(k):
    sizes = [1, 2, k, k + 1, 63, 64, 65, 128, 129, 511, 512]
    if sum(sizes) % 4 == 0:
        sizes.append(3)                                 # n_ctx not a multiple of the 4 nodes of a workgroup
    return sizes


def knn_case(k, coords, device, seed=0):
    """Graphs of knn_sizes(k) context nodes (at most 24 of them ligand atoms).  coords = 'lattice': graph 3 and 6 wholly coincident,
    every third graph on a 5 x 5 x 5 sub-lattice (repeated points), every third on [-3, 3]^3 (most distances tied), the rest on all of
    [-8, 8]^3; 'gauss': 3 N(0, 1)."""
    g = torch.Generator().manual_seed(1000 * seed + k)
    sizes = knn_sizes(k)
    na = [min(s, 1 + (7 * i) % 24) for i, s in enumerate(sizes)]
    nph = [s - a for s, a in zip(sizes, na)]
    plan, _, _ = make_plan(na, nph, device)
    assert plan.n_ctx % 4 != 0
    xs = []
    for i, s in enumerate(sizes):
        if coords == 'gauss':
            xs.append(3.0 * torch.randn(s, 3, generator=g))
        elif i in (3, 6):
            xs.append(lattice((1, 3), g).expand(s, 3).clone())
        elif i % 3 == 0:
            xs.append(lattice((s, 3), g, -2, 2))
        elif i % 3 == 1:
            xs.append(lattice((s, 3), g, -12, 12))
        else:
            xs.append(lattice((s, 3), g))
    return SimpleNamespace(plan=plan, topo=topo_arrays(plan), x=torch.cat(xs), k=k, sizes=sizes)


# ---- pg_lig_nn3 / pg_lig_normals ----
def normals_case(device, seed=0):
    """Ligands of 1, 2, 3, 4, 64, 65 and 128 atoms on distinct points of the integer lattice (nearest other atom >= 1 away, many ties);
    every atom has a pharmacophore node ON it or 0.25 beside it -- nearer than any atom, and never to be picked."""
    g = torch.Generator().manual_seed(77 + seed)
    na, nph = [1, 2, 3, 4, 64, 65, 128], [3, 5, 4, 9, 70, 65, 128]
    plan, _, _ = make_plan(na, nph, device)
    tp = topo_arrays(plan)
    x = torch.zeros(plan.n_ctx, 3)
    for gi, (a, p) in enumerate(zip(na, nph)):
        atoms = distinct_lattice(a, g, -3, 3, step=4)
        first = int(tp.g_off[gi])
        host = atoms[torch.cat([torch.arange(a), torch.randint(0, a, (p - a,), generator=g)])]      # every atom hosts a node
        shift = torch.zeros(p, 3)
        shift[torch.arange(p), torch.randint(0, 3, (p,), generator=g)] = 0.25
        shift[::2] = 0.0                                # every other node exactly on its atom
        x[first:first + p] = host + shift
        x[first + p:first + p + a] = atoms
    phore_norm = lattice((plan.n_phore, 3), g, -8, 8)
    return SimpleNamespace(plan=plan, topo=tp, x=x, phore_norm=phore_norm, na=na, nph=nph)


# ---- pg_edge_gate ----
def gate_weights(profile):
    """The six tensors of denoiser.edge_pred_layer as the deterministic generator of phoregen_amd.weights draws them."""
    from phoregen_amd.weights import make_tensor
    p = 'denoiser.edge_pred_layer.net.'
    shapes = {'0.weight': (128, 20), '0.bias': (128,), '1.weight': (128,), '1.bias': (128,), '3.weight': (1, 128), '3.bias': (1,)}
    return {p + s: make_tensor(p + s, shape, 0, profile=profile) for s, shape in shapes.items()}


def gate_case(k, device, seed=0):
    """Graphs of 1, 2, 16, 17, 18, 32 and 45 nodes: deg = min(k, count - 1) takes 0, 1, 15, 16, 17, 31 where k allows.  Coordinates
    1.5 N(0, 1); in every graph from 16 nodes up, node 1 coincides with node 0 (d = 0) and the last three nodes sit 14 .. 60 away
    (12 < d: the Gaussians fade, from ~25 on all twenty underflow)."""
    g = torch.Generator().manual_seed(500 + 10 * seed + k)
    sizes = [1, 2, 16, 17, 18, 32, 45]
    na = [1, 1, 6, 9, 4, 20, 15]
    plan, _, _ = make_plan(na, [s - a for s, a in zip(sizes, na)], device)
    xs = []
    for s in sizes:
        xg = 1.5 * torch.randn(s, 3, generator=g)
        if s >= 16:
            xg[1] = xg[0]
            xg[-3:] = xg[-3:] + torch.tensor([[14.0, 0, 0], [0, -27.0, 0], [20.0, 30.0, 45.0]])
        xs.append(xg)
    return SimpleNamespace(plan=plan, topo=topo_arrays(plan), x=torch.cat(xs), k=k, sizes=sizes)


# ---- pg_bond_smear / pg_apply_dx ----
def geom_cases(device):
    """Ragged ligands (1 and 2 atoms included) and a batch without a single bond row."""
    out = []
    for i, (na, nph) in enumerate((([5, 1, 2, 40, 17], [7, 3, 11, 1, 30]), ([1, 1, 1], [4, 2, 9]))):
        g = torch.Generator().manual_seed(31 + i)
        plan, _, _ = make_plan(na, nph, device)
        n = plan.n_ctx
        out.append(SimpleNamespace(plan=plan, topo=topo_arrays(plan), x=3.0 * torch.randn(n, 3, generator=g),
                                   dx1=0.1 * torch.randn(n, 3, generator=g), dx2=0.1 * torch.randn(n, 3, generator=g)))
    assert out[1].plan.n_bond == 0
    return out


# ---- pg_embed_ctx / pg_embed_bond ----
def embed_case(device, seed=0):
    """One graph per entry of TIME_STEPS; h_node / h_edge rows alternately one-hot and soft (softmax of N(0, 1) scores)."""
    g = torch.Generator().manual_seed(900 + seed)
    na, nph = [4, 1, 7, 2, 12, 3, 9], [3, 6, 1, 8, 2, 5, 4]
    plan, ei, be = make_plan(na, nph, device)

    def rows(n, K):
        soft = torch.softmax(torch.randn(n, K, generator=g), -1)
        hot = torch.nn.functional.one_hot(torch.randint(0, K, (n,), generator=g), K).float()
        return torch.where((torch.arange(n) % 2 == 0)[:, None], hot, soft)
    from phoregen_amd.weights import make_tensor
    return SimpleNamespace(plan=plan, topo=topo_arrays(plan), time_step=torch.tensor(TIME_STEPS, dtype=torch.int64),
                           h_node=rows(plan.n_lig, 12), h_edge=rows(plan.n_bond, 6), pos=torch.randn(plan.n_lig, 3, generator=g),
                           h_phore_emb=torch.randn(plan.n_phore, 128, generator=g), pos_phore=torch.randn(plan.n_phore, 3, generator=g),
                           W_node=make_tensor('node_embedder.weight', (118, 12), 0), W_edge=make_tensor('edge_embedder.weight', (118, 6), 0))


# ---- pg_atom_count ----
def count_case(seed=0):
    """Graph 0: no pharmacophore node; 1: EX nodes only; 2, 3, 4, 5: 1, 64, 65 and 300 nodes, EX and other kinds mixed; 6: no node
    again (the last graph).  Logits N(0, 3) with +-40 planted."""
    g = torch.Generator().manual_seed(40 + seed)
    sizes = [0, 6, 1, 64, 65, 300, 0]
    pg = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    P = pg.numel()
    is_ex = (torch.rand(P, generator=g) < 0.4)
    is_ex[pg == 1] = True
    is_ex[pg == 2] = False
    s_all, s_l = 3.0 * torch.randn(P, generator=g), 3.0 * torch.randn(P, generator=g)
    for s in (s_all, s_l):
        s[torch.randperm(P, generator=g)[:12]] = torch.tensor([40.0, -40.0]).repeat(6)
    return SimpleNamespace(s_all=s_all, s_l=s_l, is_ex=is_ex.to(torch.uint8), phore_graph=pg, n_graphs=len(sizes))


# ---- pg_guidance_grad ----
def guidance_case(device, seed=0):
    """Ligand atoms on DISTINCT lattice points (every pair >= 0.25 apart; a fp32 bond length equals a threshold only where the exact
    one does).  Graph 0: one atom.  Graph 1: every bond row class 0.  Graph 2: atoms 0, 1, 2 placed so that |01| = MIN_D and
    |02| = MAX_D exactly, both pairs bonded in both directions.  Graph 3: rows where class 0 ties the maximum (no bond), and pairs
    whose two directions disagree.  Graphs 4, 5: soft rows.  Pharmacophore centres off the lattice, >= 1 from every mean."""
    g = torch.Generator().manual_seed(1234 + seed)
    na, nph = [1, 6, 8, 9, 20, 33], [2, 1, 3, 1, 4, 2]
    plan, ei, be = make_plan(na, nph, device)
    B, E = len(na), plan.n_bond
    off = np.concatenate([[0], np.cumsum(na)])
    x = torch.cat([distinct_lattice(a, g, -10, 10) for a in na])
    x[off[2] + 0] = torch.tensor([0.0, 0.0, 0.0])
    x[off[2] + 1] = torch.tensor([0.75, 1.0, 0.0])
    x[off[2] + 2] = torch.tensor([-1.5, 0.0, 2.0])
    x[off[2] + 3:off[3]] = distinct_lattice(na[2] - 3, g, 12, 20)          # the rest of graph 2 away from the three placed atoms
    h = torch.softmax(1.5 * torch.randn(E, 6, generator=g), -1)
    eg = be.numpy()
    h[eg == 1] = torch.nn.functional.one_hot(torch.zeros(int((eg == 1).sum()), dtype=torch.long), 6).float()
    src, dst = ei[0].numpy(), ei[1].numpy()
    for e in np.nonzero(eg == 2)[0]:
        if {int(src[e]) - off[2], int(dst[e]) - off[2]} in ({0, 1}, {0, 2}):
            h[e] = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0])
    rows3 = np.nonzero(eg == 3)[0]
    for j, e in enumerate(rows3):
        if j % 3 == 0:                                  # class 0 ties the maximum: the first maximum wins, no bond
            h[e] = torch.tensor([0.4, 0.1, 0.0, 0.4, 0.1, 0.0])
        elif src[e] < dst[e]:                           # a -> b bonded ...
            h[e] = torch.tensor([0.1, 0.2, 0.7, 0.0, 0.0, 0.0])
        else:                                           # ... b -> a mostly not
            h[e] = torch.tensor([0.6, 0.2, 0.2, 0.0, 0.0, 0.0]) if j % 2 else torch.tensor([0.0, 0.0, 0.0, 0.0, 0.5, 0.5])
    mean = torch.stack([x[off[i]:off[i + 1]].mean(0) for i in range(B)])
    u = torch.randn(B, 3, generator=g)
    pc = mean + u / u.norm(dim=-1, keepdim=True) * (1.0 + 2.0 * torch.rand(B, 1, generator=g))
    return SimpleNamespace(plan=plan, topo=topo_arrays(plan), x=x, h_edge=h, edge_index=ei, batch_edge=be, phore_center=pc,
                           B=B, na=na, off=off)


GUIDANCE_MODES = ((1, 0), (0, 1), (1, 1))              # (atom_prox, center_prox)
