"""Plain restatements of the graph-side kernels (csrc/graph_ops.hip, the guidance kernels of csrc/posterior.hip) for the tests:
one loop or tensor expression per formula of the kernels' header comments, in torch at a dtype the caller chooses -- float64 is the
reference the kernels are held against, float32 measures what the bound asks of ANY fp32 evaluation (tests/test_graph_ops_host.py).
Nothing of phoregen_amd is called here: the topology (row maps, bond lists) comes in as plain index arrays.  No device code.

Index conventions (phoregen_amd/plan.py): context rows of a graph are [pharmacophore nodes..., ligand atoms...]; `g_off` [B + 1] are
the graphs' first context rows; a neighbour list holds context row ids, ascending distance, -1 past the degree."""
import numpy as np
import torch

SMEAR_OFFSETS = (0, 1, 1.25, 1.5, 1.75, 2, 2.25, 2.5, 2.75, 3, 3.5, 4, 4.5, 5, 5.5, 6, 7, 8, 9, 10)


# ---- exact in-graph kNN: ascending d2, ties by ascending index, self excluded, deg = min(k, count - 1) ----
def dist2(x, first, count, dtype=torch.float64):
    """[count, count] squared distances of the rows first .. first + count, (dx^2 + dy^2) + dz^2 in `dtype`."""
    xg = torch.as_tensor(x)[first:first + count].to(dtype)
    d = xg[:, None, :] - xg[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_lists(x, ranges, k, dtype=torch.float64):
    """ranges: (first, count) candidate ranges, one per graph.  -> nbr [n_rows, k] (global row ids, -1 past deg), deg [n_rows];
    rows outside every range keep nbr = -1, deg = 0."""
    n = int(torch.as_tensor(x).shape[0])
    nbr, deg = np.full((n, k), -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for first, count in ranges:
        if count == 0:
            continue
        d2 = dist2(x, first, count, dtype).numpy()
        idx = np.broadcast_to(np.arange(count), (count, count))
        order = np.lexsort((idx, d2), axis=-1)                  # primary key d2, then the candidate's index
        dg = min(k, count - 1)
        for i in range(count):
            row = order[i][order[i] != i][:dg]                  # self excluded
            nbr[first + i, :dg] = first + row
            deg[first + i] = dg
    return nbr, deg


def graph_ranges(g_off):
    g_off = np.asarray(g_off, dtype=np.int64)
    return [(int(a), int(b - a)) for a, b in zip(g_off[:-1], g_off[1:])]


def ligand_ranges(g_off, g_nph, g_nlig):
    return [(int(o + p), int(n)) for o, p, n in zip(np.asarray(g_off)[:-1], np.asarray(g_nph), np.asarray(g_nlig))]


# ---- direction vectors: ligand rows mean(x of the 3 nearest ligand atoms) - x (mean of nothing = 0), pharmacophore rows as given ----
def lig_nn3(x, lig_ranges, lig2ctx, dtype=torch.float64):
    """[n_lig, 3] context rows of the (up to) 3 nearest ligand atoms of the same graph, -1 beyond the count."""
    nbr, _ = knn_lists(x, lig_ranges, 3, dtype)
    return nbr[np.asarray(lig2ctx, dtype=np.int64)]


def lig_normals(x, nn3, lig2ctx, phore_norm, phore2ctx, dtype=torch.float64):
    x = torch.as_tensor(x).to(dtype)
    nrm = torch.zeros_like(x)
    nrm[torch.as_tensor(phore2ctx, dtype=torch.long)] = torch.as_tensor(phore_norm).to(dtype)
    for a, ctx in enumerate(np.asarray(lig2ctx).tolist()):
        src = [j for j in nn3[a].tolist() if j >= 0]
        s = torch.zeros(3, dtype=dtype)
        for j in src:
            s = s + x[j]
        nrm[ctx] = s / max(len(src), 1) - x[ctx]
    return nrm


# ---- Gaussian smearing of a distance: exp(-(d - offset_i)^2 / 2), 20 fixed offsets ----
def smear(d):
    off = torch.tensor(SMEAR_OFFSETS, dtype=d.dtype)
    t = d.reshape(-1, 1) - off.reshape(1, -1)
    return torch.exp(-0.5 * t * t)


# ---- global edge gate: e_w = sigmoid(W2 . ReLU(LN(W1 . smear(d) + b1)) + b2) per neighbour slot below deg, 0 from deg to k ----
def edge_gate(x, nbr, deg, W1, b1, gamma, beta, W2, b2, dtype=torch.float64):
    """nbr [n, k], deg [n]; the six tensors of the MLP as the state dict holds them ([128, 20], [128], [128], [128], [1, 128], [1])."""
    x = torch.as_tensor(x).to(dtype)
    W1, b1, gamma, beta, W2, b2 = (torch.as_tensor(w).to(dtype) for w in (W1, b1, gamma, beta, W2, b2))
    n, k = nbr.shape
    ew = torch.zeros(n, k, dtype=dtype)
    for i in range(n):
        dg = int(deg[i])
        if dg == 0:
            continue
        r = x[i][None, :] - x[torch.as_tensor(nbr[i, :dg], dtype=torch.long)]
        d = torch.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        h = smear(d) @ W1.T + b1
        mu = h.mean(-1, keepdim=True)
        var = ((h - mu) ** 2).mean(-1, keepdim=True)
        h = (h - mu) / torch.sqrt(var + 1e-5) * gamma + beta
        o = torch.relu(h) @ W2.T + b2
        ew[i, :dg] = (1.0 / (1.0 + torch.exp(-o))).reshape(-1)
    return ew


# ---- bond-length smearing and coordinate update ----
def bond_smear(x, bond_src, bond_dst, dtype=torch.float64):
    x = torch.as_tensor(x).to(dtype)
    r = x[torch.as_tensor(bond_dst, dtype=torch.long)] - x[torch.as_tensor(bond_src, dtype=torch.long)]
    return smear(torch.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]))


def apply_dx(x, dx1, dx2, is_lig, dtype=torch.float64):
    """x' = x + (dx1 + dx2) on ligand rows, x elsewhere."""
    x, dx1, dx2 = (torch.as_tensor(v).to(dtype) for v in (x, dx1, dx2))
    return x + (dx1 + dx2) * torch.as_tensor(is_lig).to(dtype).reshape(-1, 1)


# ---- embeddings: 118 linear columns (no bias) | 10 time Gaussians exp(coeff_i (clamp(t, 0, T) - offset_i)^2) ----
def time_tables(num_timesteps=1000, num_gaussians=10, dtype=torch.float64):
    """offset = linspace(0, T, 10); coeff = -0.5 / spacing^2 (the first spacing repeated for offset 0)."""
    off = torch.linspace(0.0, float(num_timesteps), num_gaussians, dtype=dtype)
    diff = off[1:] - off[:-1]
    diff = torch.cat([diff[:1], diff])
    return off, -0.5 / diff ** 2


def time_smear(t, off, coeff, num_timesteps=1000):
    t = torch.as_tensor(t).to(off.dtype).clamp(0.0, float(num_timesteps))
    d = t.reshape(-1, 1) - off.reshape(1, -1)
    return torch.exp(coeff.reshape(1, -1) * (d * d))


def embed_rows(h, W, t_rows, off, coeff, dtype=torch.float64):
    """[rows, 128] = [h @ W^T | time_smear(t of the row's graph)]; h [rows, F], W [118, F]."""
    h, W = torch.as_tensor(h).to(dtype), torch.as_tensor(W).to(dtype)
    return torch.cat([h @ W.T, time_smear(t_rows, off.to(dtype), coeff.to(dtype))], -1)


def embed_ctx(h_node, pos, t_graph, lig_graph, lig2ctx, W_node, off, coeff, h_phore_emb, pos_phore, phore2ctx,
              dtype=torch.float64):
    """-> h_ctx [n_ctx, 128], x_ctx [n_ctx, 3]: ligand rows embedded, pharmacophore rows copied, both in context order."""
    l2c, p2c = torch.as_tensor(lig2ctx, dtype=torch.long), torch.as_tensor(phore2ctx, dtype=torch.long)
    n = l2c.numel() + p2c.numel()
    h_ctx, x_ctx = torch.zeros(n, 128, dtype=dtype), torch.zeros(n, 3, dtype=dtype)
    t_rows = torch.as_tensor(t_graph)[torch.as_tensor(lig_graph, dtype=torch.long)]
    h_ctx[l2c] = embed_rows(h_node, W_node, t_rows, off, coeff, dtype)
    h_ctx[p2c] = torch.as_tensor(h_phore_emb).to(dtype)
    x_ctx[l2c] = torch.as_tensor(pos).to(dtype)
    x_ctx[p2c] = torch.as_tensor(pos_phore).to(dtype)
    return h_ctx, x_ctx


def embed_bond(h_edge, edge_ref, t_graph, bond_graph, W_edge, off, coeff, dtype=torch.float64):
    """Internal bond row e reads the caller's row edge_ref[e] (None: its own row)."""
    h_edge = torch.as_tensor(h_edge)
    if edge_ref is not None:
        h_edge = h_edge[torch.as_tensor(edge_ref, dtype=torch.long)]
    t_rows = torch.as_tensor(t_graph)[torch.as_tensor(bond_graph, dtype=torch.long)]
    return embed_rows(h_edge, W_edge, t_rows, off, coeff, dtype)


# ---- atom-count heads: per-graph means of sigmoid(s_all) over all nodes and sigmoid(s_l) over the non-EX nodes (mean of nothing
#      = 0); count_l = mean_l, count_u = mean_l + ReLU(mean_all - mean_l) ----
def atom_count(s_all, s_l, is_ex, phore_graph, n_graphs, dtype=torch.float64):
    s_all, s_l = torch.as_tensor(s_all).to(dtype), torch.as_tensor(s_l).to(dtype)
    cl, cu = torch.zeros(n_graphs, dtype=dtype), torch.zeros(n_graphs, dtype=dtype)
    pg, ex = np.asarray(phore_graph), np.asarray(is_ex).astype(bool)
    for g in range(n_graphs):
        rows = np.nonzero(pg == g)[0]
        free = rows[~ex[rows]]
        a = (1.0 / (1.0 + torch.exp(-s_all[rows]))).sum() / max(rows.size, 1)
        l = (1.0 / (1.0 + torch.exp(-s_l[free]))).sum() / max(free.size, 1)
        cl[g], cu[g] = l, l + torch.relu(a - l)
    return cl, cu


# ---- guidance: closed-form gradient of
#      atom_prox    E = (1 / B) sum_g mean_{bond rows e of g whose first maximum is a class > 0} [ReLU(d_e - max_d) + ReLU(min_d - d_e)]
#      center_prox  E = (1 / B) sum_g || mean(x_g) - c_g ||
#      (strict comparisons: no force at d == min_d or d == max_d; a graph without such a row contributes nothing) ----
def first_argmax(h):
    h = np.asarray(h, dtype=np.float64)
    out = np.zeros(h.shape[0], dtype=np.int64)
    for e in range(h.shape[0]):
        for c in range(1, h.shape[1]):
            if h[e, c] > h[e, out[e]]:
                out[e] = c
    return out


def guidance_grad(x, lig_graph, h_edge, edge_index, batch_edge, B, n_graphs, use_atom, min_d, max_d, use_center, phore_center,
                  dtype=torch.float64):
    """x [n_lig, 3] ligand order; h_edge [E, 6] / edge_index [2, E] / batch_edge [E] rows in one common order; B = the divisor
    (graphs of the logical batch), n_graphs = graphs present."""
    x = torch.as_tensor(x).to(dtype)
    lg = np.asarray(lig_graph, dtype=np.int64)
    grad = torch.zeros_like(x)
    if use_atom:
        sel = first_argmax(h_edge) > 0
        be = np.asarray(batch_edge, dtype=np.int64)
        cnt = np.bincount(be[sel], minlength=n_graphs)
        ei = np.asarray(edge_index, dtype=np.int64)
        for e in np.nonzero(sel)[0]:
            s, d = int(ei[0, e]), int(ei[1, e])
            r = x[s] - x[d]
            ln = torch.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
            sign = float(ln > max_d) - float(ln < min_d)
            g = (sign / (float(cnt[be[e]]) * B)) * r / ln
            grad[s] += g
            grad[d] -= g
    if use_center:
        pc = torch.as_tensor(phore_center).to(dtype)
        for g in range(n_graphs):
            rows = torch.as_tensor(np.nonzero(lg == g)[0], dtype=torch.long)
            if rows.numel() == 0:
                continue
            dv = x[rows].sum(0) / rows.numel() - pc[g]
            grad[rows] += dv / torch.sqrt((dv * dv).sum()) / (rows.numel() * B)
    return grad
