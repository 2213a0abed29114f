"""Inputs of the segment-attention tests (tests/test_seg_attn_host.py on the CPU, tests/test_gpu_seg_attn.py on the GPU).

Topologies come from BatchPlan + make_edge_data on lists of (ligand atoms, pharmacophore nodes) -- the only supported source of a
PgTopo, the triplet queue and tri_split.  Everything else is seeded random data, not model activations: first-layer rows with a
non-zero row mean (the contract does not need centring), b' of both signs, queries scaled so that the logits of a segment spread over
several units, neighbour lists of distinct same-graph nodes with a prescribed degree per node, gates in (0, 1), and positions with
near-coincident and collinear atoms (theta near 0 and pi, distances near 0).

Tolerances (TOL) are per output kind and relative to the per-element scale of tests/seg_attn_reference.py.  Each is MARGIN x the
distance of the float32 restatement from float64 over all cases, rounded up to one digit; tests/test_seg_attn_host.py measures that
distance and asserts it is at most TOL / MARGIN, profiles/seg_attn_parity.md records it.  None of them comes from a kernel."""
import functools
from types import SimpleNamespace as NS

import torch

import seg_attn_reference as sr
from helpers import FLOOR_MULT

NOMINAL_CU = 256
GUARD = 8                      # NaN rows behind every output
DEGS = (0, 1, 15, 16, 17, 31, 32)
DEGS48 = (0, 1, 16, 32, 33, 47, 48)

MARGIN = FLOOR_MULT
# relative to the reference's per-element scale; FLOOR_MULT x the float32 restatement's distance (measured: profiles/seg_attn_parity.md)
TOL = dict(U=6e-7, S=5e-5, swn=7e-6, out=8e-7, dx=1e-7, tri_out=2e-6, alpha=5e-5, logit=5e-7, v=6e-7)


# ---- topologies ------------------------------------------------------------------------------------------------------------------
def make_plan(sizes, device='cpu'):
    from phoregen_amd.plan import BatchPlan, make_edge_data
    nl = torch.tensor([a for a, _ in sizes])
    nph = torch.tensor([p for _, p in sizes])
    B = len(sizes)
    bn, bp = torch.repeat_interleave(torch.arange(B), nl), torch.repeat_interleave(torch.arange(B), nph)
    ei, be = make_edge_data(nl)
    return BatchPlan(bn, bp, ei, be, B, device)


def topo_of(plan, device=None):
    """The plan's index tensors as long tensors for the reference."""
    names = ('g_ctx_off', 'g_nph', 'g_nlig', 'g_eid_off', 'eid', 'ctx_graph', 'ctx_is_lig', 'bond_src', 'bond_dst', 'lig2ctx', 'phore2ctx')
    return NS(**{k: getattr(plan, k).to(device or plan.device).long() for k in names}, n_ctx=plan.n_ctx, n_bond=plan.n_bond)


KNN_SIZES = ((40, 3), (4, 36), (30, 8), (1, 2), (6, 2))
KNN48_SIZES = ((40, 12), (3, 2))
BOND_SIZES = dict(t2=((1, 2), (2, 1), (3, 2), (16, 1), (17, 2), (32, 2), (4, 1)), t3=((33, 2), (48, 1), (5, 2)), t4=((49, 1), (64, 2), (4, 2)),
                  t5=((65, 2), (78, 1), (3, 1)), generic=((81, 2), (5, 1)))
TRI_SIZES = dict(t3=((2, 1), (3, 2), (4, 1), (17, 2), (18, 1), (19, 1), (34, 2), (50, 1)), t4=((50, 1), (51, 2), (52, 1), (66, 1), (4, 2)),
                 t5=((81, 1), (3, 2)), generic=((82, 1), (3, 1)), small=((2, 1), (3, 2), (4, 1), (17, 2), (18, 1)))
PHORE_SIZES = ((3, 1), (2, 2), (1, 16), (2, 17), (4, 33))


def knn_big_sizes(cu):
    """More targets than 12 x cu (a second round of the persistent fused kernel), in graphs of 2 - 4 nodes."""
    n, sizes = 0, []
    while n <= 12 * cu + 40:
        s = ((1, 1), (2, 1), (2, 2))[len(sizes) % 3]
        sizes.append(s)
        n += s[0] + s[1]
    return tuple(sizes)


# ---- random inputs ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _positions(t, g):
    """Positions a few units apart; in every ligand of at least 4 atoms atom 1 sits 1e-3 from atom 0 and atom 3 on the line through
    atoms 0 and 2 (angles of 0 and pi, distances near 0)."""
    x = torch.randn(t.n_ctx, 3, generator=g) * 1.8
    for gi in range(t.g_nlig.numel()):
        n, l0 = int(t.g_nlig[gi]), int(t.g_ctx_off[gi] + t.g_nph[gi])
        if n >= 4:
            x[l0 + 1] = x[l0] + torch.tensor([1e-3, -5e-4, 2e-4])
            x[l0 + 3] = 2 * x[l0 + 2] - x[l0]
    return x


def _rows(n, g, mean=0.0):
    """[n, 128] first-layer rows; mean > 0: every row gets its own non-zero mean."""
    return torch.randn(n, 128, generator=g) * 0.8 + mean * torch.randn(n, 1, generator=g)


def _grid(v, steps):
    return torch.round(v * steps) / steps


def _common(c, g, n_q, pos):
    c.bk, c.bv = torch.randn(128, generator=g) * 0.5, torch.randn(128, generator=g) * 0.5
    # q on a grid of 1/16 and W2k on one of 1/32: every product and every 8-term sum of the query fold is an fp32 number, so the
    # forms that take U and the forms that fold q themselves have ONE reference (the fold's own rounding: fold_case below)
    c.q = _grid(torch.randn(n_q, 128, generator=g) * 0.5, 16)
    c.W2k = _grid(torch.randn(128, 128, generator=g) * (1.0 / 8 ** 0.5), 32)
    c.W2v = torch.randn(128, 128, generator=g) * (1.0 / 128 ** 0.5)
    c.b2v = torch.randn(128, generator=g) * 0.3
    c.W2xv = torch.randn(16, 128, generator=g) * (1.0 / 128 ** 0.5) if pos else None
    c.b2xv = torch.randn(16, generator=g) * 0.3 if pos else None
    c.efeat = c.efeat_off = None


@functools.lru_cache(maxsize=None)
def knn_case(name, sizes, k, degs, kinds='mixed', grouped=False, mean=0.3, seed=1):
    """The tensors of a knn sub-layer (node update and position update share them).  kinds: which nodes a neighbour list may hold."""
    plan = make_plan(sizes)
    t = topo_of(plan)
    g = _gen(seed)
    c = NS(name=name, sizes=sizes, knn_k=k, x=_positions(t, g), nrm=torch.randn(t.n_ctx, 3, generator=g) * 0.7)
    nbr, deg = torch.zeros(t.n_ctx, k, dtype=torch.int32), torch.zeros(t.n_ctx, dtype=torch.int32)
    for v in range(t.n_ctx):
        gi = int(t.ctx_graph[v])
        lo, hi = int(t.g_ctx_off[gi]), int(t.g_ctx_off[gi + 1])
        cand = [u for u in range(lo, hi) if u != v and (kinds == 'mixed' or bool(t.ctx_is_lig[u]) == (kinds == 'lig'))]
        if not cand:
            nbr[v] = lo                                     # unread slots still hold a node of the graph
            continue
        perm = [cand[i] for i in torch.randperm(len(cand), generator=g).tolist()]
        deg[v] = min(degs[v % len(degs)], len(perm))
        head = perm[:int(deg[v])]
        if grouped:                                         # the order pg_knn_group_by_kind leaves: ligand sources first, stable
            head = [u for u in head if t.ctx_is_lig[u]] + [u for u in head if not t.ctx_is_lig[u]]
        fill = (head + perm[int(deg[v]):] + perm * (k // len(perm) + 1))[:k]
        nbr[v] = torch.tensor(fill, dtype=torch.int32)
    c.nbr, c.deg = nbr, deg
    c.ew = torch.rand(t.n_ctx, k, generator=g) * 0.9 + 0.05
    c.Csrc_k, c.Csrc_v, c.Cdst_k, c.Cdst_v = _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean)
    c.Wf = [(torch.randn(128, 48, generator=g) * 0.3, torch.randn(128, 48, generator=g) * 0.3) for _ in range(2)]   # two target lists
    c.dx0 = torch.randn(t.n_ctx, 3, generator=g)
    _common(c, g, t.n_ctx, True)
    # target lists: a strict subset in shuffled order, cut into two lists three ways
    perm = torch.randperm(t.n_ctx, generator=g)
    ids = perm[:max(t.n_ctx - 3, 1)]
    c.ids = ids
    few = min(5, ids.numel() // 2)
    c.splits = dict(one_many=(ids[:1], ids[1:]), many_one=(ids[:-1], ids[-1:]), few_few=(ids[:few], ids[few:2 * few]))
    return c


@functools.lru_cache(maxsize=None)
def bond_case(name, mean=0.3, seed=2):
    plan = make_plan(BOND_SIZES[name])
    t = topo_of(plan)
    g = _gen(seed)
    c = NS(name=name, sizes=BOND_SIZES[name], knn_k=0, x=_positions(t, g), nrm=None, nbr=None, deg=None, ew=None)
    c.Csrc_k, c.Csrc_v = _rows(max(t.n_bond, 1), g, mean), _rows(max(t.n_bond, 1), g, mean)
    c.Cdst_k, c.Cdst_v = _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean)
    c.dx0 = torch.randn(t.n_ctx, 3, generator=g)
    _common(c, g, t.n_ctx, True)
    lig = t.lig2ctx[torch.randperm(t.lig2ctx.numel(), generator=g)]
    c.ids = lig[:-1]                                       # a strict subset of the ligand atoms, shuffled
    return c


@functools.lru_cache(maxsize=None)
def tri_case(name, mean=0.3, seed=3, sizes=None):
    """sizes: the batch of a case that is not one of TRI_SIZES (tests/seg_attn_grad_cases.py)."""
    sizes = sizes or TRI_SIZES[name]
    plan = make_plan(sizes)
    t = topo_of(plan)
    g = _gen(seed)
    nb = t.n_bond
    c = NS(name=name, sizes=sizes, x=_positions(t, g))
    c.Csrc = torch.cat([_rows(nb, g, mean), _rows(nb, g, mean)], 1)            # one [n_bond, 256] tensor: P_k | P_v
    c.Csrc_k, c.Csrc_v = c.Csrc[:, :128], c.Csrc[:, 128:]
    d = (c.x[t.bond_dst] - c.x[t.bond_src]).norm(dim=-1)
    # G and Wg2 on a grid of 1/64: smear(d_ji) . Wg2 is then exact in fp32 in any order, so the staged form (the product given as
    # rows of Cdst) and the generic form (which multiplies itself) have ONE reference
    c.G = _grid(torch.exp(-0.5 * (d[:, None] - torch.tensor(sr.SMEAR_OFF)) ** 2), 64)
    c.Wg2_k, c.Wg2_v = _grid(torch.randn(20, 128, generator=g) * 0.3, 64), _grid(torch.randn(20, 128, generator=g) * 0.3, 64)
    c.Cdst_k, c.Cdst_v = (c.G.double() @ c.Wg2_k.double()).float(), (c.G.double() @ c.Wg2_v.double()).float()
    assert bool((c.Cdst_k.double() == c.G.double() @ c.Wg2_k.double()).all())
    c.Wf_k, c.Wf_v = torch.randn(128, 12, generator=g) * 0.3, torch.randn(128, 12, generator=g) * 0.3
    c.resid = torch.randn(nb, 128, generator=g)
    _common(c, g, nb, False)
    return c


@functools.lru_cache(maxsize=None)
def phore_case(explicit, mean=0.3, seed=4):
    plan = make_plan(PHORE_SIZES)
    t = topo_of(plan)
    g = _gen(seed)
    c = NS(name='phore' + ('_efeat' if explicit else ''), sizes=PHORE_SIZES, knn_k=0, x=_positions(t, g), nrm=None, nbr=None, deg=None, ew=None)
    c.Csrc_k, c.Csrc_v, c.Cdst_k, c.Cdst_v = _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean), _rows(t.n_ctx, g, mean)
    c.Wf_k, c.Wf_v = torch.randn(128, 4, generator=g) * 0.3, torch.randn(128, 4, generator=g) * 0.3
    _common(c, g, t.n_ctx, False)
    if explicit:
        off = torch.zeros(t.g_nph.numel() + 1, dtype=torch.long)
        off[1:] = (t.g_nph * t.g_nph).cumsum(0)
        c.efeat_off = off[:-1].to(torch.int32)
        c.efeat = torch.rand(int(off[-1]), generator=g) * 6.0
    ph = t.phore2ctx[torch.randperm(t.phore2ctx.numel(), generator=g)]
    c.ids = ph[:-2]
    return c


def knn_cases(cu=NOMINAL_CU):
    """(case, forms it is run in): every case is a distinct (topology, neighbour lists) pair."""
    return [knn_case('mixed', KNN_SIZES, 32, DEGS), knn_case('grouped', KNN_SIZES, 32, DEGS, grouped=True, seed=5),
            knn_case('all_lig', KNN_SIZES, 32, DEGS, kinds='lig', seed=6), knn_case('all_phore', KNN_SIZES, 32, DEGS, kinds='phore', seed=7),
            knn_case('centred', KNN_SIZES, 32, DEGS, mean=0.0, seed=8),
            knn_case('rounds2', knn_big_sizes(cu), 32, (1, 2, 3), seed=9), knn_case('k48', KNN48_SIZES, 48, DEGS48, seed=10)]


@functools.lru_cache(maxsize=None)
def fold_case(n, seed=11):
    """pg_attn_fold_query / pg_attn_unfold_value on their own: unrestricted values."""
    g = _gen(seed + n)
    return NS(n=n, q=torch.randn(n + 3, 128, generator=g) * 0.5, W2k=torch.randn(128, 128, generator=g) * (1.0 / 8 ** 0.5),
              W2v=torch.randn(128, 128, generator=g) * (1.0 / 128 ** 0.5), b2v=torch.randn(128, generator=g) * 0.3,
              S=torch.randn(n + 3, 128, 16, generator=g), swn=torch.rand(n + 3, 16, generator=g),
              ids=torch.randperm(n + 3, generator=g)[:n].to(torch.int32))


FOLD_NS = (1, 3, 4, 5, 61)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, scale, mask=None):
    """Largest |got - ref| / scale over the elements (of `mask`); an element of scale 0 must be met exactly."""
    err = (got.double() - ref.double()).abs()
    r = torch.where(err > 0, err / scale.double().clamp_min(1e-300), torch.zeros_like(err))
    if mask is not None:
        r = r[mask]
    return float(r.max()) if r.numel() else 0.0


NODE_KINDS = (('U', 'U', 'U_scale'), ('S', 'S', 'S_scale'), ('swn', 'swn', 'swn'), ('out', 'out', 'out_scale'), ('alpha', 'aw', 'aw'))
POS_KINDS = (('dx', 'dx', 'dx_scale'), ('logit', 'logit', 'logit_scale'), ('v', 'v', 'v_scale'))
TRI_KINDS = (('U', 'U', 'U_scale'), ('S', 'S', 'S_scale'), ('swn', 'swn', 'swn'), ('tri_out', 'out', 'out_scale'), ('alpha', 'aw', 'aw'))


def ratios(a, b, kinds):
    """{kind: largest |a - b| / scale} of two results of the reference (b: float64, owner of the scales)."""
    out = {}
    for kind, field, scale in kinds:
        mask = b.valid[..., None].expand_as(b.logit) if kind in ('logit', 'v') else None
        out[kind] = ratio(getattr(a, field), getattr(b, field), getattr(b, scale), mask)
    return out
