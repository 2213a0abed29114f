"""Inputs of the transition-step kernel tests, shared by the CPU part (tests/test_posterior_host.py) and the GPU part
(tests/test_gpu_posterior.py).  Everything is seeded numpy / torch-CPU data; no model, no device.  The transition tables are the
oracle's for the default config at T = 1000, in fp32 as the kernels read them.

Also the tolerances of both parts.  They are absolute (log values reach -64) and are FLOOR_MULT x what the fp32 evaluation of the
float64 restatement itself loses on these very inputs, rounded up to one digit; tests/test_posterior_host.py measures that loss
and asserts it is at most tolerance / FLOOR_MULT, profiles/posterior_parity.md records it.  None of them comes from a kernel."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import posterior_reference as pref
from helpers import DIFF_CFG, FLOOR_MULT
from oracle import phoregen_oracle as po

T = DIFF_CFG['num_timesteps']

# ---- tolerances, one per kind of output ----
TOL_LOG = 5e-5           # log posterior, fragment log-distribution.  The floor (1.5e-5) is set by `peaked` at t = 0, where the output is
#                          log_softmax of logits 40 x randn: values down to -400, one fp32 ulp there is 3.1e-5.  Benign inputs: 1.7e-6
TOL_POS_EPS = 4e-6       # position, eps supplied (|x| up to ~15, one fp32 ulp is 9.5e-7; floor 1.0e-6)
TOL_POS_DEVICE = 4e-6    # position, device Box-Muller draw (adds the fp32 rounding of the angle 2 pi u2, times the radius; floor 1.0e-6)
TOL_FRAG_POS = 3e-6      # fragment coordinates sqrt_ab x0f + sqrt_1mab e, device draw (floor 9.0e-7)
GUMBEL_FLOOR = 5e-7      # fp32 evaluation of -log(-log(u + 1e-30) + 1e-30) over the uniforms of the cases (values in [-4.3, 16.7])
TIE_BAND = TOL_LOG + FLOOR_MULT * GUMBEL_FLOOR      # a top-two score margin below this does not pin the sampled class
TIE_SHARE_CAP = 0.01     # at most this share of a case's rows may lie inside the band (every case but `ties`)

# ---- batches ----
BATCHES = {
    # blocks of 256 rows (categorical) end inside graphs 5 and 6; blocks of 256 coordinates (position) end inside rows 85, 170, ...
    'batch': ((1, 2, 85, 86, 3, 170, 260), (0, 1, 2, 500, 998, 999, 0)),
    'single_row': ((1,), (1,)),
    'single_graph': ((256,), (500,)),
}
KEYS = (5, 2 ** 31 - 1, 0, 77, 3, 1234567, 42)      # graph keys: not monotone, both ends of the int32 range a key may take
FORMS = ('flat', 'indexed', 'keyed')
PROFILES = ('benign', 'peaked', 'ties')
SEED = (0x5DEECE66 << 32) | 0x9E3779B1              # above 2^32: both key words of the generator matter
NODE_RNG = dict(stream_id=0, step=999)              # (stream, step) pairs: two values of each across the tests
EDGE_RNG = dict(stream_id=1, step=3)
POS_RNG = (dict(stream_id=2, step=999), dict(stream_id=1, step=3))
FRAG_STREAMS = {12: 3, 6: 4, 'pos': 5}
N_PHORE = 9                                          # pharmacophore rows per graph in the context layout
ALONE = 5                                            # the graph of `batch` that is also run alone


@functools.lru_cache(None)
def tables():
    """fp32 numpy tables: node / edge (q_mats, q_onestep_T), pos (coef_x0, coef_xt, std), frag (sqrt_ab, sqrt_1mab)."""
    n = lambda v: v.numpy().copy()
    out = {}
    for K, c in ((12, DIFF_CFG['diff_atom']), (6, DIFF_CFG['diff_bond'])):
        tb = po.categorical_tables(po.beta_schedule(T, c), K, c['init_prob'])
        out[K] = (n(tb['q_mats']), n(tb['transpopse_q_onestep_mats']))
    ct = po.continuous_tables(po.beta_schedule(T, DIFF_CFG['diff_pos']))
    out['pos'] = (n(ct['coef_x0']), n(ct['coef_xt']), n(ct['std']))
    ab = n(ct['alphas_bar']).astype(np.float64)      # the forward-process scales, from the fp32 alphas_bar the model stores
    out['frag'] = (np.sqrt(ab).astype(np.float32), np.sqrt(1.0 - ab).astype(np.float32))
    return out


def torch_tables(K):
    """The oracle's table dict of a categorical transition in float64 (for po.q_v_posterior)."""
    qm, qt = tables()[K]
    return dict(q_mats=torch.from_numpy(qm).double(), transpopse_q_onestep_mats=torch.from_numpy(qt).double())


@functools.lru_cache(None)
def layout(batch='batch'):
    sizes, time = BATCHES[batch]
    sizes = np.asarray(sizes, dtype=np.int64)
    row0 = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return SimpleNamespace(name=batch, sizes=sizes, n=int(sizes.sum()), n_graphs=sizes.size,
                           row_graph=np.repeat(np.arange(sizes.size), sizes).astype(np.int32),
                           time=np.asarray(time, dtype=np.int64), row0=row0.astype(np.int32),
                           keys=np.asarray(KEYS[:sizes.size], dtype=np.int32))


def counter_args(lay, form):
    """(graph_row0, graph_key) of a counter form."""
    return {'flat': (None, None), 'indexed': (lay.row0, None), 'keyed': (lay.row0, lay.keys)}[form]


def graph_alone(lay, g):
    """Graph g of a batch as a batch of its own: same rows, same time step, same key."""
    lo, n = int(lay.row0[g]), int(lay.sizes[g])
    return slice(lo, lo + n), SimpleNamespace(name=f'{lay.name}[{g}]', sizes=lay.sizes[g:g + 1], n=n, n_graphs=1,
                                              row_graph=np.zeros(n, dtype=np.int32), time=lay.time[g:g + 1].copy(),
                                              row0=np.zeros(1, dtype=np.int32), keys=lay.keys[g:g + 1].copy())


def _gen(*salt):
    return torch.Generator().manual_seed(1_000_003 * sum((i + 1) * int(s) for i, s in enumerate(salt)) + 17)


def _f32(tensor):
    return tensor.numpy().astype(np.float32).copy()


# ---- categorical inputs ----
def tied_pair(K, row):
    """(a, b, c, d): the two classes a < b that a pair row ties, and the classes its one-hot log_vt (c) and logits (d) sit on.  All four
    are generic classes -- same prior mass: neither the mask class 11 of the atom types nor the absorbing class 0 of the bond types."""
    return ((1, 3, 2, 4), (2, 4, 1, 3))[row % 2]


@functools.lru_cache(None)
def cat_case(K, profile, batch='batch'):
    """logits, log_vt, uniform [n, K] float32.  `ties` additionally: all_equal (rows at t = 0 whose logits are all equal and whose
    supplied uniforms are all equal), pair (rows where classes a < b of pair_ab have bit-equal logits, log_vt and uniforms and lead
    the row) -- see _plant_ties."""
    lay = layout(batch)
    g = _gen(K, PROFILES.index(profile), lay.n)
    n = lay.n
    if profile == 'peaked':
        logits = 40.0 * torch.randn(n, K, generator=g)           # softmax underflows: the -32 floor of log(v0 Qbar) is reached
        hot = torch.randint(0, K, (n,), generator=g)
        log_vt = torch.full((n, K), pref.LOG_FLOOR)               # 0 / -32 one-hot: what the fragment replacement writes
        log_vt[torch.arange(n), hot] = 0.0
    else:
        logits = 2.0 * torch.randn(n, K, generator=g)
        log_vt = torch.log_softmax(3.0 * torch.randn(n, K, generator=g), -1)
    c = SimpleNamespace(K=K, profile=profile, lay=lay, logits=_f32(logits), log_vt=_f32(log_vt),
                        uniform=_f32(torch.rand(n, K, generator=g)), all_equal=np.zeros(0, np.int64), pair=np.zeros(0, np.int64))
    if profile == 'ties':
        _plant_ties(c, g)
    return c


def _plant_ties(c, g):
    """all_equal: every second row of the t = 0 graphs -- one logit value and one uniform value per row: every score is the same
    number, class 0 must win.
    pair at t = 0: the two classes share the row's largest logit and one uniform.
    pair at t > 0 (every fifth row): the scores must tie in the KERNEL's arithmetic, whatever order it sums in.  log_vt is one-hot on
    class c and the logits on class d, with -200 elsewhere, so exp() of every other entry is 0 in fp32 and both products have one
    term: out[k] = log(Q_t^T[c, k]) + log(Qbar_{t-1}[d, k]), and the tables hold one bit pattern at k = a and k = b (asserted).  The
    pair gets the largest uniform, every other class u = 0: the pair leads by several units (asserted on the host), although c and d
    carry nearly all of the posterior at small t."""
    lay, K = c.lay, c.K
    qm, qt = tables()[K]
    tb = lay.time[lay.row_graph]
    local = np.arange(lay.n) - lay.row0[lay.row_graph]
    zero = np.nonzero(tb == 0)[0]
    c.all_equal = zero[local[zero] % 2 == 0]
    pair0 = zero[local[zero] % 2 == 1][::3]
    pair1 = np.nonzero((tb > 0) & (local % 5 == 0))[0]
    c.pair = np.concatenate([pair0, pair1])
    c.pair_ab = np.array([tied_pair(K, int(r))[:2] for r in c.pair])
    vals = _f32(2.0 * torch.randn(lay.n, generator=g))
    us = _f32(torch.rand(lay.n, generator=g))
    for r in c.all_equal:
        c.logits[r], c.uniform[r] = vals[r], us[r]
    for r in pair0:
        a, b = tied_pair(K, int(r))[:2]
        c.logits[r, [a, b]] = c.logits[r].max() + np.float32(1.0)
        c.uniform[r] = us[r]
    for r in pair1:
        a, b, hv, h0 = tied_pair(K, int(r))
        t = int(tb[r])
        assert qt[t][hv, a] == qt[t][hv, b] and qm[max(t - 1, 0)][h0, a] == qm[max(t - 1, 0)][h0, b], (K, t)
        c.logits[r], c.log_vt[r] = -200.0, -200.0
        c.logits[r, h0], c.log_vt[r, hv] = 0.0, 0.0
        c.uniform[r] = 0.0
        c.uniform[r, [a, b]] = np.float32(1.0 - 2.0 ** -24)


# ---- position inputs ----
@functools.lru_cache(None)
def pos_case(batch='batch'):
    """x_t, x0, grad, eps [n, 3], center [graphs, 3]; the context layout: lig2ctx [n] (ligand row -> context row, N_PHORE pharmacophore
    rows per graph, ligand rows scattered among them in no order), n_ctx, x0_ctx [n_ctx, 3] holding x0 in the ligand slots and a
    sentinel pattern elsewhere, next_fill [n_ctx, 3] the pattern a separate next-step buffer starts from."""
    lay = layout(batch)
    g = _gen(3, lay.n)
    n = lay.n
    r = lambda *s: torch.randn(*s, generator=g)
    c = SimpleNamespace(lay=lay, x_t=_f32(3.0 * r(n, 3)), x0=_f32(3.0 * r(n, 3)), grad=_f32(0.1 * r(n, 3)), eps=_f32(r(n, 3)),
                        center=_f32(5.0 * r(lay.n_graphs, 3)))
    l2c, off = [], 0
    for s in lay.sizes.tolist():
        l2c.append(off + torch.randperm(s + N_PHORE, generator=g)[:s].numpy())
        off += s + N_PHORE
    c.lig2ctx, c.n_ctx = np.concatenate(l2c).astype(np.int32), off
    if lay.sizes.max() > 2:
        assert any((np.diff(v) < 0).any() for v in l2c)
    c.x0_ctx = _f32(100.0 + r(off, 3))
    c.x0_ctx[c.lig2ctx] = c.x0
    c.next_fill = _f32(-100.0 + r(off, 3))
    c.is_lig = np.zeros(off, dtype=bool)
    c.is_lig[c.lig2ctx] = True
    return c


# ---- fragment inputs ----
@functools.lru_cache(None)
def frag_case(mask, batch='batch'):
    """cls12 / cls6 [n] int32 (-1 = free, else the fixed class for K = 12 / 6), x0f [n, 3].  mask: 'none' (all free), 'third' (about a
    third of the rows of every graph with more than one row), 'whole' (every row of graph ALONE)."""
    lay = layout(batch)
    g = _gen(7, ('none', 'third', 'whole').index(mask), lay.n)
    local = np.arange(lay.n) - lay.row0[lay.row_graph]
    if mask == 'none':
        fixed = np.zeros(lay.n, dtype=bool)
    elif mask == 'third':
        fixed = (local % 3 == 1) & (lay.sizes[lay.row_graph] > 1)
    else:
        fixed = lay.row_graph == ALONE
    out = SimpleNamespace(mask=mask, fixed=fixed, x0f=_f32(3.0 * torch.randn(lay.n, 3, generator=g)))
    for K in (12, 6):
        cls = torch.randint(0, K, (lay.n,), generator=g).numpy()
        setattr(out, f'cls{K}', np.where(fixed, cls, -1).astype(np.int32))
    return out
