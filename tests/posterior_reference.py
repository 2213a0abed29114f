"""numpy restatements of the transition-step kernels (phoregen_amd/csrc/posterior.hip), one output element at a time.

TEST INFRASTRUCTURE: no torch, nothing of the product.  Every function takes `dtype`: np.float64 is the reference the kernels are
held against, np.float32 evaluates the very same formula in the kernels' own precision, which measures what fp32 rounding of the
formula costs on an input (tests/test_posterior_host.py).  The fp32 tables and inputs the kernels read are widened, never rebuilt:
the float64 result is the exact answer to the question the kernel is asked.

The noise is predicted, not modelled: oracle/philox_ref.py reproduces the device generator bit for bit, and the functions below
enumerate the counters exactly as the kernels do, so the uniform behind every output element is known as a float32."""
import numpy as np

from oracle import philox_ref as pr

LOG_FLOOR = -32.0
TWO_PI_F32 = np.float32(6.283185307179586)        # the kernels' constant: 2 pi rounded to fp32


# ---- Philox counters ----
def _uniform4(seed, ctr, step, stream_id):
    """The four float32 uniforms of each 64-bit counter: counter words (ctr lo, ctr hi, step, stream_id), key = the two seed words."""
    ctr = np.asarray(ctr, dtype=np.uint64).reshape(-1)
    c = np.empty((ctr.size, 4), dtype=np.uint32)
    c[:, 0] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c[:, 1] = (ctr >> np.uint64(32)).astype(np.uint32)
    c[:, 2] = np.broadcast_to(np.asarray(step, dtype=np.int64), ctr.shape).astype(np.uint32)
    c[:, 3] = np.uint32(stream_id)
    key = np.empty((ctr.size, 2), dtype=np.uint32)
    key[:, 0], key[:, 1] = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    return pr.uniform24(pr.philox4x32(c, key))


def _counter_base(n_rows, row_graph, graph_row0, graph_key):
    """(high counter bits, row index the counter counts from) of every row.  Flat form: 0 and the row itself; graph forms: the graph's
    key (its number when no key table is given) in the upper word, the row's index inside its graph below."""
    rows = np.arange(n_rows, dtype=np.int64)
    if graph_row0 is None:
        return np.zeros(n_rows, dtype=np.uint64), rows
    gr = np.asarray(row_graph, dtype=np.int64)
    key = np.asarray(graph_key, dtype=np.int64)[gr] if graph_key is not None else gr
    hi = (key & 0xFFFFFFFF).astype(np.uint64) << np.uint64(32)
    return hi, rows - np.asarray(graph_row0, dtype=np.int64)[gr]


def uniforms(n_rows, K, seed, stream_id, step, row_graph=None, graph_row0=None, graph_key=None):
    """[n_rows, K] float32: the uniform of element (row, k).  Element e = local_row * K + k reads word e & 3 of counter e >> 2.
    `step` is one number or one per row (the fragment draw counts the level of each row's graph)."""
    hi, local = _counter_base(n_rows, row_graph, graph_row0, graph_key)
    e = (local[:, None] * K + np.arange(K)[None, :]).astype(np.uint64)
    ctr = hi[:, None] | (e >> np.uint64(2))
    step = np.broadcast_to(np.asarray(step, dtype=np.int64).reshape(-1, 1), e.shape)
    u4 = _uniform4(seed, ctr, step.reshape(-1), stream_id)
    return u4[np.arange(e.size), (e & np.uint64(3)).astype(np.int64).reshape(-1)].reshape(n_rows, K)


def position_uniforms(n_rows, seed, stream_id, step, row_graph=None, graph_row0=None, graph_key=None):
    """([n_rows, 3], [n_rows, 3]) float32 u1 in (0, 1], u2 in [0, 1) of every coordinate: one counter per coordinate -- its flat
    index, or (key << 32) | its index inside the graph -- words 0 and 1."""
    hi, local = _counter_base(n_rows, row_graph, graph_row0, graph_key)
    idx = (local[:, None] * 3 + np.arange(3)[None, :]).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    step = np.broadcast_to(np.asarray(step, dtype=np.int64).reshape(-1, 1), idx.shape)
    u4 = _uniform4(seed, hi[:, None] | idx, step.reshape(-1), stream_id)
    u1 = np.float32(1.0) - u4[:, 0]                               # exact: both are multiples of 2^-24
    return u1.reshape(n_rows, 3), u4[:, 1].reshape(n_rows, 3)


def box_muller(u1, u2, dtype=np.float64):
    u1, u2 = np.asarray(u1).astype(dtype), np.asarray(u2).astype(dtype)
    return np.sqrt(dtype(-2.0) * np.log(u1)) * np.cos(dtype(TWO_PI_F32) * u2)


# ---- categorical posterior ----
def _floored_log(f, dtype):
    return np.maximum(np.log(f + dtype(1e-30)), dtype(LOG_FLOOR))


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    d = x - x.max(-1, keepdims=True)
    with np.errstate(under='ignore'):
        return d - np.log(np.exp(d).sum(-1, keepdims=True))


def categorical_log_posterior(logits, log_vt, t, row_graph, q_mats, q_onestep_T, dtype=np.float64):
    """[n, K] log q(v_{t-1} | v_t, v0 ~ softmax(logits)): log(vt Q_t^T) + log(v0 Qbar_{t-1}), each floored at -32, normalised.  Rows of
    a graph at t = 0 return log_softmax(logits); the cumulative table is read at max(t - 1, 0)."""
    lv0 = log_softmax(logits, dtype)
    tb = np.asarray(t, dtype=np.int64)[np.asarray(row_graph, dtype=np.int64)]
    tm1 = np.maximum(tb - 1, 0)
    with np.errstate(under='ignore'):
        pv0, pvt = np.exp(lv0), np.exp(np.asarray(log_vt).astype(dtype))
        f1 = np.einsum('bj,bjk->bk', pvt, np.asarray(q_onestep_T)[tb].astype(dtype))
        f2 = np.einsum('bj,bjk->bk', pv0, np.asarray(q_mats)[tm1].astype(dtype))
        out = _floored_log(f1, dtype) + _floored_log(f2, dtype)
        om = out.max(-1, keepdims=True)
        out = out - (om + np.log(np.exp(out - om).sum(-1, keepdims=True)))
    return np.where((tb == 0)[:, None], lv0, out)


def gumbel_noise(u, dtype=np.float64):
    u = np.asarray(u).astype(dtype)
    return -np.log(-np.log(u + dtype(1e-30)) + dtype(1e-30))


def gumbel_scores(log_post, u, dtype=np.float64):
    """(scores [n, K], class [n], margin [n]): Gumbel noise + log-distribution, the argmax with the FIRST maximum winning, and the
    distance of the best score from the second best."""
    v = gumbel_noise(u, dtype) + np.asarray(log_post).astype(dtype)
    cls = np.argmax(v, -1)                                        # numpy: the first occurrence of the maximum
    top2 = np.sort(v, -1)[:, -2:]
    return v, cls, (top2[:, 1] - top2[:, 0]).astype(np.float64)


# ---- Gaussian position posterior ----
def position_posterior(x_t, x0, t, row_graph, coef_x0, coef_xt, std, grad=None, eps=None, u=None, lig2ctx=None, x_ctx_next=None,
                       center=None, dtype=np.float64):
    """mu = coef_x0[t] x0 + coef_xt[t] x_t - grad, plus std[t] e unless the graph is at t = 0; e is `eps`, or Box-Muller of `u` =
    (u1, u2).  With `lig2ctx`, x0 is a context-ordered buffer read through the row map, `x_ctx_next` (a context-ordered buffer, copied)
    receives the new positions in the ligand slots, and x0_out is the gathered x0.  traj = x_prev + center[graph].
    Returns dict(x_prev, x0_out, x_ctx_next, traj, mu)."""
    gr = np.asarray(row_graph, dtype=np.int64)
    tb = np.asarray(t, dtype=np.int64)[gr]
    x0 = np.asarray(x0)
    x0v = x0[np.asarray(lig2ctx, dtype=np.int64)] if lig2ctx is not None else x0
    col = lambda tab: np.asarray(tab)[tb].astype(dtype)[:, None]
    mu = col(coef_x0) * x0v.astype(dtype) + col(coef_xt) * np.asarray(x_t).astype(dtype)
    if grad is not None:
        mu = mu - np.asarray(grad).astype(dtype)
    e = np.asarray(eps).astype(dtype) if eps is not None else box_muller(u[0], u[1], dtype)
    x_prev = np.where((tb == 0)[:, None], mu, mu + col(std) * e)
    out = dict(x_prev=x_prev, x0_out=x0v.copy(), mu=mu, x_ctx_next=None)
    if x_ctx_next is not None:
        nxt = np.asarray(x_ctx_next).astype(dtype).copy()
        nxt[np.asarray(lig2ctx, dtype=np.int64)] = x_prev
        out['x_ctx_next'] = nxt
    out['traj'] = x_prev + (np.asarray(center).astype(dtype)[gr] if center is not None else dtype(0.0))
    return out


# ---- fragment replacement of a fixed row ----
def fragment_row(v0, lvl, K=None, q_mats=None, u=None, x0f=None, sqrt_ab=None, sqrt_1mab=None, e=None, dtype=np.float64):
    """A fixed row (class v0, fragment coordinate x0f) redrawn at level lvl = t - 1 of its graph, one entry per row.
    Types (when K is given): the draw over max(log(q_mats[lvl][v0, :] + 1e-30), -32) with the uniforms `u` of the fragment stream
    (counter step = lvl); lvl = -1: logs 0 / -32, the class itself.  Coordinates (when x0f is given): sqrt_ab[lvl] x0f +
    sqrt_1mab[lvl] e; lvl = -1: x0f exactly.  Returns dict(log, cls, margin, scores, x) with the parts asked for."""
    v0, lvl = np.asarray(v0, dtype=np.int64), np.asarray(lvl, dtype=np.int64)
    at = np.maximum(lvl, 0)
    out = {}
    if K is not None:
        lg = _floored_log(np.asarray(q_mats)[at, v0].astype(dtype), dtype)
        v, cls, margin = gumbel_scores(lg, u, dtype)
        own = np.where(np.arange(K)[None, :] == v0[:, None], dtype(0.0), dtype(LOG_FLOOR))
        frag = (lvl < 0)
        out.update(log=np.where(frag[:, None], own, lg), cls=np.where(frag, v0, cls), margin=np.where(frag, np.inf, margin),
                   scores=np.where(frag[:, None], own, v))
    if x0f is not None:
        x0f = np.asarray(x0f)
        x = np.asarray(sqrt_ab)[at].astype(dtype)[:, None] * x0f.astype(dtype) + \
            np.asarray(sqrt_1mab)[at].astype(dtype)[:, None] * np.asarray(e).astype(dtype)
        out['x'] = np.where((lvl < 0)[:, None], x0f.astype(dtype), x)
    return out
