"""The transition-step entry points of the C ABI (include/phoregen_hip.h: pg_posterior_*, pg_fragment_noise, pg_guidance_grad) as keyword
calls: the one place in the package that spells their argument order.  Each function takes tensors (None for an operand left out: the
library says which ones it needs), scalars and the stream, picks the entry point from what it is given and raises through `hip.check`.
No state, no allocation."""
from . import hip
from .hip import ptr as _p


def categorical(*, logits, log_vt_in, row_graph, time_step, q_mats, q_onestep_T, n_rows, K, seed, stream_id, step, graph_row0, graph_key,
                log_vt_out, onehot_out, stream, uniform=None, traj_out=None, frag_cls=None, frag_stream_id=0, what='posterior(categorical)'):
    """pg_posterior_categorical: one Gumbel-argmax draw from the categorical posterior per row.
    frag_cls [n_rows] int32 (-1 = free row) given: pg_posterior_categorical_frag, whose fixed rows are redrawn on Philox stream
    `frag_stream_id`.  `uniform` replays given draws; `time_step` is the [B] int64 step counter the rows' graphs index."""
    lib = hip.load_library()
    args = (_p(logits), _p(log_vt_in), _p(row_graph), _p(time_step), _p(q_mats), _p(q_onestep_T), n_rows, K, _p(uniform), seed, stream_id,
            step, _p(graph_row0), _p(graph_key), _p(log_vt_out), _p(onehot_out), _p(traj_out))
    if frag_cls is None:
        hip.check(lib.pg_posterior_categorical(*args, stream), what)
    else:
        hip.check(lib.pg_posterior_categorical_frag(*args, _p(frag_cls), frag_stream_id, stream), what)


def position(*, x_t, x0, row_graph, time_step, coef_x0, coef_xt, std, n_rows, seed, stream_id, step, graph_row0, graph_key, x_prev, stream,
             energy_grad=None, eps=None, center=None, traj_out=None, lig2ctx=None, x_ctx_next=None, x0_out=None,
             frag_cls=None, x0f=None, sqrt_ab=None, sqrt_1mab=None, frag_stream_id=0, what='posterior(pos)'):
    """pg_posterior_position: one draw from the Gaussian posterior per row (x_prev may be x_t: in place).
    Any of lig2ctx / x_ctx_next / x0_out given: the _ctx form -- x0 is then the denoiser's ctx-ordered buffer, read through lig2ctx; the
    new position also goes to x_ctx_next[lig2ctx[row]] and x0 in ligand rows to x0_out.
    Any of frag_cls / x0f / sqrt_ab / sqrt_1mab given: the _frag form (the library refuses an incomplete set), fixed rows redrawn on
    Philox stream `frag_stream_id`.  `eps` replays given normal draws; `center` [B,3] is added to traj_out only."""
    ctx = not (lig2ctx is None and x_ctx_next is None and x0_out is None)
    frag = not (frag_cls is None and x0f is None and sqrt_ab is None and sqrt_1mab is None)
    args = (_p(x_t), _p(x0)) + ((_p(lig2ctx),) if ctx else ()) + (
        _p(row_graph), _p(time_step), _p(coef_x0), _p(coef_xt), _p(std), _p(energy_grad), _p(eps), seed, stream_id, step, n_rows,
        _p(graph_row0), _p(graph_key), _p(center), _p(x_prev), _p(traj_out))
    if ctx:
        args += (_p(x_ctx_next), _p(x0_out))
    if frag:
        args += (_p(frag_cls), _p(x0f), _p(sqrt_ab), _p(sqrt_1mab), frag_stream_id)
    fn = getattr(hip.load_library(), 'pg_posterior_position' + ('_ctx' if ctx else '') + ('_frag' if frag else ''))
    hip.check(fn(*args, stream), what)


def fragment_noise(*, level, seed, n_lig, n_bond, node_cls, edge_cls, x0f, lig_graph, bond_graph, g_lig_off, g_bond_off, graph_key,
                   q_node, q_edge, sqrt_ab, sqrt_1mab, node_stream_id, edge_stream_id, pos_stream_id, stream,
                   h_node=None, log_node=None, h_edge=None, log_edge=None, x_out=None, what='fragment noise'):
    """pg_fragment_noise: the forward-process draw at `level` (-1: the fragment itself) on every fixed node and bond row; free rows and
    outputs left None are not written."""
    hip.check(hip.load_library().pg_fragment_noise(
        level, seed, n_lig, n_bond, _p(node_cls), _p(edge_cls), _p(x0f), _p(lig_graph), _p(bond_graph), _p(g_lig_off), _p(g_bond_off),
        _p(graph_key), _p(q_node), _p(q_edge), _p(sqrt_ab), _p(sqrt_1mab), node_stream_id, edge_stream_id, pos_stream_id,
        _p(h_node), _p(log_node), _p(h_edge), _p(log_edge), _p(x_out), stream), what)


def guidance_grad(*, topo, x_lig, h_edge_prev, lig_graph, g_lig_off, atom_prox, min_d, max_d, center_prox, phore_center, mean_over_graphs,
                  cnt_ws, mean_ws, grad, stream, what='guidance'):
    """pg_guidance_grad: the closed-form gradient of the atom_prox and / or center_prox energy into `grad` [n_lig,3].
    `topo` = byref(PgTopo) (BatchPlan.topo_ref); cnt_ws [B] and mean_ws [B,3] are scratch."""
    hip.check(hip.load_library().pg_guidance_grad(
        topo, _p(x_lig), _p(h_edge_prev), _p(lig_graph), _p(g_lig_off), int(atom_prox), float(min_d), float(max_d), int(center_prox),
        _p(phore_center), mean_over_graphs, _p(cnt_ws), _p(mean_ws), _p(grad), stream), what)
