"""Training path on the MI355X: PhoreDiff.compute_loss (HIP forward + hand-written HIP adjoints through the C ABI)
against the reference's recorded loss / gradients (G6 fixtures) and against autograd through the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import DIFF_CFG, golden, make_oracle, rel_err, t

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-3     # relative L2 error of a parameter gradient (fp32 re-association, atomics; the random-init model
                    # amplifies input perturbations ~1e2-1e3 x at mid/low t)


@pytest.fixture(scope='module')
def model():
    from phoregen_amd.config import default_model_config
    from phoregen_amd.models.diffusion import PhoreDiff
    from phoregen_amd.weights import init_deterministic_
    return init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0).to('cuda')


def _batch(g):
    from phoregen_amd.data import TrainBatch
    keys = ('ligand_x', 'ligand_pos', 'ligand_batch', 'ligand_ptr', 'f_edge_index', 'f_edge_attr', 'f_edge_batch',
            'phore_x', 'phore_pos', 'phore_norm', 'phore_batch')
    return TrainBatch(*[t(g[k]) for k in keys], edge_index=t(g['edge_index']) if 'edge_index' in g.files else None)


def _draws(g):
    return {k: t(g[k]) for k in ('time_draw', 'pos_noise', 'u_node', 'u_edge')}


def test_dense_adjoints_match_torch():
    """pg_gemm / pg_gemm_wgrad / pg_ln_relu(_bwd) against a plain fp32 PyTorch reference of the same op."""
    from phoregen_amd import training as tr
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(5)
    for M, N, K in ((777, 130, 148), (4099, 256, 20), (33, 118, 12), (20000, 128, 128)):
        X = torch.randn(M, K, device=dev, generator=g, requires_grad=True)
        W = torch.randn(N, K, device=dev, generator=g, requires_grad=True)
        b = torch.randn(N, device=dev, generator=g, requires_grad=True)
        R = torch.randn(M, N, device=dev, generator=g)
        (tr.linear(X, W, b) * R).sum().backward()
        got = [X.grad.clone(), W.grad.clone(), b.grad.clone()]
        X.grad = W.grad = b.grad = None
        (F.linear(X.double(), W.double(), b.double()) * R.double()).sum().backward()
        for a, r in zip(got, (X.grad, W.grad, b.grad)):
            assert rel_err(a.cpu(), r.cpu()) < 2e-5
    X = torch.randn(1001, 128, device=dev, generator=g, requires_grad=True)
    ga = torch.randn(128, device=dev, generator=g, requires_grad=True)
    be = torch.randn(128, device=dev, generator=g, requires_grad=True)
    R = torch.randn(1001, 128, device=dev, generator=g)
    y = tr.LnReluFn.apply(X, ga, be)
    (y * R).sum().backward()
    got = [X.grad.clone(), ga.grad.clone(), be.grad.clone()]
    X.grad = ga.grad = be.grad = None
    y2 = F.relu(F.layer_norm(X, (128,), ga, be, 1e-5))
    (y2 * R).sum().backward()
    assert rel_err(y.detach().cpu(), y2.detach().cpu()) < 1e-5
    for a, r in zip(got, (X.grad, ga.grad, be.grad)):
        assert rel_err(a.cpu(), r.cpu()) < 2e-5


def test_bond_rows_sum_matches_index_add():
    """pg_bond_rows_sum (adjoint of pg_gemm's gathered operand over the plan's bond_src / bond_dst) against torch's index_add on
    ragged ligands (1 .. 33 atoms: a graph without bonds, tile boundaries), 256 and 128 columns, a strided input."""
    from phoregen_amd import hip
    from phoregen_amd.plan import BatchPlan, make_edge_data
    lib, DEV = hip.lib(), torch.device('cuda')
    na, nph = torch.tensor([5, 1, 17, 33, 2, 16]), torch.tensor([4, 9, 3, 12, 7, 5])
    ei, be = make_edge_data(na)
    B = na.numel()
    plan = BatchPlan(torch.repeat_interleave(torch.arange(B), na), torch.repeat_interleave(torch.arange(B), nph), ei, be, B, DEV)
    g = torch.Generator().manual_seed(4)
    for ncol, ld in ((256, 256), (128, 384)):
        Y = torch.randn(plan.n_bond, ld, generator=g).to(DEV)
        for by_src, idx in ((1, plan.bond_src), (0, plan.bond_dst)):
            out = torch.full((plan.n_ctx, ncol), 7.0, device=DEV)
            hip.check(lib.pg_bond_rows_sum(plan.topo_ref, Y.data_ptr(), Y.stride(0), ncol, by_src, out.data_ptr(), out.stride(0),
                                           hip.stream_ptr()))
            ref = torch.zeros(plan.n_ctx, ncol, dtype=torch.float64, device=DEV).index_add_(0, idx.long(), Y[:, :ncol].double())
            lig = plan.lig2ctx_long
            assert float((out[lig].double() - ref[lig]).abs().max()) <= 1e-5 * float(ref.abs().max())
            mask = torch.ones(plan.n_ctx, dtype=torch.bool, device=DEV)
            mask[lig] = False
            assert bool((out[mask] == 7.0).all())                                  # pharmacophore rows are not written


def test_fold_unfold_adjoints_match_dense_einsum():
    from phoregen_amd import training as tr
    from phoregen_amd.packing import lane_fixed_w2
    dev, n = 'cuda', 70
    g = torch.Generator(device=dev).manual_seed(6)
    q = torch.randn(n, 128, device=dev, generator=g, requires_grad=True)
    W2 = torch.randn(128, 128, device=dev, generator=g, requires_grad=True)
    ids = torch.arange(1, n, 3, device=dev, dtype=torch.int32)
    R = torch.randn(n, 2048, device=dev, generator=g)
    U = tr.FoldFn.apply(q, lane_fixed_w2(W2), ids, ids.numel())
    (U * R).sum().backward()
    got = [q.grad.clone(), W2.grad.clone()]
    q.grad = W2.grad = None
    c, h = torch.arange(128, device=dev), torch.arange(16, device=dev)
    idx = (((c >> 4) * 4 + (c & 3)) * 64 + ((c >> 2) & 3) * 16)[:, None] + h[None, :]      # lane-fixed position of (c, h)
    Ud = torch.einsum('shd,hdc->sch', q.view(n, 16, 8), W2.view(16, 8, 128))
    U2 = torch.zeros(n, 2048, device=dev).index_put((ids.long()[:, None, None], idx[None]), Ud[ids.long()])
    (U2 * R).sum().backward()
    sel = ids.long()                     # rows outside `ids` are left untouched (uninitialised) by design
    assert rel_err(U.detach()[sel].cpu(), U2.detach()[sel].cpu()) < 1e-5
    assert rel_err(got[0].cpu(), q.grad.cpu()) < 1e-5 and rel_err(got[1].cpu(), W2.grad.cpu()) < 1e-5
    S = torch.randn(n, 2048, device=dev, generator=g, requires_grad=True)
    sw = torch.rand(n, 16, device=dev, generator=g, requires_grad=True)
    b2 = torch.randn(128, device=dev, generator=g, requires_grad=True)
    R = torch.randn(n, 128, device=dev, generator=g)
    W2.grad = None
    o = tr.UnfoldFn.apply(S, sw, lane_fixed_w2(W2), b2, ids, ids.numel())
    (o * R).sum().backward()
    got = [S.grad.clone(), sw.grad.clone(), W2.grad.clone(), b2.grad.clone()]
    S.grad = sw.grad = W2.grad = b2.grad = None
    od = torch.einsum('sch,hdc->shd', S[:, idx], W2.view(16, 8, 128)).reshape(n, 128) + b2 * sw.repeat_interleave(8, 1)
    mask = torch.zeros(n, 1, device=dev)
    mask[ids.long()] = 1
    (od * mask * R).sum().backward()
    assert rel_err(o.detach().cpu(), (od * mask).detach().cpu()) < 1e-5
    assert rel_err(got[0][sel].cpu(), S.grad[sel].cpu()) < 1e-5
    for a, r in zip(got[1:], (sw.grad, W2.grad, b2.grad)):
        assert rel_err(a.cpu(), r.cpu()) < 1e-5


_PROFILE_MODELS = {}


def _model_for(name, default):
    """Fixtures named *_<profile> were recorded from the reference with that weight profile (phoregen_amd/weights.py)."""
    prof = next((p for p in ('gamma_signed', 'trained_like') if name.endswith('_' + p)), None)
    if prof is None:
        return default
    if prof not in _PROFILE_MODELS:
        from phoregen_amd.config import default_model_config
        from phoregen_amd.models.diffusion import PhoreDiff
        from phoregen_amd.weights import init_deterministic_
        _PROFILE_MODELS[prof] = init_deterministic_(PhoreDiff(default_model_config(), 'zinc_300'), 0, profile=prof).train().to('cuda')
    return _PROFILE_MODELS[prof]


@pytest.mark.parametrize('name', ['g6_loss_a', 'g6_loss_b', 'g6_loss_a_gamma_signed', 'g6_loss_a_trained_like', 'g6_loss_len'])
def test_compute_loss_matches_reference_fixture(model, name, monkeypatch):
    """G6: loss terms, every parameter-gradient norm and the stored full gradients of the reference's
    compute_loss + backward (diffusion.py:249-352) on the same batch and the same draws.  `g6_loss_len`: recorded with the
    config flag `bond_len_loss` on (diffusion.py:286-290,333,341: bond-length MSE over the molecule's bonds joins the loss)."""
    g = golden(name)
    model = _model_for(name, model)
    monkeypatch.setattr(model, 'bond_len_loss', 'edge_index' in g.files)
    model.zero_grad()
    loss, info = model.compute_loss(_batch(g), draws=_draws(g))
    loss.backward()
    ref = dict(zip([str(k) for k in g['info_keys']], g['info_vals']))
    assert set(info.keys()) == set(ref)
    assert abs(loss.item() - float(g['loss'])) <= 1e-4 * abs(float(g['loss']))
    for k in ('loss_pos', 'loss_node', 'loss_edge', 'loss_count') + (('loss_len',) if 'loss_len' in ref else ()):
        assert abs(info[k] - ref[k]) <= 1e-3 * max(abs(ref[k]), 1e-2), (k, info[k], ref[k])
    assert info['node_acc'] == ref['node_acc'] and info['edge_acc'] == ref['edge_acc']
    params = dict(model.named_parameters())
    names = [str(k) for k in g['param_names']]
    gn = np.array([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in names])
    big = g['grad_norm'] > 1e-4 * g['grad_norm'].max()           # the key-bias gradients are exactly 0 analytically
    # folded key/value LayerNorms (packing._kv_mlp): d/dgamma_c reaches gamma through W2*|gamma| and beta/|gamma|, two terms
    # of size |beta/gamma| x the result, so its fp32 relative error is ~1e-7 |beta_c/gamma_c|, and a dead channel (gamma = 0)
    # gets no gradient at all.  Those entries (only the `gamma_signed` profile has them) are masked, the rest must match.
    folded_gamma = lambda k: k.endswith('net.1.weight') and any(f in k for f in ('hk_func', 'hv_func', 'xk_func', 'xv_func', 'edge_pred_layer'))
    ok = np.array([not (name.endswith('gamma_signed') and folded_gamma(k)) for k in names])
    assert (np.abs(gn - g['grad_norm'])[big & ok] / g['grad_norm'][big & ok]).max() < GRAD_TOL
    for key in g.files:
        if key.startswith('grad::'):
            a, r = params[key[6:]].grad.cpu().double(), t(g[key]).double()
            if name.endswith('gamma_signed') and folded_gamma(key[6:]):
                keep = params[key[6:]].detach().cpu().abs() > 1e-3
                assert int((~keep).sum()) >= 6
                a, r = a[keep], r[keep]
            assert float((a - r).norm()) <= GRAD_TOL * float(r.norm()), key       # (a count-head gradient is exactly 0)


def test_every_gradient_matches_oracle_autograd(model):
    """All 600+ parameter gradients of a 3-graph batch against autograd through the oracle (CPU) on the same draws."""
    from oracle import phoregen_oracle as po
    g = golden('g6_loss_b')
    orc = make_oracle()
    names = [k for k, _ in model.named_parameters()]
    for k in names:
        orc.sd[k].requires_grad_(True)
    keys = ('ligand_x', 'ligand_pos', 'ligand_batch', 'ligand_ptr', 'f_edge_index', 'f_edge_attr', 'f_edge_batch',
            'phore_x', 'phore_pos', 'phore_norm', 'phore_batch')
    rng = po.TrainTapeRng(t(g['time_draw']), t(g['pos_noise']), t(g['u_node']), t(g['u_edge']))
    loss_ref, _ = orc.compute_loss({k: t(g[k]) for k in keys}, rng)
    loss_ref.backward()
    model.zero_grad()
    loss, _ = model.compute_loss(_batch(g), draws=_draws(g))
    loss.backward()
    params = dict(model.named_parameters())
    gmax = max(float(orc.sd[k].grad.norm()) for k in names if orc.sd[k].grad is not None)
    worst = 0.0
    for k in names:
        r = orc.sd[k].grad
        if r is None or float(r.norm()) < 1e-5 * gmax:
            continue
        a = params[k].grad
        assert a is not None, k
        err = float((a.cpu().double() - r.double()).norm() / r.double().norm())
        worst = max(worst, err)
        assert err < GRAD_TOL, (k, err)
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())


def test_training_step_reduces_the_loss(model):
    """A few SGD steps on a fixed batch / fixed draws must lower the objective (end-to-end sanity of the adjoints)."""
    import copy
    m = copy.deepcopy(model)
    g = golden('g6_loss_a')
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=2e-4)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _ = m.compute_loss(_batch(g), draws=_draws(g))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


@pytest.mark.parametrize('tri_grid', [256, 2])
def test_gradients_on_small_and_ragged_graphs(model, tri_grid):
    """2- and 3-atom ligands (bond / triplet segments with zero or one valid row), a 33-atom ligand (3 row tiles) and
    pharmacophores of 4..41 nodes (knn degree < 32) against autograd through the oracle on generated draws.  tri_grid = 2: the
    channel-split triplet adjoint on two persistent workgroups, each walking ~27 source atoms of different ligands one after the
    other (registers, LDS stages and the pending geometry step carried from atom to atom)."""
    from oracle import phoregen_oracle as po
    from oracle.make_inputs import synthetic_train_batch
    from phoregen_amd import options
    from phoregen_amd.data import TrainBatch
    b = synthetic_train_batch(77, [2, 33, 3, 17], [5, 41, 4, 23])
    gen = torch.Generator().manual_seed(5)
    N, E = b['ligand_x'].numel(), b['f_edge_attr'].numel()
    draws = dict(time_draw=torch.tensor([620, 870, 415]), pos_noise=torch.randn(N, 3, generator=gen),
                 u_node=torch.rand(N, 12, generator=gen), u_edge=torch.rand(E, 6, generator=gen))
    orc = make_oracle()
    names = [k for k, _ in model.named_parameters()]
    for k in names:
        orc.sd[k].requires_grad_(True)
    loss_ref, info_ref = orc.compute_loss(b, po.TrainTapeRng(draws['time_draw'], draws['pos_noise'], draws['u_node'],
                                                           draws['u_edge']))
    loss_ref.backward()
    keys = ('ligand_x', 'ligand_pos', 'ligand_batch', 'ligand_ptr', 'f_edge_index', 'f_edge_attr', 'f_edge_batch',
            'phore_x', 'phore_pos', 'phore_norm', 'phore_batch')
    model.zero_grad()
    with options.override(tri_bwd_grid=tri_grid):
        loss, info = model.compute_loss(TrainBatch(*[b[k] for k in keys]), draws=draws)
        loss.backward()
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    assert info['node_acc'] == info_ref['node_acc'] and info['edge_acc'] == info_ref['edge_acc']
    params = dict(model.named_parameters())
    gmax = max(float(orc.sd[k].grad.norm()) for k in names if orc.sd[k].grad is not None)
    for k in names:
        r = orc.sd[k].grad
        if r is None or float(r.norm()) < 1e-5 * gmax:
            continue
        err = float((params[k].grad.cpu().double() - r.double()).norm() / r.double().norm())
        assert err < GRAD_TOL, (k, err)


def _form_log(training, step):
    """The (direction, mode, form name) of every segment-attention launch that `step` makes."""
    training.form_log = log = []
    try:
        step()
    finally:
        training.form_log = None
    return log


def _modes_a_switch_names(switch):
    """The segment-attention modes whose kernel form a training switch changes against the defaults (tri_onepass, bwd_split='all',
    tri_bwd_form=2, ph_onepass) on a batch whose ligands all have at most 64 atoms."""
    modes = set()
    if switch.get('tri_onepass') is False:            # no per-row record: the node modes and the pharmacophore encoder (the triplet's
        modes |= {0, 1, 2, 3, 5}                      # channel-split adjoint reads none anyway)
    if switch.get('tri_bwd_form', 2) != 2:
        modes |= {4}
    if switch.get('ph_onepass') is False:
        modes |= {5}
    # bwd_split='knn' differs from 'all' in the triplet adjoint alone, and only where tri_bwd_form leaves that to csrc/seg_attn_bwd.hip
    # with the forward's record: under the default tri_bwd_form it selects nothing
    if switch.get('bwd_split') == 'knn' and switch.get('tri_bwd_form', 2) == 0 and switch.get('tri_onepass', True):
        modes |= {4}
    return modes


def test_two_pass_adjoints_equal_the_one_wave_form(model):
    """The triplet / knn-node adjoints as a value pass + a key pass (8-wave workgroups, PgSegAttnGrad.dlogit / gfeat_v) against the
    form with both MLP paths in one wave: the same sums in the same order per segment -- only the weight-gradient atomics and the
    scatter-adds of the knn rows arrive in another order.  Ragged batch: 2- / 3-atom ligands, 3 row tiles, 64 atoms (the largest
    the two-pass triplet form takes)."""
    from oracle.make_inputs import synthetic_train_batch
    from phoregen_amd import options
    from phoregen_amd.data import TrainBatch
    b = synthetic_train_batch(78, [2, 33, 3, 17, 64, 9], [5, 41, 4, 23, 12, 30])
    gen = torch.Generator().manual_seed(6)
    N, E = b['ligand_x'].numel(), b['f_edge_attr'].numel()
    draws = dict(time_draw=torch.tensor([620, 870, 415, 77, 940, 233]), pos_noise=torch.randn(N, 3, generator=gen),
                 u_node=torch.rand(N, 12, generator=gen), u_edge=torch.rand(E, 6, generator=gen))
    keys = ('ligand_x', 'ligand_pos', 'ligand_batch', 'ligand_ptr', 'f_edge_index', 'f_edge_attr', 'f_edge_batch',
            'phore_x', 'phore_pos', 'phore_norm', 'phore_batch')
    from phoregen_amd import hip, training
    grads, logs = {}, {}
    for split in (False, True):
        with options.override(bwd_split='all' if split else 'none', tri_bwd_form=0):      # (the one-wave-per-tile triplet adjoint: its two forms)
            model.zero_grad()
            logs[split] = _form_log(training, lambda: model.compute_loss(TrainBatch(*[b[k] for k in keys]), draws=draws)[0].backward())
        grads[split] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    # the two runs are the two forms: both MLP paths in one 4-wave workgroup / a value pass (the triplet's on 8 waves) and a key pass
    for mode, one, two in ((hip.SEG_KNN_NODE, 'bwd_one_wave/256/rec16', 'bwd_two_pass/256+256/rec16'),
                           (hip.SEG_KNN_POS, 'bwd_one_wave/256', 'bwd_two_pass/256+256/rec32'),
                           (hip.SEG_TRIPLET, 'bwd_one_wave/256/rec16', 'bwd_two_pass/512+256/rec16')):
        for split, name in ((False, one), (True, two)):
            ran = {n for d, m, n in logs[split] if d == 'adjoint' and m == mode}
            assert ran == {name}, (mode, split, ran)
    assert grads[True].keys() == grads[False].keys()
    gmax = max(float(v.norm()) for v in grads[False].values())
    for k, r in grads[False].items():
        if float(r.norm()) < 1e-6 * gmax:
            continue
        err = float((grads[True][k].double() - r.double()).norm() / r.double().norm())
        assert err < 2e-5, (k, err)


@pytest.mark.parametrize('switch', [dict(dgrad_mm=False), dict(rows_sum=False), dict(tri_onepass=False), dict(wide_gemm=False),
                                    dict(bwd_atom_sort=False), dict(bwd_split='knn'), dict(bwd_grid=64), dict(tri_bwd_form=0),
                                    dict(tri_bwd_form=0, bwd_atom_sort=False), dict(tri_bwd_form=0, tri_onepass=False),
                                    dict(tri_bwd_form=1), dict(tri_bwd_form=2, tri_bwd_grid=3), dict(ph_onepass=False)])
def test_every_training_switch_gives_the_default_paths_gradients(model, switch):
    """options.py keeps a handful of reachable variants of the training path (the in-tree tiled GEMM instead of the library GEMM for the
    input gradients, atomic index_add instead of pg_bond_rows_sum, the generic two-pass triplet / node adjoints instead of the one-pass
    forms fed by the forward's softmax weights, one GEMM per first-layer block instead of the wide one, the triplet adjoint without
    the cost-sorted atom order, the knn-only split, a smaller persistent grid, the triplet adjoint with one wave per row tile instead of
    the channel-split kernel, its 4-wave form, three persistent workgroups that each walk many source atoms, the pharmacophore encoder's adjoint in the generic
    form instead of the one fed by the forward's softmax weights).  Each of them must give the default path's loss and
    gradients on a ragged batch (same sums, other association / atomic order: <= 2e-5 relative per parameter; the loss to 1e-6)."""
    from oracle.make_inputs import synthetic_train_batch
    from phoregen_amd import options
    from phoregen_amd.data import TrainBatch
    b = synthetic_train_batch(79, [2, 21, 3, 50, 9], [5, 33, 4, 12, 30])
    gen = torch.Generator().manual_seed(7)
    N, E = b['ligand_x'].numel(), b['f_edge_attr'].numel()
    draws = dict(time_draw=torch.tensor([620, 870, 415, 77, 940]), pos_noise=torch.randn(N, 3, generator=gen),
                 u_node=torch.rand(N, 12, generator=gen), u_edge=torch.rand(E, 6, generator=gen))
    keys = ('ligand_x', 'ligand_pos', 'ligand_batch', 'ligand_ptr', 'f_edge_index', 'f_edge_attr', 'f_edge_batch',
            'phore_x', 'phore_pos', 'phore_norm', 'phore_batch')
    from phoregen_amd import training
    out, logs = {}, {}

    def step():
        step.loss, _ = model.compute_loss(TrainBatch(*[b[k] for k in keys]), draws=draws)
        step.loss.backward()
    for name, kw in (('default', {}), ('variant', switch)):
        with options.override(**kw):
            model._plan = None
            model.zero_grad()
            logs[name] = _form_log(training, step)
        out[name] = (float(step.loss), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    # the switch selected what it names, and nothing else: the launches of exactly those modes run in another form
    by_mode = lambda log, mode: [(d, n) for d, m, n in log if m == mode]
    assert {m for m in range(6) if by_mode(logs['variant'], m) != by_mode(logs['default'], m)} == _modes_a_switch_names(switch), \
        (switch, sorted(set(logs['default']) ^ set(logs['variant'])))
    assert all(by_mode(logs['default'], m) for m in range(6))
    assert abs(out['variant'][0] - out['default'][0]) <= 1e-6 * abs(out['default'][0]), (out['variant'][0], out['default'][0])
    ref, var = out['default'][1], out['variant'][1]
    assert ref.keys() == var.keys()
    gmax = max(float(v.norm()) for v in ref.values())
    worst = 0.0
    for k, r in ref.items():
        if float(r.norm()) < 1e-6 * gmax:
            continue
        worst = max(worst, float((var[k].double() - r.double()).norm() / r.double().norm()))
    assert worst < 2e-5, (switch, worst)


def test_gradients_with_a_maximum_size_ligand(model):
    """A 78-atom ligand (the reference's max_atom; 5 row tiles, the 2-wave triplet adjoint) next to a 5-atom one."""
    from oracle import phoregen_oracle as po
    from oracle.make_inputs import synthetic_train_batch
    from phoregen_amd.data import TrainBatch
    b = synthetic_train_batch(91, [78, 5], [30, 23])
    gen = torch.Generator().manual_seed(9)
    N, E = b['ligand_x'].numel(), b['f_edge_attr'].numel()
    draws = dict(time_draw=torch.tensor([930, 610]), pos_noise=torch.randn(N, 3, generator=gen),
                 u_node=torch.rand(N, 12, generator=gen), u_edge=torch.rand(E, 6, generator=gen))
    orc = make_oracle()
    probe = ['denoiser.base_block.0.bond_layer.hk_func.net.0.weight', 'denoiser.base_block.2.bond_layer.hv_func.net.3.weight',
             'denoiser.base_block.5.bond_layer.hq_func.net.0.weight', 'denoiser.base_block.1.node_layer_with_bond.hk_func.net.0.weight',
             'denoiser.base_block.3.pos_layer_with_bond.xv_func.net.0.weight', 'edge_embedder.weight', 'node_embedder.weight',
             'denoiser.base_block.4.lin_node.weight']
    for k in probe:
        orc.sd[k].requires_grad_(True)
    loss_ref, _ = orc.compute_loss(b, po.TrainTapeRng(draws['time_draw'], draws['pos_noise'], draws['u_node'], draws['u_edge']))
    loss_ref.backward()
    keys = ('ligand_x', 'ligand_pos', 'ligand_batch', 'ligand_ptr', 'f_edge_index', 'f_edge_attr', 'f_edge_batch',
            'phore_x', 'phore_pos', 'phore_norm', 'phore_batch')
    from phoregen_amd import hip, training
    model.zero_grad()

    def step():
        step.loss, _ = model.compute_loss(TrainBatch(*[b[k] for k in keys]), draws=draws)
        step.loss.backward()
    log = _form_log(training, step)
    loss = step.loss
    # 78 atoms: the staged forward's 5-tile instance with its record, and the one-wave triplet adjoint on 2 waves that reads it
    tri = {(d, n) for d, m, n in log if m == hip.SEG_TRIPLET}
    assert tri == {('forward', 'tri_staged_train/t5/768/rec16'), ('adjoint', 'bwd_one_wave/128/rec16')}, tri
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    params = dict(model.named_parameters())
    for k in probe:
        r = orc.sd[k].grad.double()
        err = float((params[k].grad.cpu().double() - r).norm() / r.norm())
        assert err < GRAD_TOL, (k, err)


def test_bond_len_loss_needs_the_bond_list(model, monkeypatch):
    """`bond_len_loss=True` reads `data['ligand','ligand'].edge_index` (diffusion.py:287): a batch without it is refused by name."""
    g = golden('g6_loss_a')
    monkeypatch.setattr(model, 'bond_len_loss', True)
    with pytest.raises(ValueError, match='edge_index'):
        model.compute_loss(_batch(g), draws=_draws(g))


def test_validation_pass_without_grad(model):
    """run/run.py evaluates with compute_loss under torch.no_grad(): same loss as the training-mode call, nothing retained."""
    g = golden('g6_loss_a')
    with torch.no_grad():
        loss_ng, info_ng = model.compute_loss(_batch(g), draws=_draws(g))
    loss, info = model.compute_loss(_batch(g), draws=_draws(g))
    assert not loss_ng.requires_grad and loss.requires_grad
    assert abs(loss_ng.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert info_ng['loss_edge'] == pytest.approx(info['loss_edge'], rel=1e-6)


def test_gradient_buckets_over_rccl_one_rank(model):
    """f-4 on the device (reference harness: run/run.py:160-311, `RunDdp`): a 1-rank `nccl` (= RCCL) process group on cuda:0,
    `GradientBuckets` attached to the real model, `compute_loss().backward()` through the HIP adjoints, `finish()`.  The bucket
    all-reduces are launched from the gradient hooks WHILE the backward runs (in bucket-index order), they go through RCCL on
    device memory, and with one rank the reduced gradients must be the local ones bit for bit."""
    import socket
    import torch.distributed as dist
    from phoregen_amd.parallel import GradientBuckets
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1)
    gb = None
    try:
        g = golden('g6_loss_a')
        batch, draws = _batch(g), _draws(g)
        model.train()
        params = [p for p in model.parameters() if p.requires_grad]
        gb = GradientBuckets(params, bucket_mb=1.0)
        assert len(gb.buckets) >= 4 and gb._active()
        for it in range(2):
            model.zero_grad(set_to_none=True)
            gb.launch_log.clear()
            loss, _ = model.compute_loss(batch, draws=draws)
            loss.backward()
            hooked = [b for b, h in gb.launch_log if h]
            local = [p.grad.clone() if p.grad is not None else None for p in params]
            n = gb.finish()
            torch.cuda.synchronize()
            assert [b for b, _ in gb.launch_log] == list(range(len(gb.buckets)))          # index order
            assert n == sum(p.numel() for p in params)
            for p, l in zip(params, local):
                assert p.grad is not None and p.grad.is_cuda
                assert torch.equal(p.grad, l if l is not None else torch.zeros_like(p))      # world size 1: sum / 1 == local
            if it == 1:      # (step 0 learns which parameters never receive a gradient; from then on nothing waits for finish())
                assert hooked == list(range(len(gb.buckets))), (hooked, len(gb.buckets))
        assert abs(float(loss) - float(g['loss'])) <= 1e-4 * abs(float(g['loss']))
    finally:
        if gb is not None:
            gb.remove()
        dist.destroy_process_group()
        model.zero_grad(set_to_none=True)


def test_forward_is_differentiable_like_the_reference(model):
    """diffusion.py:175-246 is an ordinary differentiable nn.Module.forward (compute_loss differentiates it at :267): a caller's own
    scalar built on PhoreDiff.forward's four outputs must reach the parameters and the perturbed inputs.  Gradients of a random
    linear functional of (v, x0, bond, counts) against torch autograd through the oracle, same inputs."""
    from oracle.make_inputs import synthetic_batch
    inp = synthetic_batch(11, [7, 12, 5], [15, 24, 9], [650, 80, 930])
    gen = torch.Generator().manual_seed(3)
    N, E, B = inp['h_node_pert'].size(0), inp['h_edge_pert'].size(0), 3
    R = [torch.randn(N, 12, generator=gen), torch.randn(N, 3, generator=gen), torch.randn(E, 6, generator=gen),
         torch.randn(B, 1, generator=gen), torch.randn(B, 1, generator=gen)]

    def functional(out, R):
        v, x0, bond, (cl, cu) = out
        return (v * R[0]).sum() + (x0 * R[1]).sum() + (bond * R[2]).sum() + (cl * R[3]).sum() + (cu * R[4]).sum()

    orc = make_oracle(0)
    probe = ['v_inference.0.weight', 'bond_inference.2.bias', 'node_embedder.weight', 'edge_embedder.weight', 'phore_embedding.weight',
             'atom_mlp.0.weight', 'phore_encoder.hk_func.net.0.weight', 'denoiser.edge_pred_layer.net.0.weight',
             'denoiser.base_block.0.node_layer_with_edge.hv_func.net.3.weight', 'denoiser.base_block.2.bond_layer.hk_func.net.0.weight',
             'denoiser.base_block.3.pos_layer_with_bond.xq_func.net.0.weight', 'denoiser.base_block.5.pos_layer_with_edge.xv_func.net.3.weight',
             'denoiser.base_block.4.lin_node.weight']
    for k in probe:
        orc.sd[k].requires_grad_(True)
    pos_ref = inp['pos_pert'].clone().requires_grad_(True)
    functional(orc.forward(**{**inp, 'pos_pert': pos_ref}), R).backward()

    model.train()
    model.zero_grad(set_to_none=True)
    dev_inp = {k: v.to('cuda') for k, v in inp.items()}
    pos = dev_inp['pos_pert'].clone().requires_grad_(True)
    out = model(**{**dev_inp, 'pos_pert': pos})
    assert all(o.requires_grad for o in (out[0], out[1], out[2], out[3][0], out[3][1]))
    with torch.no_grad():                                  # the tape changes no value: same outputs as the launch-list path
        fast = model(**dev_inp)
    for a, b in zip((out[0], out[1], out[2], out[3][0], out[3][1]), (fast[0], fast[1], fast[2], fast[3][0], fast[3][1])):
        assert a.shape == b.shape and rel_err(a.detach().cpu(), b.cpu()) <= 2e-5
    functional(out, [r.to('cuda') for r in R]).backward()
    params = dict(model.named_parameters())
    errs = {k: float((params[k].grad.cpu() - orc.sd[k].grad).norm() / orc.sd[k].grad.norm().clamp(min=1e-30)) for k in probe}
    errs['pos_pert'] = float((pos.grad.cpu() - pos_ref.grad).norm() / pos_ref.grad.norm())
    print({k: f'{e:.1e}' for k, e in errs.items()})
    assert max(errs.values()) <= GRAD_TOL, errs
    model.eval()


def test_denoiser_module_on_its_own_is_differentiable_like_the_reference(model):
    """uni_denoiser.py:396-430 called directly (`model.denoiser(h, x, None, bond_index, h_bond, mask, mask, batch, phore_norm)`) in the
    default state of a loaded model -- grad mode on, parameters requiring grad -- returns the no_grad launch list's values WITH a
    gradient function; a functional of its outputs reaches its parameters and inputs with the gradients autograd gives through the
    oracle's restatement of the same module (reference recorded inputs: G3 fixture, layer 0 in)."""
    g = golden('g3_forward_a')
    dev = 'cuda'
    h, x, bi, hb, mask, batch, pn = (t(g['L0_in_' + k]) for k in ('h', 'x', 'bond_index', 'h_bond', 'mask_ligand', 'batch', 'phore_norm'))
    gen = torch.Generator().manual_seed(3)
    R = [torch.randn(h.shape, generator=gen), torch.randn(x.shape, generator=gen), torch.randn(hb.shape, generator=gen)]
    # oracle: the same module restated, differentiated by autograd
    orc = make_oracle(0)
    probe = ['denoiser.edge_pred_layer.net.0.weight', 'denoiser.base_block.0.bond_layer.hk_func.net.0.weight',
             'denoiser.base_block.2.node_layer_with_edge.hv_func.net.3.weight', 'denoiser.base_block.5.pos_layer_with_bond.xq_func.net.0.weight',
             'denoiser.base_block.4.lin_node.weight']
    for k in probe:
        orc.sd[k].requires_grad_(True)
    h_ref = h.clone().requires_grad_(True)
    ho, hbo, xo = orc.denoiser(h_ref, x, bi, hb, mask.bool(), batch, pn)
    ((ho * R[0]).sum() + (xo * R[1]).sum() + (hbo * R[2]).sum()).backward()
    # HIP: module forward under autograd vs under no_grad
    model.zero_grad(set_to_none=True)
    args = [a.to(dev) for a in (h, x)] + [None, bi.to(dev), hb.to(dev), mask.to(dev), mask.to(dev), batch.to(dev)]
    h_in = args[0].clone().requires_grad_(True)
    out = model.denoiser(h_in, *args[1:], phore_norm=pn.to(dev))
    assert all(out[k].requires_grad for k in ('h', 'x', 'h_bond'))
    with torch.no_grad():
        fast = model.denoiser(*args, phore_norm=pn.to(dev))
    for k in ('h', 'x', 'h_bond'):
        assert rel_err(out[k].detach().cpu(), fast[k].cpu()) <= 2e-5, k
        assert rel_err(out[k].detach().cpu(), g['L5_out_' + k]) <= 2e-5, k
    ((out['h'] * R[0].to(dev)).sum() + (out['x'] * R[1].to(dev)).sum() + (out['h_bond'] * R[2].to(dev)).sum()).backward()
    params = dict(model.named_parameters())
    errs = {k: float((params[k].grad.cpu() - orc.sd[k].grad).norm() / orc.sd[k].grad.norm().clamp(min=1e-30)) for k in probe}
    errs['h'] = float((h_in.grad.cpu() - h_ref.grad).norm() / h_ref.grad.norm())
    assert max(errs.values()) <= GRAD_TOL, errs


def test_config5_full_size_gradient_of_a_graph_inside_the_batch_equals_the_graph_alone(model):
    """Size-independent property of the gradient path at BASELINE config 5's full size (256 ligand-pharmacophore pairs, n ~ N(25,5)):
    graphs are independent, so the parameter gradient of a functional of ONE graph's outputs is the same whether that graph is
    differentiated inside the 256-pair batch or alone (which is also why data-parallel training over graphs is exact).  Through
    PhoreDiff.forward under autograd = the HIP adjoints at full size (163 k bond edges, 4 M triplets)."""
    import torch.nn.functional as F
    from bench import ligphore_workload
    from phoregen_amd.plan import make_edge_data
    B = 256
    w = ligphore_workload(B, seed=4321)
    g = torch.Generator().manual_seed(99)
    na = (25 + 5 * torch.randn(B, generator=g)).round().clamp(8, 60).long()
    nph = w['n_phore']
    N = int(na.sum())
    ei, be = make_edge_data(na)
    inp = dict(h_node_pert=F.one_hot(torch.randint(0, 12, (N,), generator=g), 12).float(), pos_pert=2.0 * torch.randn(N, 3, generator=g),
               batch_node=torch.repeat_interleave(torch.arange(B), na),
               h_edge_pert=F.one_hot(torch.randint(0, 6, (ei.size(1),), generator=g), 6).float(), edge_index=ei, batch_edge=be,
               time_step=torch.randint(0, 1000, (B,), generator=g), h_phore=w['h_phore'], pos_phore=w['pos_phore'],
               phore_norm=w['phore_norm'], batch_phore=w['batch_phore'])
    assert ei.size(1) > 150000
    probe = ['node_embedder.weight', 'phore_embedding.weight', 'denoiser.base_block.0.bond_layer.hk_func.net.0.weight',
             'denoiser.base_block.2.node_layer_with_edge.hv_func.net.3.weight', 'denoiser.base_block.3.lin_node.weight',
             'denoiser.base_block.4.pos_layer_with_bond.xk_func.net.0.weight', 'denoiser.base_block.5.bond_layer.hq_func.net.3.weight',
             'v_inference.0.weight', 'bond_inference.0.weight']
    params = dict(model.named_parameters())
    model.train()

    def grads(batch_inp, rows_n, rows_e, R):
        out = model(**{k: v.to('cuda') for k, v in batch_inp.items()})
        n0, n, e0, e = rows_n[0], rows_n[1], rows_e[0], rows_e[1]
        L = (out[0][n0:n0 + n] * R[0]).sum() + (out[1][n0:n0 + n] * R[1]).sum() + (out[2][e0:e0 + e] * R[2]).sum()
        return [x.detach().clone() for x in torch.autograd.grad(L, [params[k] for k in probe])]

    worst = 0.0
    for gi in (0, 97, 255):
        n0, p0 = int(na[:gi].sum()), int(nph[:gi].sum())
        n, p = int(na[gi]), int(nph[gi])
        e0, e = int((na[:gi] * (na[:gi] - 1)).sum()), n * (n - 1)
        R = [torch.randn(n, 12, generator=g).cuda(), torch.randn(n, 3, generator=g).cuda(), torch.randn(e, 6, generator=g).cuda()]
        one = dict(h_node_pert=inp['h_node_pert'][n0:n0 + n], pos_pert=inp['pos_pert'][n0:n0 + n], batch_node=torch.zeros(n, dtype=torch.long),
                   h_edge_pert=inp['h_edge_pert'][e0:e0 + e], edge_index=inp['edge_index'][:, e0:e0 + e] - n0,
                   batch_edge=torch.zeros(e, dtype=torch.long), time_step=inp['time_step'][gi:gi + 1],
                   h_phore=inp['h_phore'][p0:p0 + p], pos_phore=inp['pos_phore'][p0:p0 + p], phore_norm=inp['phore_norm'][p0:p0 + p],
                   batch_phore=torch.zeros(p, dtype=torch.long))
        inside = grads(inp, (n0, n), (e0, e), R)
        alone = grads(one, (0, n), (0, e), R)
        for k, a, b in zip(probe, inside, alone):
            err = float((a - b).norm() / b.norm().clamp(min=1e-30))
            worst = max(worst, err)
            assert err <= 2e-4, (gi, k, err)       # same kernels on the same rows; only the order of atomic accumulations differs
    print('config-5 full size: worst relative gradient difference inside the batch vs alone', worst)
    model.eval()
