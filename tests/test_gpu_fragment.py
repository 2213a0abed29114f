"""-m gpu: fragment-conditioned sampling (phoregen_amd/fragment.py, the FRAG posterior kernels of csrc/posterior.hip).

A fragment occupies the first n_f atoms of its graph; after every reverse step its fixed rows are replaced by a draw from the
forward process at the next level (RePaint-style), at step 0 by the fragment itself.  Checked here: graphs without a fragment are
untouched bit for bit; the replacement against a CPU restatement with the Philox words of oracle/philox_ref.py, free rows bit for
bit against the same step without a fragment; the output holds the fragment; pipelined == plain; graph-keyed noise; the
distribution of the replacement draw."""
import numpy as np
import pytest
import torch
from scipy import stats

from helpers import default_model
from oracle import philox_ref as pr

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


def _fragment(nf, seed):
    from phoregen_amd.fragment import Fragment
    g = torch.Generator().manual_seed(seed)
    types = torch.randint(0, 11, (nf,), generator=g).tolist()
    bonds = [(i, i + 1, int(torch.randint(1, 5, (1,), generator=g))) for i in range(nf - 1)]
    if nf >= 4:
        bonds.append((0, nf - 1, 1))
    return Fragment.from_dict({'type': types, 'pos': (1.5 * torch.randn(nf, 3, generator=g) + torch.tensor([2., -1., 0.5])).tolist(),
                               'bonds': bonds})


def _batch(num_atoms, seed=11):
    from bench import ligphore_workload
    w = ligphore_workload(len(num_atoms), seed=seed)
    centers = torch.randn(len(num_atoms), 3, generator=torch.Generator().manual_seed(seed)) * 2.0
    return (w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(num_atoms), centers)


def _offsets(num_atoms):
    na = torch.as_tensor(num_atoms)
    n_off = torch.cat([torch.zeros(1, dtype=torch.long), na.cumsum(0)])
    e_off = torch.cat([torch.zeros(1, dtype=torch.long), (na * (na - 1)).cumsum(0)])
    return n_off.tolist(), e_off.tolist()


GUIDANCE = [{'type': 'atom_prox', 'min_d': 1.2, 'max_d': 1.9}, {'type': 'center_prox'}]


@pytest.mark.parametrize('pipeline', [False, True])
def test_bystanders_are_untouched(model, pipeline):
    """A fragment on graph 0 only: graphs 1..B-1 are bit-identical to the same seed's unconstrained run (pred and trajectory)."""
    na = [11, 9, 14, 8]
    args = _batch(na)
    frag = _fragment(5, 1)
    kw = dict(rng='device', seed=17, num_steps=12, return_traj=True, pipeline=pipeline)
    plain = model.sample_batch(*args, **kw)
    fr = model.sample_batch(*args, fragments=[frag, None, None, None], **kw)
    torch.cuda.synchronize()
    assert 'fragment' not in plain and 'fragment' in fr
    n_off, e_off = _offsets(na)
    n1, e1 = n_off[1], e_off[1]
    for i in range(3):
        assert torch.equal(fr['pred'][i][n1 if i < 2 else e1:], plain['pred'][i][n1 if i < 2 else e1:]), i
        assert torch.equal(fr['traj'][i][:, n1 if i < 2 else e1:], plain['traj'][i][:, n1 if i < 2 else e1:]), i
    # graph 0 did change, and its fixed rows are flagged
    assert not torch.equal(fr['traj'][1][:, :5], plain['traj'][1][:, :5])
    assert fr['fragment']['node_fixed'].tolist() == [True] * 5 + [False] * (sum(na) - 5)
    assert int(fr['fragment']['edge_fixed'].sum()) == 5 * 4


def _replacement_reference(model, lay, num_atoms, seed, level, frag_rows_graph):
    """CPU restatement of the replacement at `level` for the fixed node / bond rows (rule 2), with oracle/philox_ref.py."""
    n_off, e_off = _offsets(num_atoms)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    out = {}
    for tag, cls_t, offs, K, sid, tr in (('node', lay.node_cls, n_off, 12, 3, model.node_transition),
                                          ('edge', lay.edge_cls, e_off, 6, 4, model.edge_transition)):
        cls = cls_t.cpu().numpy()
        rows = np.nonzero(cls >= 0)[0]
        gr = np.searchsorted(np.asarray(offs), rows, side='right') - 1
        local = rows - np.asarray(offs)[gr]
        if level < 0:
            out[tag] = (rows, cls[rows], None)
            continue
        e = local[:, None] * K + np.arange(K)[None, :]
        ctr = np.zeros((e.size, 4), dtype=np.uint32)
        ctr[:, 0] = (e.ravel() >> 2).astype(np.uint32)
        ctr[:, 1] = gr.repeat(K).astype(np.uint32)
        ctr[:, 2], ctr[:, 3] = level, sid
        w = pr.philox4x32(ctr, np.tile(key, (e.size, 1)))
        u = pr.uniform24(w[np.arange(e.size), (e.ravel() & 3)]).astype(np.float64).reshape(-1, K)
        q = tr.q_mats[level].detach().cpu().double().numpy()[cls[rows]]
        o = np.maximum(np.log(q + 1e-30), -32.)
        gum = -np.log(-np.log(u + 1e-30) + 1e-30)
        out[tag] = (rows, (gum + o).argmax(-1), o)
    rows = out['node'][0]
    x0f = lay.x0f.cpu().double().numpy()[rows]
    if level < 0:
        out['pos'] = (rows, x0f)
        return out
    gr = np.searchsorted(np.asarray(n_off), rows, side='right') - 1
    local = rows - np.asarray(n_off)[gr]
    c = (3 * local[:, None] + np.arange(3)[None, :]).ravel()
    ctr = np.zeros((c.size, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = c, gr.repeat(3), level, 5
    w = pr.philox4x32(ctr, np.tile(key, (c.size, 1)))
    u1 = 1.0 - pr.uniform24(w[:, 0]).astype(np.float64)
    u2 = pr.uniform24(w[:, 1]).astype(np.float64)
    eps = (np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)).reshape(-1, 3)
    ab = model.pos_transition.alphas_bar.detach().cpu().double().numpy()[level]
    out['pos'] = (rows, np.sqrt(ab) * x0f + np.sqrt(1 - ab) * eps)
    return out


def test_teacher_forced_replacement(model):
    """Plain loop, steps T-1, 700, 400, 1, 0 from the same input state with and without the fragment: fixed rows = the CPU
    restatement of the replacement (classes exactly, coordinates <= 1e-5), free rows bit-identical."""
    na = [10, 13, 7]
    args = _batch(na, seed=5)
    frags = [_fragment(4, 2), None, _fragment(7, 3)]
    seed = 0x1234_5678_9ABC
    T = model.num_timesteps
    st = model.begin_sampling(*args, rng='device', seed=seed, return_traj=False, fragments=frags)
    lay = st.frag
    w = st.eng.ws
    nf, ef = lay.node_fixed, lay.edge_fixed

    def snap():
        return [t.clone() for t in (w.in_h_node, w.in_pos, w.in_h_edge, st.log_node[st.cur], st.log_edge[st.cur])]

    def put(s):
        for dst, src in zip((w.in_h_node, w.in_pos, w.in_h_edge, st.log_node[st.cur], st.log_edge[st.cur]), s):
            dst.copy_(src)

    # the initial state: fixed rows drawn at level T - 1
    ref = _replacement_reference(model, lay, na, seed, T - 1, None)
    torch.cuda.synchronize()
    assert np.array_equal(w.in_h_node.argmax(-1).cpu().numpy()[ref['node'][0]], ref['node'][1])
    assert np.array_equal(w.in_h_edge.argmax(-1).cpu().numpy()[ref['edge'][0]], ref['edge'][1])
    assert np.abs(w.in_pos.cpu().double().numpy()[ref['pos'][0]] - ref['pos'][1]).max() <= 1e-5
    for i, step in enumerate((T - 1, 700, 400, 1, 0)):
        s0, cur0 = snap(), st.cur
        model.reverse_step(st, i, step)
        a = [t.clone() for t in (w.in_h_node, w.in_pos, w.in_h_edge, st.log_node[st.cur], st.log_edge[st.cur], w.out_v, w.out_bond)]
        a_cur = st.cur
        # the same step from the same input state without the fragment
        st.cur = cur0
        put(s0)
        keep, st.frag = st.frag, None
        model.reverse_step(st, i, step)
        b = [t.clone() for t in (w.in_h_node, w.in_pos, w.in_h_edge, st.log_node[st.cur], st.log_edge[st.cur], w.out_v, w.out_bond)]
        st.frag = keep
        torch.cuda.synchronize()
        for k, fixed in enumerate((nf, None, ef, nf, ef)):
            fixed = nf if k == 1 else fixed
            assert torch.equal(a[k][~fixed], b[k][~fixed]), (step, k)
        assert torch.equal(a[5], b[5]) and torch.equal(a[6], b[6])          # the denoiser saw the same input
        ref = _replacement_reference(model, lay, na, seed, step - 1, None)
        assert np.array_equal(a[0].argmax(-1).cpu().numpy()[ref['node'][0]], ref['node'][1]), step
        assert np.array_equal(a[2].argmax(-1).cpu().numpy()[ref['edge'][0]], ref['edge'][1]), step
        assert float(a[0][nf].sum()) == float(nf.sum()) and float(a[2][ef].sum()) == float(ef.sum())     # one-hot
        assert np.abs(a[1].cpu().double().numpy()[ref['pos'][0]] - ref['pos'][1]).max() <= 1e-5, step
        if step > 0:
            assert np.abs(a[3].cpu().double().numpy()[ref['node'][0]] - ref['node'][2]).max() <= 1e-5
            assert np.abs(a[4].cpu().double().numpy()[ref['edge'][0]] - ref['edge'][2]).max() <= 1e-5
        else:
            for lg, rows, cls in ((a[3], *ref['node'][:2]), (a[4], *ref['edge'][:2])):
                exp = np.full((len(rows), lg.size(1)), -32.)
                exp[np.arange(len(rows)), cls] = 0.
                assert np.array_equal(lg.cpu().double().numpy()[rows], exp)
        # go on from the fragment-conditioned state
        st.cur = a_cur
        put(a[:5])


@pytest.mark.parametrize('guided', [False, True])
def test_output_contains_the_fragment(model, guided):
    """A full 1000-step sample(): pred holds the fragment's coordinates exactly, decode_batch its elements and bonds, the last
    trajectory frame is within 1e-5."""
    from phoregen_amd.data import PhoreGraph
    from phoregen_amd.utils.sample_utils import decode_batch
    hp, pp, pn, _, _, _ = _batch([1], seed=7)
    data = PhoreGraph(hp, pp, pn, torch.tensor([1.0, -2.0, 0.5])).to(DEV)
    frag = _fragment(5, 9)
    na = torch.tensor([9, 6, 12])
    res = model.sample(data, 3, DEV, pos_guidance_opt=GUIDANCE if guided else None, num_atoms=na, seed=3, fragment=frag)
    torch.cuda.synchronize()
    n_off, e_off = _offsets(na)
    want_bonds = {tuple(b) for b in frag.bonds.tolist()}
    for g in range(3):
        rows = slice(n_off[g], n_off[g] + 5)
        assert torch.equal(res['pred'][1][rows].cpu(), frag.pos)
        assert torch.equal(res['pred'][0][rows].argmax(-1).cpu(), frag.types)
        assert (res['traj'][1][-1][rows].cpu() - frag.pos).abs().max() <= 1e-5
        assert torch.equal(res['traj'][0][-1][rows].argmax(-1).cpu(), frag.types)
        assert torch.isfinite(res['pred'][1][n_off[g]:n_off[g + 1]]).all()
    for g, d in enumerate(decode_batch(res)):
        assert d['element'][:5] == frag.elements
        assert torch.equal(d['atom_pos'][:5], frag.pos)
        got = set()
        for (i, j), c in zip(d['bond_index'].t().tolist(), d['bond_type'].tolist()):
            if i < 5 and j < 5:
                got.add((min(i, j), max(i, j), c))
        assert got == want_bonds, g
    assert res['fragment']['node_fixed'].sum() == 15


@pytest.mark.parametrize('guided', [False, True])
def test_pipelined_equals_plain(model, guided):
    na = [12, 9, 16]
    args = _batch(na, seed=21)
    frags = [_fragment(4, 4), _fragment(9, 5), _fragment(6, 6)]
    out = []
    for pipe in (False, True):
        r = model.sample_batch(*args, rng='device', seed=29, num_steps=30, pos_guidance_opt=GUIDANCE if guided else None,
                               pipeline=pipe, fragments=frags)
        out.append(r)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(out[0]['pred'][i], out[1]['pred'][i]), i
        assert torch.equal(out[0]['traj'][i], out[1]['traj'][i]), i


def test_graph_keyed(model):
    """Graph 2 sampled alone with graph_ids=[2] against its rows in the 4-graph batch: the fixed rows bit for bit in every
    trajectory frame (the replacement noise is keyed by graph id and index inside the graph); the whole graph's types and
    coordinates as the unconstrained sampler's batch invariance guarantees (tests/test_gpu_sharding.py)."""
    na = [10, 14, 11, 8]
    hp, pp, pn, bp, nat, centers = _batch(na, seed=31)
    frags = [_fragment(3, 7), None, _fragment(6, 8), _fragment(5, 9)]
    kw = dict(rng='device', seed=41, num_steps=8, return_traj=True)
    whole = model.sample_batch(hp, pp, pn, bp, nat, centers, fragments=frags, **kw)
    g = 2
    sel = bp == g
    alone = model.sample_batch(hp[sel], pp[sel], pn[sel], torch.zeros(int(sel.sum()), dtype=torch.long), nat[g:g + 1],
                               centers[g:g + 1], fragments=[frags[g]], graph_ids=torch.tensor([g]), **kw)
    torch.cuda.synchronize()
    n_off, e_off = _offsets(na)
    sn, se = slice(n_off[g], n_off[g + 1]), slice(e_off[g], e_off[g + 1])
    nf, ef = alone['fragment']['node_fixed'], alone['fragment']['edge_fixed']
    assert torch.equal(whole['fragment']['node_fixed'][sn], nf) and torch.equal(whole['fragment']['edge_fixed'][se], ef)
    for i, (sl, fx) in enumerate(((sn, nf), (sn, nf), (se, ef))):
        assert torch.equal(alone['traj'][i][:, fx], whole['traj'][i][:, sl][:, fx]), i
        assert torch.equal(alone['pred'][i][fx], whole['pred'][i][sl][fx]), i
    assert torch.equal(alone['pred'][0].argmax(-1), whole['pred'][0][sn].argmax(-1))
    assert torch.equal(alone['pred'][2].argmax(-1), whole['pred'][2][se].argmax(-1))
    assert float((alone['pred'][1] - whole['pred'][1][sn]).abs().max()) <= 1e-6 * max(1.0, float(whole['pred'][1].abs().max()))


@pytest.mark.parametrize('level', [999, 600, 10])
def test_replacement_distribution(model, level):
    """pg_fragment_noise on 512 graphs x 20 fixed rows: class frequencies against q_mats[level][v0] (chi^2), coordinates against
    sqrt(ab) x0f and 1 - ab."""
    from phoregen_amd import hip
    lib, pk = hip.lib(), model.packed()
    G, R = 512, 20
    n = G * R
    row_graph = torch.arange(n, dtype=torch.int32, device=DEV) // R
    row0 = torch.arange(G, dtype=torch.int32, device=DEV) * R
    key = torch.arange(G, dtype=torch.int32, device=DEV) + 1000
    v0n, v0e = 2, 1
    ncls = torch.full((n,), v0n, dtype=torch.int32, device=DEV)
    ecls = torch.full((n,), v0e, dtype=torch.int32, device=DEV)
    x0f = (torch.randn(n, 3, generator=torch.Generator().manual_seed(level)) * 3).to(DEV)
    h_n, l_n = torch.full((n, 12), -7., device=DEV), torch.full((n, 12), -7., device=DEV)
    h_e, l_e = torch.full((n, 6), -7., device=DEV), torch.full((n, 6), -7., device=DEV)
    x = torch.full((n, 3), -7., device=DEV)
    hip.check(lib.pg_fragment_noise(level, 987654321, n, n, ncls.data_ptr(), ecls.data_ptr(), x0f.data_ptr(), row_graph.data_ptr(),
                                    row_graph.data_ptr(), row0.data_ptr(), row0.data_ptr(), key.data_ptr(), pk.node_tab[0].data_ptr(),
                                    pk.edge_tab[0].data_ptr(), pk.frag_tab[0].data_ptr(), pk.frag_tab[1].data_ptr(), 3, 4, 5,
                                    h_n.data_ptr(), l_n.data_ptr(), h_e.data_ptr(), l_e.data_ptr(), x.data_ptr(), hip.stream_ptr()),
              'fragment noise')
    torch.cuda.synchronize()
    for h, lg, tr, v0, K in ((h_n, l_n, model.node_transition, v0n, 12), (h_e, l_e, model.edge_transition, v0e, 6)):
        assert torch.equal(h.sum(-1).cpu(), torch.ones(n)) and torch.equal(h.max(-1).values.cpu(), torch.ones(n))
        q = tr.q_mats[level][v0].detach().cpu().double()
        assert torch.allclose(lg[0].cpu().double(), torch.log(q + 1e-30).clamp(min=-32.), atol=1e-5)
        cnt = torch.bincount(h.argmax(-1).cpu(), minlength=K).double()
        p = q.clamp(min=0) / q.sum()
        exp = p * n
        big = exp >= 5
        f_obs = torch.cat([cnt[big], cnt[~big].sum().reshape(1)]) if (~big).any() else cnt[big]
        f_exp = torch.cat([exp[big], exp[~big].sum().reshape(1)]) if (~big).any() else exp[big]
        assert float(cnt[~big].sum()) <= max(20.0, 10 * float(exp[~big].sum()))
        if f_obs.numel() > 1:
            assert stats.chisquare(f_obs.numpy(), f_exp.numpy() * (f_obs.sum() / f_exp.sum()).item()).pvalue > 1e-4, (K, cnt, exp)
    ab = float(model.pos_transition.alphas_bar[level])
    d = x.cpu().double() - np.sqrt(ab) * x0f.cpu().double()
    m = d.numel()
    var = 1.0 - ab
    assert abs(float(d.mean())) <= 5 * np.sqrt(var / m)
    assert abs(float(d.var()) - var) <= 5 * var * np.sqrt(2.0 / m)
    # level -1: the fragment itself
    hip.check(lib.pg_fragment_noise(-1, 1, n, 0, ncls.data_ptr(), None, x0f.data_ptr(), row_graph.data_ptr(), None, row0.data_ptr(),
                                    None, key.data_ptr(), pk.node_tab[0].data_ptr(), None, None, None, 3, 4, 5,
                                    h_n.data_ptr(), None, None, None, x.data_ptr(), hip.stream_ptr()), 'fragment noise')
    torch.cuda.synchronize()
    assert torch.equal(x, x0f) and bool((h_n.argmax(-1) == v0n).all())
