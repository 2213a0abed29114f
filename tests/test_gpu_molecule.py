"""-m gpu: the molecule screen (csrc/mol_screen.hip through phoregen_amd/molecule.py) against the plain restatement of
tests/mol_reference.py.  The kernel does integer work only, so every comparison is `==`."""
import os

import numpy as np
import pytest
import torch

import mol_reference as R
from helpers import default_model
from mol_support import split_frame, mol_result as _result
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


def _compare_frame(sc, f, refs, sizes):
    """Frame f of a Screen against the restated graphs: every output array, every graph."""
    got = split_frame(sizes, f, per_atom={k: getattr(sc, k) for k in ('cls', 'compact', 'valence2', 'comp')}, per_pair={'order': sc.order},
                      per_graph={'status': sc.status, 'counts': sc.counts, 'valid': sc.valid})
    for g, (n, x, r) in enumerate(zip(sizes, got, refs)):
        assert x['status'] == r['status'], (f, g, n, x['status'], r['status'])
        assert x['counts'].tolist() == r['counts'].tolist(), (f, g, n, x['counts'].tolist(), r['counts'].tolist())
        assert bool(x['valid']) == r['valid']
        for k in ('cls', 'compact', 'valence2', 'comp', 'order'):
            assert x[k].dtype == r[k].dtype and np.array_equal(x[k], r[k]), (f, g, n, k)


def test_kernel_equals_restatement_on_ragged_batches():
    node, pos, edge, sizes = R.generate_batch()
    refs = R.screen_batch(node, pos, edge, sizes)
    # the batch must hold every kind of graph, judged by the restatement alone, before the kernel is looked at
    c = R.census(refs)
    print('census of the generated batch:', c)
    assert c['valid'] >= 10 and c['DISCONNECTED'] >= 10 and c['VALENCE'] >= 10 and min(c.values()) >= 1, c
    for n in (1, 2, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
    res = _result(node, pos, edge, sizes)
    sc = M.screen(res)
    torch.cuda.synchronize()
    assert sc.status.shape == (1, len(sizes)) and sc.counts.shape == (1, len(sizes), 4) and sc.order.shape == (1, edge.shape[0] // 2)
    _compare_frame(sc, 0, refs, sizes)
    assert sc.lig_off.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    # one-hot scores (ties everywhere but at the maximum: first maximum wins) give the same answer as the logits they came from
    hot = _result(torch.nn.functional.one_hot(node.argmax(-1), 12).float(), pos,
                  torch.nn.functional.one_hot(edge.argmax(-1), 6).float(), sizes)
    sc1 = M.screen(hot)
    for k in ('status', 'counts', 'cls', 'compact', 'valence2', 'comp', 'order'):
        assert torch.equal(getattr(sc, k), getattr(sc1, k)), k
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    del sc1
    sc2 = M.screen(res)
    for k in ('status', 'counts', 'cls', 'compact', 'valence2', 'comp', 'order'):
        assert torch.equal(getattr(sc, k), getattr(sc2, k)), k


def test_hand_built_molecules_on_the_device():
    """The CPU cases of tests/test_molecule_host.py as one batch, plus all-equal scores (first maximum wins)."""
    C_, N_, O_, F_ = 1, 2, 3, 4
    cases = [([C_] * 6, {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 4): 4, (4, 5): 4, (0, 5): 4}, {}),
             ([C_, C_, O_, O_], {(0, 1): 1, (1, 2): 1}, {}),
             ([C_] * 6, {(0, b): 1 for b in range(1, 6)}, {}),
             ([N_] + [C_] * 4, {(0, b): 1 for b in range(1, 5)}, {}),
             ([F_, C_], {(0, 1): 2}, {}),
             ([C_, 11, C_, O_], {(0, 1): 1, (0, 2): 1, (2, 3): 2}, {}),
             ([C_, C_, C_], {(0, 1): 1, (1, 2): 1, (0, 2): 5}, {}),
             ([C_, C_, C_], {(0, 1): 1}, {(1, 2): 1, (0, 2): 5}),
             ([11, 11, 11], {(0, 1): 1}, {}),
             ([C_], {}, {}), ([C_, O_], {(0, 1): 2}, {}), ([C_, C_], {(0, 1): 1}, {})]
    parts = [R.scores_from_classes(a, b, reversed_only=r) for a, b, r in cases]
    parts[-1][0][0] = 0.0               # all-equal atom scores: class 0
    parts[-1][2][0, :] = 1.0            # all-equal bond scores: class 0, no bond
    node, pos, edge = (torch.cat([p[i] for p in parts]) for i in range(3))
    sizes = [len(c[0]) for c in cases]
    refs = R.screen_batch(node, pos, edge, sizes)
    assert [r['status'] for r in refs] == [0, 2, 4, 0, 4, 16, 32, 2, 17, 0, 0, 2]
    _compare_frame(M.screen(_result(node, pos, edge, sizes)), 0, refs, sizes)


NA = [11, 9, 14, 8]


def _batch(num_atoms, seed=11):
    from bench import ligphore_workload
    w = ligphore_workload(len(num_atoms), seed=seed)
    centers = torch.randn(len(num_atoms), 3, generator=torch.Generator().manual_seed(seed)) * 2.0
    return (w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(num_atoms), centers)


def _fragment(nf, seed):
    from phoregen_amd.fragment import Fragment
    g = torch.Generator().manual_seed(seed)
    types = torch.randint(0, 11, (nf,), generator=g).tolist()
    bonds = [(i, i + 1, int(torch.randint(1, 5, (1,), generator=g))) for i in range(nf - 1)] + [(0, nf - 1, 1)]
    return Fragment.from_dict({'type': types, 'pos': (1.5 * torch.randn(nf, 3, generator=g) + torch.tensor([2., -1., 0.5])).tolist(),
                               'bonds': bonds})


def _sampled(model, fragments=None):
    res = model.sample_batch(*_batch(NA), rng='device', seed=17, num_steps=12, return_traj=True, fragments=fragments)
    torch.cuda.synchronize()
    return res


def _tensors(res):
    """Every tensor of a result dict, in a fixed order."""
    out = []
    for k in sorted(res):
        vals = res[k].values() if isinstance(res[k], dict) else res[k]
        out += [t for t in vals if torch.is_tensor(t)]
    return out


def test_trajectory_frames(model):
    """Every (frame, graph) of a saved trajectory in one launch == the restatement frame by frame; the result is only read.
    (The last trajectory frame is a draw and the final prediction an argmax: nothing compares the two.)"""
    res = _sampled(model)
    before = [t.clone() for t in _tensors(res)]
    sc = M.screen(res, frames='traj')
    torch.cuda.synchronize()
    assert len(before) >= 9 and all(torch.equal(a, b) for a, b in zip(before, _tensors(res)))
    T1 = res['traj'][0].shape[0]
    assert T1 == 13 and sc.status.shape == (T1, 4) and sc.counts.shape == (T1, 4, 4) and sc.cls.shape == (T1, sum(NA))
    node, pos, edge = (t.cpu() for t in res['traj'])
    for f in range(T1):
        _compare_frame(sc, f, R.screen_batch(node[f], pos[f], edge[f], NA), NA)
    # the final prediction through the same kernel (F = 1, stride 0)
    _compare_frame(M.screen(res), 0, R.screen_batch(*(t.cpu() for t in res['pred']), NA), NA)
    with pytest.raises(ValueError, match='return_traj'):
        M.screen(dict(res, traj=[None, None, None]), frames='traj')
    with pytest.raises(ValueError, match='atom rows'):
        M.screen(dict(res, lig_info=[torch.tensor([11, 9, 14, 9])] + res['lig_info'][1:]))


def _assert_assemble_is_decode_batch(res):
    from phoregen_amd.utils.sample_utils import decode_batch
    before = [t.clone() for t in _tensors(res)]
    mols = M.assemble(res)
    assert all(torch.equal(a, b) for a, b in zip(before, _tensors(res)))
    dec = decode_batch(res)
    assert len(mols) == len(dec) == len(NA)
    refs = R.screen_batch(*(t.cpu() for t in res['pred']), NA)
    for m, d, r in zip(mols, dec, refs):
        assert m['element'] == d['element']
        assert m['atom_pos'].dtype == torch.float32 and torch.equal(m['atom_pos'], d['atom_pos'])
        half = d['bond_index'][0] < d['bond_index'][1]
        assert m['bond_index'].dtype == d['bond_index'].dtype and torch.equal(m['bond_index'], d['bond_index'][:, half])
        assert m['bond_type'].dtype == d['bond_type'].dtype and torch.equal(m['bond_type'], d['bond_type'][half])
        assert m['status'] == r['status'] and m['valid'] == r['valid'] and m['n_components'] == int(r['counts'][2])
        assert np.array_equal(m['valence'], r['valence2'][r['cls'] >= 0] / 2.0)
        if m['bond_type'].numel() <= 999:
            assert M.mol_block(m, 'x').count('\n') == 5 + len(m['element']) + m['bond_type'].numel()
    return mols


def test_assemble_is_the_existing_hand_off(model):
    _assert_assemble_is_decode_batch(_sampled(model))


def test_assemble_with_a_fragment(model):
    frag = _fragment(5, 1)
    mols = _assert_assemble_is_decode_batch(_sampled(model, fragments=[frag, None, frag, None]))
    # the fragment's atoms and bonds are all there (none of its atoms is of the masked class, so compact == local index)
    assert frag.bonds.shape[0] == 5
    for g in (0, 2):
        assert mols[g]['element'][:5] == frag.elements
        have = {(a, b): t for (a, b), t in zip(mols[g]['bond_index'].T.tolist(), mols[g]['bond_type'].tolist())}
        for a, b, t in frag.bonds.tolist():
            assert have.get((a, b)) == t, (g, a, b, t)


def _same_entry(a, b):
    """Equal in type and value: dicts key by key in their order, arrays and tensors with their dtype, a NaN equal to a NaN."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same_entry(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    if torch.is_tensor(a):
        return a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_entry(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and a != a and b != b)


def test_assemble_with_every_carrier_equals_each_carrier_alone():
    """The one blob of `assemble`: with every carrier at once (and keys) each carrier's entries are those of `assemble` with that carrier
    alone, and the base keys those of the plain call.  The batch makes the byte counts odd wherever they can be -- 23 atom rows, 3
    points (15 point outputs, 3 point kinds), text rows of 33 bytes, one pattern -- so a part that is cut at the wrong place or lies
    misaligned behind a narrower one shows.  Graphs of 0, 1, 2, 7 (a pyridine-like ring with a methyl group) and 13 atoms (a ring and
    two chains, atom 5 of the dropped class 11)."""
    from phoregen_amd import substructure as S
    C_, N_, O_ = 1, 2, 3
    ring = {(0, 1): 4, (1, 2): 4, (2, 3): 4, (3, 4): 4, (4, 5): 4, (0, 5): 4}
    graphs = [([], {}), ([C_], {}), ([C_, O_], {(0, 1): 2}), ([N_] + [C_] * 6, {**ring, (1, 6): 1}),
              ([C_, C_, O_, C_, C_, 11, C_, C_, C_, N_, C_, C_, O_],
               {(0, 1): 1, (1, 2): 1, (1, 3): 2, (3, 4): 1, (4, 5): 1, (4, 6): 1, (6, 7): 1, (7, 8): 1, (8, 9): 1, (9, 10): 1, (10, 11): 1, (6, 11): 1,
                (11, 12): 1})]
    sizes = [len(c) for c, _ in graphs]
    assert sizes == [0, 1, 2, 7, 13]
    rows = [R.scores_from_classes(c, b) for c, b in graphs]
    res = _result(*(torch.cat([r[i] for r in rows]) for i in range(3)), sizes)
    pts = torch.tensor([[0.25, 0.5, 0.75], [3.0, 3.25, 3.5], [1.0, 1.0, 1.0]])
    is_ex, kinds = torch.tensor([0, 0, 1]), torch.tensor([3, 4, M.POINT_IGNORED], dtype=torch.int8)
    pattern = S.Pattern.from_dict({'name': 'C-O', 'atoms': [{'elements': ['C']}, {'elements': ['O']}], 'bonds': [{'a': 0, 'b': 1, 'orders': [1, 2]}]})
    sc = M.screen(res)
    rg, kk = M.rings(res, screen=sc), M.kekulize(res, screen=sc)
    st = M.stereo(res, screen=sc, kekule=kk, rings=rg)
    carriers = dict(geometry=M.geometry(res, pts, is_ex, screen=sc), rings=rg, kekule=kk,
                    features=M.features(res, pts, kinds, screen=sc, kekule=kk, rings=rg), smiles=M.smiles(res, screen=sc, kekule=kk, capacity=33, stereo=st),
                    stereo=st, fingerprints=M.fingerprints(sc, 1), substructure=S.substructure(res, [pattern], screen=sc, rings=rg, kekule=kk))
    entries = dict(geometry=['geom'], rings=['rings'], kekule=['kekule'], features=['features'], smiles=['smiles'], stereo=['stereo'],
                   fingerprints=['fingerprint', 'fp_bits', 'fp_radius'], substructure=['substructure', 'substructure_ok'])
    every, plain = M.assemble(res, keys=True, **carriers), M.assemble(res)
    base = list(plain[0])
    assert len(every) == len(plain) == 5 and base == ['element', 'atom_pos', 'bond_index', 'bond_type', 'status', 'valid', 'n_components', 'valence']
    for m, p in zip(every, plain):
        assert list(m) == base + ['key', 'atom_colour'] + [k for what in carriers for k in entries[what]]
        assert all(_same_entry(m[k], p[k]) for k in base)
    for m, k in zip(every, M.assemble(res, keys=True)):
        assert _same_entry(m['key'], k['key']) and _same_entry(m['atom_colour'], k['atom_colour'])
    for what, x in carriers.items():
        alone = M.assemble(res, **{what: x})
        for g, (m, a) in enumerate(zip(every, alone)):
            assert list(a) == base + entries[what], (what, g)
            assert all(_same_entry(m[k], a[k]) for k in base + entries[what]), (what, g)
    # what the batch was built to hold: the decoded graphs, a dropped atom, texts that fit their 33 bytes, a pattern that is found
    assert [len(m['element']) for m in every] == [0, 1, 2, 7, 12] and every[4]['status'] & M.STATUS_HAD_MASKED_ATOM and every[3]['valid']
    assert [m['smiles']['smiles_ok'] for m in every] == [True] * 5 and every[2]['smiles']['text'] == 'C=O' and every[0]['smiles']['text'] == ''
    assert every[3]['kekule']['formula'] == 'C6H7N' and every[3]['rings']['rings'] == 1 and every[4]['rings']['rings'] == 1
    assert [m['substructure']['C-O']['anchors'] for m in every] == [0, 0, 1, 0, 2] and every[3]['fp_radius'] == 1
    assert all(m['geom']['point_dist'].shape == (3,) and m['features']['point_kind'].tolist() == [3, 4, -2] for m in every)
    # the graph without atoms: empty arrays of the right dtype in every carrier
    e = every[0]
    empty = {'atom_colour': (e['atom_colour'], np.uint64), 'valence': (e['valence'], np.float64),
             'bond_ring_size': (e['rings']['bond_ring_size'], np.uint8), 'atom_ring': (e['rings']['atom_ring'], np.uint8),
             'ring_sys': (e['rings']['ring_sys'], np.int16), 'hcount': (e['kekule']['hcount'], np.uint8), 'charge': (e['kekule']['charge'], np.int8),
             'atom_fp': (e['features']['atom_fp'], np.uint8), 'atom_rank': (e['smiles']['atom_rank'], np.int16),
             **{k: (e['stereo'][k], np.int8) for k in ('atom_parity', 'atom_label', 'bond_stereo', 'bond_label')}}
    for k, (arr, dt) in empty.items():
        assert isinstance(arr, np.ndarray) and arr.dtype == dt and arr.shape == (0,), k
    assert e['element'] == [] and e['atom_pos'].shape == (0, 3) and e['bond_index'].shape == (2, 0) and e['kekule']['bond_type'].dtype == torch.int64
    assert e['kekule']['bond_type'].shape == (0,) and e['features']['atom_types'] == [] and e['kekule']['formula'] == ''
    assert e['geom']['point_dist'].dtype == np.float32 and e['geom']['point_atom'].dtype == np.int16 and e['geom']['point_atom'].tolist() == [-1] * 3
    assert e['features']['point_dist'].dtype == np.float32 and e['features']['point_matched'].dtype == np.bool_
    assert e['fingerprint'].dtype == np.uint64 and e['fingerprint'].shape == (M.FP_WORDS,) and not e['fingerprint'].any() and e['fp_bits'] == 0
    assert e['substructure']['C-O'] == {'embeddings': 0, 'anchors': 0, 'atoms': [], 'first': None, 'status': 0, 'status_names': ()}
    assert e['key'] == M.KEY_EMPTY and type(e['stereo']['stereo_key']) is int and e['status'] == M.STATUS_NO_ATOMS
    # every status is a Python int
    for m in every:
        assert type(m['status']) is int and type(m['substructure']['C-O']['status']) is int
        assert all(type(m[k]['status']) is int for k in ('geom', 'rings', 'kekule', 'features', 'smiles', 'stereo'))


class _Rota:
    """Test double for the network: `.sample` returns device tensors that encode a fixed rota of three-atom molecules."""
    KINDS = {'valid': ([1, 1, 3], {(0, 1): 1, (1, 2): 1}), 'disconnected': ([1, 1, 3], {(0, 1): 1}),
             'valence': ([4, 1, 1], {(0, 1): 1, (0, 2): 1})}

    def __init__(self, rota):
        self.rota, self.i, self.calls = rota, 0, []

    def sample(self, data, n, device, **kw):
        assert kw.pop('return_traj') is False
        self.calls.append((n, kw))
        kinds = [self.rota[(self.i + j) % len(self.rota)] for j in range(n)]
        self.i += n
        parts = [R.scores_from_classes(*self.KINDS[k]) for k in kinds]
        node, pos, edge = (torch.cat([p[i] for p in parts]) for i in range(3))
        return _result(node, pos, edge, [3] * n)


def test_sample_valid_loop():
    dbl = _Rota(['valid', 'valid', 'disconnected', 'valence', 'valid'])
    out = M.sample_valid(dbl, None, num_samples=7, batch_size=4, seed_marker=1)
    # by hand: draw 4 (v v d x) -> 2 finished; 4 (v v v d) -> 5; 2 (x v) -> 6; 1 (v) -> 7
    assert [c[0] for c in dbl.calls] == [4, 4, 2, 1] and out['n_calls'] == 4
    assert all(c[1] == {'seed_marker': 1} for c in dbl.calls)
    assert len(out['finished']) == 7 and all(m['valid'] and m['status'] == 0 for m in out['finished'])
    assert [m['status'] for m in out['failed']] == [M.STATUS_DISCONNECTED, M.STATUS_VALENCE, M.STATUS_DISCONNECTED, M.STATUS_VALENCE]
    assert all(m['element'] == [6, 6, 8] and m['bond_index'].tolist() == [[0, 1], [1, 2]] for m in out['finished'])
    # never a valid one: draws of 2; the check before a draw first sees len(failed) > 3 * 2 with 8 failed, after 4 draws
    never = _Rota(['disconnected', 'valence'])
    out = M.sample_valid(never, None, num_samples=2, batch_size=4)
    assert out['finished'] == [] and len(out['failed']) == 8 and out['n_calls'] == 4 and [c[0] for c in never.calls] == [2] * 4


def test_sample_valid_with_the_model(model):
    """Deterministic noise weights: what share of their molecules passes is unknown; only the accounting is checked."""
    from phoregen_amd.data import parse_phore_file
    data = parse_phore_file(os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')).to(DEV)
    torch.manual_seed(5)
    out = M.sample_valid(model, data, num_samples=4, batch_size=4, max_failed_factor=1, num_steps=10)
    assert len(out['finished']) <= 4 and out['n_calls'] >= 1
    assert all(m['valid'] for m in out['finished']) and not any(m['valid'] for m in out['failed'])
    assert len(out['finished']) == 4 or len(out['failed']) > 4


def test_oversize_graph_is_refused_before_any_launch():
    """A refusal, not a fault: the library returns its error before launching, so the kernel never sees the oversize graph."""
    from phoregen_amd import hip
    n = M.MAX_ATOMS + 1
    e = n * (n - 1)
    res = _result(torch.zeros(n, 12), torch.zeros(n, 3), torch.zeros(e, 6), [n])
    with pytest.raises(RuntimeError, match='PG_MOL_MAX_ATOMS'):
        M.screen(res)
    # the same through the launch helper with sentinel-filled outputs: nothing is written
    node, pos, edge = res['pred']
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    boff = torch.tensor([0, e], dtype=torch.int32, device=DEV)
    out = {k: torch.full(shape, 77, dtype=dt, device=DEV) for k, shape, dt in (
        ('status', (1, 1), torch.int32), ('counts', (1, 1, 4), torch.int32), ('cls', (1, n), torch.int8), ('compact', (1, n), torch.int16),
        ('valence2', (1, n), torch.uint8), ('comp', (1, n), torch.int16), ('order', (1, e // 2), torch.int8))}
    with pytest.raises(RuntimeError) as err:
        M._launch(hip.lib(), node, 0, edge, 0, pos, 0, off, boff, 1, 1, n, e, n, out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and str(n) in str(err.value)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == 77).all(), k
    # empty batches return without a launch
    empty = _result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])
    assert M.screen(empty).status.shape == (1, 0) and M.assemble(empty) == []
