"""-m gpu: the identity key kernel (csrc/mol_key.hip through phoregen_amd/molecule.py) against the plain restatement of
tests/molkey_reference.py, bit for bit, and the functions that use it against networkx.  Integer work only: every comparison is `==`."""
import os

import numpy as np
import pytest
import torch

import mol_reference as R
import molkey_reference as K
from helpers import default_model
from mol_support import M64, mol_result as _result, permute_batch as _permute_batch
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


def _unsigned(t):
    return [v & M64 for v in t.cpu().reshape(-1).tolist()]


def _restated(refs):
    """Keys and per-row colours of a restated batch (tests/mol_reference.screen_batch) by the restated key."""
    keys, colours = [], []
    for r in refs:
        k, c = K.key_of_rows(r['cls'], r['order'])
        keys.append(k)
        colours += c
    return keys, colours


def test_kernel_equals_restatement_on_the_ragged_batch():
    node, pos, edge, sizes = R.generate_batch()
    for n in (1, 2, 3, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
    refs = R.screen_batch(node, pos, edge, sizes)
    c = R.census(refs)
    assert c['HAD_MASKED_ATOM'] >= 1 and c['NO_ATOMS'] >= 1 and c['HAD_ABSORBING_BOND'] >= 1 and c['DISCONNECTED'] >= 10, c
    want_keys, want_colours = _restated(refs)
    assert want_keys.count(M.KEY_EMPTY) == c['NO_ATOMS']
    sc = M.screen(_result(node, pos, edge, sizes))
    mk = M.molecule_keys(sc)
    torch.cuda.synchronize()
    assert mk.key.shape == (1, len(sizes)) and mk.colour.shape == (1, sum(sizes)) and mk.key.dtype == mk.colour.dtype == torch.int64
    got_keys, got_colours = _unsigned(mk.key), _unsigned(mk.colour)
    for g, (a, b) in enumerate(zip(got_keys, want_keys)):
        assert a == b, (g, sizes[g], hex(a), hex(b))
    assert got_colours == want_colours
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    del mk
    mk2 = M.molecule_keys(sc)
    assert _unsigned(mk2.key) == want_keys and _unsigned(mk2.colour) == want_colours


def test_renumbered_batch_has_the_same_keys():
    node, pos, edge, sizes = R.generate_batch()
    node2, pos2, edge2, perms = _permute_batch(node, pos, edge, sizes, seed=5)
    assert not torch.equal(node, node2)
    mk = M.molecule_keys(M.screen(_result(node, pos, edge, sizes)))
    mk2 = M.molecule_keys(M.screen(_result(node2, pos2, edge2, sizes)))
    assert torch.equal(mk.key, mk2.key)
    col, col2 = _unsigned(mk.colour), _unsigned(mk2.colour)
    n0 = 0
    for n, p in zip(sizes, perms):
        assert sorted(col[n0:n0 + n]) == sorted(col2[n0:n0 + n])
        assert [col2[n0 + int(p[i])] for i in range(n)] == col[n0:n0 + n]     # (stronger: atom by atom under the renumbering)
        n0 += n
    # and the permuted batch equals its own restatement, so the agreement is not two equal mistakes
    want_keys, want_colours = _restated(R.screen_batch(node2, pos2, edge2, sizes))
    assert _unsigned(mk2.key) == want_keys and col2 == want_colours


def test_trajectory_frames_and_strided_views():
    """frames='traj' in one launch == frame by frame; a strided [F, rows, .] view (every second frame) works too."""
    sizes = [5, 17, 64, 3, 30]
    rng = np.random.default_rng(3)
    N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
    node = torch.from_numpy(rng.normal(0, 1, (6, N, 12)).astype(np.float32))
    edge = torch.from_numpy(rng.normal(0, 1, (6, E, 6)).astype(np.float32))
    edge[..., 0] += 2.5                                                # mostly "no bond", else everything is one clique
    pos = torch.from_numpy(rng.normal(0, 3, (6, N, 3)).astype(np.float32))
    full = _result(node[-1], pos[-1], edge[-1], sizes, traj=(node.to(DEV), pos.to(DEV), edge.to(DEV)))
    mk = M.molecule_keys(M.screen(full, frames='traj'))
    assert mk.key.shape == (6, len(sizes)) and mk.colour.shape == (6, N)
    for f in range(6):
        one = M.molecule_keys(M.screen(_result(node[f], pos[f], edge[f], sizes)))
        assert torch.equal(one.key[0], mk.key[f]) and torch.equal(one.colour[0], mk.colour[f])
        want_keys, want_colours = _restated(R.screen_batch(node[f], pos[f], edge[f], sizes))
        assert _unsigned(mk.key[f]) == want_keys and _unsigned(mk.colour[f]) == want_colours
    assert len(set(_unsigned(mk.key))) > len(sizes)                    # the frames differ
    strided = dict(full, traj=[t[::2] for t in full['traj']])
    assert not strided['traj'][0].is_contiguous()
    mk2 = M.molecule_keys(M.screen(strided, frames='traj'))
    assert torch.equal(mk2.key, mk.key[::2]) and torch.equal(mk2.colour, mk.colour[::2])


def test_oversize_graph_is_refused_before_any_launch():
    from phoregen_amd import hip
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    cls = torch.zeros(1, n, dtype=torch.int8, device=DEV)
    order = torch.zeros(1, h, dtype=torch.int8, device=DEV)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    boff = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    key = torch.full((1, 1), 77, dtype=torch.int64, device=DEV)
    colour = torch.full((1, n), 77, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError) as err:
        M._launch_key(hip.lib(), cls, order, off, boff, 1, 1, n, key, colour)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_key'):
        M._launch_key(hip.lib(), cls, order, off, boff, 1, 1, -1, key, colour)
    torch.cuda.synchronize()
    assert (key == 77).all() and (colour == 77).all()
    # a null colour pointer is accepted: the keys are the same, nothing else is written
    node, pos, edge, sizes = R.generate_batch(n_graphs=len(R.GEN_SIZES) + 6)
    sc = M.screen(_result(node, pos, edge, sizes))
    want = M.molecule_keys(sc)
    key = torch.full((1, len(sizes)), 77, dtype=torch.int64, device=DEV)
    M._launch_key(hip.lib(), sc.cls, sc.order, sc.lig_off, sc.bond_off, len(sizes), 1, max(sizes), key, None)
    assert torch.equal(key, want.key)
    # empty batches return without a launch
    empty = M.molecule_keys(M.screen(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), [])))
    assert empty.key.shape == (1, 0) and empty.colour.shape == (1, 0)


def test_assemble_with_keys_end_to_end(model):
    from bench import ligphore_workload
    NA = [11, 9, 14, 8]
    w = ligphore_workload(len(NA), seed=11)
    centers = torch.randn(len(NA), 3, generator=torch.Generator().manual_seed(11)) * 2.0
    res = model.sample_batch(w['h_phore'], w['pos_phore'], w['phore_norm'], w['batch_phore'], torch.tensor(NA), centers, rng='device',
                             seed=17, num_steps=10)
    torch.cuda.synchronize()
    plain, keyed = M.assemble(res), M.assemble(res, keys=True)
    assert len(plain) == len(keyed) == len(NA)
    for p, k in zip(plain, keyed):
        assert set(k) == set(p) | {'key', 'atom_colour'}
        for name in p:                                                 # the default output, key for key
            same = torch.equal(p[name], k[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], k[name])
            assert same, name
        want_key, want_colour = K.key_of_mol(k)
        assert isinstance(k['key'], int) and k['key'] == want_key
        assert k['atom_colour'].dtype == np.uint64 and k['atom_colour'].tolist() == want_colour


def test_sample_valid_unique_with_the_model(model):
    """Deterministic noise weights: what they decode to is unknown, only the accounting and the exactness are checked."""
    from phoregen_amd.data import parse_phore_file
    data = parse_phore_file(os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')).to(DEV)
    torch.manual_seed(5)
    out = M.sample_valid(model, data, num_samples=4, batch_size=4, max_failed_factor=1, unique=True, num_steps=10)
    assert set(out) == {'finished', 'failed', 'duplicates', 'n_calls'} and out['n_calls'] >= 1
    fin = out['finished']
    assert len(fin) <= 4 and all(m['valid'] for m in fin + out['duplicates']) and not any(m['valid'] for m in out['failed'])
    assert len(fin) == 4 or len(out['failed']) > 4 or len(out['duplicates']) > 4
    graphs = [K.nx_graph(m) for m in fin]
    assert not any(K.nx_same(graphs[i], graphs[j]) for i in range(len(fin)) for j in range(i))
    for d in out['duplicates']:
        assert any(K.nx_same(K.nx_graph(d), g) for g in graphs)
    for m in fin + out['failed'] + out['duplicates']:
        assert m['key'] == K.key_of_mol(m)[0]
    # a stand-in model that repeats one device-decoded molecule: the whole path (screen, key kernel, copy, comparison) on the device
    parts = [R.scores_from_classes([1, 1, 3], {(0, 1): 1, (1, 2): 1}), R.scores_from_classes([3, 1, 1], {(0, 1): 1, (1, 2): 1}),
             R.scores_from_classes([1, 3, 1], {(0, 1): 1, (1, 2): 1})]

    class Rota:
        i = 0

        def sample(self, data, n, device, **kw):
            pick = [parts[(self.i + j) % 3] for j in range(n)]
            self.i += n
            return _result(*(torch.cat([p[k] for p in pick]) for k in range(3)), [3] * n)
    out = M.sample_valid(Rota(), None, num_samples=3, batch_size=3, unique=True)
    assert [m['element'] for m in out['finished']] == [[6, 6, 8], [6, 8, 6]] and len(out['duplicates']) == 10
    assert {m['key'] for m in out['duplicates']} == {out['finished'][0]['key']} | {out['finished'][1]['key']}


def test_duplicate_groups_on_the_device():
    rng = np.random.default_rng(9)
    distinct = rng.integers(-2 ** 63, 2 ** 63 - 1, 300, dtype=np.int64)
    keys = distinct[rng.integers(0, 300, 5000)]
    keys[[0, 17, 4999]] = np.int64(M.KEY_EMPTY - 2 ** 64)             # planted repeats, as the kernel's int64 pattern
    first, counts, group = M.duplicate_groups(torch.from_numpy(keys).to(DEV))
    assert first.device.type == 'cuda'
    census = {}
    for i, k in enumerate(keys.tolist()):
        census.setdefault(k, []).append(i)
    assert first.tolist() == [v[0] for v in census.values()] and counts.tolist() == [len(v) for v in census.values()]
    order = {k: g for g, k in enumerate(census)}
    assert group.tolist() == [order[k] for k in keys.tolist()]
    assert first[0].item() == 0 and counts[0].item() == len(census[keys[0].item()]) >= 3
    # on the keys of a screened batch with a planted copy of its first graphs
    node, pos, edge, sizes = R.generate_batch(n_graphs=len(R.GEN_SIZES) + 6)
    mk = M.molecule_keys(M.screen(_result(node, pos, edge, sizes)))
    both = torch.cat([mk.key[0], mk.key[0][:5]])
    first, counts, group = M.duplicate_groups(both)
    assert group[len(sizes):].tolist() == group[:5].tolist() and int(counts.sum()) == both.numel()
