"""-m gpu: the ring kernel (csrc/mol_rings.hip through phoregen_amd/molecule.py) against the plain restatement of
tests/ring_reference.py, and the functions that carry its answers.  Integer work only: every comparison is `==`."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import mol_reference as R
import ring_reference as G
from helpers import default_model
from mol_support import C_, renumbered_rows, split_frame, mol_result as _result, permute_batch as _permute_batch, onehot_graph as _onehot, cat_graphs as _cat
from phoregen_amd import molecule as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def model():
    return default_model(DEV)


def _split(rg, sizes, f=0):
    """Frame f of a `Rings` as one dict of numpy arrays per graph, in the restatement's form."""
    return split_frame(sizes, f, per_atom={'atom_ring': rg.atom_ring, 'ring_sys': rg.ring_sys}, per_pair={'ring_size': rg.ring_size},
                       per_graph={'counts': rg.counts, 'status': rg.status, 'ok': rg.ok})


def _same(got, want, where=''):
    for g, (a, b) in enumerate(zip(got, want)):
        assert a['counts'].tolist() == b['counts'].tolist(), (where, g, dict(zip(M.RING_COUNTS, zip(a['counts'].tolist(), b['counts'].tolist()))))
        assert a['status'] == b['status'] and a['ok'] == b['ok'], (where, g, a['status'], b['status'])
        for k in ('ring_size', 'atom_ring', 'ring_sys'):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (where, g, k, np.nonzero(a[k] != b[k])[0][:8])


def _check(node, pos, edge, sizes, limits=M.RingLimits(), where=''):
    """The kernel on one frame == the restatement of the restated screen; returns (Rings, restated rings)."""
    want = G.rings_of_batch(R.screen_batch(node, pos, edge, sizes), limits)
    rg = M.rings(_result(node, pos, edge, sizes), limits=limits)
    torch.cuda.synchronize()
    N, H = sum(sizes), sum(n * (n - 1) // 2 for n in sizes)
    assert rg.status.shape == rg.ok.shape == (1, len(sizes)) and rg.counts.shape == (1, len(sizes), 10) and rg.ring_size.shape == (1, H)
    assert rg.atom_ring.shape == rg.ring_sys.shape == (1, N) and rg.limits == limits
    assert (rg.status.dtype, rg.counts.dtype, rg.ok.dtype) == (torch.int32, torch.int32, torch.bool)
    assert (rg.ring_size.dtype, rg.atom_ring.dtype, rg.ring_sys.dtype) == (torch.uint8, torch.uint8, torch.int16)
    _same(_split(rg, sizes), want, where)
    return rg, want


def test_named_molecules_by_hand_and_by_the_restatement():
    names = list(G.NAMED)
    node, pos, edge, sizes = G.batch_from([G.NAMED[k][:2] for k in names])
    rg, want = _check(node, pos, edge, sizes, where='named')
    got = _split(rg, sizes)
    for k, r in zip(names, got):
        assert r['counts'].tolist() == G.NAMED[k][2] and r['status'] == G.NAMED[k][3], k
    by = dict(zip(names, got))
    assert by['norbornane']['ring_size'][by['norbornane']['ring_size'] > 0].tolist() == [5] * 8
    assert by['cubane']['ring_size'][by['cubane']['ring_size'] > 0].tolist() == [4] * 12
    assert by['spiro[4.5]decane']['ring_sys'].tolist() == [0] * 10 and by['biphenyl']['ring_sys'].tolist() == [0] * 6 + [6] * 6
    assert by['toluene_aromatic_methyl']['status'] == M.RING_AROMATIC_OUTSIDE | M.RING_AROMATIC_LONE and not by['toluene_aromatic_methyl']['ok']
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    del rg
    _same(_split(M.rings(_result(node, pos, edge, sizes)), sizes), want, 'again')


def test_limits_set_exactly_the_expected_bits():
    names = list(G.NAMED)
    node, pos, edge, sizes = G.batch_from([G.NAMED[k][:2] for k in names])
    rg, _ = _check(node, pos, edge, sizes, limits=M.RingLimits(**G.FILTER), where='filter')
    assert rg.status[0].tolist() == [G.NAMED[k][4] for k in names]
    assert rg.ok[0].tolist() == [G.NAMED[k][4] & M.RING_FAIL_MASK == 0 for k in names]
    dflt = M.rings(_result(node, pos, edge, sizes))
    assert all(s & M.RING_FAIL_MASK in (0, M.RING_AROMATIC_OUTSIDE) for s in dflt.status[0].tolist())
    assert dflt.status[0].tolist() == [G.NAMED[k][3] for k in names]


def _straddle(n, ring):
    """n carbon atoms in a chain 0 - 1 - .. - n-1 closed to a ring over the atoms `ring` (in order), the others left as a tail."""
    bonds = {(i, i + 1): 1 for i in range(n - 1)}
    bonds[(ring[0], ring[-1])] = 2
    return [C_] * n, bonds


def test_smallest_shapes_and_the_mask_word_boundary():
    graphs = [([], {}), ([C_], {}), ([C_, C_], {(0, 1): 1}), ([C_] * 3, G.cycle(3)),
              _straddle(64, range(58, 64)), _straddle(65, range(60, 65)), _straddle(128, range(61, 67)),
              ([C_] * 128, G.cycle(128)),                              # ring_size 128 fits the uint8
              ([C_] * 65, {**G.cycle(6, off=0), **G.cycle(7, off=58), (5, 58): 1}),      # a ring in each word, one across the boundary (58..64)
              ([C_] * 12, {**G.cycle(5), **G.cycle(4, off=6)})]       # disconnected: a ring in each piece, atoms 5, 10, 11 alone
    node, pos, edge, sizes = G.batch_from(graphs)
    assert sizes == [0, 1, 2, 3, 64, 65, 128, 128, 65, 12]
    rg, want = _check(node, pos, edge, sizes, where='shapes')
    got = _split(rg, sizes)
    assert [r['counts'].tolist() for r in got[:4]] == [[0] * 10, [0] * 10, [0] * 10, [1, 3, 3, 1, 3, 3, 3, 0, 0, 0]]
    assert got[4]['counts'].tolist()[:7] == [1, 6, 6, 1, 6, 6, 6] and got[4]['ring_sys'].tolist() == [-1] * 58 + [58] * 6
    assert got[5]['counts'].tolist()[:7] == [1, 5, 5, 1, 5, 5, 5] and got[5]['atom_ring'].tolist() == [0] * 60 + [5] * 5
    assert got[6]['counts'].tolist()[:7] == [1, 6, 6, 1, 6, 6, 6] and got[6]['ring_sys'].tolist() == [-1] * 61 + [61] * 6 + [-1] * 61
    assert got[7]['counts'].tolist() == [1, 128, 128, 1, 128, 128, 128, 0, 0, 0] and set(got[7]['atom_ring'].tolist()) == {128}
    assert got[8]['counts'].tolist()[:7] == [2, 13, 13, 2, 6, 7, 7] and got[9]['counts'].tolist() == [2, 9, 9, 2, 4, 5, 5, 0, 0, 0]


def test_dropped_atoms_and_absorbing_rows():
    """A ring that passes rows next to a dropped atom (class 11) and absorbing class-5 rows: the dropped atom takes its bonds with it."""
    ring = {**G.cycle(7), (2, 7): 1, (7, 8): 1, (3, 8): 5, (0, 3): 5, (1, 5): 5}
    graphs = [([C_, C_, C_, 11, C_, C_, C_, C_, C_], ring),            # the 7-ring opens at atom 3; 2 - 7 - 8 hangs off it
              ([C_, C_, 11, C_, C_, C_, C_, C_, C_], {**G.cycle(6, off=3), (0, 1): 1, (1, 2): 1, (2, 3): 1, (1, 3): 4, (2, 4): 5}),
              ([11] * 5, G.cycle(5))]
    node, pos, edge, sizes = G.batch_from(graphs)
    rg, _ = _check(node, pos, edge, sizes, where='dropped')
    got = _split(rg, sizes)
    assert got[0]['counts'].tolist() == [0, 0, 0, 0, 0, 0, 0, 5, 0, 0] and (got[0]['ring_sys'] == -1).all()
    assert got[1]['counts'].tolist() == [1, 6, 6, 1, 6, 6, 6, 0, 1, 2] and got[1]['ring_sys'].tolist() == [-1] * 3 + [3] * 6
    assert got[2]['counts'].tolist() == [0] * 10 and got[2]['status'] == 0
    sc = rg.screen
    assert int(sc.status[0, 0]) & M.STATUS_HAD_MASKED_ATOM and int(sc.status[0, 0]) & M.STATUS_HAD_ABSORBING_BOND


def test_mixed_batch_and_batch_independence():
    rng = np.random.default_rng(21)
    sizes = [0, 1, 7, 65, 128]
    parts = []
    for n in sizes:
        h = n * (n - 1) // 2
        et = np.where(rng.random(h) < 2.0 / max(n, 1), rng.integers(1, 5, h), 0)
        parts.append(_onehot(rng.choice([1, 1, 2, 3, 11], n), et))
    node, pos, edge = _cat(parts)
    rg, want = _check(node, pos, edge, sizes, where='mixed')
    assert sum(int(w['counts'][0]) for w in want) >= 5                 # (there are rings to find)
    for g, (n, p) in enumerate(zip(sizes, parts)):                     # a graph's rows alone == inside the batch
        alone = _split(M.rings(_result(*p, [n])), [n])
        _same(alone, [want[g]], 'alone %d' % n)


@pytest.mark.parametrize('n', [20, 128])
def test_dense_random_graphs(n):
    """Random logits bond about two thirds of all pairs: every pair loop runs over all n (n - 1) / 2 rows."""
    B = 3
    gen = torch.Generator().manual_seed(n)
    node, edge = torch.randn(B * n, 12, generator=gen), torch.randn(B * n * (n - 1), 6, generator=gen)
    node[:, 11] -= 2.0                                                 # (few dropped atoms)
    pos = torch.randn(B * n, 3, generator=gen)
    rg, want = _check(node, pos, edge, [n] * B, where='dense %d' % n)
    h = n * (n - 1) // 2
    assert all(0.55 * h < int(w['counts'][1]) for w in want) and all(int(w['counts'][4]) == 3 for w in want)


@pytest.mark.parametrize('n', [40, 128])
def test_sparse_random_graphs(n):
    """Bond probability about 1.2 / n: bridges, trees and long rings all occur."""
    rng = np.random.default_rng(100 + n)
    B, h = 6, n * (n - 1) // 2
    parts = [_onehot(rng.choice([1, 1, 1, 2, 3], n), np.where(rng.random(h) < 1.2 / n, rng.integers(1, 5, h), 0)) for _ in range(B)]
    node, pos, edge = _cat(parts)
    rg, want = _check(node, pos, edge, [n] * B, where='sparse %d' % n)
    counts = np.stack([w['counts'] for w in want])
    ci = M.RING_COUNTS.index
    assert counts[:, ci('ring_max')].max() >= 8 and counts[:, ci('rotatable')].sum() > 0 and counts[:, ci('aromatic_outside_ring')].sum() > 0
    assert (counts[:, ci('ring_bonds')] < rg.screen.counts[0, :, 1].cpu().numpy()).all()          # (every graph has a bridge)


def test_trajectory_frames():
    """frames='traj', F = 3 in one launch: the frames differ in one bond that opens a ring."""
    frames = [[([C_] * 8, {**G.cycle(6), (0, 6): 1, (6, 7): 1}), ([C_] * 5, G.cycle(5, 4))],
              [([C_] * 8, {**G.chain(6), (0, 6): 1, (6, 7): 1}), ([C_] * 5, G.cycle(5, 4))],
              [([C_] * 8, {**G.cycle(6), (0, 6): 1, (6, 7): 1}), ([C_] * 5, G.chain(5, 4))]]
    per = [G.batch_from(f) for f in frames]
    sizes = per[0][3]
    traj = tuple(torch.stack([p[k] for p in per]).to(DEV) for k in range(3))
    res = _result(*per[-1][:3], sizes, traj=traj)
    rg = M.rings(res, frames='traj')
    assert rg.status.shape == (3, 2) and rg.ring_size.shape == (3, 28 + 10) and rg.ring_sys.shape == (3, 13)
    for f, p in enumerate(per):
        want = G.rings_of_batch(R.screen_batch(*p))
        _same(_split(rg, sizes, f), want, 'frame %d' % f)
    assert rg.counts[:, 0, 0].tolist() == [1, 0, 1] and rg.counts[:, 1, 0].tolist() == [1, 1, 0]
    assert rg.counts[:, 0, 7].tolist() == [1, 5, 1]                    # the opened ring's bonds turn rotatable
    assert rg.status[:, 1].tolist() == [0, 0, M.RING_AROMATIC_OUTSIDE | M.RING_AROMATIC_LONE]
    # a screen handed in is reused; one of other frames is refused
    sc = M.screen(res, frames='traj')
    assert M.rings(res, frames='traj', screen=sc).screen is sc
    with pytest.raises(ValueError, match='screen'):
        M.rings(res, frames='final', screen=sc)


def test_renumbered_batch():
    rng = np.random.default_rng(8)
    sizes = [12, 30, 65, 128, 9]
    named = G.batch_from([G.NAMED['biphenyl'][:2], G.NAMED['spiro[4.5]decane'][:2]])
    parts = [_onehot(rng.choice([1, 2, 3, 11], n, p=[0.6, 0.2, 0.15, 0.05]),
                     np.where(rng.random(n * (n - 1) // 2) < 1.5 / n, rng.integers(1, 5, n * (n - 1) // 2), 0)) for n in sizes]
    node, pos, edge = _cat(parts + [named[:3]])
    sizes = sizes + named[3]
    node2, pos2, edge2, perms = _permute_batch(node, pos, edge, sizes, seed=5)
    rg, _ = _check(node, pos, edge, sizes, where='base')
    rg2, _ = _check(node2, pos2, edge2, sizes, where='renumbered')
    assert torch.equal(rg.counts, rg2.counts) and torch.equal(rg.status, rg2.status)
    for g, (a, b, p) in enumerate(zip(_split(rg, sizes), _split(rg2, sizes), perms)):
        n = sizes[g]
        assert [int(b['atom_ring'][p[i]]) for i in range(n)] == a['atom_ring'].tolist()
        assert np.array_equal(b['ring_size'][renumbered_rows(p)], a['ring_size'])
        part = lambda sys, img: {frozenset(int(img[i]) for i in range(n) if sys[i] == s) for s in set(sys.tolist()) - {-1}}   # noqa: E731
        assert part(a['ring_sys'], p) == part(b['ring_sys'], np.arange(n))
        assert all(int(b['ring_sys'][i]) == min(s) for s in part(b['ring_sys'], np.arange(n)) for i in s)


def test_assemble_carries_the_rings():
    rng = np.random.default_rng(4)
    sizes = [14, 40, 9, 7]
    parts = [_onehot(rng.choice([1, 2, 3, 11], n, p=[0.55, 0.15, 0.15, 0.15]),
                     np.where(rng.random(n * (n - 1) // 2) < 2.5 / n, rng.integers(1, 6, n * (n - 1) // 2), 0)) for n in sizes[:2]]
    named = G.batch_from([([11, C_, C_, 11, C_, C_, C_, 11, C_], {**G.cycle(9), (1, 2): 4, (4, 5): 4, (2, 4): 1, (6, 8): 1, (2, 6): 1}),
                          G.NAMED['toluene_aromatic_methyl'][:2]])
    node, pos, edge = _cat(parts + [named[:3]])
    res = _result(node, pos, edge, sizes)
    refs = R.screen_batch(node, pos, edge, sizes)
    want = G.rings_of_batch(refs)
    rg = M.rings(res)
    plain, ringed = M.assemble(res), M.assemble(res, rings=rg)
    assert len(plain) == len(ringed) == len(sizes)
    for g, (p, m, ref, w) in enumerate(zip(plain, ringed, refs, want)):
        assert set(m) == set(p) | {'rings'}
        for name in p:                                                 # the default output, key for key
            same = torch.equal(p[name], m[name]) if torch.is_tensor(p[name]) else np.array_equal(p[name], m[name])
            assert same, name
        r = m['rings']
        assert set(r) == {'status', 'rings_ok', 'bond_ring_size', 'atom_ring', 'ring_sys'} | set(M.RING_COUNTS)
        assert [r[k] for k in M.RING_COUNTS] == w['counts'].tolist() and r['status'] == w['status'] and r['rings_ok'] == w['ok']
        keep = ref['cls'] >= 0
        assert r['atom_ring'].dtype == np.uint8 and r['atom_ring'].tolist() == w['atom_ring'][keep].tolist()
        sys_want = [int(ref['compact'][s]) if s >= 0 else -1 for s in w['ring_sys'][keep].tolist()]
        assert r['ring_sys'].dtype == np.int16 and r['ring_sys'].tolist() == sys_want
        # per entry of 'bond_type', in its order: the pair rows that hold a bond
        n = sizes[g]
        rows = [R.pair_row(int(np.nonzero(ref['compact'] == a)[0][0]), int(np.nonzero(ref['compact'] == b)[0][0]), n)
                for a, b in m['bond_index'].T.tolist()]
        assert rows == np.nonzero(ref['order'])[0].tolist() and r['bond_ring_size'].tolist() == w['ring_size'][rows].tolist()
        assert len(r['bond_ring_size']) == len(m['bond_type'])
    assert any((m['rings']['ring_sys'] > 0).any() for m in ringed) and ringed[2]['rings']['ring_sys'].tolist() == [-1, 1, 1, 1, 1, -1]
    # keys, geometry and rings together ride in one copy; geometry and rings must come from one screen
    pts, ex = torch.tensor([[0.0, 0.0, 0.0], [4.0, 1.0, 0.0]]), torch.tensor([0, 1])
    geo = M.geometry(res, pts, ex, screen=rg.screen)
    full = M.assemble(res, keys=True, geometry=geo, rings=rg)
    only_geo = M.assemble(res, keys=True, geometry=geo)
    for m, q, w in zip(full, only_geo, ringed):
        assert set(m) == set(q) | {'rings'} and m['key'] == q['key'] and m['geom']['status'] == q['geom']['status']
        assert np.array_equal(m['geom']['point_dist'], q['geom']['point_dist']) and np.array_equal(m['geom']['point_atom'], q['geom']['point_atom'])
        assert all(np.array_equal(m['rings'][k], w['rings'][k]) for k in w['rings'])
    assert M.assemble(res, geometry=M.geometry(res, pts, ex), rings=rg)[3]['rings']['status'] == ringed[3]['rings']['status']   # equal screens
    with pytest.raises(ValueError, match='rings='):                     # of another result
        M.assemble(res, rings=M.rings(_result(*G.batch_from([G.NAMED['benzene'][:2]])[:3], [6])))
    with pytest.raises(ValueError, match='rings='):                     # of more than the final frame
        M.assemble(res, rings=dataclasses.replace(rg, status=rg.status.repeat(2, 1)))
    swapped = _result(node, pos, edge, sizes[:2] + sizes[:1:-1])       # as many atom and bond rows, other graphs
    with pytest.raises(ValueError, match='different results'):
        M.assemble(res, geometry=M.geometry(swapped, pts, ex), rings=rg)


def test_sample_valid_with_ring_limits(model):
    """Deterministic noise weights: what they decode to is unknown; with ring_min = 129 every ring is too small, so whatever is
    finished has none."""
    from phoregen_amd.data import parse_phore_file
    data = parse_phore_file(os.path.join(ROOT, 'tests', 'data', 'synthetic_test.phore')).to(DEV)
    torch.manual_seed(5)
    out = M.sample_valid(model, data, num_samples=4, batch_size=4, max_failed_factor=1, rings=M.RingLimits(ring_min=129), num_steps=10)
    assert set(out) == {'finished', 'failed', 'n_calls'} and out['n_calls'] >= 1
    assert len(out['finished']) == 4 or len(out['failed']) > 4
    for m in out['finished']:
        assert m['valid'] and m['rings']['rings_ok'] and m['rings']['rings'] == 0 and m['rings']['ring_bonds'] == 0
    for m in out['failed']:
        assert not m['valid'] or not m['rings']['rings_ok']
        assert (m['rings']['rings'] > 0) == bool(m['rings']['status'] & M.RING_SMALL)
    # a stand-in model that hands out cyclohexane and hexane in turn: only the chain is finished, rings=True finishes both
    parts = [R.scores_from_classes([C_] * 6, G.cycle(6)), R.scores_from_classes([C_] * 6, G.chain(6))]

    class Rota:
        i = 0

        def sample(self, data, n, device, **kw):
            pick = [parts[(self.i + j) % 2] for j in range(n)]
            self.i += n
            return _result(*(torch.cat([p[k] for p in pick]) for k in range(3)), [6] * n)
    out = M.sample_valid(Rota(), None, num_samples=3, batch_size=2, rings=M.RingLimits(ring_min=7))
    assert [m['rings']['rings'] for m in out['finished']] == [0, 0, 0] and [m['rings']['status'] for m in out['failed']] == [M.RING_SMALL] * 3
    out = M.sample_valid(Rota(), None, num_samples=3, batch_size=2, rings=True)
    assert [m['rings']['rings'] for m in out['finished']] == [1, 0, 1] and out['failed'] == []


def test_cpu_result_and_oversize_graph_are_refused():
    from phoregen_amd import hip
    node, pos, edge, _ = R.scores_from_classes([1, 3], {(0, 1): 1})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.rings({'pred': [node, pos, edge], 'traj': [None, None, None], 'lig_info': [torch.tensor([2])]})
    n = M.MAX_ATOMS + 1
    h = n * (n - 1) // 2
    cls = torch.zeros(1, n, dtype=torch.int8, device=DEV)
    order = torch.zeros(1, h, dtype=torch.int8, device=DEV)
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    boff = torch.tensor([0, 2 * h], dtype=torch.int32, device=DEV)
    out = dict(status=torch.full((1, 1), 77, dtype=torch.int32, device=DEV), counts=torch.full((1, 1, 10), 77, dtype=torch.int32, device=DEV),
               ring_size=torch.full((1, h), 77, dtype=torch.uint8, device=DEV), atom_ring=torch.full((1, n), 77, dtype=torch.uint8, device=DEV),
               ring_sys=torch.full((1, n), 77, dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError) as err:
        M._launch_rings(hip.lib(), cls, order, off, boff, 1, 1, n, (3, 128, 128, 8128), out)
    assert 'PG_MOL_MAX_ATOMS' in str(err.value) and 'pg_mol_rings' in str(err.value) and str(n) in str(err.value)
    with pytest.raises(RuntimeError, match='pg_mol_rings'):
        M._launch_rings(hip.lib(), cls, order, off, boff, 1, 1, -1, (3, 128, 128, 8128), out)
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in out.values())
    # empty batches return without a launch
    empty = M.rings(_result(torch.zeros(0, 12), torch.zeros(0, 3), torch.zeros(0, 6), []))
    assert empty.status.shape == (1, 0) and empty.ring_size.shape == (1, 0) and empty.counts.shape == (1, 0, 10)
