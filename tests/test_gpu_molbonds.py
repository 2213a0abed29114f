"""-m gpu: the distance bond screen (csrc/mol_screen_dist.hip through phoregen_amd/molecule.py screen(bonds='distance') and
bond_agreement) against the plain restatement of tests/bonds_reference.py and against what the reference's utils/predict_bonds.py
answered (tests/golden/distance_bonds_v1.npz).  Every input keeps its distances clear of the thresholds (bonds_reference.MARGIN_PM),
so every comparison is `==`."""
import os

import numpy as np
import pytest
import torch

import bonds_reference as BR
from mol_support import split_frame, mol_result as _result, permute_batch
from phoregen_amd import molecule as M
from phoregen_amd.utils.sample_utils import ATOM_TYPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ('status', 'counts', 'valid', 'cls', 'compact', 'valence2', 'comp', 'order')


@pytest.fixture(scope='module')
def batch():
    """The ragged batch, its restatement (computed once, never changed) and its result on the device."""
    node, pos, edge, sizes = BR.generate_batch()
    refs = BR.screen_batch(node, pos, edge, sizes)
    return dict(node=node, pos=pos, edge=edge, sizes=sizes, refs=refs, res=_result(node, pos, edge, sizes))


def _compare_frame(sc, f, refs, sizes, agree=True):
    """Frame f of a Screen against the restated graphs: every output array, every graph."""
    got = split_frame(sizes, f, per_atom={k: getattr(sc, k) for k in ('cls', 'compact', 'valence2', 'comp')}, per_pair={'order': sc.order},
                      per_graph=dict({'status': sc.status, 'counts': sc.counts, 'valid': sc.valid}, **({'agree': sc.agree} if agree else {})))
    for g, (n, x, r) in enumerate(zip(sizes, got, refs)):
        assert x['status'] == r['status'], (f, g, n, x['status'], r['status'])
        assert x['counts'].tolist() == r['counts'].tolist(), (f, g, n, x['counts'].tolist(), r['counts'].tolist())
        assert bool(x['valid']) == r['valid']
        for k in ('cls', 'compact', 'valence2', 'comp', 'order'):
            assert x[k].dtype == r[k].dtype and np.array_equal(x[k], r[k]), (f, g, n, k)
        if agree:
            ag = x['agree']
            assert ag.dtype == r['agree'].dtype and ag.tolist() == r['agree'].tolist(), (f, g, n, ag.tolist(), r['agree'].tolist())
            assert int(ag.sum()) == int(r['counts'][0]) * (int(r['counts'][0]) - 1) // 2 or r['status'] & M.STATUS_NONFINITE


def _same(a, b, names=ARRAYS):
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_kernel_equals_restatement_on_the_ragged_batch(batch):
    sizes, refs = batch['sizes'], batch['refs']
    # the batch must hold every kind of graph, judged by the restatement alone, before the kernel is looked at
    c = BR.census(refs)
    print('census of the generated batch:', c)
    assert c['valid'] >= 10 and c['DISCONNECTED'] >= 10 and c['VALENCE'] >= 10 and min(c.values()) >= 1, c
    assert sorted(c) == sorted(['valid'] + list(M.DISTANCE_STATUS_NAMES.values()))
    orders = np.bincount(np.concatenate([r['order'] for r in refs]), minlength=4)
    assert (orders[1:] >= 10).all() and orders.size == 4, orders
    for n in (1, 2, 16, 17, 63, 64, 65, 78, M.MAX_ATOMS):
        assert n in sizes
    sc = M.bond_agreement(batch['res'])
    torch.cuda.synchronize()
    B = len(sizes)
    assert sc.bonds == 'distance' and sc.status.shape == (1, B) and sc.counts.shape == (1, B, 4) and sc.agree.shape == (1, B, 6)
    assert sc.agree.dtype == torch.int32 and sc.order.shape == (1, batch['edge'].shape[0] // 2)
    _compare_frame(sc, 0, refs, sizes)
    assert not bool((sc.status & M.STATUS_HAD_ABSORBING_BOND).any())
    # without the agreement counts the edge scores are not read: the same screen
    plain = M.screen(batch['res'], bonds='distance')
    assert plain.agree is None and plain.bonds == 'distance'
    _same(sc, plain)
    # the outputs do not depend on what their buffers held: a call into recycled memory agrees
    del plain
    again = M.bond_agreement(batch['res'])
    _same(sc, again, ARRAYS + ('agree',))
    # other margins are another table: the restatement with them, same batch (nothing lies within 1e-3 pm of these thresholds either)
    wide = M.BondMargins(single=10.5, double=5.5, triple=3.5)
    t, n0 = M.bond_thresholds(wide), 0
    for n in sizes:
        assert BR.min_margin_pm(batch['node'][n0:n0 + n].argmax(-1).numpy(), batch['pos'][n0:n0 + n].numpy(), t) >= BR.MARGIN_PM
        n0 += n
    _compare_frame(M.screen(batch['res'], bonds='distance', margins=wide), 0,
                   BR.screen_batch(batch['node'], batch['pos'], None, sizes, wide), sizes, agree=False)


def test_fixture_molecules_equal_the_reference_bonds():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'distance_bonds_v1.npz'))
    sizes = g['sizes'].tolist()
    cls = torch.tensor([ATOM_TYPES.index(z) for z in g['elements'].tolist()])
    node = torch.nn.functional.one_hot(cls, 12).float()
    E = sum(n * (n - 1) for n in sizes)
    res = _result(node, torch.from_numpy(g['pos']), torch.zeros(E, 6), sizes)
    sc = M.screen(res, bonds='distance')
    mols = M.assemble(res, screen=sc)
    assert not bool((sc.status & (M.STATUS_DIST_UNMAPPED_ELEMENT | M.STATUS_HAD_MASKED_ATOM | M.STATUS_NONFINITE)).any())
    census = np.zeros(4, dtype=np.int64)
    for m, mol in enumerate(mols):
        b0, b1 = g['bond_off'][m], g['bond_off'][m + 1]
        # the reference records (i, j) then (j, i) for every bonded pair i < j in row-major order
        assert np.array_equal(mol['bond_index'].numpy(), g['bond_index'][:, b0:b1:2]), m
        assert np.array_equal(mol['bond_type'].numpy(), g['bond_type'][b0:b1:2]), m
        assert mol['bonds'] == 'distance' and mol['element'] == g['elements'][sum(sizes[:m]):sum(sizes[:m + 1])].tolist()
        census += np.bincount(mol['bond_type'].numpy(), minlength=4)
    assert (census[1:] >= 50).all(), census


def test_three_strided_frames_equal_three_single_calls(batch):
    """A trajectory whose frames are not dense (rows of a larger allocation) == one call per frame."""
    k = 40                                                                        # the first graphs: every fixed size is among them
    sizes = batch['sizes'][:k]
    N, E = sum(sizes), sum(n * (n - 1) for n in sizes)
    gen = torch.Generator().manual_seed(5)
    frames = []
    for f in range(3):
        node, pos, edge = batch['node'][:N].clone(), batch['pos'][:N].clone(), batch['edge'][:E].clone()
        if f:                                                                     # other atoms, coordinates and scores per frame
            pos += 0.05 * f * torch.randn(N, 3, generator=gen)
            node[torch.randint(0, N, (N // 20,), generator=gen)] = torch.nn.functional.one_hot(torch.tensor(11), 12).float() * 20
            edge = edge[torch.randperm(E, generator=gen)]
        frames.append((node, pos, edge))
    pad = 7
    big = [torch.full((3, rows + pad, k_), float('nan'), device='cuda') for rows, k_ in ((N, 12), (N, 3), (E, 6))]
    for f, parts in enumerate(frames):
        for t, part in zip(big, parts):
            t[f, :part.shape[0]] = part.cuda()
    traj = [t[:, :rows] for t, rows in zip(big, (N, N, E))]
    assert all(not t.is_contiguous() and t[0].is_contiguous() for t in traj)
    res = _result(*frames[0], sizes, traj=traj)
    sc = M.bond_agreement(res, frames='traj')
    assert sc.status.shape == (3, k) and sc.agree.shape == (3, k, 6) and sc.order.shape == (3, E // 2)
    assert len({tuple(sc.order[f].tolist()) for f in range(3)}) == 3              # the frames differ
    for f, parts in enumerate(frames):
        one = M.bond_agreement(_result(*parts, sizes))
        for name in ARRAYS + ('agree',):
            assert torch.equal(getattr(sc, name)[f], getattr(one, name)[0]), (f, name)


def _onehot_of(sc, batch):
    """A result whose edge scores are one-hot of the screen's orders (both halves), same atoms and coordinates."""
    order, h0, parts = sc.order[0].cpu().numpy(), 0, []
    for n in batch['sizes']:
        h = n * (n - 1) // 2
        parts.append(BR.onehot_edges(order[h0:h0 + h]))
        h0 += h
    return _result(batch['node'], batch['pos'], torch.cat(parts), batch['sizes'])


def test_agreement_with_its_own_orders(batch):
    dist = M.screen(batch['res'], bonds='distance')
    sc = M.bond_agreement(_onehot_of(dist, batch))
    _same(sc, dist)
    agree, refs = sc.agree[0].cpu().numpy(), batch['refs']
    assert np.array_equal(agree[:, 0], sc.counts[0, :, 1].cpu().numpy()) and agree[:, 0].sum() > 1000    # every bonded pair: both_same
    assert not agree[:, 1:5].any()
    assert np.array_equal(agree[:, 5], np.array([r['agree'].sum() - r['counts'][1] for r in refs]))       # the others: neither


def test_downstream_kernels_do_not_see_the_bond_source(batch):
    """molecule_keys, rings, kekulize and smiles on the distance Screen == on a predicted Screen of one-hot scores of those orders."""
    res = batch['res']
    dist = M.screen(res, bonds='distance')
    hot = _onehot_of(dist, batch)
    pred = M.screen(hot)
    assert pred.bonds == 'predicted' and bool((dist.status & M.STATUS_DIST_UNMAPPED_ELEMENT).any())
    _same(pred, dist, tuple(k for k in ARRAYS if k != 'status'))
    assert torch.equal(pred.status, dist.status & ~M.STATUS_DIST_UNMAPPED_ELEMENT)
    kd, kp = M.molecule_keys(dist), M.molecule_keys(pred)
    assert torch.equal(kd.key, kp.key) and torch.equal(kd.colour, kp.colour)
    rd, rp = M.rings(res, screen=dist), M.rings(hot, screen=pred)
    _same(rd, rp, ('status', 'counts', 'ok', 'ring_size', 'atom_ring', 'ring_sys'))
    assert int(rd.counts[0, :, 0].sum()) > 0                                      # there are rings to see
    ed, ep = M.kekulize(res, screen=dist), M.kekulize(hot, screen=pred)
    _same(ed, ep, ('status', 'counts', 'ok', 'kekule_order', 'hcount', 'charge'))
    sd, sp = M.smiles(res, screen=dist, kekule=ed), M.smiles(hot, screen=pred, kekule=ep)
    _same(sd, sp, ('status', 'counts', 'text', 'length', 'atom_rank'))
    assert sd.strings() == sp.strings() and sum(bool(s) for s in sd.strings()) > 20
    assert rd.screen is dist and sd.screen is dist
    with pytest.raises(ValueError, match='different results'):                    # results of the two bond sources cannot be mixed
        M.smiles(res, screen=dist, kekule=ep)
    with pytest.raises(ValueError, match='bond sources'):
        M.assemble(res, rings=rp, screen=dist)
    mols = M.assemble(res, rings=rd, kekule=ed, smiles=sd, screen=M.bond_agreement(res))
    assert [m['bonds'] for m in mols] == ['distance'] * len(mols)
    assert [list(m['bond_agreement'].values()) for m in mols] == [r['agree'].tolist() for r in batch['refs']]
    assert [m['smiles']['text'] for m in mols] == sd.strings()


def test_keys_do_not_depend_on_the_numbering(batch):
    keys = M.molecule_keys(M.screen(batch['res'], bonds='distance'))
    node, pos, edge, _ = permute_batch(batch['node'], batch['pos'], batch['edge'], batch['sizes'], seed=3)
    sc = M.bond_agreement(_result(node, pos, edge, batch['sizes']))
    assert torch.equal(M.molecule_keys(sc).key, keys.key)
    assert len(set(keys.key[0].tolist())) > len(batch['sizes']) // 2
    # the agreement counts are sums over the pairs: the same under renumbering
    assert sc.agree[0].tolist() == [r['agree'].tolist() for r in batch['refs']]
    assert sc.counts[0].tolist() == [r['counts'].tolist() for r in batch['refs']]
