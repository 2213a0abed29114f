"""CPU: tests/mol_support.py itself, so that what the molecule tests share cannot quietly hand them the wrong rows or slices."""
import numpy as np
import pytest
import torch

from mol_reference import pair_row
from mol_support import C_, O_, batch_from, pair_walk, permute_batch, renumbered_rows, rows_of, split_frame

# graphs of 1, 2 and 3 atoms and one of 4 with atom 1 dropped (class 11), whose bonds are no bonds; class 5 is no bond either
GRAPHS = [([C_], {}), ([C_, O_], {(0, 1): 2}), ([C_, C_, O_], {(0, 1): 1, (1, 2): 4, (0, 2): 5}),
          ([C_, 11, O_, C_], {(0, 1): 1, (1, 2): 2, (0, 2): 1, (2, 3): 3, (0, 3): 4})]


@pytest.mark.parametrize('classes, bonds', GRAPHS)
def test_rows_and_the_walk_agree_with_pair_row(classes, bonds):
    n = len(classes)
    cls, order = rows_of(classes, bonds)
    kept = [c <= 10 for c in classes]
    real = {p: t for p, t in bonds.items() if t <= 4 and kept[p[0]] and kept[p[1]]}
    assert cls.tolist() == [c if k else -1 for c, k in zip(classes, kept)] and order.shape == (n * (n - 1) // 2,)
    want = np.zeros(n * (n - 1) // 2, dtype=np.int8)
    for (a, b), t in real.items():
        want[pair_row(a, b, n)] = t
    assert cls.dtype == order.dtype == np.int8 and np.array_equal(order, want)
    w = pair_walk(cls, order)
    assert w.kept == kept and w.rows == {p: pair_row(*p, n) for p in sorted(real)} and list(w.rows) == sorted(real)
    assert w.nbrs == [sorted([b for a, b in real if a == i] + [a for a, b in real if b == i]) for i in range(n)]
    assert {p: w.order[row] for p, row in w.rows.items()} == real
    double = pair_walk(cls, order, (2,))                               # only the orders asked for
    assert set(double.rows) == {p for p, t in real.items() if t == 2}
    with pytest.raises(AssertionError):
        rows_of(classes + [C_], {(n, 0): 1})                           # a > b


def test_split_frame_gives_each_graph_its_own_atoms_pairs_and_row():
    sizes = [1, 2, 0, 3]
    N, H, B, F = sum(sizes), sum(n * (n - 1) // 2 for n in sizes), len(sizes), 2
    atom = torch.arange(F * N * 3, dtype=torch.float32).reshape(F, N, 3) + 1000
    pair = torch.arange(F * H, dtype=torch.int16).reshape(F, H) + 2000
    row = torch.arange(F * B * 2, dtype=torch.int32).reshape(F, B, 2) + 3000
    one = torch.arange(F * B, dtype=torch.int64).reshape(F, B) + 4000
    for f in range(F):
        got = split_frame(sizes, f, per_atom={'a': atom}, per_pair={'p': pair}, per_graph={'r': row, 's': one})
        assert len(got) == B and all(set(r) == {'a', 'p', 'r', 's'} for r in got)
        assert [r['a'].shape for r in got] == [(n, 3) for n in sizes] and [r['p'].shape for r in got] == [(n * (n - 1) // 2,) for n in sizes]
        assert np.array_equal(np.concatenate([r['a'] for r in got]), atom[f].numpy())
        assert np.array_equal(np.concatenate([r['p'] for r in got]), pair[f].numpy()) and got[3]['p'].tolist() == pair[f, 1:].tolist()
        assert [r['r'].tolist() for r in got] == row[f].tolist() and [r['s'] for r in got] == one[f].tolist()
        assert all(type(r['s']) is int and r['a'].dtype == np.float32 and r['p'].dtype == np.int16 for r in got)
    assert split_frame([], per_atom={'a': atom[:, :0]}) == [] and split_frame(sizes) == [{}] * B


def test_renumbered_rows_and_permute_batch_move_every_pair_to_its_new_row():
    graphs = GRAPHS + [([C_, O_, C_, C_, O_], {(0, 1): 1, (1, 2): 2, (2, 3): 3, (3, 4): 4, (0, 4): 5})]
    node, pos, edge, sizes = batch_from(graphs)
    node2, pos2, edge2, perms = permute_batch(node, pos, edge, sizes, seed=3)
    assert any((p != np.arange(len(p))).any() for p in perms)
    moved = []
    for (classes, bonds), p in zip(graphs, perms):
        n = len(classes)
        rows = renumbered_rows(p)
        for a in range(n):
            for b in range(a + 1, n):
                assert rows[pair_row(a, b, n)] == pair_row(min(p[a], p[b]), max(p[a], p[b]), n)
        cl = [0] * n
        for i, c in enumerate(classes):
            cl[p[i]] = c
        moved.append((cl, {(int(min(p[a], p[b])), int(max(p[a], p[b]))): t for (a, b), t in bonds.items()}))
    want = batch_from(moved)
    assert torch.equal(node2, want[0]) and torch.equal(edge2, want[2])
    assert torch.equal(pos2[torch.from_numpy(np.concatenate([o + p for o, p in zip(np.cumsum([0] + sizes[:-1]), perms)]))], pos)


def test_batch_from_with_and_without_positions():
    graphs = GRAPHS[1:]
    pos = [np.arange(3 * len(c), dtype=np.float64).reshape(-1, 3) * 0.5 - 7.0 for c, _ in graphs]
    node, made_up, edge, sizes = batch_from(graphs)
    node3, given, edge3, sizes3 = batch_from([(c, b, p.tolist()) for (c, b), p in zip(graphs, pos)])
    assert sizes == sizes3 == [2, 3, 4] and torch.equal(node, node3) and torch.equal(edge, edge3)
    assert node.shape == (9, 12) and edge.shape == (2 * (1 + 3 + 6), 6) and made_up.shape == (9, 3)
    assert node.argmax(-1).tolist() == [c for g in graphs for c in g[0]] and (node.sum(-1) == 1).all() and (edge.sum(-1) == 1).all()
    assert given.dtype == torch.float32 and torch.equal(given, torch.from_numpy(np.concatenate(pos).astype(np.float32)))
    # both halves of the second graph's bond rows carry its classes, the absorbing class 5 included
    assert edge[2:8].argmax(-1).tolist() == [1, 5, 4] * 2
