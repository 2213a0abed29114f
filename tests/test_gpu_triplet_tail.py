"""-m gpu: the tail tile of the staged triplet kernel (csrc/triplet2.hip).  A segment's last row tile holds 1 ... 16 rows; the kernel
transposes them into whole k-steps of the aggregate product and skips the k-steps that hold no row (csrc/triplet2_rows.h).

  * every remainder (1 ... 16 rows in the tail) at every tile count, in every instance and form, element by element against the
    float64 reference of tests/seg_attn_reference.py with the bounds of tests/seg_attn_cases.py -- the launch helpers, the NaN
    prefill and the guard rows are those of tests/test_gpu_seg_attn.py;
  * nothing leaks out of a skipped or padded slot: a ligand's rows are the same bits whether it runs alone or between ligands
    whose first-layer rows and coordinates are NaN, and whether the 3-tile or the 4-tile instance runs it."""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

import seg_attn_cases as sc
import test_gpu_seg_attn as tg

pytestmark = pytest.mark.gpu

# ligand atoms n -> n - 2 rows per segment.  tail3: one tile with 1 ... 16 rows (3 ... 18), then 17 ... 48 rows in two and three
# tiles with tails of 1, 4, 5, 16 rows and their neighbours; tail4 / tail5: the same edges of the 4- and 5-tile instances
TAIL_SIZES = dict(
    tail3=tuple((n, 1 + n % 2) for n in (*range(3, 20), 22, 23, 34, 35, 38, 39, 50)),
    tail4=((51, 1), (54, 2), (55, 1), (66, 1), (7, 2)),
    tail5=((67, 1), (81, 2), (6, 1)))
TILES = dict(tail3=3, tail4=4, tail5=5)
for _name, _sizes in TAIL_SIZES.items():
    sc.TRI_SIZES.setdefault(_name, _sizes)                  # (tri_case builds its inputs from a named entry)


def test_the_plans_cover_every_remainder():
    rems = {}
    for name, sizes in TAIL_SIZES.items():
        for n, _ in sizes:
            nr = n - 2
            rems.setdefault(-(-nr // 16), set()).add(nr - 16 * (-(-nr // 16) - 1))
        assert -(-(max(n for n, _ in sizes) - 2) // 16) == TILES[name]
    assert rems[1] == set(range(1, 17))
    assert {1, 4, 5, 16} <= rems[2] and {1, 4, 5, 16} <= rems[3] and {1, 4, 5, 16} <= rems[4] and {1, 15} <= rems[5]


@pytest.mark.parametrize('name', list(TAIL_SIZES))
def test_every_tail_against_float64(name):
    c, plan, t, d, ref = tg._tri_ref(name)
    every = torch.arange(plan.n_bond)
    assert plan.n_tri_iters > 0
    queue = (plan.tri_iters, plan.n_tri_iters, 0, plan.tri_counter)
    tiles = TILES[name]
    for grid in (0, 3):
        p, o = tg._tri_args(plan, d, queue, tri_grid=grid)
        tg._tri_launch(plan, p, o, ('tri_staged', tiles, 768))
        tg._tri_check(f'triplet staged grid={grid}', name, o, ref, every)
    p, o = tg._tri_args(plan, d, queue)
    tg._tri_launch(plan, p, o, ('tri_staged', tiles, 512), force=4)
    tg._tri_check('triplet staged 8 waves', name, o, ref, every)
    p, o = tg._tri_args(plan, d, queue, train=True, alpha=True)
    tg._tri_launch(plan, p, o, ('tri_staged_train', tiles, 768))
    tg._tri_check('triplet staged S-form', name, o, ref, every)


# ---- no leak from skipped or padded slots ----------------------------------------------------------------------------------------
PER_BOND = ('Csrc', 'Cdst_k', 'Cdst_v', 'G', 'q', 'resid')


@functools.lru_cache(maxsize=None)
def _trio(n, left, right):
    """Inputs of the batch (left, n, right) and of the middle ligand alone: the same numbers for its bonds and atoms; in the batch
    every first-layer row and every coordinate of the two neighbours is NaN."""
    key = f'leak_{left}_{n}_{right}'
    sc.TRI_SIZES.setdefault(key, ((left, 1), (n, 2), (right, 1)))
    c = sc.tri_case(key)
    plan3, t3 = tg._plan(c.sizes)
    plan1, t1 = tg._plan(((n, 2),))
    mine_b = (t3.ctx_graph[t3.bond_src] == 1).cpu()
    b0, nb = int(mine_b.nonzero()[0]), int(mine_b.sum())
    assert nb == n * (n - 1) == plan1.n_bond and bool(mine_b[b0:b0 + nb].all())
    c0, c1 = int(t3.g_ctx_off[1]), int(t3.g_ctx_off[2])
    # the ligand's bonds come in the same order in both plans (ids relative to the ligand's first context node)
    assert torch.equal(t3.bond_src[b0:b0 + nb] - c0, t1.bond_src) and torch.equal(t3.bond_dst[b0:b0 + nb] - c0, t1.bond_dst)
    both, alone = NS(**vars(c)), NS(**vars(c))
    for k in PER_BOND:
        v = getattr(c, k).clone()
        setattr(alone, k, v[b0:b0 + nb].clone())
        if k == 'Csrc':
            v[~mine_b] = float('nan')
        setattr(both, k, v)
    x = c.x.clone()
    alone.x = x[c0:c1].clone()
    x[:c0], x[c1:] = float('nan'), float('nan')
    both.x = x
    for e in (both, alone):
        e.Csrc_k, e.Csrc_v = e.Csrc[:, :128], e.Csrc[:, 128:]
    return (plan3, tg._stage(both, contiguous_src=True), slice(b0, b0 + nb)), (plan1, tg._stage(alone, contiguous_src=True), slice(0, nb))


def _run(plan, d, rows, n, tiles, train=False):
    """The ligand's rows of one launch: out (sampling form) or S, swn and the record of its own n atoms (training form)."""
    queue = (plan.tri_iters, plan.n_tri_iters, 0, plan.tri_counter)
    p, o = tg._tri_args(plan, d, queue, train=train, alpha=train)
    tg._tri_launch(plan, p, o, ('tri_staged_train' if train else 'tri_staged', tiles, 768))
    outs = (o.S[rows], o.swn[rows], o.alpha[rows][:, :n]) if train else (o.out[rows],)
    return [v.clone() for v in outs]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('n', (7, 19, 38, 51))
def test_no_leak_from_skipped_or_padded_slots(n):
    alone_tiles = max(-(-(n - 2) // 16), 3)                  # the instance the ligand gets alone
    # small neighbours keep that instance; between neighbours of 51 atoms the same segments run in the 4-tile instance
    for (left, right), tiles in (((5, 4), alone_tiles),) + ((((51, 51), 4),) if n <= 50 else ()):
        (plan3, d3, rows3), (plan1, d1, rows1) = _trio(n, left, right)
        for train in (False, True):
            alone = _run(plan1, d1, rows1, n, alone_tiles, train)
            between = _run(plan3, d3, rows3, n, tiles, train)
            for a, b in zip(alone, between):
                assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), (n, left, right, train)
                assert _same_bits(a, b), (n, left, right, train)
