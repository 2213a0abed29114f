"""BatchPlan.lig_windows: the 64-row windows the ligand-only first-layer products run over (PgGemm.tile_rows).  The engine hands the list
to the library as device memory, which the library cannot check: what it relies on is asserted here (every first row in [0, n_ctx - 64],
every ligand row covered)."""
import pytest
import torch

from phoregen_amd.plan import BatchPlan, make_edge_data


def _plan(n_lig, n_phore):
    na = torch.tensor(n_lig)
    B = len(n_lig)
    ei, be = make_edge_data(na)
    bn = torch.repeat_interleave(torch.arange(B), na)
    bp = torch.repeat_interleave(torch.arange(B), torch.tensor(n_phore))
    return BatchPlan(bn, bp, ei, be, B, torch.device('cpu'))


@pytest.mark.parametrize('n_lig,n_phore', [
    ([1, 20, 63, 64, 65, 81], [23, 107, 203, 23, 107, 203]),
    ([81, 65, 64, 63, 20, 1], [203, 23, 107, 203, 23, 107]),          # a one-atom ligand as the last context row
    ([65], [23]),                                                    # the second window is clamped to n_ctx - 64 = 24
    ([1], [107]),
    ([41], [23]),                                                    # exactly one window's worth of context rows
    ([64, 64], [23, 0]),                                             # a graph without pharmacophore nodes: back-to-back ligand runs
])
def test_windows_cover_every_ligand_row_inside_the_context(n_lig, n_phore):
    p = _plan(n_lig, n_phore)
    wins = p.lig_windows.tolist()
    assert p.lig_windows.dtype == torch.int32 and p.n_lig_windows == len(wins) == sum((n + 63) // 64 for n in n_lig)
    assert all(0 <= w <= p.n_ctx - 64 for w in wins), (wins, p.n_ctx)
    covered = torch.zeros(p.n_ctx, dtype=torch.bool)
    for w in wins:
        covered[w:w + 64] = True
    assert bool(covered[p.lig2ctx.long()].all())
    # the k-th window of a ligand run [s, s + n) starts at min(s + 64 k, n_ctx - 64)
    first = (p.g_ctx_off[:-1] + p.g_nph).tolist()
    assert wins == [min(s + 64 * k, p.n_ctx - 64) for s, n in zip(first, n_lig) for k in range((n + 63) // 64)]


@pytest.mark.parametrize('n_lig,n_phore', [([20], [23]), ([40], [23]), ([1, 20], [23, 19])])
def test_no_window_list_below_64_context_rows(n_lig, n_phore):
    p = _plan(n_lig, n_phore)
    assert p.n_ctx < 64 and p.lig_windows is None and p.n_lig_windows == 0
