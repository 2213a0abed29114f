"""The row mapping of the staged triplet kernel's tail tile (csrc/triplet2_rows.h), compiled for the host
(tools/triplet_tail_rows_host_check.cpp) and held against the MFMA layout it has to serve, without a GPU.

The layout (csrc/triplet2.hip): pass A computes tile row m in lane (., m) and leaves tile row 4 g + r in element r of lane (g, .);
pass B holds tile row 4 g + r in element r of lane (g, .), and k-step r of the aggregate product sums over the elements r of the
four lane groups.  The mapping says which of the tile's rows a tile row holds; in the tail tile the rem valid rows must fill the first
ceil(rem / 4) k-steps exactly, so that the kernel can skip the others."""
import shutil

import pytest

from mol_support import build_host_check, run_program

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++ to compile the host check with')


@pytest.fixture(scope='module')
def table(tmp_path_factory):
    exe = build_host_check('triplet_tail_rows_host_check', tmp_path_factory.mktemp('tail_rows'))
    out = dict(tile_row={}, elem_row={}, tail={})
    for line in run_program(exe):
        w = line.split()
        if not w:
            continue
        if w[0] == 'tail':
            nr, n_tiles, rem, slices = map(int, w[1:])
            out['tail'][nr] = (n_tiles, rem, slices)
        else:
            out[w[0]][int(w[1])] = [int(v) for v in w[2:]]
    return out


def test_full_tiles_keep_their_rows(table):
    assert table['tile_row'][0] == list(range(16))
    assert table['elem_row'][0] == list(range(16))                       # element (g, r) is tile row 4 g + r


def test_tail_tile_is_a_permutation_with_whole_k_steps(table):
    rows = table['tile_row'][1]
    assert sorted(rows) == list(range(16))
    assert rows == [4 * (m & 3) + (m >> 2) for m in range(16)]
    for rem in range(1, 17):
        n_slices = -(-rem // 4)
        # the k-step of a row: element r of the lane group g that holds it, i.e. its tile row 4 g + r
        step_of = {rows[m]: m & 3 for m in range(16)}
        assert {step_of[k] for k in range(rem)} == set(range(n_slices)), rem
        # and no k-step behind them holds a valid row, while every k-step in front of the last is full
        for r in range(4):
            held = sorted(k for k in range(16) if step_of[k] == r)
            assert held == [4 * r, 4 * r + 1, 4 * r + 2, 4 * r + 3]
            assert all(k >= rem for k in held) == (r >= n_slices), (rem, r)


def test_both_passes_name_the_same_row(table):
    """Pass A leaves the logit of tile row 4 g + r in element (g, r); pass B reads the value row of element (g, r): the row the
    kernel takes for the element must be the row that pass A's lane m = 4 g + r computed."""
    for tail in (0, 1):
        for g in range(4):
            for r in range(4):
                assert table['elem_row'][tail][4 * g + r] == table['tile_row'][tail][4 * g + r]
    assert [table['elem_row'][1][4 * g + r] for g in range(4) for r in range(4)] == [4 * r + g for g in range(4) for r in range(4)]


def test_tail_rows_and_slices_of_every_segment_length(table):
    for nr in range(1, 81):
        n_tiles, rem, slices = table['tail'][nr]
        assert n_tiles == -(-nr // 16) and 1 <= rem <= 16 and 16 * (n_tiles - 1) + rem == nr
        assert slices == -(-rem // 4)
