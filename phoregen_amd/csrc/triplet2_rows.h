// Which row of a segment a row of a 16-row tile is, in the staged triplet kernel (triplet2.hip).  Plain constexpr arithmetic with
// no device types, so that a host program can check it (tests/test_triplet_tail_rows_host.py).
//
// A segment has nr rows in n_tiles = ceil(nr / 16) tiles.  The MFMA layout fixes which tile rows meet where:
//   * pass A computes tile row m in lane (., m) and leaves the logit of tile row 4 g + r in element r of lane (g, .);
//   * pass B holds tile row 4 g + r in element r of lane (g, .) again, and k-step r of the aggregate product S^T += z_v^T . alpha
//     sums over the tile rows {r, 4 + r, 8 + r, 12 + r}.
// In a full tile, tile row m is the segment's row 16 tile + m.  In the TAIL tile (the last one, rem = nr - 16 (n_tiles - 1) rows,
// 1 ... 16) the rows are transposed in the 4 x 4 grid: tile row m holds row 16 tile + 4 (m & 3) + (m >> 2), so that element (g, r)
// is row 16 tile + 4 r + g and k-step r covers the rows 4 r ... 4 r + 3.  The rem valid rows then fill the first ceil(rem / 4)
// k-steps, and the k-steps behind them hold no row at all: pass B skips them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PG_T2_HD __host__ __device__
#else
#define PG_T2_HD
#endif

namespace pg {

// row within its tile that tile row m (0 ... 15) holds
PG_T2_HD constexpr int t2_tile_row(bool tail, int m) { return tail ? 4 * (m & 3) + (m >> 2) : m; }

// the same for element r of lane (g, .): the output of pass A and the operand of pass B
PG_T2_HD constexpr int t2_elem_row(bool tail, int g, int r) { return t2_tile_row(tail, 4 * g + r); }

// rows of the tail tile (1 ... 16; a segment without rows has no tile)
PG_T2_HD constexpr int t2_tail_rows(int nr, int n_tiles) { return nr - 16 * (n_tiles - 1); }

// k-steps of the tail tile's aggregate product that hold a row
PG_T2_HD constexpr int t2_tail_slices(int rem) { return (rem + 3) >> 2; }

}  // namespace pg
