// The row mapping of the staged triplet kernel's tail tile (phoregen_amd/csrc/triplet2_rows.h) compiled for the host: prints what
// the kernel's functions give, for tests/test_triplet_tail_rows_host.py to hold against the layout's definition.
//   tile_row <tail> <16 values>            t2_tile_row(tail, m), m = 0 ... 15
//   elem_row <tail> <16 values>            t2_elem_row(tail, g, r), index 4 g + r
//   tail <nr> <n_tiles> <rem> <slices>     for every nr = 1 ... 80
#include <cstdio>

#include "../phoregen_amd/csrc/triplet2_rows.h"

static_assert(pg::t2_tile_row(false, 7) == 7 && pg::t2_tile_row(true, 7) == 13, "usable in constant expressions");

int main() {
  for (int tail = 0; tail < 2; ++tail) {
    std::printf("tile_row %d", tail);
    for (int m = 0; m < 16; ++m) std::printf(" %d", pg::t2_tile_row(tail != 0, m));
    std::printf("\nelem_row %d", tail);
    for (int g = 0; g < 4; ++g)
      for (int r = 0; r < 4; ++r) std::printf(" %d", pg::t2_elem_row(tail != 0, g, r));
    std::printf("\n");
  }
  for (int nr = 1; nr <= 80; ++nr) {
    const int n_tiles = (nr + 15) >> 4;
    const int rem = pg::t2_tail_rows(nr, n_tiles);
    std::printf("tail %d %d %d %d\n", nr, n_tiles, rem, pg::t2_tail_slices(rem));
  }
  return 0;
}
