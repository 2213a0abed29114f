// Runs the host/device core of the fingerprints and the set kernels (phoregen_amd/csrc/fp_core.h) as a plain host program, for the
// host sanitizers: tests/test_molfp_host.py builds it with -fsanitize=address,undefined and compares every answer with the plain
// restatement of tests/fp_reference.py.  Usage: fp_host_check MODE [IN] OUT
//   bit IN OUT     IN: one identifier (hex) per line.  OUT: 'bit word mask(hex)' per line.
//   tanimoto OUT   OUT: raw uint32, the bits of fp_tanimoto(c, u) for u = 0 .. 2048, c = 0 .. u, in that order.
//   pack IN OUT    IN: 'sim_bits(hex) index' per line.  OUT: 'pack_min(hex) min_index min_sim_bits pack_max(hex) max_index max_sim_bits'.
//   tiles IN OUT   IN: 'n_a n_b target' per line.  OUT: 'tiles_a tiles_b n_split tiles_per_split' then 'j0 j1' per run, then the rows
//                  of lane 0 and of the last lane of every tile of a, then the offset of element (n_a - 1, n_b - 1) (0 if empty).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../phoregen_amd/csrc/fp_core.h"

using namespace pg;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const char* mode = argv[1];
  const bool has_in = strcmp(mode, "tanimoto") != 0;
  if (argc != (has_in ? 4 : 3)) return 2;
  FILE* in = has_in ? fopen(argv[2], "r") : nullptr;
  FILE* out = fopen(argv[has_in ? 3 : 2], "wb");
  if ((has_in && !in) || !out) return 3;
  if (!strcmp(mode, "bit")) {
    unsigned long long id;
    while (fscanf(in, "%llx", &id) == 1) {
      const int b = fp_bit(id);
      fprintf(out, "%d %d %llx\n", b, fp_bit_word(b), fp_bit_mask(b));
    }
  } else if (!strcmp(mode, "tanimoto")) {
    std::vector<uint32_t> row;
    for (int u = 0; u <= kFpBits; ++u) {
      row.clear();
      for (int c = 0; c <= u; ++c) row.push_back(fp_float_bits(fp_tanimoto(c, u)));
      if (fwrite(row.data(), 4, row.size(), out) != row.size()) return 4;
    }
  } else if (!strcmp(mode, "pack")) {
    unsigned int bits;
    int index;
    while (fscanf(in, "%x %d", &bits, &index) == 2) {
      const float s = fp_bits_float(bits);
      const fp_u64 lo = fp_pack_min(s, index), hi = fp_pack_max(s, index);
      fprintf(out, "%llx %d %x %llx %d %x\n", lo, fp_min_index(lo), fp_float_bits(fp_packed_sim(lo)), hi, fp_max_index(hi),
              fp_float_bits(fp_max_sim(hi)));
    }
    fprintf(out, "%d %x\n", fp_max_index(kFpMaxNone), fp_float_bits(fp_max_sim(kFpMaxNone)));
  } else if (!strcmp(mode, "tiles")) {
    int na, nb, target;
    fprintf(out, "%d %d %d %d\n", kFpTileA, kFpTileB, kFpWords, kFpMaxRadius);
    while (fscanf(in, "%d %d %d", &na, &nb, &target) == 3) {
      const FpSplit sp = fp_split(na, nb, target);
      const int ta = fp_tiles(na, kFpTileA);
      fprintf(out, "%d %d %d %d", ta, fp_tiles(nb, kFpTileB), sp.n_split, sp.tiles_per_split);
      for (int s = 0; s < sp.n_split; ++s) {
        int j0, j1;
        fp_split_rows(s, sp.tiles_per_split, nb, j0, j1);
        fprintf(out, " %d %d", j0, j1);
      }
      for (int t = 0; t < ta; ++t) fprintf(out, " %d %d", fp_lane_row((unsigned)t, 0, na), fp_lane_row((unsigned)t, kFpTileA - 1, na));
      fprintf(out, " %zu\n", na > 0 && nb > 0 ? fp_matrix_at(na - 1, nb - 1, nb) : (size_t)0);
    }
  } else {
    return 2;
  }
  if (in) fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
