// The index arithmetic the molecule kernels share (phoregen_amd/csrc/mol_common.h: the pair walk and the frame and point-range guards,
// the text the six mol_*.hip kernels compile for the device) compiled for the host, so that it can run under the host sanitizers and
// be held against the tests' restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mol_common_host_check.cpp -o mol_common_host_check
//   ./mol_common_host_check pairs N > walk.txt            every n in 0..N, every lane: a line `n lane p a b` per visited pair, in order
//   ./mol_common_host_check frames cases.txt > out.txt
//
// (tests/test_molcommon_host.py does all three steps.)
//
// cases.txt, per case: a line `F B n_lig n_half n_point n_out`, then lig_off [B + 1], bond_off [B + 1] (directed rows, as the kernels
// are handed them), point_range [2 B] and point_out_off [B + 1].  Per block f * B + g one line comes out: `ok f g a0 n h0 n_pair arow
// hrow` (only `0` for a refused frame), then ` ok ps pe o0 orow` for the points of an accepted frame (only ` 0` for a refused range).
// The arrays are exactly as long as the kernels' contract says, so a read outside them is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../phoregen_amd/csrc/mol_common.h"

static bool read_ints(std::FILE* fh, std::vector<int>& v) {
  for (auto& x : v)
    if (std::fscanf(fh, "%d", &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "pairs")) {
    const int n_max = std::atoi(argv[2]);
    for (int n = 0; n <= n_max; ++n)
      for (int lane = 0; lane < 64; ++lane)
        pg::for_each_pair(lane, n, n * (n - 1) / 2, [&](int p, int a, int b) { std::printf("%d %d %d %d %d\n", n, lane, p, a, b); });
    return 0;
  }
  if (argc != 3 || std::strcmp(argv[1], "frames")) {
    std::fprintf(stderr, "usage: %s pairs N | frames cases.txt\n", argv[0]);
    return 2;
  }
  std::FILE* fh = std::fopen(argv[2], "r");
  if (!fh) {
    std::perror(argv[2]);
    return 2;
  }
  int F, B, n_lig, n_half, n_point, n_out;
  while (std::fscanf(fh, "%d %d %d %d %d %d", &F, &B, &n_lig, &n_half, &n_point, &n_out) == 6) {
    if (F < 0 || B < 1 || n_lig < 0 || n_half < 0 || n_point < 0 || n_out < 0) return 3;   // (what the entry points refuse)
    std::vector<int> lig_off(B + 1), bond_off(B + 1), range(2 * B), out_off(B + 1);
    if (!read_ints(fh, lig_off) || !read_ints(fh, bond_off) || !read_ints(fh, range) || !read_ints(fh, out_off)) return 3;
    for (unsigned block = 0; block < (unsigned)(F * B); ++block) {
      pg::MolFrame m;
      if (!pg::mol_frame(m, block, B, lig_off.data(), bond_off.data(), n_lig, n_half)) {
        std::printf("0\n");
        continue;
      }
      std::printf("1 %d %d %d %d %d %d %zu %zu", m.f, m.g, m.a0, m.n, m.h0, m.n_pair, m.arow, m.hrow);
      pg::MolPoints q;
      if (pg::mol_points(q, m, range.data(), out_off.data(), n_point, n_out))
        std::printf(" 1 %d %d %d %zu\n", q.ps, q.pe, q.o0, q.orow);
      else
        std::printf(" 0\n");
    }
  }
  std::fclose(fh);
  return 0;
}
