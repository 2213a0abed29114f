// The feature rules (phoregen_amd/csrc/feature_core.h: the text the kernel of csrc/mol_feat.hip compiles for the device) compiled for
// the host, so that they can run under the host sanitizers and be held against the tests' restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/feature_host_check.cpp -o feature_host_check
//   ./feature_host_check cases.txt > results.txt
//
// (tests/feature_reference.py writes the cases and reads the results; tests/test_molfeat_host.py does all three steps.)
//
// cases.txt: per case a line `n n_rows`, a line with n triples `class h q` (class -1 = dropped) and a line with n_rows quintuples
// `a b order kekule_order ring_size` (a < b; the pair rows that are not listed are no bonds).  Per case one line comes out: the n atom
// bytes.  The arrays are exactly as large as the core's contract says, so an access outside it is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/feature_core.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  int n, n_rows;
  while (std::fscanf(fh, "%d %d", &n, &n_rows) == 2) {
    if (n < 0 || n > 128 || n_rows < 0) return 3;
    std::vector<int8_t> el(n);
    std::vector<uint8_t> h(n), q(n), deg(n), flags(n), pair((size_t)n * (n > 0 ? n - 1 : 0) / 2, 0);
    std::vector<uint16_t> v(n);
    std::vector<unsigned long long> adj(2 * (size_t)n, 0ull);
    for (int i = 0; i < n; ++i) {
      int c, hh, qq;
      if (std::fscanf(fh, "%d %d %d", &c, &hh, &qq) != 3 || c < -1 || c > 10 || hh < 0 || hh > 255 || qq < 0 || qq > 1) return 3;
      el[i] = (int8_t)c, h[i] = (uint8_t)(c >= 0 ? hh : 0), q[i] = (uint8_t)(c >= 0 ? qq : 0);
    }
    for (int r = 0; r < n_rows; ++r) {
      int a, b, o, k, rs;
      if (std::fscanf(fh, "%d %d %d %d %d", &a, &b, &o, &k, &rs) != 5 || a < 0 || a >= b || b >= n) return 3;
      if (o < 1 || o > 4 || el[a] < 0 || el[b] < 0) continue;
      pair[(size_t)a * n - (size_t)a * (a + 1) / 2 + b - a - 1] =
          (uint8_t)(((k >= 1 && k <= 3) ? k : 1) | (o == 4 ? pg::kPairArom : 0) | (rs > 0 ? pg::kPairRing : 0));
      adj[2 * a + (b >> 6)] |= 1ull << (b & 63);
      adj[2 * b + (a >> 6)] |= 1ull << (a & 63);
    }
    const pg::FeatGraph g = {n, el.data(), h.data(), q.data(), adj.data(), pair.data(), deg.data(), v.data(), flags.data()};
    for (int i = 0; i < n; ++i) {
      int d, vv, ar;
      pg::feat_atom_sums(g, i, &d, &vv, &ar);
      deg[i] = (uint8_t)d, v[i] = (uint16_t)vv, flags[i] = (uint8_t)(ar ? pg::kAtomArom : 0);
    }
    std::vector<int> dbl(n);
    for (int i = 0; i < n; ++i) dbl[i] = pg::feat_atom_dbl(g, i);
    for (int i = 0; i < n; ++i) flags[i] = (uint8_t)(flags[i] | dbl[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", pg::feat_atom_bits(g, i));
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
