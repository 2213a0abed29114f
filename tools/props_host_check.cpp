// The rules of the property descriptors (phoregen_amd/csrc/props_core.h) -- the text the kernel of csrc/mol_props.hip compiles for the
// device -- compiled for the host, so that they can run under the host sanitizers and be held against the tests' restatement without
// a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/props_host_check.cpp -o props_host_check
//   ./props_host_check cases.txt > results.txt
//
// (tests/props_reference.py writes the cases and the expected lines; tests/test_molprops_host.py does all three steps.)
//
// cases.txt: per case a line `n n_rows n_tables max_violations kekule_status`; n quadruples `cls hcount charge atom_ring`; n_rows
// quintuples `a b order kekule_order ring_size` (a < b); per table its row count and its rows `mask value atom per_h`; the
// PG_PROP_N_LIMITS pairs `lo hi`.  Per case three lines come out: status, violated, weight_milli, the four sums and the sixteen
// counts; the word of every atom; the row of every atom, table after table.  Where the kernel has a lane per atom and a wave sum, this
// walks the atoms; the arrays are exactly as long as the graph needs, so an access outside them is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/mol_common.h"
#include "../phoregen_amd/csrc/props_core.h"

static const int kWeights[PG_PROP_N_WEIGHTS] = {10810, 12011, 14007, 15999, 18998, 28085, 30974, 32060, 35450, 79904, 126904, 1008};

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
  int n, n_rows, n_tables, max_violations, kek_status;
  while (std::fscanf(fh, "%d %d %d %d %d", &n, &n_rows, &n_tables, &max_violations, &kek_status) == 5) {
    if (n < 0 || n > PG_MOL_MAX_ATOMS || n_rows < 0 || n_tables < 0 || n_tables > PG_PROP_MAX_TABLES || max_violations < 0) return 3;
    std::vector<int8_t> el(n), q(n);
    std::vector<uint8_t> h(n), aring(n);
    for (int i = 0; i < n; ++i) {
      int c, hh, qq, ar;
      if (std::fscanf(fh, "%d %d %d %d", &c, &hh, &qq, &ar) != 4 || hh < 0 || hh > 255 || qq < -128 || qq > 127 || ar < 0 || ar > 255) return 3;
      const int k = pg::mol_class(c);
      el[i] = (int8_t)k, h[i] = (uint8_t)(k >= 0 ? hh : 0), q[i] = (int8_t)(k >= 0 ? qq : 0), aring[i] = (uint8_t)(k >= 0 ? ar : 0);
    }
    const int n_pair = n * (n - 1) / 2;
    std::vector<uint8_t> pair(n_pair, 0);
    std::vector<unsigned long long> adj(2 * (size_t)n, 0ull);
    for (int r = 0; r < n_rows; ++r) {
      int a, b, o, k, rs;
      if (std::fscanf(fh, "%d %d %d %d %d", &a, &b, &o, &k, &rs) != 5 || a < 0 || a >= b || b >= n) return 3;
      if (pg::mol_is_bond(o) && el[a] >= 0 && el[b] >= 0) {
        pair[a * n - a * (a + 1) / 2 + b - a - 1] = (uint8_t)pg::prop_pair_byte(o, k, rs);
        adj[2 * a + (b >> 6)] |= 1ull << (b & 63), adj[2 * b + (a >> 6)] |= 1ull << (a & 63);
      }
    }
    std::vector<std::vector<int>> tables(n_tables);
    for (auto& t : tables) {
      int rows;
      if (std::fscanf(fh, "%d", &rows) != 1 || rows < 0 || rows > PG_PROP_MAX_ROWS) return 3;
      t.resize((size_t)rows * PG_PROP_ROW_INTS);
      for (auto& x : t)
        if (std::fscanf(fh, "%d", &x) != 1) return 3;
    }
    int lim[2 * PG_PROP_N_LIMITS];
    for (auto& x : lim)
      if (std::fscanf(fh, "%d", &x) != 1) return 3;

    const bool kek_ok = (kek_status & PG_KEKULE_FAILED) == 0;
    std::vector<int> env(n, -1), own(n, -1);
    std::vector<int> row((size_t)PG_PROP_MAX_TABLES * n, 255);
    int cnt[PG_PROP_N_COUNTS] = {0}, sum[PG_PROP_MAX_TABLES] = {0}, weight = 0, viol = 0;
    if (kek_ok) {
      pg::PropGraph g = {n, el.data(), h.data(), q.data(), aring.data(), adj.data(), pair.data(), own.data()};
      for (int i = 0; i < n; ++i) own[i] = pg::prop_env_own(g, i);
      for (int i = 0; i < n; ++i) env[i] = own[i] >= 0 ? own[i] | pg::prop_env_nbr(g, i) : -1;
      for (int i = 0; i < n; ++i) {
        if (env[i] < 0) continue;
        pg::prop_atom_counts(env[i], h[i], q[i], cnt);
        weight += kWeights[pg::prop_el(env[i])] + h[i] * kWeights[PG_PROP_N_WEIGHTS - 1];
        for (int t = 0; t < n_tables; ++t) {
          const int r = pg::prop_match(tables[t].data(), (int)tables[t].size() / PG_PROP_ROW_INTS, env[i]);
          if (r >= 0) {
            sum[t] += pg::prop_contribution(tables[t].data() + PG_PROP_ROW_INTS * r, h[i]);
            row[(size_t)t * n + i] = r;
          } else {
            ++cnt[PG_PROP_C_UNTYPED];
          }
        }
      }
      for (int a = 0, p = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b, ++p)
          if (pair[p] & pg::kPropBond) {
            const int kind = pg::prop_bond_kind(pair[p], env[a], env[b]);
            cnt[PG_PROP_C_ROTATABLE] += kind == 1;
            cnt[PG_PROP_C_AMIDE_BONDS] += kind == 2;
          }
      int v[PG_PROP_N_LIMITS] = {weight, cnt[PG_PROP_C_HEAVY_ATOMS], cnt[PG_PROP_C_NHOH], cnt[PG_PROP_C_NO_COUNT], cnt[PG_PROP_C_ROTATABLE]};
      for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) v[PG_PROP_L_SUM0 + t] = sum[t];
      viol = pg::prop_violated(v, lim);
      cnt[PG_PROP_C_VIOLATIONS] = pg::prop_popc((unsigned int)viol);
    }
    std::printf("%d %d %d", pg::prop_status(kek_ok, viol, max_violations, cnt[PG_PROP_C_UNTYPED]), viol, weight);
    for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) std::printf(" %d", sum[t]);
    for (int k = 0; k < PG_PROP_N_COUNTS; ++k) std::printf(" %d", cnt[k]);
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%s%d", i ? " " : "", env[i]);
    std::printf("\n");
    for (size_t k = 0; k < row.size(); ++k) std::printf("%s%d", k ? " " : "", row[k]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
