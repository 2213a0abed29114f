// The Kekulé core (phoregen_amd/csrc/kekule_core.h: the text the kernel of csrc/mol_kekule.hip compiles for the device) compiled for
// the host, so that it can run under the host sanitizers and be held against the tests' restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kekule_host_check.cpp -o kekule_host_check
//   ./kekule_host_check cases.txt > results.txt
//
// (tests/kekule_reference.py writes the cases and reads the results; tests/test_molkekule_host.py does all three steps.)
//
// cases.txt: four lines with the tables (11, 11, 11 and 44 numbers: DBL_NEUTRAL, DBL_CHARGED, MUST, H_VALENCES zero-padded to four per
// element), then per case a line `n allow_charged n_rows`, a line with the n atom classes (-1 = dropped) and a line with n_rows
// triples `a b order` (a < b).  Per case three lines come out: `status` and the ten counts; one Kekulé order per triple, in order;
// `h q` per atom.  The work arrays are exactly as large as the core's contract says, so an access outside it is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/kekule_core.h"

struct Row {
  int a, b, o;
};

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
  std::vector<uint8_t> tab(33 + 44);
  for (auto& t : tab) {
    int x;
    if (std::fscanf(fh, "%d", &x) != 1 || x < 0 || x > 255) return 3;
    t = (uint8_t)x;
  }
  const uint8_t *neutral = tab.data(), *charged = neutral + 11, *must = charged + 11, *hval = must + 11;
  int n, allow, n_rows;
  while (std::fscanf(fh, "%d %d %d", &n, &allow, &n_rows) == 3) {
    if (n < 0 || n > 128 || n_rows < 0) return 3;
    std::vector<int> cls(n);
    for (auto& c : cls)
      if (std::fscanf(fh, "%d", &c) != 1 || c < -1 || c > 10) return 3;
    std::vector<Row> rows(n_rows);
    for (auto& r : rows)
      if (std::fscanf(fh, "%d %d %d", &r.a, &r.b, &r.o) != 3 || r.a < 0 || r.a >= r.b || r.b >= n) return 3;
    std::vector<int> s(n, 0), a(n, 0);
    std::vector<unsigned long long> arom(2 * n, 0ull), allowed(2 * n, 0ull);
    int n_arom_bond = 0;
    for (const Row& r : rows) {
      if (r.o < 1 || r.o > 4 || cls[r.a] < 0 || cls[r.b] < 0) continue;
      if (r.o == 4) {
        ++n_arom_bond;
        ++a[r.a], ++a[r.b];
        arom[2 * r.a + (r.b >> 6)] |= 1ull << (r.b & 63);
        arom[2 * r.b + (r.a >> 6)] |= 1ull << (r.a & 63);
      } else {
        s[r.a] += r.o, s[r.b] += r.o;
      }
    }
    std::vector<uint8_t> kind(n), flags(n);
    std::vector<int16_t> match(2 * n), parent(2 * n), base(n), queue(n);
    int feasible = 1, pass_used = 0, n_arom = 0, n_must = 0;
    for (int pass = 0; pass < 2; ++pass) {
      unsigned long long ok[2] = {0ull, 0ull};
      n_arom = n_must = 0;
      for (int i = 0; i < n; ++i) {
        int k = pg::kKekNone;
        if (cls[i] >= 0) {
          const int cap = pass == 0 ? neutral[cls[i]] : (neutral[cls[i]] > charged[cls[i]] ? neutral[cls[i]] : charged[cls[i]]);
          k = pg::kekule_kind(s[i], a[i], cap, must[cls[i]]);
        }
        kind[i] = (uint8_t)k;
        n_arom += k != pg::kKekNone;
        n_must += k == pg::kKekMust;
        if (k >= pg::kKekMay) ok[i >> 6] |= 1ull << (i & 63);
      }
      for (int i = 0; i < n; ++i)
        for (int w = 0; w < 2; ++w) allowed[2 * i + w] = kind[i] >= pg::kKekMay ? arom[2 * i + w] & ok[w] : 0ull;
      for (auto& m : match) m = -1;
      feasible = pg::kekule_match(n, allowed.data(), kind.data(), match.data(), parent.data(), base.data(), queue.data(), flags.data());
      pass_used = pass;
      if (feasible || !allow) break;
    }
    int n_dbl2 = 0, n_may = 0, n_h = 0, n_q = 0, n_hbd = 0, n_hba = 0, n_kept = 0;
    std::vector<int> h(n, 0), q(n, 0);
    for (int i = 0; i < n; ++i) {
      if (cls[i] < 0) continue;
      ++n_kept;
      const int d = (feasible && match[i] >= 0) ? 1 : 0;
      pg::kekule_atom(cls[i] == 2, s[i], a[i], d, neutral[cls[i]], hval + 4 * cls[i], &h[i], &q[i]);
      n_dbl2 += d;
      n_may += d && kind[i] == pg::kKekMay;
      n_h += h[i], n_q += q[i];
      const bool no = cls[i] == 2 || cls[i] == 3;
      n_hbd += no && h[i] >= 1;
      n_hba += no;
    }
    const int st = (feasible ? 0 : 1) | ((feasible && pass_used == 1) ? 2 : 0) | (n_arom > 0 ? 4 : 0) | (n_q != 0 ? 8 : 0);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d\n", st, n_arom, n_arom_bond, n_dbl2 / 2, n_must, n_may, n_h, n_q, n_hbd, n_hba, n_kept);
    for (const Row& r : rows) {
      int o = r.o;
      if (feasible && o == 4 && cls[r.a] >= 0 && cls[r.b] >= 0) o = match[r.a] == r.b ? 2 : 1;
      std::printf("%d ", o);
    }
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%d %d ", h[i], q[i]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
