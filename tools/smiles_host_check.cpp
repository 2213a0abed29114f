// The SMILES core (phoregen_amd/csrc/smiles_core.h: the text the kernel of csrc/mol_smiles.hip compiles for the device) compiled for
// the host together with mol_common.h's host part, so that it can run under the host sanitizers and be held against the tests'
// restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/smiles_host_check.cpp -o smiles_host_check
//   ./smiles_host_check cases.txt > results.txt
//
// (tests/smiles_reference.py writes the cases and reads the results; tests/test_molsmiles_host.py does all three steps.)
//
// cases.txt: one line with the notation's valence table (44 numbers: four per element, zero-padded), then per case a line
// `n capacity kekule_status n_rows`, a line with the n atom classes (-1 = dropped), a line with the n hydrogen counts, a line with the
// n charges and a line with n_rows triples `a b order` (a < b; the Kekulé order).  Per case three lines come out: `status length` and
// the eight counts; the text (an empty line without one); the n ranks.  The program follows the kernel step by step: the pairs are
// dealt by for_each_pair, lane by lane; the traversal and the labels are the core's; every atom's text is counted, the counts are
// summed in preorder, and the text is written into a row of exactly `capacity` bytes.  The work arrays are exactly as large as the
// core's contract says, so an access outside it is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/mol_common.h"
#include "../phoregen_amd/csrc/smiles_core.h"

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
  std::vector<uint8_t> val(4 * pg::kSmiEl);
  for (auto& t : val) {
    int x;
    if (std::fscanf(fh, "%d", &x) != 1 || x < 0 || x > 255) return 3;
    t = (uint8_t)x;
  }
  int n, capacity, kstatus, n_rows;
  while (std::fscanf(fh, "%d %d %d %d", &n, &capacity, &kstatus, &n_rows) == 4) {
    if (n < 0 || n > pg::kMolMax || capacity < 1 || n_rows < 0) return 3;
    std::vector<int> cls(n), h(n), q(n);
    for (auto& c : cls)
      if (std::fscanf(fh, "%d", &c) != 1 || c < -1 || c > 10) return 3;
    for (auto& x : h)
      if (std::fscanf(fh, "%d", &x) != 1 || x < 0 || x > 255) return 3;
    for (auto& x : q)
      if (std::fscanf(fh, "%d", &x) != 1 || x < -128 || x > 127) return 3;
    const int n_pair = n * (n - 1) / 2;
    std::vector<int8_t> kek(n_pair, 0);
    for (int r = 0; r < n_rows; ++r) {
      int a, b, o;
      if (std::fscanf(fh, "%d %d %d", &a, &b, &o) != 3 || a < 0 || a >= b || b >= n || o < -128 || o > 127) return 3;
      kek[pg::smi_pair(n, a, b)] = (int8_t)o;
    }
    std::vector<uint8_t> text(capacity, 0xAA);                        // (the row is written whole: no 0xAA may be left)
    std::vector<int16_t> rank(n, -1), order(n), parent(n, -1), stack(n);
    std::vector<uint8_t> flags(n, 0), label(n_pair);
    std::vector<int> len(n, 0), cnt(8, 0);
    int status = 0, length = 0;
    if (kstatus & PG_KEKULE_FAILED) {
      status = PG_SMILES_NO_KEKULE;
      for (auto& t : text) t = 0;
    } else {
      // ---- the bonds, dealt as the wave deals them ----
      std::vector<unsigned long long> p0(2 * n, 0ull), p1(2 * n, 0ull);
      unsigned long long kept[2] = {0ull, 0ull};
      int n_kept = 0, n_bond = 0;
      for (int i = 0; i < n; ++i)
        if (pg::mol_class(cls[i]) >= 0) {
          kept[i >> 6] |= 1ull << (i & 63);
          ++n_kept;
        }
      for (int lane = 0; lane < 64; ++lane)
        pg::for_each_pair(lane, n, n_pair, [&](int p, int a, int b) {
          const int o = kek[p];
          if (o >= 1 && o <= 3 && cls[a] >= 0 && cls[b] >= 0) {
            ++n_bond;
            if (o & 1) p0[2 * a + (b >> 6)] |= 1ull << (b & 63), p0[2 * b + (a >> 6)] |= 1ull << (a & 63);
            if (o & 2) p1[2 * a + (b >> 6)] |= 1ull << (b & 63), p1[2 * b + (a >> 6)] |= 1ull << (a & 63);
          }
        });
      int comps = 0, branches = 0, closures = 0;
      const int seen = pg::smiles_tree(n, p0.data(), p1.data(), kept[0], kept[1], rank.data(), order.data(), parent.data(), flags.data(),
                                       stack.data(), &comps, &branches);
      if (seen != n_kept) return 4;
      const int max_label = pg::smiles_labels(n, seen, p0.data(), p1.data(), rank.data(), order.data(), parent.data(), label.data(), &closures);
      if (max_label == pg::kSmiLabelOverflow) {
        status = PG_SMILES_RING_LABELS;
        for (auto& t : text) t = 0;
        for (auto& r : rank) r = -1;
      } else {
        // ---- count, sum in preorder, write ----
        int n_bracket = 0;
        for (int i = 0; i < n; ++i) {
          if (cls[i] < 0) continue;
          int k = 0;
          n_bracket += pg::smiles_atom_text(i, n, cls[i], h[i], q[i], &val[4 * cls[i]], p0.data(), p1.data(), rank.data(), parent.data(),
                                            flags.data(), label.data(), [&](char) { ++k; });
          len[rank[i]] = k;
        }
        int need = 0;
        for (int k = 0; k < n_kept; ++k) {
          const int l = len[k];
          len[k] = need;
          need += l;
        }
        const bool fits = need <= capacity;
        if (fits)
          for (int i = 0; i < n; ++i) {
            if (cls[i] < 0) continue;
            uint8_t* at = text.data() + len[rank[i]];
            pg::smiles_atom_text(i, n, cls[i], h[i], q[i], &val[4 * cls[i]], p0.data(), p1.data(), rank.data(), parent.data(), flags.data(),
                                 label.data(), [&](char ch) { *at++ = (uint8_t)ch; });
          }
        else
          for (auto& r : rank) r = -1;
        for (int i = fits ? need : 0; i < capacity; ++i) text[i] = 0;
        status = (fits ? 0 : PG_SMILES_TOO_LONG) | (comps > 1 ? PG_SMILES_DISCONNECTED : 0) | (n_kept == 0 ? PG_SMILES_EMPTY : 0) |
                 (n_bracket > 0 ? PG_SMILES_BRACKET : 0);
        length = fits ? need : 0;
        cnt = {need, n_kept, n_bond, comps, closures, branches, max_label, n_bracket};
      }
    }
    std::printf("%d %d", status, length);
    for (int c : cnt) std::printf(" %d", c);
    std::printf("\n");
    for (int i = 0; i < capacity; ++i) {
      if (i < length && (text[i] < 0x21 || text[i] > 0x7e)) return 5;  // ASCII, nothing that would break the line
      if (i >= length && text[i] != 0) return 6;                       // zeros from `length` on
      if (i < length) std::fputc(text[i], stdout);
    }
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)rank[i]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
