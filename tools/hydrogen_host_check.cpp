// The hydrogen core (phoregen_amd/csrc/hydrogen_core.h: the shape rule and the direction arithmetic the kernel of csrc/mol_hydrogens.hip
// compiles for the device) compiled for the host together with mol_common.h's host part, so that it can run under the host sanitizers
// and be held against the tests' restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/hydrogen_host_check.cpp -o hydrogen_host_check
//   ./hydrogen_host_check cases.txt > results.txt
//
// (tests/hydrogen_reference.py writes the cases and reads the results; tests/test_molhydrogens_host.py does all three steps.)
//
// cases.txt: one line with the eleven X-H lengths, one line `clash_min max_contacts` (floats in C's hexadecimal form), then per case
// a line `n kekule_status n_rows`, n lines `class hydrogens x y z` and n_rows lines `a b order kekule_order` (a < b).  Per case three
// lines come out: `status min_contact` and the eight counts; the n pairs `h_placed site_shape`; the 12 n coordinates of h_pos.  The
// program follows the kernel step by step: the atoms one by one, the pairs into the adjacency words and the bond bits, the sites by
// hyd_site, the contacts hydrogen by hydrogen; the work arrays are exactly as large as the graph.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/hydrogen_core.h"

static bool read_float(std::FILE* fh, float* x) {
  char word[64];
  if (std::fscanf(fh, "%63s", word) != 1) return false;
  *x = std::strtof(word, nullptr);
  return true;
}

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
  std::vector<float> xh(11);
  for (auto& v : xh)
    if (!read_float(fh, &v)) return 3;
  float clash_min;
  int max_contacts;
  if (!read_float(fh, &clash_min) || std::fscanf(fh, "%d", &max_contacts) != 1) return 3;
  int n, kstatus, n_rows;
  while (std::fscanf(fh, "%d %d %d", &n, &kstatus, &n_rows) == 3) {
    if (n < 0 || n > pg::kMolMax || n_rows < 0) return 3;
    std::vector<pg::HydAtom> atoms(n);
    std::vector<unsigned long long> adj(2 * (size_t)n, 0ull);
    bool nonfinite = false, too_many = false;
    int kept = 0;
    for (int i = 0; i < n; ++i) {
      int cls, h;
      float x, y, z;
      if (std::fscanf(fh, "%d %d", &cls, &h) != 2 || cls < -1 || cls > 11 || h < 0 || h > 255) return 3;
      if (!read_float(fh, &x) || !read_float(fh, &y) || !read_float(fh, &z)) return 3;
      const int k = pg::mol_class(cls);
      const bool bad = k >= 0 && !(std::isfinite(x) && std::isfinite(y) && std::isfinite(z));
      const unsigned hh = k >= 0 ? (unsigned)h : 0u;
      atoms[i] = {x, y, z, (k >= 0 ? (unsigned)k : pg::kHydDropped) | (bad ? pg::kHydNonfinite : 0u) | hh << pg::kHydHShift};
      nonfinite = nonfinite || bad;
      too_many = too_many || hh > (unsigned)pg::kHydMaxH;
      kept += k >= 0;
    }
    for (int r = 0; r < n_rows; ++r) {
      int a, b, o, ko;
      if (std::fscanf(fh, "%d %d %d %d", &a, &b, &o, &ko) != 4 || a < 0 || a >= b || b >= n) return 3;
      if ((atoms[a].info & 15u) == pg::kHydDropped || (atoms[b].info & 15u) == pg::kHydDropped) continue;
      const unsigned flags = (o == 4 ? pg::kHydArom : 0u) | (ko == 3 ? pg::kHydTriple : 0u);
      if (ko >= 1 && ko <= 3) {
        adj[2 * a + (b >> 6)] |= 1ull << (b & 63);
        adj[2 * b + (a >> 6)] |= 1ull << (a & 63);
      }
      atoms[a].info |= flags, atoms[b].info |= flags;
      if (ko == 2) atoms[a].info += 1u << pg::kHydDoubleShift, atoms[b].info += 1u << pg::kHydDoubleShift;
    }
    int counts[PG_HYD_N_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0}, status = 0;
    float min_contact = INFINITY;
    std::vector<pg::HydOut> out(n);
    std::vector<int> placed(n, 0), shape(n, 0);
    const pg::HydVec zero = {0.0f, 0.0f, 0.0f};
    for (auto& o : out) o = {zero, zero, zero, zero};
    if (kstatus & PG_KEKULE_FAILED) {
      status = PG_HYD_NO_KEKULE;
      min_contact = 0.0f;
    } else {
      struct Placed {
        pg::HydVec p;
        int parent;
      };
      std::vector<Placed> hs;
      for (int i = 0; i < n && !too_many; ++i) {
        placed[i] = pg::hyd_site(atoms.data(), adj.data(), i, xh.data(), out[i], shape[i]);
        const pg::HydVec slot[4] = {out[i].h0, out[i].h1, out[i].h2, out[i].h3};
        for (int k = 0; k < placed[i]; ++k) hs.push_back({slot[k], i});
        counts[0] += placed[i], counts[1] += placed[i] > 0;
        if (shape[i]) ++counts[1 + shape[i]];
      }
      for (size_t q = 0; q < hs.size(); ++q) {
        for (int j = 0; j < n; ++j) {
          if ((atoms[j].info & 15u) == pg::kHydDropped || j == hs[q].parent) continue;
          const float d = pg::hyd_dist(hs[q].p, pg::hv_of(atoms[j]));
          counts[6] += d < clash_min;
          min_contact = fminf(min_contact, d);
        }
        for (size_t r = q + 1; r < hs.size(); ++r) {
          if (hs[r].parent == hs[q].parent) continue;
          const float d = pg::hyd_dist(hs[q].p, hs[r].p);
          counts[6] += d < clash_min;
          min_contact = fminf(min_contact, d);
        }
      }
      counts[7] = kept;
      status |= nonfinite ? PG_HYD_NONFINITE : 0;
      status |= too_many ? PG_HYD_TOO_MANY : 0;
      status |= counts[6] > max_contacts ? PG_HYD_CONTACTS : 0;
      status |= counts[5] > 0 ? PG_HYD_GENERIC : 0;
      status |= counts[0] > 0 ? PG_HYD_HAS_HYDROGEN : 0;
    }
    std::printf("%d %a", status, (double)min_contact);
    for (int c : counts) std::printf(" %d", c);
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%d %d ", placed[i], shape[i]);
    std::printf("\n");
    for (int i = 0; i < n; ++i) {
      const pg::HydVec slot[4] = {out[i].h0, out[i].h1, out[i].h2, out[i].h3};
      for (const auto& v : slot) std::printf("%a %a %a ", (double)v.x, (double)v.y, (double)v.z);
    }
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
