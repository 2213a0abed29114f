// The scaffold's selection logic (phoregen_amd/csrc/scaffold_core.h) and the ring search (phoregen_amd/csrc/ring_search.h) -- the text
// the kernel of csrc/mol_scaffold.hip compiles for the device -- compiled for the host, so that they can run under the host sanitizers
// and be held against the tests' restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scaffold_host_check.cpp -o scaffold_host_check
//   ./scaffold_host_check cases.txt > results.txt
//
// (tests/scaffold_reference.py writes the cases and the expected lines; tests/test_molscaffold_host.py does all three steps.)
//
// cases.txt: per case a line `n flags n_rows`, a line with the n atom classes (-1 = dropped) and a line with n_rows triples
// `a b order` (a < b).  Per case three lines come out: the status, the four screen counts and the eight scaffold counts; `part cls
// compact valence2 comp` per atom; the scaffold order of every triple, in order.  Where the kernel has a lane per atom and a wave-wide
// vote, this walks the atoms and collects the set; the arrays are exactly n long, so an access outside them is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/ring_search.h"
#include "../phoregen_amd/csrc/scaffold_core.h"

struct Row {
  unsigned long long w[pg::kMolCh];
};
struct Triple {
  int a, b, o;
};

static void set_bit(unsigned long long* set, int i) { set[i >> 6] |= 1ull << (i & 63); }
static void join(std::vector<Row>& adj, int a, int b) { set_bit(adj[a].w, b), set_bit(adj[b].w, a); }

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
  int n, flags, n_rows;
  while (std::fscanf(fh, "%d %d %d", &n, &flags, &n_rows) == 3) {
    if (n < 0 || n > PG_MOL_MAX_ATOMS || n_rows < 0 || flags < 0 || flags > 3) return 3;
    std::vector<int> cls(n);
    for (auto& c : cls)
      if (std::fscanf(fh, "%d", &c) != 1 || c < -1 || c > 10) return 3;
    std::vector<Triple> rows(n_rows);
    for (auto& r : rows)
      if (std::fscanf(fh, "%d %d %d", &r.a, &r.b, &r.o) != 3 || r.a < 0 || r.a >= r.b || r.b >= n) return 3;
    const Row none = {{0ull, 0ull}};
    std::vector<Row> adj(n, none), dbl(n, none), radj(n, none);
    unsigned long long kept[2] = {0ull, 0ull};
    for (int i = 0; i < n; ++i)
      if (pg::mol_class(cls[i]) >= 0) set_bit(kept, i);
    auto bond = [&](const Triple& r) { return pg::mol_is_bond(r.o) && pg::scaf_has(kept, r.a) && pg::scaf_has(kept, r.b); };
    for (const Triple& r : rows)
      if (bond(r)) {
        join(adj, r.a, r.b);
        if (r.o == 2) join(dbl, r.a, r.b);
      }
    // core: rounds of leaf removal, every test of a round on the same set
    unsigned long long core[2] = {kept[0], kept[1]};
    for (int round = 0; round <= n; ++round) {
      unsigned long long leaf[2] = {0ull, 0ull};
      for (int i = 0; i < n; ++i)
        if (pg::scaf_is_leaf(adj[i].w, core, i)) set_bit(leaf, i);
      if (!(leaf[0] | leaf[1])) break;
      core[0] &= ~leaf[0], core[1] &= ~leaf[1];
    }
    int n_linkb = 0;
    for (const Triple& r : rows)
      if (bond(r) && pg::scaf_has(core, r.a) && pg::scaf_has(core, r.b)) {
        if (pg::ring_through(adj.data(), r.a, r.b) > 0)
          join(radj, r.a, r.b);
        else
          ++n_linkb;
      }
    std::vector<int> part(n);
    unsigned long long ringm[2] = {0ull, 0ull}, exom[2] = {0ull, 0ull};
    for (int i = 0; i < n; ++i) {
      const bool k = pg::scaf_has(kept, i), in_core = pg::scaf_has(core, i);
      const bool exo = (flags & PG_SCAF_EXOCYCLIC) && pg::scaf_is_exocyclic(dbl[i].w, core, k, in_core);
      part[i] = pg::scaf_part(k, in_core, radj[i].w, exo);
      if (part[i] == PG_SCAF_PART_RING) set_bit(ringm, i);
      if (exo) set_bit(exom, i);
    }
    const unsigned long long sel[2] = {core[0] | exom[0], core[1] | exom[1]}, all[2] = {~0ull, ~0ull};
    std::vector<unsigned int> val(n, 0u), size(n, 0u);
    std::vector<int> so(n_rows, 0);
    int n_sbond = 0;
    for (int t = 0; t < n_rows; ++t) {
      const Triple& r = rows[t];
      if (bond(r) && pg::scaf_has(sel, r.a) && pg::scaf_has(sel, r.b)) {
        so[t] = pg::scaf_order(r.o, flags);
        ++n_sbond;
        val[r.a] += pg::scaf_valence2(so[t]), val[r.b] += pg::scaf_valence2(so[t]);
      }
    }
    std::vector<int> comp(n), sys(n);
    for (int i = 0; i < n; ++i) comp[i] = sys[i] = i;
    for (int round = 0; round <= n; ++round) {
      bool changed = false;
      for (int i = 0; i < n; ++i) {
        if (!pg::scaf_has(sel, i)) continue;
        const int lc = pg::scaf_min_label(adj[i].w, sel, comp.data(), comp[i]), ly = pg::scaf_min_label(radj[i].w, all, sys.data(), sys[i]);
        changed |= lc < comp[i] || ly < sys[i];
        comp[i] = lc, sys[i] = ly;
      }
      if (!changed) break;
    }
    int n_comp = 0, n_sys = 0, largest = 0;
    for (int i = 0; i < n; ++i) {
      if (!pg::scaf_has(sel, i)) continue;
      ++size[comp[i]];
      n_comp += comp[i] == i;
      n_sys += part[i] == PG_SCAF_PART_RING && sys[i] == i;
    }
    for (int i = 0; i < n; ++i) largest = (int)size[i] > largest ? (int)size[i] : largest;
    const int n_sel = pg::scaf_count(sel), n_ring = pg::scaf_count(ringm);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", (n_sel == 0 ? PG_MOL_NO_ATOMS : 0) | (n_comp > 1 ? PG_MOL_DISCONNECTED : 0), n_sel,
                n_sbond, n_comp, largest, n_sel, n_sbond, n_ring, pg::scaf_count(core) - n_ring, pg::scaf_count(exom),
                pg::scaf_count(kept) - n_sel, n_sys, n_linkb);
    for (int i = 0; i < n; ++i) {
      const bool in = pg::scaf_has(sel, i);
      std::printf("%s%d %d %d %u %d", i ? " " : "", part[i], in ? pg::scaf_class(cls[i], flags) : -1, in ? pg::scaf_compact(sel, i) : -1,
                  in ? (val[i] < 255u ? val[i] : 255u) : 0u, in ? comp[i] : -1);
    }
    std::printf("\n");
    for (int t = 0; t < n_rows; ++t) std::printf("%s%d", t ? " " : "", so[t]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
