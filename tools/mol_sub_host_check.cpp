// The core of the substructure search (phoregen_amd/csrc/sub_core.h) compiled for the host, for tests/test_molsub_host.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mol_sub_host_check.cpp -o mol_sub_host_check
//   mol_sub_host_check cases.txt
// The same text the kernel compiles (the row checks, the property word and the constraint test, the candidate step, the search from a
// root), driven as mol_sub.hip drives it: one store per lane, root r on lane r mod 64, the lanes' results merged as the kernel merges
// them.  Reads cases, prints one line per case.  A case is
//   n n_bonds max_steps kekule_failed
//   n lines:        class hcount charge in_ring      (the kept atoms in compact numbering)
//   n_bonds lines:  a b order ring_bond
//   one line:       the PG_SUB_PATTERN_BYTES bytes of the pattern row
// and its answer `check embeddings anchors mask0 mask1 status first[16]`, check = sub_row_check's code (the rest zero / -1 if not 0).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/sub_core.h"

using namespace pg;

namespace {

struct HostStore {
  SubMask (*adj_)[kSubTargetMax];
  const SubMask* compat_;
  const unsigned* back_;
  unsigned char (*classes_)[kSubMaxAtoms];
  SubMask stack_[kSubMaxAtoms];
  int map_[kSubMaxAtoms], first_[kSubMaxAtoms];

  static int level(int d) {
    if (d < 0 || d >= kSubMaxAtoms) abort();
    return d;
  }
  static int atom(int t) {
    if (t < 0 || t >= kSubTargetMax) abort();
    return t;
  }
  SubMask compat(int d) const { return compat_[level(d)]; }
  unsigned back(int d) const { return back_[level(d)]; }
  unsigned classes(int d, int e) const { return classes_[level(d)][level(e)]; }
  SubMask adj(int c, int t) const {
    if (c < 0 || c >= kSubClasses) abort();
    return adj_[c][atom(t)];
  }
  int image(int d) const { return map_[level(d)]; }
  void set_image(int d, int t) { map_[level(d)] = atom(t); }
  SubMask cand(int d) const { return stack_[level(d)]; }
  void set_cand(int d, const SubMask& m) { stack_[level(d)] = m; }
  void save_first(int k, int last) {
    for (int d = 0; d + 1 < k; ++d) first_[level(d)] = map_[level(d)];
    first_[level(k - 1)] = atom(last);
  }
};

int read_int(FILE* fh) {
  long long v;
  if (fscanf(fh, "%lld", &v) != 1) {
    fprintf(stderr, "mol_sub_host_check: the case file ends early\n");
    exit(2);
  }
  return (int)v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: mol_sub_host_check cases.txt\n");
    return 2;
  }
  FILE* fh = fopen(argv[1], "r");
  if (!fh) {
    perror(argv[1]);
    return 2;
  }
  const int n_cases = read_int(fh);
  static SubMask adj[kSubClasses][kSubTargetMax];
  for (int cs = 0; cs < n_cases; ++cs) {
    const int n = read_int(fh), n_bonds = read_int(fh), max_steps = read_int(fh), kekule_failed = read_int(fh);
    if (n < 0 || n > kSubTargetMax || n_bonds < 0 || max_steps < 1) {
      fprintf(stderr, "mol_sub_host_check: case %d is out of range\n", cs);
      return 2;
    }
    std::vector<int> cls(n), hcount(n), charge(n), in_ring(n), degree(n, 0), aromatic(n, 0);
    for (int i = 0; i < n; ++i) cls[i] = read_int(fh), hcount[i] = read_int(fh), charge[i] = read_int(fh), in_ring[i] = read_int(fh);
    for (int c = 0; c < kSubClasses; ++c)
      for (int i = 0; i < kSubTargetMax; ++i) adj[c][i] = SubMask{{0ull, 0ull}};
    for (int e = 0; e < n_bonds; ++e) {
      const int a = read_int(fh), b = read_int(fh), o = read_int(fh), ring = read_int(fh);
      if (a < 0 || a >= n || b < 0 || b >= n || a == b || o < 1 || o > 4) {
        fprintf(stderr, "mol_sub_host_check: case %d, bond %d is out of range\n", cs, e);
        return 2;
      }
      const int c = sub_bond_class(o, ring != 0);
      sub_mask_set(adj[c][a], b);
      sub_mask_set(adj[c][b], a);
      ++degree[a], ++degree[b];
      aromatic[a] |= o == 4, aromatic[b] |= o == 4;
    }
    std::vector<uint8_t> row(PG_SUB_PATTERN_BYTES);
    for (auto& v : row) v = (uint8_t)read_int(fh);

    const int check = sub_row_check(row.data());
    sub_u64 embeddings = 0;
    SubMask mask = {{0ull, 0ull}}, anchor = {{0ull, 0ull}};
    int first[kSubMaxAtoms], status = 0;
    for (int& v : first) v = -1;
    if (check == kSubRowOk) {
      const int k = sub_row_k(row.data());
      const bool uses_kekule = sub_row_uses_kekule(row.data(), k);
      const bool no_kekule = uses_kekule && kekule_failed;
      bool truncated = false;
      if (!no_kekule) {
        SubMask compat[kSubMaxAtoms];
        unsigned back[kSubMaxAtoms];
        unsigned char classes[kSubMaxAtoms][kSubMaxAtoms];
        for (int d = 0; d < kSubMaxAtoms; ++d) {
          compat[d] = SubMask{{0ull, 0ull}}, back[d] = 0u;
          for (int e = 0; e < kSubMaxAtoms; ++e) classes[d][e] = 0;
        }
        for (int d = 1; d < k; ++d)
          for (int e = 0; e < d; ++e) {
            classes[d][e] = (unsigned char)sub_class_mask(sub_row_bond(row.data(), sub_row_order(row.data(), d), sub_row_order(row.data(), e)));
            back[d] |= classes[d][e] ? 1u << e : 0u;
          }
        for (int i = 0; i < n; ++i) {
          const uint32_t prop = sub_prop_pack(cls[i], degree[i], uses_kekule ? hcount[i] : 0, uses_kekule && charge[i] != 0, in_ring[i] != 0,
                                              aromatic[i] != 0);
          for (int d = 0; d < k; ++d)
            if (sub_atom_ok(sub_row_atom(row.data(), sub_row_order(row.data(), d)), prop)) sub_mask_set(compat[d], i);
        }
        unsigned min_root = 0xffffffffu;
        int min_first[kSubMaxAtoms] = {0};
        for (int lane = 0; lane < 64; ++lane) {
          HostStore st = {adj, compat, back, classes, {}, {}, {}};
          SubFound found = {0ull, {{0ull, 0ull}}, false, false};
          unsigned first_root = 0xffffffffu;
          for (int c = 0; c < 2; ++c) {
            const int root = c * 64 + lane;
            if (!sub_mask_has(compat[0], root)) continue;
            const bool had = found.have_first;
            if (sub_search_root(st, k, root, (sub_u64)max_steps, found)) sub_mask_set(anchor, root);
            if (!had && found.have_first) first_root = (unsigned)root;
          }
          embeddings += found.embeddings;
          mask.w[0] |= found.atoms.w[0], mask.w[1] |= found.atoms.w[1];
          truncated = truncated || found.truncated;
          if (found.have_first && first_root < min_root) {
            min_root = first_root;
            for (int d = 0; d < k; ++d) min_first[d] = st.first_[d];
          }
        }
        if (min_root != 0xffffffffu)
          for (int d = 0; d < k; ++d) first[sub_row_order(row.data(), d)] = min_first[d];
      }
      const int anchors = __builtin_popcountll(anchor.w[0]) + __builtin_popcountll(anchor.w[1]);
      status = sub_status(embeddings, anchors, no_kekule, truncated, sub_row_int(row.data(), PG_SUB_OFF_MIN), sub_row_int(row.data(), PG_SUB_OFF_MAX));
    }
    printf("%d %d %d %llu %llu %d", check, sub_saturate(embeddings), __builtin_popcountll(anchor.w[0]) + __builtin_popcountll(anchor.w[1]),
           mask.w[0], mask.w[1], status);
    for (int v : first) printf(" %d", v);
    printf("\n");
  }
  fclose(fh);
  return 0;
}
