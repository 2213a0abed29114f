// The selection logic of the Murcko scaffold (DESIGN.md 2.9 "Scaffolds"): the leaf test of the pruning, the part of an atom, the
// exocyclic rule, an atom's index among the scaffold atoms, a scaffold bond's order and valence, and the label step of the
// components.  Plain functions over mask words -- a set of atoms is kScafWords words, bit i & 63 of word i >> 6 = atom i, as an
// adjacency row is -- compiled for the device by mol_scaffold.hip (a lane calls them for each of its atoms, the sets come from wave-wide
// votes) and for the host by tools/scaffold_host_check.cpp (the same text under the host sanitizers, atom after atom).  Integer work
// only; no loop here depends on what the arrays hold beyond the 64 bits of a word.
#pragma once
#include <stdint.h>
#include "../../include/phoregen_hip.h"

#if defined(__HIPCC__)
#define PG_SCAF_HD __host__ __device__ __forceinline__
#else
#define PG_SCAF_HD inline
#endif

namespace pg {

constexpr int kScafWords = PG_MOL_MAX_ATOMS / 64;
static_assert(kScafWords == 2, "a set of atoms is two mask words: scaf_word selects, it does not index");

PG_SCAF_HD int scaf_popc(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// word i >> 6 of a set, by selection (a set in registers stays there)
PG_SCAF_HD unsigned long long scaf_word(const unsigned long long* set, int i) { return (i >> 6) ? set[1] : set[0]; }

PG_SCAF_HD bool scaf_has(const unsigned long long* set, int i) { return (scaf_word(set, i) >> (i & 63)) & 1ull; }

PG_SCAF_HD int scaf_count(const unsigned long long* set) { return scaf_popc(set[0]) + scaf_popc(set[1]); }

// the atoms of a row that are in the set
PG_SCAF_HD int scaf_degree(const unsigned long long* row, const unsigned long long* set) {
  return scaf_popc(row[0] & set[0]) + scaf_popc(row[1] & set[1]);
}

// Pruning: atom i goes in this round if it is still there and has at most one neighbour that is.  A round removes every such atom
// at once (all tests of a round read the same `alive`); the rounds end when one removes nothing, and what is left, the 2-core, does
// not depend on the order of the removals.
PG_SCAF_HD bool scaf_is_leaf(const unsigned long long* row, const unsigned long long* alive, int i) {
  return scaf_has(alive, i) && scaf_degree(row, alive) <= 1;
}

// Exocyclic rule: a kept atom outside the core with a bond of order exactly 2 (dbl_row: its bonds of that order) to an atom of it.
PG_SCAF_HD bool scaf_is_exocyclic(const unsigned long long* dbl_row, const unsigned long long* core, bool kept, bool in_core) {
  return kept && !in_core && scaf_degree(dbl_row, core) > 0;
}

// PG_SCAF_PART_* of an atom; ring_row: its ring bonds (inside the core by construction)
PG_SCAF_HD int scaf_part(bool kept, bool in_core, const unsigned long long* ring_row, bool exocyclic) {
  if (!kept) return PG_SCAF_PART_NONE;
  if (in_core) return (ring_row[0] | ring_row[1]) ? PG_SCAF_PART_RING : PG_SCAF_PART_LINKER;
  return exocyclic ? PG_SCAF_PART_EXOCYCLIC : PG_SCAF_PART_SIDE_CHAIN;
}

// index of atom i among the atoms of the set (i is one of them): the atoms of the set below i
PG_SCAF_HD int scaf_compact(const unsigned long long* set, int i) {
  const unsigned long long below = (1ull << (i & 63)) - 1ull;
  return (i >> 6) ? scaf_popc(set[0]) + scaf_popc(set[1] & below) : scaf_popc(set[0] & below);
}

// class of a scaffold atom, order of a scaffold bond (o = 1..4), and what the bond adds to twice the valence of its two atoms
PG_SCAF_HD int scaf_class(int k, int flags) { return (flags & PG_SCAF_GENERIC) ? PG_SCAF_CARBON : k; }
PG_SCAF_HD int scaf_order(int o, int flags) { return (flags & PG_SCAF_GENERIC) ? 1 : o; }
PG_SCAF_HD unsigned int scaf_valence2(int o) { return o == 4 ? 3u : 2u * (unsigned int)o; }

// Label step of the components: the smallest label among l, the labels of the row's atoms inside the set, and that label's label.
// Labels are local atom indices, start as the atom's own, only decrease and stay inside the component: at the fixed point every atom
// of a component holds the index of its first atom.
template <class Label>
PG_SCAF_HD int scaf_min_label(const unsigned long long* row, const unsigned long long* set, const Label* label, int l) {
#pragma unroll
  for (int w = 0; w < kScafWords; ++w) {
    unsigned long long m = row[w] & set[w];
    while (m) {
      const int j = w * 64 + __builtin_ctzll(m);
      m &= m - 1ull;
      const int lj = (int)label[j];
      l = lj < l ? lj : l;
    }
  }
  const int ll = (int)label[l];
  return ll < l ? ll : l;
}

}  // namespace pg
