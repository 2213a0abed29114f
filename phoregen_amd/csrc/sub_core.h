// The core of the substructure search (DESIGN.md 2.9 "Substructure"; pg_mol_sub, include/phoregen_hip.h): the layout of a pattern
// row and its checks, an atom's packed property word and the constraint test on it, the bond classes, the candidate-set step and the
// depth-first search from one root.  Plain functions over values and small arrays with explicit bounds; where the search keeps its
// state (LDS in mol_sub.hip, plain arrays in tools/mol_sub_host_check.cpp) is the caller's, handed in as a `store` with the accessors
// named below.  Compiled for the device by mol_sub.hip and for the host by tools/mol_sub_host_check.cpp (the same text under the host
// sanitizers).  Integer work only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/phoregen_hip.h"

#if defined(__HIPCC__)
#define PG_SUB_HD __host__ __device__ inline
#else
#define PG_SUB_HD inline
#endif

namespace pg {

typedef unsigned long long sub_u64;

constexpr int kSubMaxAtoms = PG_SUB_MAX_ATOMS;   // query atoms of a pattern
constexpr int kSubTargetMax = PG_MOL_MAX_ATOMS;  // kept atoms of a target
constexpr int kSubClasses = 8;                   // bond classes: (order 1..4) x (bridge, ring bond)
static_assert(kSubMaxAtoms == 16 && kSubTargetMax == 128, "a set of target atoms is two 64-bit words, a set of query atoms 16 bits");
static_assert(PG_SUB_OFF_ATOMS + kSubMaxAtoms * PG_SUB_ATOM_BYTES == PG_SUB_OFF_BONDS, "the atom records end where the bond bytes begin");
static_assert(PG_SUB_OFF_BONDS + kSubMaxAtoms * kSubMaxAtoms == PG_SUB_PATTERN_BYTES && PG_SUB_PATTERN_BYTES % 16 == 0, "dense rows");

// a set of target atoms by compact index
struct SubMask {
  sub_u64 w[2];
};
// (no word is picked by a computed index: on the device the two words stay in registers)
PG_SUB_HD bool sub_mask_has(const SubMask& m, int c) { return c >= 0 && c < kSubTargetMax && ((c < 64 ? m.w[0] : m.w[1]) >> (c & 63) & 1ull) != 0; }
PG_SUB_HD void sub_mask_set(SubMask& m, int c) {
  const sub_u64 bit = 1ull << (c & 63);
  m.w[0] |= (c & 64) ? 0ull : bit, m.w[1] |= (c & 64) ? bit : 0ull;
}
PG_SUB_HD void sub_mask_clear(SubMask& m, int c) {
  const sub_u64 bit = 1ull << (c & 63);
  m.w[0] &= (c & 64) ? ~0ull : ~bit, m.w[1] &= (c & 64) ? ~bit : ~0ull;
}
// the lowest atom of a set, -1 for the empty set
PG_SUB_HD int sub_mask_lowest(const SubMask& m) {
  return m.w[0] ? __builtin_ctzll(m.w[0]) : m.w[1] ? 64 + __builtin_ctzll(m.w[1]) : -1;
}

// ---- an atom's properties ---------------------------------------------------------------------------------------------------------------
// class 0..10 | in a ring << 4 | has an aromatic bond << 5 | charged << 6 | degree << 8 | hydrogens << 16
PG_SUB_HD uint32_t sub_prop_pack(int cls, int degree, int hcount, bool charged, bool in_ring, bool aromatic) {
  return (uint32_t)(cls & 15) | (in_ring ? 16u : 0u) | (aromatic ? 32u : 0u) | (charged ? 64u : 0u) | (uint32_t)(degree & 255) << 8 |
         (uint32_t)(hcount & 255) << 16;
}

// a three-way flag of a record: PG_SUB_ANY, PG_SUB_YES (the property must hold), PG_SUB_NO (it must not)
PG_SUB_HD bool sub_flag_ok(unsigned want, bool have) { return want == PG_SUB_ANY || (want == PG_SUB_YES) == have; }

// does the atom with property word `prop` meet the record `a` (PG_SUB_ATOM_BYTES bytes of a pattern row)?
PG_SUB_HD bool sub_atom_ok(const uint8_t* a, uint32_t prop) {
  const unsigned elements = (unsigned)a[PG_SUB_ATOM_ELEMENTS] | (unsigned)a[PG_SUB_ATOM_ELEMENTS + 1] << 8;
  const unsigned degree = prop >> 8 & 255u, h = prop >> 16 & 255u, flags = a[PG_SUB_ATOM_FLAGS];
  return (elements >> (prop & 15u) & 1u) && degree >= a[PG_SUB_ATOM_DEGREE] && degree <= a[PG_SUB_ATOM_DEGREE + 1] &&
         h >= a[PG_SUB_ATOM_HCOUNT] && h <= a[PG_SUB_ATOM_HCOUNT + 1] && sub_flag_ok(flags & 3u, (prop & 64u) != 0) &&
         sub_flag_ok(flags >> 2 & 3u, (prop & 16u) != 0) && sub_flag_ok(flags >> 4 & 3u, (prop & 32u) != 0);
}

// does the record constrain the hydrogens or the charge (the two properties that need the Kekulé form)?
PG_SUB_HD bool sub_atom_uses_kekule(const uint8_t* a) {
  return a[PG_SUB_ATOM_HCOUNT] != 0 || a[PG_SUB_ATOM_HCOUNT + 1] != 255 || (a[PG_SUB_ATOM_FLAGS] & 3u) != PG_SUB_ANY;
}

// ---- bond classes -----------------------------------------------------------------------------------------------------------------------
// the class of a target bond of order 1..4
PG_SUB_HD int sub_bond_class(int order, bool ring_bond) { return ((order - 1) & 3) | (ring_bond ? 4 : 0); }
// the classes a query bond byte (orders as bits 0..3 | ring flag << 4) accepts, as 8 bits; 0 for "no bond"
PG_SUB_HD unsigned sub_class_mask(unsigned bond) {
  const unsigned orders = bond & 15u, ring = bond >> 4 & 3u;
  return (ring == PG_SUB_YES ? 0u : orders) | (ring == PG_SUB_NO ? 0u : orders << 4);
}

// ---- a pattern row ----------------------------------------------------------------------------------------------------------------------
PG_SUB_HD int sub_row_k(const uint8_t* row) { return row[PG_SUB_OFF_K]; }
PG_SUB_HD const uint8_t* sub_row_atom(const uint8_t* row, int q) { return row + PG_SUB_OFF_ATOMS + (q & 15) * PG_SUB_ATOM_BYTES; }
PG_SUB_HD unsigned sub_row_bond(const uint8_t* row, int a, int b) { return row[PG_SUB_OFF_BONDS + (a & 15) * kSubMaxAtoms + (b & 15)]; }
PG_SUB_HD int sub_row_order(const uint8_t* row, int d) { return row[PG_SUB_OFF_ORDER + (d & 15)] & 15; }
PG_SUB_HD int32_t sub_row_int(const uint8_t* row, int off) {
  return (int32_t)((uint32_t)row[off] | (uint32_t)row[off + 1] << 8 | (uint32_t)row[off + 2] << 16 | (uint32_t)row[off + 3] << 24);
}
PG_SUB_HD bool sub_row_uses_kekule(const uint8_t* row, int k) {
  bool uses = false;
  for (int q = 0; q < k && q < kSubMaxAtoms; ++q) uses = uses || sub_atom_uses_kekule(sub_row_atom(row, q));
  return uses;
}

// 0 for a well-formed row, else which rule it breaks (sub_row_error_text)
enum { kSubRowOk = 0, kSubRowK, kSubRowElements, kSubRowRange, kSubRowFlags, kSubRowBond, kSubRowOrder, kSubRowConnected, kSubRowBounds };
inline const char* sub_row_error_text(int e) {
  static const char* const text[] = {"ok",
                                     "k outside 1 .. PG_SUB_MAX_ATOMS",
                                     "a query atom with an empty element set (or a class above 10)",
                                     "a degree or hydrogen range with lo > hi",
                                     "a flag that is none of any / yes / no",
                                     "a bond byte with an empty order set, a flag outside any / yes / no, on the diagonal or unlike its mirror",
                                     "a matching order that is no permutation of the query atoms starting at atom 0",
                                     "a query atom after the first without a bond to an earlier one in matching order",
                                     "bounds with min < 0, max < -1 or 0 <= max < min"};
  return text[e < 0 || e > kSubRowBounds ? 0 : e];
}
inline int sub_row_check(const uint8_t* row) {
  const int k = sub_row_k(row);
  if (k < 1 || k > kSubMaxAtoms) return kSubRowK;
  for (int q = 0; q < k; ++q) {
    const uint8_t* a = sub_row_atom(row, q);
    const unsigned elements = (unsigned)a[PG_SUB_ATOM_ELEMENTS] | (unsigned)a[PG_SUB_ATOM_ELEMENTS + 1] << 8, flags = a[PG_SUB_ATOM_FLAGS];
    if (elements == 0 || elements >> 11) return kSubRowElements;
    if (a[PG_SUB_ATOM_DEGREE] > a[PG_SUB_ATOM_DEGREE + 1] || a[PG_SUB_ATOM_HCOUNT] > a[PG_SUB_ATOM_HCOUNT + 1]) return kSubRowRange;
    if ((flags & 3u) == 3u || (flags >> 2 & 3u) == 3u || (flags >> 4 & 3u) == 3u || flags >> 6) return kSubRowFlags;
  }
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) {
      const unsigned bond = sub_row_bond(row, a, b);
      if (bond == 0) continue;
      if (a == b || (bond & 15u) == 0 || (bond >> 4 & 3u) == 3u || bond >> 6 || bond != sub_row_bond(row, b, a)) return kSubRowBond;
    }
  unsigned seen = 0;
  for (int d = 0; d < k; ++d) {
    const int q = row[PG_SUB_OFF_ORDER + d];
    if (q >= k || (seen >> q & 1u) || (d == 0 && q != 0)) return kSubRowOrder;
    bool joined = d == 0;
    for (int e = 0; e < d; ++e) joined = joined || sub_row_bond(row, q, row[PG_SUB_OFF_ORDER + e]) != 0;
    if (!joined) return kSubRowConnected;
    seen |= 1u << q;
  }
  const int32_t lo = sub_row_int(row, PG_SUB_OFF_MIN), hi = sub_row_int(row, PG_SUB_OFF_MAX);
  if (lo < 0 || hi < -1 || (hi >= 0 && hi < lo)) return kSubRowBounds;
  return kSubRowOk;
}

// the status word of one (graph, pattern) from its outputs and the row's bounds on `anchors` (max -1: none)
PG_SUB_HD int sub_status(sub_u64 embeddings, int anchors, bool no_kekule, bool truncated, int32_t lo, int32_t hi) {
  const bool bounded = lo > 0 || hi >= 0;
  const bool out = anchors < lo || (hi >= 0 && anchors > hi) || (bounded && truncated);
  return (embeddings ? PG_SUB_MATCHED : 0) | (no_kekule ? PG_SUB_NO_KEKULE : 0) | (truncated ? PG_SUB_TRUNCATED : 0) |
         (out ? PG_SUB_OUT_OF_BOUNDS : 0);
}
PG_SUB_HD int sub_saturate(sub_u64 embeddings) { return embeddings > 0x7fffffffull ? 0x7fffffff : (int)embeddings; }

// ---- the search -------------------------------------------------------------------------------------------------------------------------
// What a `store` provides, positions d, e in matching order (0 <= e < d < k), target atoms t by compact index, classes c < kSubClasses:
//   SubMask compat(d)        the target atoms that meet the constraints of the query atom at position d
//   unsigned back(d)         bit e: the query atom at d has a bond to the one at e
//   unsigned classes(d, e)   the classes that bond accepts (sub_class_mask)
//   SubMask adj(c, t)        the atoms joined to t by a bond of class c
//   int image(d) / void set_image(d, t)      the partial embedding
//   SubMask cand(d) / void set_cand(d, m)    the candidates of position d that are still to be tried
//   void save_first(k, last) the embedding image(0 .. k - 2), last is the lane's first find

// The candidates for position d of a partial embedding of size d: the atoms that meet its constraints, are not used, and are joined to
// the image of every earlier neighbour by a bond of an accepted class.  `tried` = how many of them there are before any neighbour
// but the walk parent (the earliest position d has a bond to) is looked at: the steps of this expansion.
template <class Store>
PG_SUB_HD SubMask sub_candidates(Store& s, int d, const SubMask& used, int& tried) {
  SubMask m = s.compat(d);
  m.w[0] &= ~used.w[0], m.w[1] &= ~used.w[1];
  unsigned back = s.back(d) & ((1u << d) - 1u);
  bool parent = true;
  tried = 0;
  while (back && (parent || (m.w[0] | m.w[1]))) {
    const int e = __builtin_ctz(back);
    back &= back - 1u;
    const int t = s.image(e);
    unsigned classes = s.classes(d, e) & 255u;
    SubMask row = {{0ull, 0ull}};
    while (classes) {
      const SubMask r = s.adj(__builtin_ctz(classes), t);
      classes &= classes - 1u;
      row.w[0] |= r.w[0], row.w[1] |= r.w[1];
    }
    m.w[0] &= row.w[0], m.w[1] &= row.w[1];
    if (parent) tried = __builtin_popcountll(m.w[0]) + __builtin_popcountll(m.w[1]);
    parent = false;
  }
  return m;
}

// what one lane has found over its roots
struct SubFound {
  sub_u64 embeddings;   // (a root adds at most max_steps <= 2^30)
  SubMask atoms;        // images of its embeddings
  bool have_first, truncated;
};

// Depth-first search over the embeddings whose anchor (position 0) is `root`, candidates in ascending order, so the first embedding
// found is the root's lexicographically smallest in matching order.  A step is one way to continue a partial embedding by one atom
// along the walk: an unused atom that meets the next query atom's constraints and is joined as the pattern asks to the image of its
// walk parent; the root is abandoned (truncated) as soon as its steps exceed max_steps, keeping what it had found.  Returns whether
// the root has an embedding.  1 <= k <= kSubMaxAtoms; root must be in compat(0).
template <class Store>
PG_SUB_HD bool sub_search_root(Store& s, int k, int root, sub_u64 max_steps, SubFound& f) {
  SubMask used = {{0ull, 0ull}};
  sub_mask_set(used, root);
  s.set_image(0, root);
  if (k == 1) {
    ++f.embeddings;
    sub_mask_set(f.atoms, root);
    if (!f.have_first) s.save_first(1, root);
    f.have_first = true;
    return true;
  }
  bool found = false;
  int tried;
  SubMask c = sub_candidates(s, 1, used, tried);
  sub_u64 steps = (sub_u64)tried;
  if (steps > max_steps) {
    f.truncated = true;
    return false;
  }
  s.set_cand(1, c);
  int d = 1;
  while (d >= 1) {
    c = s.cand(d);
    const int t = sub_mask_lowest(c);
    if (t < 0) {                                 // position d is exhausted: back to d - 1, whose image is free again
      --d;
      if (d >= 1) sub_mask_clear(used, s.image(d));
      continue;
    }
    sub_mask_clear(c, t);
    s.set_cand(d, c);
    if (d == k - 1) {
      ++f.embeddings;
      found = true;
      f.atoms.w[0] |= used.w[0], f.atoms.w[1] |= used.w[1];
      sub_mask_set(f.atoms, t);
      if (!f.have_first) s.save_first(k, t);
      f.have_first = true;
    } else {
      s.set_image(d, t);
      sub_mask_set(used, t);
      ++d;
      c = sub_candidates(s, d, used, tried);
      steps += (sub_u64)tried;
      if (steps > max_steps) {
        f.truncated = true;
        break;
      }
      s.set_cand(d, c);
    }
  }
  return found;
}

}  // namespace pg
