// The serial core of the Kekulé assignment (DESIGN.md 2.9 "Kekulé form"): classification of an aromatic atom, the matching on the
// allowed graph, and an atom's hydrogens and charge.  Plain functions over caller-supplied arrays, compiled for the device by
// mol_kekule.hip (all arrays in LDS, the matching on one lane) and for the host by tools/kekule_host_check.cpp (the same text under
// the host sanitizers).  Integer work only.
//
// Every loop here has a trip count bounded by n (or by the 64 bits of a mask word): termination never rests on what the arrays hold,
// so a wrong `parent` cannot spin.  The `break`s marked (guard) are never taken on consistent arrays.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_KEK_HD __host__ __device__ inline
#else
#define PG_KEK_HD inline
#endif

namespace pg {

constexpr int kKekNone = 0;   // not aromatic (no bond of order 4)
constexpr int kKekNot = 1;    // aromatic, cannot take the double bond: outside the allowed graph
constexpr int kKekMay = 2;    // may be matched
constexpr int kKekMust = 3;   // must be matched

constexpr uint8_t kKekUsed = 1, kKekBlossom = 2, kKekMark = 4;   // bits of `flags`

// s = sum of the orders of the atom's non-aromatic bonds, a = its bonds of order 4, cap = the pass's table entry of its element
PG_KEK_HD int kekule_kind(int s, int a, int cap, int must) {
  if (a < 1) return kKekNone;
  if (s + a + 1 > cap) return kKekNot;
  return must ? kKekMust : kKekMay;
}

// Hydrogens h and charge q of a kept atom: d = 1 if it carries a double bond of the matching; hval = its element's valence list,
// ascending, zero-padded to four entries.
PG_KEK_HD void kekule_atom(bool is_n, int s, int a, int d, int dbl_neutral, const uint8_t* hval, int* h, int* q) {
  const int v = s + a + d;
  const int qq = ((is_n && v == 4) || (d == 1 && v > dbl_neutral)) ? 1 : 0;
  const int x = v - qq;
  int hh = 0;
  for (int k = 3; k >= 0; --k)
    if (hval[k] != 0 && (int)hval[k] >= x) hh = (int)hval[k] - x;   // (descending: the smallest entry >= x is the last one taken)
  *h = hh;
  *q = qq;
}

PG_KEK_HD int kek_ctz64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)m) - 1;
#else
  return __builtin_ctzll(m);
#endif
}

// Lowest common ancestor of the outer vertices a and b in the search tree, as a blossom base.
PG_KEK_HD int kek_lca(int n, int root, int a, int b, const int16_t* match, const int16_t* parent, const int16_t* base, uint8_t* flags) {
  for (int i = 0; i < n; ++i) flags[i] &= (uint8_t)~kKekMark;
  for (int k = 0; k <= n; ++k) {
    a = base[a];
    flags[a] |= kKekMark;
    if (match[a] < 0) break;                                        // the root
    a = parent[match[a]];
    if (a < 0) break;                                               // (guard)
  }
  for (int k = 0; k <= n; ++k) {
    b = base[b];
    if (flags[b] & kKekMark) return b;
    if (match[b] < 0) break;                                        // (guard)
    b = parent[match[b]];
    if (b < 0) break;                                               // (guard)
  }
  return base[root];                                                // (guard)
}

// Marks the blossom's bases on the tree path from v down to the base b and turns the parents round, so that the odd cycle can be
// walked either way.
PG_KEK_HD void kek_mark_path(int n, int v, int b, int child, const int16_t* match, int16_t* parent, const int16_t* base, uint8_t* flags) {
  for (int k = 0; k < n && base[v] != b; ++k) {
    const int mv = match[v];
    if (mv < 0) break;                                              // (guard)
    flags[base[v]] |= kKekBlossom;
    flags[base[mv]] |= kKekBlossom;
    parent[v] = (int16_t)child;
    child = mv;
    v = parent[mv];
    if (v < 0) break;                                               // (guard)
  }
}

// One breadth-first search of Edmonds' algorithm from the uncovered vertex `root` over the allowed graph adj (two 64-bit words per
// atom).  Returns the far end of an augmenting path (parents set), or -1.  to_may (phase A): an outer MAY atom other than the root
// ends the search too -- it owns a virtual, always-uncovered pendant vertex n + v, which has degree 1 and is therefore never inside
// a blossom; the pendant is returned.
PG_KEK_HD int kek_search(int n, const unsigned long long* adj, const uint8_t* kind, bool to_may, int root, int16_t* match, int16_t* parent,
                         int16_t* base, int16_t* queue, uint8_t* flags) {
  for (int i = 0; i < n; ++i) {
    flags[i] = 0;
    base[i] = (int16_t)i;
    parent[i] = -1;
  }
  flags[root] = kKekUsed;
  queue[0] = (int16_t)root;
  int qh = 0, qt = 1;
  for (int pops = 0; pops < n && qh < qt; ++pops) {                 // every vertex is queued at most once (kKekUsed)
    const int v = queue[qh++];
    if (to_may && v != root && kind[v] == kKekMay) {
      parent[n + v] = (int16_t)v;
      return n + v;
    }
    for (int w = 0; w < 2; ++w) {
      unsigned long long m = adj[2 * v + w];
      for (int k = 0; k < 64 && m; ++k) {
        const int to = w * 64 + kek_ctz64(m);
        m &= m - 1ull;
        if (to >= n || base[v] == base[to] || match[v] == to) continue;
        const int mt = match[to];
        if (to == root || (mt >= 0 && parent[mt] >= 0)) {           // `to` is outer as well: an odd cycle, contract it
          const int cb = kek_lca(n, root, v, to, match, parent, base, flags);
          for (int i = 0; i < n; ++i) flags[i] &= (uint8_t)~kKekBlossom;
          kek_mark_path(n, v, cb, to, match, parent, base, flags);
          kek_mark_path(n, to, cb, v, match, parent, base, flags);
          for (int i = 0; i < n; ++i) {
            if (flags[base[i]] & kKekBlossom) {
              base[i] = (int16_t)cb;
              if (!(flags[i] & kKekUsed)) {
                flags[i] |= kKekUsed;
                if (qt < n) queue[qt++] = (int16_t)i;
              }
            }
          }
        } else if (parent[to] < 0) {
          parent[to] = (int16_t)v;
          if (mt < 0) return to;
          if (!(flags[mt] & kKekUsed)) {
            flags[mt] |= kKekUsed;
            if (qt < n) queue[qt++] = (int16_t)mt;
          }
        }
      }
    }
  }
  return -1;
}

// Flips the path that ends at `end`; a pendant end (>= n) leaves its atom uncovered again.
PG_KEK_HD void kek_augment(int n, int end, int16_t* match, const int16_t* parent) {
  int v = end;
  for (int k = 0; k <= n && v >= 0; ++k) {
    const int pv = parent[v];
    if (pv < 0) break;                                              // (guard)
    const int ppv = match[pv];
    match[v] = (int16_t)pv;
    match[pv] = (int16_t)v;
    v = ppv;
  }
  if (end >= n) match[end - n] = match[end] = -1;
}

// The matching of one pass.  n atoms; adj [2 n]: the allowed graph as a bit per local atom index (rows of atoms outside it are 0);
// kind [n]: kKek*; match [2 n], all -1 on entry: the result in match[0 .. n); parent [2 n], base [n], queue [n], flags [n]: work
// space.  Returns 1 if every MUST atom is covered -- the matching then has maximum cardinality in the allowed graph -- and 0 if the
// pass is infeasible (match is then of no use).
// Phase A covers the MUST atoms one by one; a covered atom stays covered, a MAY atom may be uncovered again.  Phase B augments from
// every atom still uncovered, which uncovers nobody: one search per atom is enough, since an atom without an augmenting path has
// none after later augmentations either.
PG_KEK_HD int kekule_match(int n, const unsigned long long* adj, const uint8_t* kind, int16_t* match, int16_t* parent, int16_t* base,
                           int16_t* queue, uint8_t* flags) {
  for (int r = 0; r < n; ++r) {
    if (kind[r] != kKekMust || match[r] >= 0) continue;
    const int end = kek_search(n, adj, kind, true, r, match, parent, base, queue, flags);
    if (end < 0) return 0;
    kek_augment(n, end, match, parent);
  }
  for (int r = 0; r < n; ++r) {
    if (kind[r] < kKekMay || match[r] >= 0 || (adj[2 * r] | adj[2 * r + 1]) == 0ull) continue;
    const int end = kek_search(n, adj, kind, false, r, match, parent, base, queue, flags);
    if (end >= 0) kek_augment(n, end, match, parent);
  }
  return 1;
}

}  // namespace pg
