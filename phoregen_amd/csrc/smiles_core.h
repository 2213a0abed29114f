// The core of the SMILES writer (DESIGN.md 2.9 "SMILES"): the depth-first traversal, the assignment of the ring-closure labels, and
// the text of one atom.  Plain functions over caller-supplied arrays, compiled for the device by mol_smiles.hip (all arrays in LDS;
// the traversal and the labels on one lane, the atoms' texts one atom per lane) and for the host by tools/smiles_host_check.cpp (the
// same text under the host sanitizers).  Integer work only.
//
// The bonds are two bit planes of adjacency rows, two 64-bit words per atom each: a bond of Kekulé order o between a and b has bit b of
// row a (and bit a of row b) set in p0 if o is odd and in p1 if o >= 2.  Rows hold bits below n only, and only between kept atoms.
//
// Every loop here has a trip count bounded by n, by the bond count (the 64 bits of a mask word, per word) or by a constant:
// termination never rests on what the arrays hold.  The `break`s marked (guard) are never taken on consistent arrays.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_SMI_HD __host__ __device__ inline
#else
#define PG_SMI_HD inline
#endif

namespace pg {

constexpr int kSmiMaxLabel = 99;            // ring-closure labels 1 .. 99
constexpr int kSmiLabelOverflow = -1;       // smiles_labels: more than kSmiMaxLabel labels in use at once
constexpr int kSmiEl = 11;                  // elements (atom classes 0..10)
constexpr int kSmiSi = 5;                   // the class of Si: a two-letter symbol outside the bare subset

// bits of an atom's `flags`
constexpr uint8_t kSmiHasChild = 1;         // the traversal's own: the atom has a child already
constexpr uint8_t kSmiPrev = 2;             // not its parent's first child: a ')' comes before it
constexpr uint8_t kSmiNext = 4;             // not its parent's last child: a '(' comes before it
constexpr uint8_t kSmiDot = 8;              // the root of a component that is not the first: a '.' comes before it

typedef unsigned long long smi_u64;

PG_SMI_HD int smi_ctz64(smi_u64 m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)m) - 1;
#else
  return __builtin_ctzll(m);
#endif
}

PG_SMI_HD int smi_popc64(smi_u64 m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// the lowest set bit of the 128-bit mask (m0, m1), -1 if it is empty
PG_SMI_HD int smi_lowest(smi_u64 m0, smi_u64 m1) { return m0 ? smi_ctz64(m0) : m1 ? 64 + smi_ctz64(m1) : -1; }

// the row of the pair a != b among the n (n - 1) / 2 pairs (mol_common.h, for_each_pair)
PG_SMI_HD int smi_pair(int n, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * n - lo * (lo + 1) / 2 + (hi - lo - 1);
}

// the order of the bond v - u (0: none)
PG_SMI_HD int smi_order(const smi_u64* p0, const smi_u64* p1, int v, int u) {
  const int w = 2 * v + (u >> 6), s = u & 63;
  return (int)((p0[w] >> s) & 1ull) + 2 * (int)((p1[w] >> s) & 1ull);
}

// The traversal.  n atoms, kept0 / kept1: the kept atoms as a mask; rank [n] = -1, parent [n] = -1, flags [n] = 0 on entry; order [n],
// stack [n]: work space (order[k] = the atom of rank k is a result).  From every kept atom not yet visited, ascending, a depth-first
// search that takes an atom's unvisited neighbours in ascending order.  Returns the atoms visited; *n_comp: the roots; *n_branch:
// the atoms with kSmiNext.  Whether a child is its parent's last one is known when the search comes back from it: a neighbour
// still unvisited then becomes the next child.
PG_SMI_HD int smiles_tree(int n, const smi_u64* p0, const smi_u64* p1, smi_u64 kept0, smi_u64 kept1, int16_t* rank, int16_t* order,
                          int16_t* parent, uint8_t* flags, int16_t* stack, int* n_comp, int* n_branch) {
  smi_u64 vis0 = ~kept0, vis1 = ~kept1;                              // a dropped atom is never visited
  int count = 0, comps = 0, branches = 0, sp = 0;
  for (int step = 0; step < 2 * n; ++step) {                          // every step visits an atom or leaves one
    int w, from = -1;
    if (sp == 0) {
      w = smi_lowest(~vis0, ~vis1);
      if (w < 0 || w >= n) break;                                     // all visited
      flags[w] = comps > 0 ? kSmiDot : 0;
      ++comps;
    } else {
      from = stack[sp - 1];
      w = smi_lowest((p0[2 * from] | p1[2 * from]) & ~vis0, (p0[2 * from + 1] | p1[2 * from + 1]) & ~vis1);
      if (w >= n) break;                                              // (guard)
      if (w < 0) {                                                    // leave `from`: if its parent has another child to come, it is a branch
        --sp;
        if (sp > 0) {
          const int up = stack[sp - 1];
          if (smi_lowest((p0[2 * up] | p1[2 * up]) & ~vis0, (p0[2 * up + 1] | p1[2 * up + 1]) & ~vis1) >= 0) {
            flags[from] |= kSmiNext;
            ++branches;
          }
        }
        continue;
      }
      flags[w] = (flags[from] & kSmiHasChild) ? kSmiPrev : 0;
      flags[from] |= kSmiHasChild;
    }
    parent[w] = (int16_t)from;
    rank[w] = (int16_t)count;
    order[count++] = (int16_t)w;
    if (w < 64) vis0 |= 1ull << w; else vis1 |= 1ull << (w - 64);
    if (sp >= n) break;                                               // (guard)
    stack[sp++] = (int16_t)w;
  }
  *n_comp = comps;
  *n_branch = branches;
  return count;
}

// The ring-closure labels.  A bond that is not a tree bond joins an atom to one of its ancestors (the search is depth-first); it is
// opened at the ancestor -- the end of lower rank -- and closed at the other.  The atoms are walked in preorder; at an atom the
// labels of the closures that close there stay in use while its opening closures, by ascending index of the far end, each take the
// smallest free label.  label [n (n - 1) / 2]: the label of a ring-closure bond at its pair row (other rows are not touched).
// Returns the largest label given (0: none), or kSmiLabelOverflow; *n_closure: the ring closures (not set on overflow).
PG_SMI_HD int smiles_labels(int n, int n_visited, const smi_u64* p0, const smi_u64* p1, const int16_t* rank, const int16_t* order,
                            const int16_t* parent, uint8_t* label, int* n_closure) {
  smi_u64 use0 = 1ull, use1 = ~0ull << (kSmiMaxLabel + 1 - 64);       // label L in use: bit L (0 and 100 .. 127 are never free)
  int largest = 0, closures = 0;
  for (int k = 0; k < n_visited; ++k) {
    const int v = order[k];
    smi_u64 done0 = 0ull, done1 = 0ull;
    for (int w = 0; w < 2; ++w) {
      smi_u64 m = p0[2 * v + w] | p1[2 * v + w];
      for (int i = 0; i < 64 && m; ++i) {
        const int u = w * 64 + smi_ctz64(m);
        m &= m - 1ull;
        if (u >= n || u == parent[v] || parent[u] == v) continue;     // (u >= n: guard) a tree bond
        if (rank[u] < rank[v]) {                                      // closes here: free after this atom
          const int L = label[smi_pair(n, u, v)];
          if (L < 64) done0 |= 1ull << L; else done1 |= 1ull << (L - 64);
        } else {                                                      // opens here
          const int L = smi_lowest(~use0, ~use1);
          if (L < 0) return kSmiLabelOverflow;
          if (L < 64) use0 |= 1ull << L; else use1 |= 1ull << (L - 64);
          label[smi_pair(n, v, u)] = (uint8_t)L;
          largest = L > largest ? L : largest;
          ++closures;
        }
      }
    }
    use0 &= ~(done0 & ~1ull);
    use1 &= ~(done1 & ((1ull << (kSmiMaxLabel + 1 - 64)) - 1ull));
  }
  *n_closure = closures;
  return largest;
}

// ---- the text of one atom -----------------------------------------------------------------------------------------------------------
template <class Put>
PG_SMI_HD void smi_put_bond(int o, Put&& put) {
  if (o == 2) put('=');
  if (o == 3) put('#');
}

template <class Put>
PG_SMI_HD void smi_put_label(int L, Put&& put) {
  if (L >= 10) {
    put('%');
    put((char)('0' + L / 10));
  }
  put((char)('0' + L % 10));
}

// The OpenSMILES implicit hydrogens of a bare atom: the smallest of the element's normal valences (val [4], ascending, zero-padded)
// that is not below the sum of its bond orders, minus that sum; 0 without one.
PG_SMI_HD int smi_implicit_h(const uint8_t* val, int sum) {
  int h = 0;
  for (int k = 3; k >= 0; --k)
    if (val[k] != 0 && (int)val[k] >= sum) h = (int)val[k] - sum;     // (descending: the smallest entry >= sum is the last one taken)
  return h;
}

// Everything the atom v puts into the text, through put(char), in order: the '.', ')' and '(' its place in the tree asks for, the
// symbol of the bond to its parent, the atom token, the labels of the ring closures that close at v by ascending index of the
// ancestor, then bond symbol and label of those that open at v by ascending index of the descendant.  el: its class 0..10, h, q: its
// hydrogens and charge, val: the notation's valence list of its element (empty: never bare).  Returns true for a bracket atom.
template <class Put>
PG_SMI_HD bool smiles_atom_text(int v, int n, int el, int h, int q, const uint8_t* val, const smi_u64* p0, const smi_u64* p1,
                                const int16_t* rank, const int16_t* parent, const uint8_t* flags, const uint8_t* label, Put&& put) {
  const uint8_t f = flags[v];
  const int up = parent[v];
  if (f & kSmiDot) put('.');
  if (f & kSmiPrev) put(')');
  if (f & kSmiNext) put('(');
  if (up >= 0) smi_put_bond(smi_order(p0, p1, v, up), put);
  // ---- the atom token ----
  const int sum = smi_popc64(p0[2 * v]) + smi_popc64(p0[2 * v + 1]) + 2 * (smi_popc64(p1[2 * v]) + smi_popc64(p1[2 * v + 1]));
  const bool bracket = !(val[0] != 0 && q == 0 && smi_implicit_h(val, sum) == h);
  // B C N O F Si P S | Cl Br I: the first letters packed a byte each, the second letters by class
  const char c1 = (char)(((el < 8 ? 0x535053464F4E4342ull >> (8 * el) : 0x494243ull >> (8 * (el - 8)))) & 0xffull);
  const char c2 = el == kSmiSi ? 'i' : el == 8 ? 'l' : el == 9 ? 'r' : (char)0;
  if (bracket) put('[');
  put(c1);
  if (c2) put(c2);
  if (bracket) {
    if (h >= 1) put('H');
    if (h >= 100) put((char)('0' + h / 100));
    if (h >= 10) put((char)('0' + h / 10 % 10));
    if (h >= 2) put((char)('0' + h % 10));
    if (q == 1) put('+');
    put(']');
  }
  // ---- ring closures: those that close here, then those that open here ----
  for (int pass = 0; pass < 2; ++pass) {
    for (int w = 0; w < 2; ++w) {
      smi_u64 m = p0[2 * v + w] | p1[2 * v + w];
      for (int i = 0; i < 64 && m; ++i) {
        const int u = w * 64 + smi_ctz64(m);
        m &= m - 1ull;
        if (u >= n || u == up || parent[u] == v) continue;            // (u >= n: guard) a tree bond
        if ((rank[u] < rank[v]) != (pass == 0)) continue;
        if (pass == 1) smi_put_bond(smi_order(p0, p1, v, u), put);
        smi_put_label(label[smi_pair(n, v, u)], put);
      }
    }
  }
  return bracket;
}

}  // namespace pg
