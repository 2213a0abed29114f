// The core of the SMILES writer (DESIGN.md 2.9 "SMILES"): the depth-first traversal, the assignment of the ring-closure labels, and
// the text of one atom.  Plain functions over caller-supplied arrays, compiled for the device by mol_smiles.hip (all arrays in LDS;
// the traversal and the labels on one lane, the atoms' texts one atom per lane) and for the host by tools/smiles_host_check.cpp (the
// same text under the host sanitizers).  Integer work only.  The stereo marks of pg_mol_smiles_stereo (DESIGN.md 2.9 "Stereo") are here
// too: which centres and double bonds of the stereo inputs the text can express, the '/' and '\\' of the single bonds next to a double
// bond, and '@' / '@@'; tools/stereo_host_check.cpp runs them on the host.
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

// what smiles_atom_text_stereo returns
constexpr int kSmiBracket = 1, kSmiCentre = 2, kSmiClockwise = 4;
// the mark of a bond, read from the atom written first to the atom written later: none, '/', '\\', marked and not yet decided
constexpr uint8_t kSmiUp = 1, kSmiDown = 2, kSmiTodo = 3;

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

// ---- stereo (DESIGN.md 2.9 "Stereo") ------------------------------------------------------------------------------------------------
// the atom's bonds
PG_SMI_HD int smi_degree(const smi_u64* p0, const smi_u64* p1, int v) {
  return smi_popc64(p0[2 * v] | p1[2 * v]) + smi_popc64(p0[2 * v + 1] | p1[2 * v + 1]);
}

// a parity the text can express: +1 or -1 on an atom with four neighbours and no hydrogen, or three and one
PG_SMI_HD bool smi_centre_ok(int parity, int degree, int h) {
  return (parity == 1 || parity == -1) && ((degree == 4 && h == 0) || (degree == 3 && h == 1));
}

// The sign of the permutation that takes the ligands of the centre v from index order (hydrogen last) to the order the text gives
// them: the parent, the hydrogen, the closures that close at v by ascending ancestor, those that open at v by ascending descendant,
// the children ascending.  A ligand's place in the text is a key (its group, then its index); the sign is the parity of the pairs
// that index order and key order put differently.  At most four ligands: the three keys before the current one are held by value.
PG_SMI_HD int smi_centre_sign(int v, int n, int h, const smi_u64* p0, const smi_u64* p1, const int16_t* rank, const int16_t* parent) {
  int k0 = -1, k1 = -1, k2 = -1, inv = 0;
  for (int w = 0; w < 2; ++w) {
    smi_u64 m = p0[2 * v + w] | p1[2 * v + w];
    for (int i = 0; i < 64 && m; ++i) {
      const int u = w * 64 + smi_ctz64(m);
      m &= m - 1ull;
      if (u >= n) continue;                                           // (guard)
      const int group = u == parent[v] ? 0 : parent[u] == v ? 4 : rank[u] < rank[v] ? 2 : 3;
      const int key = group * 128 + u;
      inv += (k0 > key) + (k1 > key) + (k2 > key);
      k2 = k1, k1 = k0, k0 = key;
    }
  }
  if (h == 1) inv += (k0 > 128) + (k1 > 128) + (k2 > 128);            // the hydrogen: group 1, last in index order
  return (inv & 1) ? -1 : 1;
}

// An end x of a double bond x = y that the text can mark: besides y it has one or two neighbours, all joined by single bonds.
PG_SMI_HD bool smi_stereo_end_ok(const smi_u64* p0, const smi_u64* p1, int x, int y) {
  const smi_u64 y0 = y < 64 ? 1ull << y : 0ull, y1 = y < 64 ? 0ull : 1ull << (y - 64);
  const int others = smi_popc64((p0[2 * x] | p1[2 * x]) & ~y0) + smi_popc64((p0[2 * x + 1] | p1[2 * x + 1]) & ~y1);
  return (others == 1 || others == 2) && (p1[2 * x] & ~y0) == 0ull && (p1[2 * x + 1] & ~y1) == 0ull;
}

// a stereo value on the pair a < b that the text can express: +1 or -1 on a double bond whose ends both are smi_stereo_end_ok
PG_SMI_HD bool smi_stereo_bond_ok(int stereo, const smi_u64* p0, const smi_u64* p1, int a, int b) {
  return (stereo == 1 || stereo == -1) && smi_order(p0, p1, a, b) == 2 && smi_stereo_end_ok(p0, p1, a, b) && smi_stereo_end_ok(p0, p1, b, a);
}

// the substituents of the end x of the double bond x = y: the neighbours other than y, ascending; *r1 = -1 if there is one only
PG_SMI_HD void smi_stereo_subs(const smi_u64* p0, const smi_u64* p1, int x, int y, int* r0, int* r1) {
  const smi_u64 m0 = (p0[2 * x] | p1[2 * x]) & ~(y < 64 ? 1ull << y : 0ull);
  const smi_u64 m1 = (p0[2 * x + 1] | p1[2 * x + 1]) & ~(y < 64 ? 0ull : 1ull << (y - 64));
  *r0 = smi_lowest(m0, m1);
  const smi_u64 n0 = m0 ? m0 & (m0 - 1ull) : 0ull, n1 = m0 ? m1 : m1 & (m1 - 1ull);
  *r1 = smi_lowest(n0, n1);
}

// The marks of the single bonds next to the double bonds that carry cis / trans.  partner [n]: the other end of the atom's expressible
// double bond (smi_stereo_bond_ok), -1 without one; sval [n]: that bond's stereo value at both its ends; mark [n (n - 1) / 2] = 0 on
// entry; queue [n]: work space.  side(x, r) of an end x and its substituent r is the bond's mark if x is written before r, else its
// opposite ('/' = +1, '\\' = -1).  The two substituents of an end have opposite sides, and side(a, r_a) side(b, r_b) = the stereo
// value for the lowest-index substituents r of the two ends: relative to one sign g per double bond every mark next to it is
// known, and double bonds that share a single bond share the sign.  The marked bonds are taken in the order of the text (the bond
// to the parent, then the opening closures ascending, atom by atom in preorder); one that has no mark yet becomes '/', and the
// double bonds reached from it over shared single bonds are settled breadth-first.  A component in which a bond would need both marks
// loses all of them (never with perceived input: stereo double bonds are bridges).  Returns the components dropped; *n_marked: the
// bonds with a mark, *n_expressed: the double bonds whose marks were kept.
PG_SMI_HD int smiles_stereo_marks(int n, int n_visited, const smi_u64* p0, const smi_u64* p1, const int16_t* rank, const int16_t* order,
                                  const int16_t* parent, const int16_t* partner, const int8_t* sval, uint8_t* mark, int16_t* queue,
                                  int* n_marked, int* n_expressed) {
  for (int x = 0; x < n; ++x) {
    if (partner[x] < 0) continue;
    int r0, r1;
    smi_stereo_subs(p0, p1, x, partner[x], &r0, &r1);
    if (r0 >= 0 && r0 < n) mark[smi_pair(n, x, r0)] = kSmiTodo;
    if (r1 >= 0 && r1 < n) mark[smi_pair(n, x, r1)] = kSmiTodo;
  }
  smi_u64 vis0 = 0ull, vis1 = 0ull;                                    // the ends of the double bonds in the queue
  int tail = 0, dropped = 0, marked = 0, expressed = 0;
  for (int k = 0; k < n_visited; ++k) {
    const int v = order[k];
    // the marked bonds written at v, in the order of the text: pass 0 the bond to the parent, pass 1 the opening closures
    for (int pass = 0; pass < 2; ++pass) {
      for (int w = 0; w < 2; ++w) {
        smi_u64 m = pass == 0 ? (w == 0 ? 1ull : 0ull) : p0[2 * v + w] | p1[2 * v + w];
        for (int i = 0; i < 64 && m; ++i) {
          const int u = pass == 0 ? parent[v] : w * 64 + smi_ctz64(m);
          m &= m - 1ull;
          if (u < 0 || u >= n) continue;                              // no parent; (u >= n: guard)
          if (pass == 1 && (u == parent[v] || parent[u] == v || rank[u] < rank[v])) continue;
          if (mark[smi_pair(n, v, u)] != kSmiTodo) continue;
          // ---- a new component: this bond is '/' ----
          mark[smi_pair(n, v, u)] = kSmiUp;
          const int head0 = tail;
          int comp_marked = 1;
          bool bad = false;
          for (int side = 0; side < 2; ++side) {
            const int x = side == 0 ? v : u;
            const bool seen = ((x < 64 ? vis0 >> x : vis1 >> (x - 64)) & 1ull) != 0ull;
            if (partner[x] < 0 || seen || tail >= n) continue;
            const int y = partner[x];
            if (x < 64) vis0 |= 1ull << x; else vis1 |= 1ull << (x - 64);
            if (y < 64) vis0 |= 1ull << y; else vis1 |= 1ull << (y - 64);
            queue[tail++] = (int16_t)x;
          }
          for (int head = head0; head < tail; ++head) {               // (tail <= n: every double bond enters once)
            const int qa = queue[head], qb = partner[qa];
            const int a = qa < qb ? qa : qb, b = qa < qb ? qb : qa, s = sval[a];
            int r[4];
            smi_stereo_subs(p0, p1, a, b, &r[0], &r[1]);
            smi_stereo_subs(p0, p1, b, a, &r[2], &r[3]);
            // c: the mark of the bond x - r relative to the double bond's sign
            int c[4], g = 0;
            for (int j = 0; j < 4; ++j) {
              const int x = j < 2 ? a : b;
              c[j] = 0;
              if (r[j] < 0 || r[j] >= n) continue;
              c[j] = (rank[x] < rank[r[j]] ? 1 : -1) * ((j & 1) ? -1 : 1) * (j < 2 ? 1 : s);
              const int mk = mark[smi_pair(n, x, r[j])];
              if (g == 0 && mk == kSmiUp) g = c[j];
              if (g == 0 && mk == kSmiDown) g = -c[j];
            }
            if (g == 0) continue;                                     // (guard: a double bond enters over a bond that has its mark)
            for (int j = 0; j < 4; ++j) {
              if (c[j] == 0) continue;
              const int x = j < 2 ? a : b, row = smi_pair(n, x, r[j]);
              const uint8_t want = g * c[j] > 0 ? kSmiUp : kSmiDown;
              if (mark[row] == kSmiTodo) {
                mark[row] = want;
                ++comp_marked;
              } else if (mark[row] != want) {
                bad = true;
              }
              const int z = r[j];
              const bool seen = ((z < 64 ? vis0 >> z : vis1 >> (z - 64)) & 1ull) != 0ull;
              if (partner[z] < 0 || seen || tail >= n) continue;
              const int y = partner[z];
              if (z < 64) vis0 |= 1ull << z; else vis1 |= 1ull << (z - 64);
              if (y < 64) vis0 |= 1ull << y; else vis1 |= 1ull << (y - 64);
              queue[tail++] = (int16_t)z;
            }
          }
          if (bad) {                                                  // the component's marks are dropped
            ++dropped;
            for (int head = head0; head < tail; ++head) {
              const int qa = queue[head], qb = partner[qa];
              int r[4];
              smi_stereo_subs(p0, p1, qa, qb, &r[0], &r[1]);
              smi_stereo_subs(p0, p1, qb, qa, &r[2], &r[3]);
              for (int j = 0; j < 4; ++j)
                if (r[j] >= 0 && r[j] < n) mark[smi_pair(n, j < 2 ? qa : qb, r[j])] = 0;
            }
          } else {
            marked += comp_marked;
            expressed += tail - head0;
          }
        }
      }
    }
  }
  *n_marked = marked;
  *n_expressed = expressed;
  return dropped;
}

// ---- the text of one atom -----------------------------------------------------------------------------------------------------------
template <class Put>
PG_SMI_HD void smi_put_bond(int o, Put&& put) {
  if (o == 2) put('=');
  if (o == 3) put('#');
}

// a single bond that carries a stereo mark is written as the mark
template <class Put>
PG_SMI_HD void smi_put_bond_mark(int o, int mk, Put&& put) {
  if (o == 1 && mk == kSmiUp) put('/');
  if (o == 1 && mk == kSmiDown) put('\\');
  smi_put_bond(o, put);
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
// hydrogens and charge, val: the notation's valence list of its element (empty: never bare).  A centre (smi_centre_ok) is a bracket
// atom with '@' or '@@' between symbol and 'H'; a single bond with a mark is written as '/' or '\\' where its symbol would stand.
// parity: the atom's stereo parity (0: none), mark: the marks of the bonds at their pair rows (smiles_stereo_marks; nullptr: none).
// Returns kSmiBracket | kSmiCentre (written with '@' or '@@') | kSmiClockwise ('@@').
template <class Put>
PG_SMI_HD int smiles_atom_text_stereo(int v, int n, int el, int h, int q, const uint8_t* val, const smi_u64* p0, const smi_u64* p1,
                                      const int16_t* rank, const int16_t* parent, const uint8_t* flags, const uint8_t* label, int parity,
                                      const uint8_t* mark, Put&& put) {
  const uint8_t f = flags[v];
  const int up = parent[v];
  if (f & kSmiDot) put('.');
  if (f & kSmiPrev) put(')');
  if (f & kSmiNext) put('(');
  if (up >= 0) smi_put_bond_mark(smi_order(p0, p1, v, up), mark ? mark[smi_pair(n, v, up)] : 0, put);
  // ---- the atom token ----
  const int sum = smi_popc64(p0[2 * v]) + smi_popc64(p0[2 * v + 1]) + 2 * (smi_popc64(p1[2 * v]) + smi_popc64(p1[2 * v + 1]));
  const bool centre = smi_centre_ok(parity, smi_degree(p0, p1, v), h);
  const bool clockwise = centre && parity * smi_centre_sign(v, n, h, p0, p1, rank, parent) < 0;
  const bool bracket = centre || !(val[0] != 0 && q == 0 && smi_implicit_h(val, sum) == h);
  // B C N O F Si P S | Cl Br I: the first letters packed a byte each, the second letters by class
  const char c1 = (char)(((el < 8 ? 0x535053464F4E4342ull >> (8 * el) : 0x494243ull >> (8 * (el - 8)))) & 0xffull);
  const char c2 = el == kSmiSi ? 'i' : el == 8 ? 'l' : el == 9 ? 'r' : (char)0;
  if (bracket) put('[');
  put(c1);
  if (c2) put(c2);
  if (centre) put('@');
  if (clockwise) put('@');
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
        if (pass == 1) smi_put_bond_mark(smi_order(p0, p1, v, u), mark ? mark[smi_pair(n, v, u)] : 0, put);
        smi_put_label(label[smi_pair(n, v, u)], put);
      }
    }
  }
  return (bracket ? kSmiBracket : 0) | (centre ? kSmiCentre : 0) | (clockwise ? kSmiClockwise : 0);
}

// the text without stereo; returns true for a bracket atom
template <class Put>
PG_SMI_HD bool smiles_atom_text(int v, int n, int el, int h, int q, const uint8_t* val, const smi_u64* p0, const smi_u64* p1,
                                const int16_t* rank, const int16_t* parent, const uint8_t* flags, const uint8_t* label, Put&& put) {
  return (smiles_atom_text_stereo(v, n, el, h, q, val, p0, p1, rank, parent, flags, label, 0, nullptr, put) & kSmiBracket) != 0;
}

}  // namespace pg
