// The per-atom rules of the pharmacophore feature typing (DESIGN.md 2.9 "Features"): the reference's SMARTS per feature type
// (datasets/generate_phorefp.py:39-98), restated as integer rules over the screen's, the rings' and the Kekulé form's arrays.  Plain
// functions over caller-supplied arrays, compiled for the device by mol_feat.hip (all arrays in LDS) and for the host by
// tools/feature_host_check.cpp (the same text under the host sanitizers).  Integer work only.
//
// Every loop here walks the set bits of a 64-bit mask word with a trip count bounded by 64, or a fixed number of slots: termination
// never rests on what the arrays hold.  An atom index is only ever taken from a mask bit below n.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FEAT_HD __host__ __device__ inline
#else
#define PG_FEAT_HD inline
#endif

namespace pg {

// bits of an atom's byte, in the order of FEATURE_TYPES
constexpr int kFeatHD = 1, kFeatAR = 2, kFeatPO = 4, kFeatHA = 8, kFeatHY = 16, kFeatNE = 32, kFeatXB = 64;
constexpr int kFeatTypes = 7;
// atom classes (ATOM_TYPES order)
constexpr int kElC = 1, kElN = 2, kElO = 3, kElF = 4, kElP = 6, kElS = 7, kElCl = 8, kElBr = 9, kElI = 10;
// a pair row's byte: the Kekulé order (1..3) of a bond between kept atoms, 0 = no bond; screen order 4; ring_size > 0
constexpr uint8_t kPairOrder = 3, kPairArom = 4, kPairRing = 8;
// an atom's flags: `arom`; has a double bond to an aliphatic O, N, P or S; has such a bond that is no ring bond
constexpr uint8_t kAtomArom = 1, kAtomDbl = 2, kAtomDblOpen = 4;

// One graph.  el [n]: atom class, -1 = dropped; h, q [n]: hydrogens and charge; adj [2 n]: an atom's bonds as a bit per local index
// (rows of dropped atoms are 0, no bit at or above n); pair [n (n - 1) / 2]: the pair rows' bytes; deg, v, flags [n]: filled by the
// caller from feat_atom_sums (all atoms) and then feat_atom_dbl (all atoms) before feat_atom_bits is asked.
struct FeatGraph {
  int n;
  const int8_t* el;
  const uint8_t* h;
  const uint8_t* q;
  const unsigned long long* adj;
  const uint8_t* pair;
  const uint8_t* deg;
  const uint16_t* v;
  const uint8_t* flags;
};

PG_FEAT_HD int feat_ctz64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)m) - 1;
#else
  return __builtin_ctzll(m);
#endif
}

PG_FEAT_HD int feat_popc64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// byte of the pair (a, b), a != b: row a n - a (a + 1) / 2 + b - a - 1 for a < b
PG_FEAT_HD int feat_pair(const FeatGraph& g, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return g.pair[lo * g.n - lo * (lo + 1) / 2 + hi - lo - 1];
}

PG_FEAT_HD bool feat_is_single(int pb) { return (pb & kPairOrder) == 1; }
PG_FEAT_HD bool feat_is_double(int pb) { return (pb & (kPairOrder | kPairArom)) == 2; }   // Kekulé order 2, screen order not 4
PG_FEAT_HD bool feat_is_onps(int el) { return el == kElO || el == kElN || el == kElP || el == kElS; }

// deg = kept heavy neighbours, v = sum of the Kekulé orders + h, arom = a bond of screen order 4 that is a ring bond
PG_FEAT_HD void feat_atom_sums(const FeatGraph& g, int i, int* deg, int* v, int* arom) {
  int d = 0, s = g.h[i], ar = 0;
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * i + w];
    for (int k = 0; k < 64 && m; ++k) {
      const int b = w * 64 + feat_ctz64(m);
      m &= m - 1ull;
      const int pb = feat_pair(g, i, b);
      ++d;
      s += pb & kPairOrder;
      ar |= (pb & (kPairArom | kPairRing)) == (kPairArom | kPairRing);
    }
  }
  *deg = d, *v = s, *arom = ar;
}

// kAtomDbl / kAtomDblOpen of atom i: `*=[O,N,P,S]` and `*=!@[O,N,P,S]` (needs every atom's kAtomArom)
PG_FEAT_HD int feat_atom_dbl(const FeatGraph& g, int i) {
  int out = 0;
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * i + w];
    for (int k = 0; k < 64 && m; ++k) {
      const int z = w * 64 + feat_ctz64(m);
      m &= m - 1ull;
      const int pb = feat_pair(g, i, z);
      if (feat_is_double(pb) && feat_is_onps(g.el[z]) && !(g.flags[z] & kAtomArom)) out |= kAtomDbl | ((pb & kPairRing) ? 0 : kAtomDblOpen);
    }
  }
  return out;
}

// Rule 6c's tail: the O atom o (bonded to the centre c) has a single-bonded neighbour other than c and x whose h is not 1
PG_FEAT_HD bool feat_ne_tail(const FeatGraph& g, int o, int c, int x) {
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * o + w];
    for (int k = 0; k < 64 && m; ++k) {
      const int t = w * 64 + feat_ctz64(m);
      m &= m - 1ull;
      if (t != c && t != x && feat_is_single(feat_pair(g, o, t)) && g.h[t] != 1) return true;
    }
  }
  return false;
}

// Rule 6 from its centre c: the atoms it marks NE, as a bit per local index in out[2].
//   [CX3,SX3,PD3](=[O,S])[O;H0&-1,OH1]            marks the =O/S and the OH             (6a)
//   [PX4](=[O,S])([O;H0&-1,OH1])[O;H0&-1,OH1]      marks all three                       (6b)
//   [PX4](=[O,S])([O;H0&-1,OH1])[O][*;!H]          marks the =O/S and the OH             (6c)
//   [SX4](=[O,S])(=[O,S])([O;H0&-1,OH1])           marks all three                       (6d)
// (no anions: every H0&-1 alternative is dead).  A centre has X = deg + h of 3 or 4, so at most four neighbours.  An O with h = 1 has
// valence 1, i.e. the centre is its only neighbour: it is never the tail's atom and never a second role.  Every match marks its own
// atoms, so the union over the matches of a pattern is: all =O/S and all OH once the pattern has one match (6a, 6b, 6d); for 6c the
// =O/S atoms x for which a tail exists, and all OH.
PG_FEAT_HD void feat_ne_marks(const FeatGraph& g, int c, unsigned long long* out) {
  out[0] = out[1] = 0ull;
  const int el = g.el[c], deg = g.deg[c], X = deg + g.h[c];
  if ((el != kElC && el != kElS && el != kElP) || (g.flags[c] & kAtomArom) || deg > 4) return;
  const bool a6 = (el == kElC && X == 3) || (el == kElS && X == 3) || (el == kElP && deg == 3);
  const bool b6 = el == kElP && X == 4, d6 = el == kElS && X == 4;
  if (!(a6 || b6 || d6)) return;
  int nb[4], role[4], n_nb = 0, n_dbl = 0, n_oh = 0;                // role: 1 = the =O/S, 2 = O with h = 1, 4 = single-bonded O
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * c + w];
    for (int k = 0; k < 64 && m && n_nb < 4; ++k) {
      const int z = w * 64 + feat_ctz64(m);
      m &= m - 1ull;
      const int pb = feat_pair(g, c, z), ez = g.el[z];
      int r = 0;
      if (!(g.flags[z] & kAtomArom)) {
        if (feat_is_double(pb) && (ez == kElO || ez == kElS)) r = 1;
        if (feat_is_single(pb) && ez == kElO) r = g.h[z] == 1 ? 6 : 4;
      }
      n_dbl += r == 1;
      n_oh += (r & 2) != 0;
      nb[n_nb] = z, role[n_nb] = r;
      ++n_nb;
    }
  }
  if (n_oh < 1 || n_dbl < 1) return;
  const bool all = a6 || (b6 && n_oh >= 2) || (d6 && n_dbl >= 2);
  bool any = all;
  for (int i = 0; i < n_nb; ++i) {
    if (role[i] != 1) continue;
    bool hit = all;
    if (!hit && b6)
      for (int j = 0; j < n_nb; ++j) hit = hit || ((role[j] & 4) && feat_ne_tail(g, nb[j], c, nb[i]));
    if (hit) out[nb[i] >> 6] |= 1ull << (nb[i] & 63);
    any = any || hit;
  }
  if (!any) return;
  for (int i = 0; i < n_nb; ++i)
    if (role[i] & 2) out[nb[i] >> 6] |= 1ull << (nb[i] & 63);
}

// The byte of atom i (0 for a dropped atom)
PG_FEAT_HD int feat_atom_bits(const FeatGraph& g, int i) {
  const int el = g.el[i];
  if (el < 0) return 0;
  const int h = g.h[i], q = g.q[i], deg = g.deg[i], v = g.v[i], X = deg + h;
  const bool ar = (g.flags[i] & kAtomArom) != 0;
  const bool os = el == kElO || el == kElS;
  // one walk over the neighbours collects what the rules ask of them
  int n_single = 0, n_dbl = 0;                                      // aliphatic N neighbours, bonded single / double (3b)
  bool nof = false, free_single = false, amide_like = false, single_c = false, ne = false;
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * i + w];
    for (int k = 0; k < 64 && m; ++k) {
      const int b = w * 64 + feat_ctz64(m);
      m &= m - 1ull;
      const int pb = feat_pair(g, i, b), eb = g.el[b], fb = g.flags[b];
      const bool single = feat_is_single(pb);
      if (eb == kElN && !(fb & kAtomArom)) {
        n_single += single;
        n_dbl += feat_is_double(pb);
      }
      nof = nof || eb == kElN || eb == kElO || eb == kElF;
      free_single = free_single || (single && !(fb & kAtomDbl));
      amide_like = amide_like || (single && (fb & kAtomDblOpen));
      single_c = single_c || (single && eb == kElC);
      if (os && !ne) {                                              // rule 6, seen from the marked atom: is b a centre that marks i
        unsigned long long marks[2];
        feat_ne_marks(g, b, marks);
        ne = (marks[i >> 6] >> (i & 63)) & 1ull;
      }
    }
  }
  int out = 0;
  // HD  [#7,#8,#16;+0,+1,+2;!H0]
  if ((el == kElN || os) && h >= 1) out |= kFeatHD;
  // AR  [a]
  if (ar) out |= kFeatAR;
  // PO  [+;!$([N+]-[O-])]  |  N-C(-N)=N at the C
  if (q > 0 || (el == kElC && !ar && n_single >= 2 && n_dbl >= 1)) out |= kFeatPO;
  // HA  $([O,S;H1;v2]-[!$(*=[O,N,P,S])])  $([O,S;H0;v2])  $([N;v3;!$(N-*=!@[O,N,P,S])])  $([nH0,o,s;+0])
  if (!ar && os && v == 2 && (h == 0 || (h == 1 && free_single))) out |= kFeatHA;
  if (!ar && el == kElN && v == 3 && !amide_like) out |= kFeatHA;
  if (ar && q == 0 && ((el == kElN && h == 0) || os)) out |= kFeatHA;
  // HY  [c,s,S&H0&v2,Br,I,$([#6;+0;!$([#6;$([#6]~[#7,#8,#9])])])]
  if ((ar && (el == kElC || el == kElS)) || (!ar && el == kElS && h == 0 && v == 2) || el == kElBr || el == kElI ||
      (el == kElC && q == 0 && !nof))
    out |= kFeatHY;
  // NE  (feat_ne_marks)
  if (ne) out |= kFeatNE;
  // XB  [#6]-[Cl,Br,I;X1]
  if ((el == kElCl || el == kElBr || el == kElI) && X == 1 && deg == 1 && single_c) out |= kFeatXB;
  return out;
}

}  // namespace pg
