// The rules of the property descriptors (DESIGN.md 2.9 "Properties"): an atom's environment word in its two passes, the row an atom
// takes in a contribution table, what an atom and a bond add to the counts, and the limits.  Plain functions over caller-supplied
// arrays, compiled for the device by mol_props.hip (all arrays in LDS) and for the host by tools/props_host_check.cpp (the same text
// under the host sanitizers).  Integer work only.
//
// Every loop here walks the set bits of a 64-bit mask word with a trip count bounded by 64, or the rows of a table with a trip count
// bounded by PG_PROP_MAX_ROWS, or a fixed number of slots: termination never rests on what the arrays hold.  An atom index is only
// ever taken from a mask bit below n.
#pragma once
#include <stdint.h>
#include "../../include/phoregen_hip.h"

#if defined(__HIPCC__)
#define PG_PROP_HD __host__ __device__ inline
#else
#define PG_PROP_HD inline
#endif

namespace pg {

// atom classes (ATOM_TYPES order)
constexpr int kPropC = 1, kPropN = 2, kPropO = 3, kPropF = 4, kPropP = 6, kPropS = 7, kPropCl = 8, kPropBr = 9, kPropI = 10;
// a pair row's byte: the Kekulé order if it is 1..3 (else 0) of a bond between kept atoms; screen order 4; ring_size > 0; a bond at all
constexpr uint8_t kPropOrder = 3, kPropArom = 4, kPropRingBond = 8, kPropBond = 16;
// the one-bit fields of the word
constexpr int kEnvQ = 1 << PG_PROP_ENV_Q, kEnvArom = 1 << PG_PROP_ENV_AROM, kEnvTriple = 1 << PG_PROP_ENV_TRIPLE,
              kEnvRing = 1 << PG_PROP_ENV_RING, kEnvRing3 = 1 << PG_PROP_ENV_RING3, kEnvDblO = 1 << PG_PROP_ENV_DBL_O,
              kEnvDblHet = 1 << PG_PROP_ENV_DBL_HET, kEnvNbDblHet = 1 << PG_PROP_ENV_NB_DBL_HET;

// One graph.  el [n]: atom class, -1 = dropped; h, q [n]: hydrogens and charge; aring [n]: the rings' atom_ring; adj [2 n]: an atom's
// bonds as a bit per local index (rows of dropped atoms are 0, no bit at or above n); pair [n (n - 1) / 2]: the pair rows' bytes;
// env [n]: the words of the first pass (prop_env_own) of all atoms, which the second (prop_env_nbr) reads.
struct PropGraph {
  int n;
  const int8_t* el;
  const uint8_t* h;
  const int8_t* q;
  const uint8_t* aring;
  const unsigned long long* adj;
  const uint8_t* pair;
  const int* env;
};

PG_PROP_HD int prop_ctz64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)m) - 1;
#else
  return __builtin_ctzll(m);
#endif
}

PG_PROP_HD int prop_popc(unsigned int m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(m);
#else
  return __builtin_popcount(m);
#endif
}

PG_PROP_HD int prop_min(int a, int b) { return a < b ? a : b; }

// the byte of a pair row from the screen's order o (a bond between kept atoms), the Kekulé order k and the row's ring_size
PG_PROP_HD int prop_pair_byte(int o, int k, int ring_size) {
  return kPropBond | ((k >= 1 && k <= 3) ? k : 0) | (o == 4 ? kPropArom : 0) | (ring_size > 0 ? kPropRingBond : 0);
}

// byte of the pair (a, b), a != b: row a n - a (a + 1) / 2 + b - a - 1 for a < b
PG_PROP_HD int prop_pair(const PropGraph& g, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return g.pair[lo * g.n - lo * (lo + 1) / 2 + hi - lo - 1];
}

PG_PROP_HD bool prop_is_single(int pb) { return (pb & (kPropOrder | kPropArom)) == 1; }   // Kekulé order 1, screen order not 4
PG_PROP_HD bool prop_is_double(int pb) { return (pb & (kPropOrder | kPropArom)) == 2; }   // Kekulé order 2, screen order not 4
PG_PROP_HD bool prop_is_triple(int pb) { return (pb & kPropOrder) == 3; }
PG_PROP_HD bool prop_is_halogen(int el) { return el == kPropF || el == kPropCl || el == kPropBr || el == kPropI; }
PG_PROP_HD bool prop_is_nops(int el) { return el == kPropN || el == kPropO || el == kPropP || el == kPropS; }

PG_PROP_HD int prop_field(int env, int shift, int width) { return (env >> shift) & ((1 << width) - 1); }
PG_PROP_HD int prop_el(int env) { return prop_field(env, PG_PROP_ENV_EL, 4); }
PG_PROP_HD int prop_deg(int env) { return prop_field(env, PG_PROP_ENV_DEG, 3); }

// First pass: every field of atom i's word that reads the atom's own bonds and its neighbours' classes (-1 for a dropped atom).
PG_PROP_HD int prop_env_own(const PropGraph& g, int i) {
  const int el = g.el[i];
  if (el < 0) return -1;
  int deg = 0, n_dbl = 0, nb_het = 0, nb_hal = 0, nb_no = 0, flags = 0;
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * i + w];
    for (int k = 0; k < 64 && m; ++k) {
      const int b = w * 64 + prop_ctz64(m);
      m &= m - 1ull;
      const int pb = prop_pair(g, i, b), eb = g.el[b];
      ++deg;
      if ((pb & (kPropArom | kPropRingBond)) == (kPropArom | kPropRingBond)) flags |= kEnvArom;
      if (prop_is_double(pb)) {
        ++n_dbl;
        if (eb == kPropO) flags |= kEnvDblO;
        if (prop_is_nops(eb)) flags |= kEnvDblHet;
      }
      if (prop_is_triple(pb)) flags |= kEnvTriple;
      nb_het += eb != kPropC;
      nb_hal += prop_is_halogen(eb);
      nb_no += eb == kPropN || eb == kPropO;
    }
  }
  const int ar = g.aring[i];
  return el | prop_min(g.h[i], 7) << PG_PROP_ENV_H | (g.q[i] > 0 ? kEnvQ : 0) | prop_min(deg, 7) << PG_PROP_ENV_DEG |
         prop_min(n_dbl, 3) << PG_PROP_ENV_N_DBL | (ar > 0 ? kEnvRing : 0) | (ar == 3 ? kEnvRing3 : 0) |
         prop_min(nb_het, 7) << PG_PROP_ENV_NB_HET | prop_min(nb_hal, 3) << PG_PROP_ENV_NB_HAL | prop_min(nb_no, 7) << PG_PROP_ENV_NB_NO |
         flags;
}

// Second pass: the fields that read a neighbour's flags in g.env -- nb_arom and nb_dbl_het -- to be or-ed into the first pass's word
// of a kept atom.
PG_PROP_HD int prop_env_nbr(const PropGraph& g, int i) {
  int nb_arom = 0, flags = 0;
  for (int w = 0; w < 2; ++w) {
    unsigned long long m = g.adj[2 * i + w];
    for (int k = 0; k < 64 && m; ++k) {
      const int b = w * 64 + prop_ctz64(m);
      m &= m - 1ull;
      const int eb = g.env[b];
      nb_arom += (eb & kEnvArom) != 0;
      if (prop_is_single(prop_pair(g, i, b)) && (eb & kEnvDblHet)) flags |= kEnvNbDblHet;
    }
  }
  return prop_min(nb_arom, 3) << PG_PROP_ENV_NB_AROM | flags;
}

// The first of the n_rows rows (mask, value, atom, per_h) with (env & mask) == value: its index, or -1.  n_rows <= PG_PROP_MAX_ROWS.
PG_PROP_HD int prop_match(const int* rows, int n_rows, int env) {
  for (int r = 0; r < n_rows && r < PG_PROP_MAX_ROWS; ++r)
    if ((env & rows[PG_PROP_ROW_INTS * r]) == rows[PG_PROP_ROW_INTS * r + 1]) return r;
  return -1;
}

// what an atom with h hydrogens adds under a row (|atom|, |per_h| < 2^20 and h < 256: no overflow)
PG_PROP_HD int prop_contribution(const int* row, int h) { return row[2] + h * row[3]; }

// What the kept atom with the final word `env`, h hydrogens and charge q adds to the count columns (the per-bond columns, untyped
// and violations stay 0 here).
PG_PROP_HD void prop_atom_counts(int env, int h, int q, int* c) {
  const int el = prop_el(env);
  const bool no = el == kPropN || el == kPropO;
  c[PG_PROP_C_HEAVY_ATOMS] += 1;
  c[PG_PROP_C_HYDROGENS] += h;
  c[PG_PROP_C_CARBONS] += el == kPropC;
  c[PG_PROP_C_SP3_CARBONS] += el == kPropC && !(env & (kEnvArom | kEnvTriple | (3 << PG_PROP_ENV_N_DBL)));
  c[PG_PROP_C_HETEROATOMS] += el != kPropC;
  c[PG_PROP_C_HALOGENS] += prop_is_halogen(el);
  c[PG_PROP_C_NHOH] += no ? h : 0;
  c[PG_PROP_C_NO_COUNT] += no;
  c[PG_PROP_C_AROMATIC_ATOMS] += (env & kEnvArom) != 0;
  c[PG_PROP_C_RING_ATOMS] += (env & kEnvRing) != 0;
  c[PG_PROP_C_NET_CHARGE] += q;
}

// A bond with the pair byte pb between atoms with the final words ea and eb: 0 = neither, 1 = rotatable, 2 = an amide bond.
PG_PROP_HD int prop_bond_kind(int pb, int ea, int eb) {
  if (!prop_is_single(pb) || (pb & kPropRingBond)) return 0;
  const int la = prop_el(ea), lb = prop_el(eb);
  if ((la == kPropC && (ea & kEnvDblO) && lb == kPropN) || (lb == kPropC && (eb & kEnvDblO) && la == kPropN)) return 2;
  return prop_deg(ea) >= 2 && prop_deg(eb) >= 2 && !((ea | eb) & kEnvTriple);
}

// The bits of `violated`: quantity k (PG_PROP_L_*) of v [PG_PROP_N_LIMITS] below lim[2 k] or above lim[2 k + 1].
PG_PROP_HD int prop_violated(const int* v, const int* lim) {
  int out = 0;
  for (int k = 0; k < PG_PROP_N_LIMITS; ++k) out |= (v[k] < lim[2 * k] || v[k] > lim[2 * k + 1]) ? 1 << k : 0;
  return out;
}

PG_PROP_HD int prop_status(bool kekule_ok, int violated, int max_violations, int untyped) {
  if (!kekule_ok) return PG_PROP_NO_KEKULE;
  return (prop_popc((unsigned int)violated) > max_violations ? PG_PROP_LIMITS : 0) | (untyped > 0 ? PG_PROP_UNTYPED : 0);
}

}  // namespace pg
