// The core of the hydrogen placement (DESIGN.md 2.9 "Hydrogens"): the shape of a site by the integer rule, and the directions of its
// hydrogens by (shape, heavy neighbours, hydrogens).  One function per site over the graph's atoms and adjacency rows, compiled for the
// device by mol_hydrogens.hip (one atom per lane and pass) and for the host by tools/hydrogen_host_check.cpp (the same text under the
// host sanitizers).  It reads atoms[0 .. n) and adj[0 .. 2 n) at the indices the adjacency rows hold, so rows that only name atoms
// below n cannot make it index out of bounds; it writes nothing but its result.
//
// The geometry is fp32.  A vector is normalised only if its squared norm passes `q >= limit && q < inf`, written so that a NaN fails
// without a test of its own.  The dot products with the four fixed vertices are a sum of +/- components times 1/sqrt(3): the build may
// contract a * b + c, and this form leaves nothing to contract, so exactly tied vertices stay tied.
#pragma once
#include <math.h>
#include "mol_common.h"

namespace pg {

constexpr int kHydTet = PG_HYD_SHAPE_TETRAHEDRAL, kHydTrig = PG_HYD_SHAPE_TRIGONAL, kHydLin = PG_HYD_SHAPE_LINEAR,
              kHydGeneric = PG_HYD_SHAPE_GENERIC;
constexpr int kHydMaxH = PG_HYD_MAX_PER_ATOM;
constexpr float kHydEps2 = PG_HYD_DEG_EPS * PG_HYD_DEG_EPS;

// An atom as the core reads it.  info: bits 0..3 the class (kHydDropped: not kept), kHydNonfinite, kHydTriple (it has a bond of
// Kekulé order 3), kHydArom (a bond of the screen's order 4), bits 8..15 its hydrogens, bits 16..23 its bonds of Kekulé order 2.
struct alignas(16) HydAtom {
  float x, y, z;
  unsigned info;
};
constexpr unsigned kHydDropped = 15u, kHydNonfinite = 1u << 4, kHydTriple = 1u << 5, kHydArom = 1u << 6;
constexpr int kHydHShift = 8, kHydDoubleShift = 16;
constexpr int kHydClassN = 2;               // ATOM_TYPES order: B C N O F Si P S Cl Br I

struct HydVec {
  float x, y, z;
};
struct HydOut {                             // the hydrogens of one site, slot by slot (named, so that no index puts them into memory)
  HydVec h0, h1, h2, h3;
};

PG_MOL_HD HydVec hv_add(HydVec a, HydVec b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
PG_MOL_HD HydVec hv_sub(HydVec a, HydVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
PG_MOL_HD HydVec hv_scale(HydVec a, float s) { return {a.x * s, a.y * s, a.z * s}; }
PG_MOL_HD HydVec hv_neg(HydVec a) { return {-a.x, -a.y, -a.z}; }
PG_MOL_HD float hv_dot(HydVec a, HydVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PG_MOL_HD HydVec hv_cross(HydVec a, HydVec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
PG_MOL_HD HydVec hv_of(const HydAtom& a) { return {a.x, a.y, a.z}; }
// the distance of two points as the contact pass takes it (sqrtf of the squared distance, as pg_mol_geom does)
PG_MOL_HD float hyd_dist(HydVec a, HydVec b) {
  const HydVec d = hv_sub(a, b);
  return sqrtf(hv_dot(d, d));
}

// v / |v| into u if limit <= |v|^2 < inf (limit 0: any positive squared norm); false, and u untouched, otherwise
PG_MOL_HD bool hyd_unit(HydVec v, float limit, HydVec& u) {
  const float q = hv_dot(v, v);
  if (!(q >= limit) || !(q > 0.0f) || !(q < INFINITY)) return false;
  const float len = sqrtf(q);
  u = {v.x / len, v.y / len, v.z / len};
  return true;
}

// ---- the four fixed vertices (1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1) / sqrt(3) ----------------------------------------------------------
constexpr float kHydInvSqrt3 = 0.57735026918962576f;
PG_MOL_HD HydVec hyd_vertex(int m) {
  const float c = kHydInvSqrt3;
  return {m < 2 ? c : -c, (m == 0 || m == 2) ? c : -c, (m == 0 || m == 3) ? c : -c};
}
// per vertex the largest dot product with the directions added so far (-inf: none)
struct HydMax {
  float m0, m1, m2, m3;
};
PG_MOL_HD void hyd_max_add(HydMax& v, HydVec e) {
  const float c = kHydInvSqrt3;
  v.m0 = fmaxf(v.m0, c * ((e.x + e.y) + e.z));
  v.m1 = fmaxf(v.m1, c * ((e.x - e.y) - e.z));
  v.m2 = fmaxf(v.m2, c * ((e.y - e.x) - e.z));
  v.m3 = fmaxf(v.m3, c * ((e.z - e.x) - e.y));
}
// the vertex with the smallest such maximum (the first minimum), which then counts as a direction itself
PG_MOL_HD HydVec hyd_max_pick(HydMax& v) {
  const float c = kHydInvSqrt3;
  float best = v.m0, sy = c, sz = c;                                // (selects of the signs, not an index: nothing to put into memory)
  const bool b1 = v.m1 < best;
  best = b1 ? v.m1 : best, sy = b1 ? -c : sy, sz = b1 ? -c : sz;
  const bool b2 = v.m2 < best;
  best = b2 ? v.m2 : best, sy = b2 ? c : sy, sz = b2 ? -c : sz;
  const bool b3 = v.m3 < best;
  sy = b3 ? -c : sy, sz = b3 ? c : sz;
  const HydVec e = {(b2 || b3) ? -c : c, sy, sz};
  hyd_max_add(v, e);
  return e;
}

// ---- the integer rule ---------------------------------------------------------------------------------------------------------------------
// n_double: the atom's bonds of Kekulé order 2; conj: a heavy neighbour has a bond of Kekulé order 2 or of the screen's order 4
PG_MOL_HD int hyd_shape(int cls, int n_double, bool triple, bool arom, int d, int h, bool conj) {
  if (triple || n_double >= 2) return kHydLin;
  if (n_double >= 1 || arom || (cls == kHydClassN && d + h == 3 && conj)) return kHydTrig;
  return kHydTet;
}

// cos u0 + sin (cp e1 + sp e2)
PG_MOL_HD HydVec hyd_cone(HydVec u0, HydVec e1, HydVec e2, float cs, float sn, float cp, float sp) {
  const HydVec w = hv_add(hv_scale(e1, cp), hv_scale(e2, sp));
  return hv_add(hv_scale(u0, cs), hv_scale(w, sn));
}

// The hydrogens of atom i: their number (0: no site -- dropped, without hydrogens or with more than kHydMaxH, or a non-finite
// coordinate at it or next to it), their positions in o (unused slots 0) and the shape that placed them.  adj: two 64-bit words per
// atom, bit j of row i = i and j are joined by a pair row of Kekulé order 1..3 and both are kept; xh: the X-H length per class.
PG_MOL_HD int hyd_site(const HydAtom* atoms, const unsigned long long* adj, int i, const float* xh, HydOut& o, int& shape_used) {
  const HydVec zero = {0.0f, 0.0f, 0.0f};
  o = {zero, zero, zero, zero};
  shape_used = 0;
  const HydAtom a = atoms[i];
  const int cls = (int)(a.info & 15u), h = (int)((a.info >> kHydHShift) & 255u);
  if (cls > 10 || h < 1 || h > kHydMaxH || (a.info & kHydNonfinite)) return 0;
  const HydVec p = hv_of(a);
  const unsigned long long row0 = adj[2 * i], row1 = adj[2 * i + 1];
  const int d = __builtin_popcountll(row0) + __builtin_popcountll(row1);

  // ---- one pass over the heavy neighbours, ascending: unit vectors, their sum, the vertices' dot products ---------------------------
  HydVec u0 = zero, u1 = zero, sum = zero;                          // the first neighbour's (below) and the last one's (d = 2: the two)
  HydMax vmax = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int valid = 0, j0 = -1;
  bool conj = false, next_bad = false;
  for (int w = 0; w < 2; ++w) {
    for (unsigned long long m = w ? row1 : row0; m; m &= m - 1ull) {
      const int j = w * 64 + __builtin_ctzll(m);
      const HydAtom b = atoms[j];
      next_bad = next_bad || (b.info & kHydNonfinite);
      conj = conj || (b.info & kHydArom) || ((b.info >> kHydDoubleShift) & 255u) >= 1u;
      j0 = j0 < 0 ? j : j0;
      HydVec u;
      if (hyd_unit(hv_sub(hv_of(b), p), 0.0f, u)) {      // (a neighbour that coincides with the atom is left out)
        u1 = u;
        sum = hv_add(sum, u);
        hyd_max_add(vmax, u);
        ++valid;
      }
    }
  }
  if (next_bad) return 0;
  if (j0 >= 0) hyd_unit(hv_sub(hv_of(atoms[j0]), p), 0.0f, u0);       // (again, not kept from the pass: a select by `valid` becomes an indexed copy in memory)
  const int shape = hyd_shape(cls, (int)((a.info >> kHydDoubleShift) & 255u), (a.info & kHydTriple) != 0, (a.info & kHydArom) != 0, d, h, conj);

  // ---- the table ----------------------------------------------------------------------------------------------------------------------
  const float cs = shape == kHydTet ? -1.0f / 3.0f : -0.5f, sn = shape == kHydTet ? 0.94280904158206337f : 0.86602540378443865f;
  HydVec d0 = zero, d1 = zero, d2 = zero, d3 = zero, t = zero;
  bool generic = valid != d;
  if (generic) {
  } else if (d == 0) {
    d0 = hyd_vertex(0), d1 = hyd_vertex(1), d2 = hyd_vertex(2), d3 = hyd_vertex(3);
  } else if (d == 1 && ((shape == kHydTet && h <= 3) || (shape == kHydTrig && h <= 2))) {
    // the reference direction: the neighbour's lowest other neighbour, else the coordinate axis most across the bond -- turned round for
    // the higher of the two atoms, which are then the whole skeleton, so that their hydrogens stagger
    unsigned long long x0 = adj[2 * j0], x1 = adj[2 * j0 + 1];
    x0 &= ~(i < 64 ? 1ull << (i & 63) : 0ull), x1 &= ~(i < 64 ? 0ull : 1ull << (i & 63));
    const int w = x0 ? __builtin_ctzll(x0) : x1 ? 64 + __builtin_ctzll(x1) : -1;
    const float ax = fabsf(u0.x), ay = fabsf(u0.y), az = fabsf(u0.z);
    const float one = i < j0 ? 1.0f : -1.0f;
    HydVec r = (ax <= ay && ax <= az) ? HydVec{one, 0.0f, 0.0f} : (ay <= az) ? HydVec{0.0f, one, 0.0f} : HydVec{0.0f, 0.0f, one};
    bool ok = true;
    if (w >= 0) ok = hyd_unit(hv_sub(hv_of(atoms[w]), hv_of(atoms[j0])), 0.0f, r);
    HydVec e1 = zero;
    ok = ok && hyd_unit(hv_sub(r, hv_scale(u0, hv_dot(u0, r))), kHydEps2, e1);
    const HydVec e2 = hv_cross(u0, e1);
    const bool tet = shape == kHydTet;
    d0 = hyd_cone(u0, e1, e2, cs, sn, -1.0f, 0.0f);                                   // 180 degrees: anti to w
    d1 = tet ? hyd_cone(u0, e1, e2, cs, sn, 0.5f, -0.86602540378443865f)              // 300
             : hyd_cone(u0, e1, e2, cs, sn, 1.0f, 0.0f);                              // 0: in the plane of w
    d2 = hyd_cone(u0, e1, e2, cs, sn, 0.5f, 0.86602540378443865f);                    // 60
    generic = !ok;
  } else if (shape == kHydLin && d == 1 && h == 1) {
    d0 = hv_neg(u0);
  } else if ((shape == kHydTet && d == 3 && h == 1) || (shape == kHydTrig && d == 2 && h == 1)) {
    generic = !hyd_unit(sum, kHydEps2, t);
    d0 = hv_neg(t);
  } else if (shape == kHydTet && d == 2 && h <= 2) {
    HydVec nn = zero;
    const bool ok_b = hyd_unit(sum, kHydEps2, t), ok_n = hyd_unit(hv_cross(u0, u1), kHydEps2, nn);
    const float c = kHydInvSqrt3, s = 0.81649658092772603f;
    d0 = hv_add(hv_scale(t, -c), hv_scale(nn, s));
    d1 = hv_sub(hv_scale(t, -c), hv_scale(nn, s));
    generic = !(ok_b && ok_n);
  } else {
    generic = true;
  }
  // ---- the generic rule: opposite the sum of the neighbours, then the freest vertices -----------------------------------------------------
  if (generic) {
    if (hyd_unit(sum, kHydEps2, t)) {
      d0 = hv_neg(t);
      hyd_max_add(vmax, d0);
    } else {
      d0 = hyd_max_pick(vmax);
    }
    d1 = hyd_max_pick(vmax), d2 = hyd_max_pick(vmax), d3 = hyd_max_pick(vmax);
  }
  const float L = xh[cls];
  o.h0 = hv_add(p, hv_scale(d0, L));
  o.h1 = h >= 2 ? hv_add(p, hv_scale(d1, L)) : zero;
  o.h2 = h >= 3 ? hv_add(p, hv_scale(d2, L)) : zero;
  o.h3 = h >= 4 ? hv_add(p, hv_scale(d3, L)) : zero;
  shape_used = generic ? kHydGeneric : shape;
  return h;
}

}  // namespace pg
