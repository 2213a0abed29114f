// The core of the stereo perception (DESIGN.md 2.9 "Stereo"): which atoms and double bonds can be stereo elements, the sign of the
// permutation that sorts a centre's ligands by colour, the two geometric tests, and the words the stereo key sums.  Plain functions
// over values, compiled for the device by mol_stereo.hip (one atom or one pair per lane) and for the host by
// tools/stereo_host_check.cpp (the same text under the host sanitizers).  No arrays, no loops: nothing here can index out of bounds.
//
// The geometry is fp32.  Every comparison against a threshold is written `!(|x| >= limit)` = undefined, so that a NaN -- from a
// zero-length vector (0 / 0) or a non-finite coordinate (inf - inf, inf / inf) -- is undefined without a test of its own.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_ST_HD __host__ __device__ inline
#else
#define PG_ST_HD inline
#endif

namespace pg {

typedef unsigned long long st_u64;

constexpr int kStereoUndefined = 2;         // parity / stereo of an element that is stereogenic but whose geometry does not decide
// the key's words for a centre with label +1 / -1 and a double bond with label +1 / -1
constexpr st_u64 kStereoA = 0x243F6A8885A308D3ull, kStereoB = 0x13198A2E03707344ull;
constexpr st_u64 kStereoC = 0xA4093822299F31D0ull, kStereoD = 0x082EFA98EC4E6C89ull;

// the identity key's splitmix64 step (DESIGN.md 2.9 "Identity")
PG_ST_HD st_u64 stereo_mix(st_u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// ---- centres ----------------------------------------------------------------------------------------------------------------------------
// class C, N, Si, P or S with four heavy neighbours and no hydrogen, or three and one
PG_ST_HD bool stereo_centre_candidate(int cls, int degree, int h) {
  const bool el = cls == 1 || cls == 2 || cls == 5 || cls == 6 || cls == 7;
  return el && ((degree == 4 && h == 0) || (degree == 3 && h == 1));
}

// The sign of the permutation that sorts c0 .. c(m-1), m = 3 or 4, ascending (unsigned): +1 even, -1 odd, 0 if two are equal.  (An
// implicit hydrogen is last before and after the sort, so a centre with one sorts its three heavy neighbours only.)
PG_ST_HD int stereo_sort_sign(st_u64 c0, st_u64 c1, st_u64 c2, st_u64 c3, int m) {
  int inv = (c0 > c1) + (c0 > c2) + (c1 > c2);
  bool eq = c0 == c1 || c0 == c2 || c1 == c2;
  if (m == 4) {
    inv += (c0 > c3) + (c1 > c3) + (c2 > c3);
    eq = eq || c0 == c3 || c1 == c3 || c2 == c3;
  }
  return eq ? 0 : (inv & 1) ? -1 : 1;
}

struct StereoVec {
  float x, y, z;
};

PG_ST_HD StereoVec st_sub(StereoVec a, StereoVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
PG_ST_HD float st_dot(StereoVec a, StereoVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PG_ST_HD StereoVec st_cross(StereoVec a, StereoVec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// the unit vector from c to p (NaN components if the two coincide or either is non-finite)
PG_ST_HD StereoVec st_unit(StereoVec c, StereoVec p) {
  const StereoVec d = st_sub(p, c);
  const float len = sqrtf(st_dot(d, d));
  return {d.x / len, d.y / len, d.z / len};
}

// The parity of a centre at c with the neighbours p0, p1, p2 (, p3) in local index order: with u_k the unit vector to p_k, and
// u3 = -(u0 + u1 + u2) (not normalised) where the fourth ligand is the implicit hydrogen, V = (u0 - u3) . ((u1 - u3) x (u2 - u3)):
// +1 / -1 = the sign of V if |V| >= vol_min, else kStereoUndefined.  vol_min > 0.
PG_ST_HD int stereo_centre_parity(StereoVec c, StereoVec p0, StereoVec p1, StereoVec p2, StereoVec p3, bool four, float vol_min) {
  const StereoVec u0 = st_unit(c, p0), u1 = st_unit(c, p1), u2 = st_unit(c, p2);
  StereoVec u3 = {-(u0.x + u1.x + u2.x), -(u0.y + u1.y + u2.y), -(u0.z + u1.z + u2.z)};
  if (four) u3 = st_unit(c, p3);
  const float v = st_dot(st_sub(u0, u3), st_cross(st_sub(u1, u3), st_sub(u2, u3)));
  if (!(fabsf(v) >= vol_min)) return kStereoUndefined;
  return v > 0.0f ? 1 : -1;
}

// ---- double bonds -----------------------------------------------------------------------------------------------------------------------
// an end of a double bond: it has no other bond of Kekulé order >= 2 (n_multi counts the bond itself), and two substituents, or one
// and at most one hydrogen
PG_ST_HD bool stereo_bond_end(int degree, int n_multi, int h) { return n_multi == 1 && (degree == 3 || (degree == 2 && h <= 1)); }

// The bond a - b with the lowest-index substituents ra of a and rb of b: e = b - a, d_x = r_x - x, w_x = d_x - e (d_x . e) / (e . e),
// t = (w_a . w_b) / (|d_a| |d_b|): +1 (cis) if t >= planar_min, -1 (trans) if t <= -planar_min, else kStereoUndefined.  planar_min > 0.
PG_ST_HD int stereo_bond_side(StereoVec a, StereoVec b, StereoVec ra, StereoVec rb, float planar_min) {
  const StereoVec e = st_sub(b, a), da = st_sub(ra, a), db = st_sub(rb, b);
  const float ee = st_dot(e, e), fa = st_dot(da, e) / ee, fb = st_dot(db, e) / ee;
  const StereoVec wa = {da.x - e.x * fa, da.y - e.y * fa, da.z - e.z * fa}, wb = {db.x - e.x * fb, db.y - e.y * fb, db.z - e.z * fb};
  const float t = st_dot(wa, wb) / (sqrtf(st_dot(da, da)) * sqrtf(st_dot(db, db)));
  if (!(fabsf(t) >= planar_min)) return kStereoUndefined;
  return t > 0.0f ? 1 : -1;
}

// The factor an end puts on the bond's label: -1 if its largest-colour substituent is not its lowest-index one.  c_low: the colour of
// the lowest-index substituent; two: it has a second heavy substituent, of colour c_other; h: its hydrogens (a hydrogen is the last
// substituent in index order and in colour order, so an end with one heavy substituent and a hydrogen gives -1).
PG_ST_HD int stereo_end_factor(st_u64 c_low, bool two, st_u64 c_other, int h) {
  if (two) return c_other > c_low ? -1 : 1;
  return h >= 1 ? -1 : 1;
}

// ---- the key ----------------------------------------------------------------------------------------------------------------------------
PG_ST_HD st_u64 stereo_centre_word(st_u64 colour, int label) { return stereo_mix(colour ^ (label > 0 ? kStereoA : kStereoB)); }
PG_ST_HD st_u64 stereo_bond_word(st_u64 colour_a, st_u64 colour_b, int label) {
  return stereo_mix((stereo_mix(colour_a) + stereo_mix(colour_b)) ^ (label > 0 ? kStereoC : kStereoD));
}
// sum: the wrapping sum of the words of every element with label +1 or -1 (at least one)
PG_ST_HD st_u64 stereo_key(st_u64 key, st_u64 sum) { return stereo_mix(key ^ stereo_mix(sum)); }

}  // namespace pg
