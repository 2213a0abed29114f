// The core of the Gaussian shape and colour overlap of molecules where they lie (DESIGN.md 2.9 "Shape"): how an atom is packed, the
// table of the element pairs, one pair term, the Tanimoto value of three overlaps, the combined score, and the index arithmetic of the
// tiles and runs.  Plain functions over values, compiled for the device by shape_sim.hip and for the host by
// tools/shape_host_check.cpp (the same text under the host sanitizers).  The (score, index) words the nearest-neighbour search reduces
// by are fp_core.h's: a score is an fp32 value >= 0, so its bit pattern orders as the value does.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "fp_core.h"

#if defined(__HIPCC__)
#define PG_SHAPE_HD __host__ __device__ inline
#else
#define PG_SHAPE_HD inline
#endif

namespace pg {

constexpr int kShapeClasses = 11;           // the kept elements, in ATOM_TYPES' order
constexpr int kShapeAlphas = 12;            // alpha of every class, then the colour alpha (PG_SHAPE_N_ALPHA)
constexpr int kShapeMaxAtoms = 128;         // atoms of a molecule (PG_MOL_MAX_ATOMS): two per lane of a wave
// The sweep: a workgroup of kShapeWaves waves owns kShapeTileA rows of the set in registers (a wave takes them one at a time, a lane
// holds atoms l and l + 64 of the row) and sweeps the other set in LDS tiles of kShapeTileB molecules (shape.TILE_A / TILE_B).
constexpr int kShapeTileA = 16;
constexpr int kShapeTileB = 16;
constexpr int kShapeWaves = 4;
constexpr int kShapeRowsPerWave = kShapeTileA / kShapeWaves;
static_assert(kShapeTileA % kShapeWaves == 0 && kShapeTileB <= 64, "a wave takes whole rows; a lane keeps one value per staged molecule");

// status of a packed row (PG_SHAPE_* of the header); a row with any bit has no atoms
constexpr int kShapeEmpty = 1, kShapeNonfinite = 2, kShapeUnselected = 4;

// ---- a packed atom: (x, y, z, word); word = class | feature byte << 8, -1 = dropped ------------------------------------------------
PG_SHAPE_HD int shape_atom_word(int cls, int fp) { return (cls >= 0 && cls < kShapeClasses) ? (cls | (fp & 0xff) << 8) : -1; }
PG_SHAPE_HD int shape_word_class(int w) { return w & 0xff; }
PG_SHAPE_HD int shape_word_fp(int w) { return (w >> 8) & 0xff; }

// ---- the table of the element pairs ----------------------------------------------------------------------------------------------
// A shape term p^2 (pi / (ai + aj))^(3/2) exp(-(ai aj / (ai + aj)) d^2) is exp2(t0 + t1 d^2) with t0 = log2 of the weight and
// t1 = -(ai aj / (ai + aj)) log2(e); a colour term is popcount * exp2(c0 + c1 d^2) with ai = aj = the colour alpha.  Computed in
// double, rounded once to fp32.
struct ShapePair {
  float t0, t1;
};
struct ShapeTable {
  ShapePair pair[kShapeClasses * kShapeClasses];    // [class of the staged atom][class of the lane's atom]: symmetric
  ShapePair colour;
};
constexpr double kShapeP = 2.8284271247461900976;   // 2 sqrt(2)
constexpr double kShapePi = 3.14159265358979323846;
constexpr double kShapeLog2e = 1.44269504088896340736;

inline bool shape_alpha_ok(float a) { return a > 0.0f && a < INFINITY; }      // (false for a NaN)
inline ShapePair shape_pair_entry(double ai, double aj) {
  const double s = ai + aj;
  ShapePair e;
  e.t0 = (float)log2(kShapeP * kShapeP * pow(kShapePi / s, 1.5));
  e.t1 = (float)(-(ai * aj / s) * kShapeLog2e);
  return e;
}
// false where an alpha is not positive and finite (the table is then not written)
inline bool shape_table(const float* alpha /*[kShapeAlphas]*/, ShapeTable& t) {
  for (int i = 0; i < kShapeAlphas; ++i)
    if (!shape_alpha_ok(alpha[i])) return false;
  for (int i = 0; i < kShapeClasses; ++i)
    for (int j = 0; j < kShapeClasses; ++j) t.pair[i * kShapeClasses + j] = shape_pair_entry(alpha[i], alpha[j]);
  t.colour = shape_pair_entry(alpha[kShapeClasses], alpha[kShapeClasses]);
  return true;
}

// ---- one pair term -----------------------------------------------------------------------------------------------------------------
// d^2 in one fixed order of three fmas
PG_SHAPE_HD float shape_dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
PG_SHAPE_HD float shape_exp2(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(x);                 // v_exp_f32: no subnormal results, a term below 2^-126 is 0
#else
  return exp2f(x);
#endif
}
PG_SHAPE_HD float shape_term(float d2, ShapePair e) { return shape_exp2(fmaf(d2, e.t1, e.t0)); }

// ---- similarity --------------------------------------------------------------------------------------------------------------------
// ab / (aa + bb - ab) with one division; 0 where the denominator is not positive (an empty molecule is similar to nothing)
PG_SHAPE_HD float shape_tanimoto(float ab, float aa, float bb) {
  const float den = (aa + bb) - ab;
  if (!(den > 0.0f)) return 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(ab, den);
#else
  return ab / den;
#endif
}
// (1 - w) st + w ct: two products and one sum, each rounded (never contracted into an fma)
PG_SHAPE_HD float shape_score(float st, float ct, float w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(__fmul_rn(1.0f - w, st), __fmul_rn(w, ct));
#else
  volatile float a = (1.0f - w) * st, b = w * ct;
  return a + b;
#endif
}
inline bool shape_weight_ok(float w) { return w >= 0.0f && w <= 1.0f; }       // (false for a NaN)

// ---- tiles and runs ----------------------------------------------------------------------------------------------------------------
// The sweep over the n_b molecules of the set in LDS is cut into n_split runs of tiles_per_split tiles, one workgroup each per tile of
// the rows in registers, so that about `target` workgroups exist even where that set is small (fp_split with this file's tiles).
PG_SHAPE_HD FpSplit shape_split(int n_a, int n_b, int target) {
  const int ta = fp_tiles(n_a, kShapeTileA), tb = fp_tiles(n_b, kShapeTileB);
  int want = ta > 0 ? target / ta + (target % ta != 0) : 1;
  want = want < 1 ? 1 : want > tb ? tb : want;
  FpSplit s = {1, tb};
  if (want > 1) {
    s.tiles_per_split = tb / want + (tb % want != 0);
    s.n_split = tb / s.tiles_per_split + (tb % s.tiles_per_split != 0);
  }
  return s;
}
// molecules [j0, j1) of run `split`
PG_SHAPE_HD void shape_split_rows(int split, int tiles_per_split, int n_b, int& j0, int& j1) {
  const long long lo = (long long)split * tiles_per_split * kShapeTileB, hi = lo + (long long)tiles_per_split * kShapeTileB;
  j0 = (int)(lo < n_b ? lo : n_b), j1 = (int)(hi < n_b ? hi : n_b);
}
// the row of set A that wave `wave` of block `block` takes as its r-th, -1 past the end of the set
PG_SHAPE_HD int shape_wave_row(unsigned block, int wave, int r, int n) {
  const long long i = (long long)block * kShapeTileA + (long long)wave * kShapeRowsPerWave + r;
  return i < n ? (int)i : -1;
}
// a molecule's atoms: [start, start + count) of the set's n_atoms atom rows; anything else reads as no atoms
PG_SHAPE_HD int shape_atom_count(int start, int count, int n_atoms) {
  return (start >= 0 && count >= 0 && count <= kShapeMaxAtoms && start <= n_atoms - count) ? count : 0;
}

}  // namespace pg
