// The core of the rigid overlay of molecule pairs (DESIGN.md 2.9 "Shape alignment"): the frame of a molecule (centroid, principal axes
// by cyclic Jacobi in double, radius of gyration), the quaternion algebra of a pose, the five starts, the chain-rule weight of a
// Tanimoto value and the step rule.  Plain functions over values, compiled for the device by shape_align.hip and for the host by
// tools/shape_align_host_check.cpp (the same text under the host sanitizers).  A pose is (q, p): B's atom y lies at
// R(q) (y - c_B) + p; the frame is computed in double and rounded once to fp32, everything after it is fp32.
#pragma once
#include "shape_core.h"

namespace pg {

constexpr int kAlignStarts = 5;             // start 0 in place, starts 1..4 inertial (PG_SHAPE_ALIGN_N_STARTS)
constexpr int kAlignStartInPlace = 0x01;    // the bits of the starts mask (PG_SHAPE_ALIGN_IN_PLACE / _INERTIAL)
constexpr int kAlignStartInertial = 0x1e;
constexpr int kAlignMaxSteps = 1024;        // the largest max_steps (PG_SHAPE_ALIGN_MAX_STEPS)
constexpr int kAlignFrame = 16;             // floats of a frame (PG_SHAPE_FRAME_FLOATS): centroid 3, axes 9 (axis k at 3 + 3k), rho, eigenvalues 3
constexpr int kAlignJacobiSweeps = 8;       // fixed: a 3 x 3 matrix is diagonal to rounding after 4 or 5
constexpr float kAlignGrow = 1.5f, kAlignShrink = 0.5f;
constexpr float kAlignMinRho = 0.5f;        // Angstrom: the floor of rho, and the rho of an empty row

// ---- the frame ------------------------------------------------------------------------------------------------------------------------
// one Jacobi rotation that zeroes a[P][Q]; v's columns collect the eigenvectors
template <int P, int Q>
PG_SHAPE_HD void align_jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double akp = a[k][P], akq = a[k][Q];
    a[k][P] = c * akp - s * akq, a[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double apk = a[P][k], aqk = a[Q][k];
    a[P][k] = c * apk - s * aqk, a[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq, v[k][Q] = s * vkp + c * vkq;
  }
}
// columns I and J of (lambda, v) change places where lambda[J] > lambda[I]
template <int I, int J>
PG_SHAPE_HD void align_sort_step(double (&lam)[3], double (&v)[3][3]) {
  if (!(lam[J] > lam[I])) return;
  const double l = lam[I];
  lam[I] = lam[J], lam[J] = l;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = v[k][I];
    v[k][I] = v[k][J], v[k][J] = x;
  }
}
// the largest-magnitude component of column I positive, the first such component deciding a tie
template <int I>
PG_SHAPE_HD void align_fix_sign(double (&v)[3][3]) {
  double big = fabs(v[0][I]), val = v[0][I];
  if (fabs(v[1][I]) > big) big = fabs(v[1][I]), val = v[1][I];
  if (fabs(v[2][I]) > big) val = v[2][I];
  if (val < 0.0) v[0][I] = -v[0][I], v[1][I] = -v[1][I], v[2][I] = -v[2][I];
}
// Eigenvalues (descending) and a right-handed orthonormal set of eigenvectors (the columns of v) of a symmetric matrix: cyclic Jacobi
// over (0,1), (0,2), (1,2), a fixed number of sweeps; a stable sort; signs; e3 = e1 x e2.  The zero matrix gives the identity.
PG_SHAPE_HD void align_eigen(double (&a)[3][3], double (&lam)[3], double (&v)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < kAlignJacobiSweeps; ++sweep) {
    align_jacobi_rotate<0, 1>(a, v);
    align_jacobi_rotate<0, 2>(a, v);
    align_jacobi_rotate<1, 2>(a, v);
  }
  lam[0] = a[0][0], lam[1] = a[1][1], lam[2] = a[2][2];
  align_sort_step<0, 1>(lam, v);
  align_sort_step<1, 2>(lam, v);
  align_sort_step<0, 1>(lam, v);
  align_fix_sign<0>(v);
  align_fix_sign<1>(v);
  v[0][2] = v[1][0] * v[2][1] - v[2][0] * v[1][1];
  v[1][2] = v[2][0] * v[0][1] - v[0][0] * v[2][1];
  v[2][2] = v[0][0] * v[1][1] - v[1][0] * v[0][1];
}
// The frame of the n kept atoms at `atoms` (anything with x, y, z), out [kAlignFrame].  Summation order: the centroid adds the atoms
// in packed order, the covariance adds (x - c)(x - c)^T in packed order, both in double; n = 0 gives the identity frame at the origin.
template <typename Atom>
PG_SHAPE_HD void align_frame(const Atom* atoms, int n, float* out) {
  double c[3] = {0.0, 0.0, 0.0}, a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, lam[3], v[3][3];
  for (int i = 0; i < n; ++i) c[0] += (double)atoms[i].x, c[1] += (double)atoms[i].y, c[2] += (double)atoms[i].z;
  if (n > 0) c[0] /= n, c[1] /= n, c[2] /= n;
  for (int i = 0; i < n; ++i) {
    const double dx = (double)atoms[i].x - c[0], dy = (double)atoms[i].y - c[1], dz = (double)atoms[i].z - c[2];
    a[0][0] += dx * dx, a[0][1] += dx * dy, a[0][2] += dx * dz, a[1][1] += dy * dy, a[1][2] += dy * dz, a[2][2] += dz * dz;
  }
  if (n > 0) a[0][0] /= n, a[0][1] /= n, a[0][2] /= n, a[1][1] /= n, a[1][2] /= n, a[2][2] /= n;
  a[1][0] = a[0][1], a[2][0] = a[0][2], a[2][1] = a[1][2];
  const double gyration = sqrt(a[0][0] + a[1][1] + a[2][2]);
  align_eigen(a, lam, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out[k] = (float)c[k];
    out[3 + 3 * k] = (float)v[0][k], out[4 + 3 * k] = (float)v[1][k], out[5 + 3 * k] = (float)v[2][k];
    out[13 + k] = (float)lam[k];
  }
  out[12] = (float)(gyration > (double)kAlignMinRho ? gyration : (double)kAlignMinRho);
}

// ---- quaternions (w, x, y, z) and rotations (row-major 3 x 3), fp32 --------------------------------------------------------------------
struct AlignQuat {
  float w, x, y, z;
};
PG_SHAPE_HD AlignQuat align_quat_normalised(AlignQuat q) {
  const float n = sqrtf(fmaf(q.z, q.z, fmaf(q.y, q.y, fmaf(q.x, q.x, q.w * q.w))));
  const float r = 1.0f / n;
  return AlignQuat{q.w * r, q.x * r, q.y * r, q.z * r};
}
PG_SHAPE_HD AlignQuat align_quat_mul(AlignQuat a, AlignQuat b) {           // a b: b's rotation first
  return AlignQuat{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                   a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
// exp of half the rotation vector r: the rotation by |r| about r / |r|
PG_SHAPE_HD AlignQuat align_quat_exp(float rx, float ry, float rz) {
  const float angle = sqrtf(fmaf(rz, rz, fmaf(ry, ry, rx * rx)));
  const float k = angle > 1e-6f ? sinf(0.5f * angle) / angle : 0.5f;
  return AlignQuat{cosf(0.5f * angle), k * rx, k * ry, k * rz};
}
// q = (1, 0, 0, 0) gives the identity exactly
PG_SHAPE_HD void align_quat_matrix(AlignQuat q, float (&r)[9]) {
  const float xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z, wx = q.w * q.x,
              wy = q.w * q.y, wz = q.w * q.z;
  r[0] = 1.0f - 2.0f * (yy + zz), r[1] = 2.0f * (xy - wz), r[2] = 2.0f * (xz + wy);
  r[3] = 2.0f * (xy + wz), r[4] = 1.0f - 2.0f * (xx + zz), r[5] = 2.0f * (yz - wx);
  r[6] = 2.0f * (xz - wy), r[7] = 2.0f * (yz + wx), r[8] = 1.0f - 2.0f * (xx + yy);
}
// Shepperd's choice of the largest of (trace, r00, r11, r22), then normalised
PG_SHAPE_HD AlignQuat align_matrix_quat(const float (&r)[9]) {
  const float tr = r[0] + r[4] + r[8];
  AlignQuat q;
  if (tr >= r[0] && tr >= r[4] && tr >= r[8]) {
    q = AlignQuat{1.0f + tr, r[7] - r[5], r[2] - r[6], r[3] - r[1]};
  } else if (r[0] >= r[4] && r[0] >= r[8]) {
    q = AlignQuat{r[7] - r[5], 1.0f + r[0] - r[4] - r[8], r[1] + r[3], r[2] + r[6]};
  } else if (r[4] >= r[8]) {
    q = AlignQuat{r[2] - r[6], r[1] + r[3], 1.0f - r[0] + r[4] - r[8], r[5] + r[7]};
  } else {
    q = AlignQuat{r[3] - r[1], r[2] + r[6], r[5] + r[7], 1.0f - r[0] - r[4] + r[8]};
  }
  return align_quat_normalised(q);
}

// ---- starts ---------------------------------------------------------------------------------------------------------------------------
// the diagonal of D_k, k = 1..4: the four proper sign changes of the axes
PG_SHAPE_HD float align_start_sign(int k, int axis) { return (k == 1 || k == axis + 2) ? 1.0f : -1.0f; }
// start 0: (identity, c_B); start k = 1..4: (E_A D_k E_B^T, c_A).  fa, fb: the two frames.
PG_SHAPE_HD void align_start(int k, const float* fa, const float* fb, AlignQuat& q, float (&p)[3]) {
  if (k == 0) {
    q = AlignQuat{1.0f, 0.0f, 0.0f, 0.0f};
    p[0] = fb[0], p[1] = fb[1], p[2] = fb[2];
    return;
  }
  float r[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float s = 0.0f;
#pragma unroll
      for (int m = 0; m < 3; ++m) s = fmaf(align_start_sign(k, m) * fa[3 + 3 * m + i], fb[3 + 3 * m + j], s);
      r[3 * i + j] = s;
    }
  q = align_matrix_quat(r);
  p[0] = fa[0], p[1] = fa[1], p[2] = fa[2];
}

// ---- a pose applied ---------------------------------------------------------------------------------------------------------------------
// R (y - c_B) + p, one fixed order
PG_SHAPE_HD void align_apply(const float (&r)[9], const float* cb, const float (&p)[3], float yx, float yy, float yz, float& ox, float& oy,
                             float& oz) {
  const float dx = yx - cb[0], dy = yy - cb[1], dz = yz - cb[2];
  ox = fmaf(r[2], dz, fmaf(r[1], dy, fmaf(r[0], dx, p[0])));
  oy = fmaf(r[5], dz, fmaf(r[4], dy, fmaf(r[3], dx, p[1])));
  oz = fmaf(r[8], dz, fmaf(r[7], dy, fmaf(r[6], dx, p[2])));
}
// t = p - R c_B, so that y' = R y + t on B's stored coordinates
PG_SHAPE_HD void align_translation(const float (&r)[9], const float* cb, const float (&p)[3], float (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = p[i] - fmaf(r[3 * i + 2], cb[2], fmaf(r[3 * i + 1], cb[1], r[3 * i] * cb[0]));
}

// ---- objective and step rule ------------------------------------------------------------------------------------------------------------
// d/d(ab) of ab / (aa + bb - ab): (aa + bb) / (aa + bb - ab)^2, 0 where the denominator is not positive
PG_SHAPE_HD float align_tanimoto_slope(float ab, float aa, float bb) {
  const float sum = aa + bb, den = sum - ab;
  return den > 0.0f ? sum / (den * den) : 0.0f;
}
// 2 k of a pair term exp2(t0 + t1 d^2) = exp(-k d^2) times its weight: k = -t1 / log2 e
constexpr float kAlignTwoOverLog2e = (float)(2.0 / kShapeLog2e);
// d = g6 / |g6| with g6 = (F, tau / rho); false where |g6| is not positive (the start stands still)
PG_SHAPE_HD bool align_direction(const float (&force)[3], const float (&torque)[3], float rho, float (&d)[6]) {
  const float inv = 1.0f / rho;
  const float g[6] = {force[0], force[1], force[2], torque[0] * inv, torque[1] * inv, torque[2] * inv};
  float n2 = g[0] * g[0];
#pragma unroll
  for (int i = 1; i < 6; ++i) n2 = fmaf(g[i], g[i], n2);
  const float n = sqrtf(n2);
  if (!(n > 0.0f) || !(n < INFINITY)) return false;
#pragma unroll
  for (int i = 0; i < 6; ++i) d[i] = g[i] / n;
  return true;
}
// the trial pose: p + s d[0:3], exp([s d[3:6] / rho]x) R, renormalised
PG_SHAPE_HD void align_trial(AlignQuat q, const float (&p)[3], const float (&d)[6], float s, float rho, AlignQuat& q_out, float (&p_out)[3]) {
  const float a = s / rho;
  p_out[0] = fmaf(s, d[0], p[0]), p_out[1] = fmaf(s, d[1], p[1]), p_out[2] = fmaf(s, d[2], p[2]);
  q_out = align_quat_normalised(align_quat_mul(align_quat_exp(a * d[3], a * d[4], a * d[5]), q));
}
// accept a strictly better trial and lengthen the step, else shorten it
PG_SHAPE_HD bool align_accept(float f_trial, float f, float& s) {
  const bool better = f_trial > f;
  s *= better ? kAlignGrow : kAlignShrink;
  return better;
}
PG_SHAPE_HD bool align_stop(float s, int evaluations, float min_step, int max_steps) { return s < min_step || evaluations >= max_steps; }
// the arguments every caller checks
inline bool align_options_ok(int max_steps, float first_step, float min_step, int starts) {
  return max_steps >= 1 && max_steps <= kAlignMaxSteps && first_step > 0.0f && first_step < INFINITY && min_step > 0.0f && min_step <= first_step
         && starts != 0 && (starts & ~(kAlignStartInPlace | kAlignStartInertial)) == 0;
}

}  // namespace pg
