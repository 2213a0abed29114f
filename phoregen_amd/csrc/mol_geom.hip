// Geometry and pharmacophore fit of the molecules the screen decoded: bond lengths, clashes, exclusion spheres, feature coverage of
// every (frame, graph) in one launch (pg_mol_geom, include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9
// "Geometry").  Reads the coordinates and the screen's outputs (cls, order), not the scores.  One wave per (frame, graph)
// (mol_common.h); the two loops with a lane-dependent trip count (pairs, points) hold no barrier, vote or cross-lane move.  Distances
// are fp32; the two energies (metrics 5 and 6) are differences of nearly equal numbers, so their sums run in fp64 from the fp32 inputs
// and are rounded to fp32 once.  Every sum is a per-lane partial over a fixed lane-to-element assignment followed by a fixed
// butterfly: a graph's answer does not depend on the batch it sits in.
#include "mol_common.h"
#include "wave_prims.h"

namespace pg {

constexpr int kGeomMax = kMolMax, kGeomCh = kMolCh;

struct GeomLimits {
  float bond_min, bond_max, clash_min, ex_clear, feat_cut;
};

__global__ __launch_bounds__(64) void mol_geom_kernel(
    const float* __restrict__ pos, long pos_fs, const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
    const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B, int n_lig, int n_half,
    const float* __restrict__ point_pos, const uint8_t* __restrict__ point_is_ex, int n_point, const int* __restrict__ g_point_range,
    const int* __restrict__ g_point_out_off, int n_out, GeomLimits lim, float* __restrict__ point_dist,
    int16_t* __restrict__ point_atom, float* __restrict__ metrics, int* __restrict__ counts, int* __restrict__ status) {
  __shared__ float4 s_atom[kGeomMax];                    // x, y, z, compact index as bits (-1 = not kept)

  const int lane = threadIdx.x;
  MolFrame m;
  MolPoints pt;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  if (!mol_points(pt, m, g_point_range, g_point_out_off, n_point, n_out)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  const float* prow = pos + (size_t)m.f * pos_fs + (size_t)m.a0 * 3;
  const float inf = __builtin_inff();

  // ---- atoms: kept = class 0..10 and finite; the compact index counts the atoms of a kept class, as the screen does -------
  int n_class = 0, n_kept = 0;
  bool bad = false;
  double ax = 0.0, ay = 0.0, az = 0.0;                    // this lane's part of the coordinate sums of the kept atoms
#pragma unroll
  for (int c = 0; c < kGeomCh; ++c) {
    const int i = c * 64 + lane;
    bool kc = false, fin = false;
    float x = 0.f, y = 0.f, z = 0.f;
    if (i < n) {
      kc = mol_class(cls_i[arow + i]) >= 0;
      if (kc) {
        const float* p = prow + (size_t)i * 3;
        x = p[0], y = p[1], z = p[2];
        fin = !(mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z));
        bad |= !fin;
      }
    }
    const unsigned long long km = __ballot(kc);
    const int compact = n_class + __popcll(km & ((1ull << lane) - 1ull));
    n_class += __popcll(km);
    if (i < n) s_atom[i] = make_float4(x, y, z, __int_as_float((kc && fin) ? compact : -1));
    if (kc && fin) {
      ax += (double)x, ay += (double)y, az += (double)z;
      ++n_kept;
    }
  }
  __syncthreads();

  // ---- pairs of kept atoms --------------------------------------------------------------------------------------------------
  float bmin = inf, bmax = -inf, nbmin = inf;
  int c_short = 0, c_long = 0, c_clash = 0, n_bond = 0;
  double e_bond = 0.0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const float4 pa = s_atom[a], pb = s_atom[b];
    if (__float_as_int(pa.w) < 0 || __float_as_int(pb.w) < 0) return;
    const float dx = pa.x - pb.x, dy = pa.y - pb.y, dz = pa.z - pb.z;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    if (mol_is_bond(order_i[hrow + p])) {
      ++n_bond;
      bmin = fminf(bmin, d), bmax = fmaxf(bmax, d);
      c_short += d < lim.bond_min, c_long += d > lim.bond_max;
      const double ex = (double)pa.x - (double)pb.x, ey = (double)pa.y - (double)pb.y, ez = (double)pa.z - (double)pb.z;
      const double dd = sqrt(ex * ex + ey * ey + ez * ez);
      e_bond += fmax(dd - (double)lim.bond_max, 0.0) + fmax((double)lim.bond_min - dd, 0.0);
    } else {
      nbmin = fminf(nbmin, d);
      c_clash += d < lim.clash_min;
    }
  });

  // ---- points, lane-strided: every lane walks all atoms for its own points (one LDS address per step: a broadcast) ----------
  float exmin = inf, featmax = -inf;
  int c_ex = 0, n_feat = 0, n_cov = 0;
  double fx = 0.0, fy = 0.0, fz = 0.0;                    // this lane's part of the coordinate sums of the feature points
  for (int q = pt.ps + lane; q < pt.pe; q += 64) {
    const float* pp = point_pos + (size_t)q * 3;
    const float x = pp[0], y = pp[1], z = pp[2];
    float best = inf;
    int best_i = -1;
    if (mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z)) {
      bad = true;                                        // left out of everything but its own two outputs
    } else {
      const bool is_ex = point_is_ex[q] != 0;
      int close = 0;
      mol_nearest_atom(s_atom, n, x, y, z, lim.ex_clear, [](int) { return true; }, best, best_i, close);
      if (is_ex) {
        exmin = fminf(exmin, best);
        c_ex += close;
      } else {
        featmax = fmaxf(featmax, best);
        ++n_feat;
        n_cov += best < lim.feat_cut;
        fx += (double)x, fy += (double)y, fz += (double)z;
      }
    }
    point_dist[pt.orow + (q - pt.ps)] = best;
    point_atom[pt.orow + (q - pt.ps)] = (int16_t)best_i;
  }

  // ---- the wave's totals (all lanes are back together here), then lane 0 writes the graph's row ------------------------------
  bmin = wave_min(bmin), bmax = wave_max(bmax), nbmin = wave_min(nbmin), exmin = wave_min(exmin), featmax = wave_max(featmax);
  c_short = wave_sum(c_short), c_long = wave_sum(c_long), c_clash = wave_sum(c_clash), c_ex = wave_sum(c_ex);
  n_bond = wave_sum(n_bond), n_kept = wave_sum(n_kept), n_feat = wave_sum(n_feat), n_cov = wave_sum(n_cov);
  e_bond = wave_sum(e_bond);
  ax = wave_sum(ax), ay = wave_sum(ay), az = wave_sum(az), fx = wave_sum(fx), fy = wave_sum(fy), fz = wave_sum(fz);
  const bool any_bad = __any(bad);
  if (lane != 0) return;
  float centre = __builtin_nanf("");
  if (n_kept > 0 && n_feat > 0) {
    const double cx = ax / n_kept - fx / n_feat, cy = ay / n_kept - fy / n_feat, cz = az / n_kept - fz / n_feat;
    centre = (float)sqrt(cx * cx + cy * cy + cz * cz);
  }
  float* mrow = metrics + (size_t)blockIdx.x * 8;
  mrow[0] = bmin, mrow[1] = bmax, mrow[2] = nbmin, mrow[3] = exmin, mrow[4] = featmax, mrow[5] = centre;
  mrow[6] = n_bond > 0 ? (float)(e_bond / n_bond) : 0.f;
  mrow[7] = 0.f;
  int* crow = counts + (size_t)blockIdx.x * 6;
  crow[0] = c_short, crow[1] = c_long, crow[2] = c_clash, crow[3] = c_ex, crow[4] = n_cov, crow[5] = n_feat;
  int st = 0;
  st |= c_short ? PG_GEOM_BOND_SHORT : 0;
  st |= c_long ? PG_GEOM_BOND_LONG : 0;
  st |= c_clash ? PG_GEOM_CLASH : 0;
  st |= c_ex ? PG_GEOM_EX_CLASH : 0;
  st |= n_cov < n_feat ? PG_GEOM_FEATURE_MISSED : 0;
  st |= any_bad ? PG_GEOM_NONFINITE : 0;
  status[blockIdx.x] = st;
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_geom(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int* g_lig_off,
                           const int* g_bond_off, int B, int F, int n_lig, int n_bond, int max_n, const float* point_pos,
                           const uint8_t* point_is_ex, int n_point, const int* g_point_range, const int* g_point_out_off,
                           int n_point_out, const float* limits, float* point_dist, int16_t* point_atom, float* metrics,
                           int* counts, int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_geom", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (n_point < 0 || n_point_out < 0) {
    set_error("pg_mol_geom: n_point %d, n_point_out %d", n_point, n_point_out);
    return PG_ERR_ARG;
  }
  if (!limits) {
    set_error("pg_mol_geom: limits is null (five floats in host memory)");
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  const GeomLimits lim = {limits[0], limits[1], limits[2], limits[3], limits[4]};
  hipLaunchKernelGGL(mol_geom_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, pos, (long)pos_fs, cls, order,
                     g_lig_off, g_bond_off, B, n_lig, n_bond / 2, point_pos, point_is_ex, n_point, g_point_range, g_point_out_off,
                     n_point_out, lim, point_dist, point_atom, metrics, counts, status);
  return check_launch("pg_mol_geom");
}
