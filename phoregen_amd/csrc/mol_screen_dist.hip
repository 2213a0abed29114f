// The molecule screen with bonds perceived from the coordinates (pg_mol_screen_dist, include/phoregen_hip.h; phoregen_amd/molecule.py
// screen(bonds='distance'); the rule of the reference's utils/predict_bonds.py, DESIGN.md 2.9 "Distance bonds").  One wave per
// (frame, graph) (mol_common.h).  The order of a pair is three strict fp32 compares of 100 * distance against the thresholds of its two
// elements; everything after the bonds is mol_screen_core.h, shared with mol_screen.hip.  Nothing is summed in floating point.
#include "mol_screen_core.h"

namespace pg {

constexpr int kDistThr = 11 * 11 * 3;   // the threshold table: [class][class][single, double, triple], 0 = no such bond

__global__ __launch_bounds__(64) void mol_screen_dist_kernel(
    const float* __restrict__ node_scores, long node_fs, const float* __restrict__ pos, long pos_fs,
    const float* __restrict__ edge_scores, long edge_fs, const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
    int n_lig, int n_half, const uint8_t* __restrict__ max_valence2, const float* __restrict__ thresholds, int* __restrict__ status,
    int* __restrict__ counts, int8_t* __restrict__ cls_o, int16_t* __restrict__ compact_o, uint8_t* __restrict__ val2_o,
    int16_t* __restrict__ comp_o, int8_t* __restrict__ order_o, int* __restrict__ agree_o) {
  __shared__ MolScreenLds s;
  __shared__ float4 s_atom[kMolMax];                      // x, y, z, class as bits (-1: dropped, or a non-finite coordinate)
  __shared__ float s_thr[kDistThr];

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  const float* nrow = node_scores + (size_t)m.f * node_fs + (size_t)m.a0 * 12;
  const float* prow = pos + (size_t)m.f * pos_fs + (size_t)m.a0 * 3;

  for (int t = lane; t < kDistThr; t += 64) s_thr[t] = thresholds[t];

  // ---- atoms: class, compact index; coordinates and class staged once --------------------------------------------------------
  bool bad_pos = false, masked = false;
  int info = 0;
  const int n_kept = mol_screen_atoms(s, lane, n, nrow, arow, cls_o, compact_o, masked, [&](int i, int k) {
    const float* p = prow + (size_t)i * 3;
    const float x = p[0], y = p[1], z = p[2];
    const bool keep = k < 11, bad = mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z);
    bad_pos |= keep && bad;
    info |= (k == 0 || k == 5) ? PG_MOL_DIST_UNMAPPED_ELEMENT : 0;     // B, Si: elements the reference's rule cannot name
    s_atom[i] = make_float4(x, y, z, __int_as_float((keep && !bad) ? k : -1));
  });

  // ---- bonds: order from the distance; with edge scores, how it agrees with their argmax --------------------------------------
  const bool with_pred = edge_scores != nullptr;
  const float* erow = with_pred ? edge_scores + (size_t)m.f * edge_fs + (size_t)m.h0 * 12 : nullptr;   // first half only
  int n_bond = 0;
  int ag[6] = {0, 0, 0, 0, 0, 0};
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const float4 pa = s_atom[a], pb = s_atom[b];
    const int ka = __float_as_int(pa.w), kb = __float_as_int(pb.w);
    const bool both = ka >= 0 && kb >= 0;
    int o = 0;
    if (both) {
      const float dx = pa.x - pb.x, dy = pa.y - pb.y, dz = pa.z - pb.z;
      const float d = sqrtf(dx * dx + dy * dy + dz * dz);
      const float d100 = 100.0f * d;
      const float* t = s_thr + (ka * 11 + kb) * 3;
      o = d100 < t[0] ? (d100 < t[1] ? (d100 < t[2] ? 3 : 2) : 1) : 0;
    }
    order_o[hrow + p] = (int8_t)o;
    if (o) {
      ++n_bond;
      mol_screen_bond(s, a, b, o);
    }
    if (with_pred && both) {
      float v[6];
      const float2* r = reinterpret_cast<const float2*>(erow + (size_t)p * 6);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float2 e = r[q];
        v[2 * q] = e.x, v[2 * q + 1] = e.y;
      }
      const int am = first_argmax<6>(v), pr = mol_is_bond(am) ? am : 0;
      const int col = (pr && o) ? (pr == o ? 0 : (pr == 4 && o <= 2) ? 1 : 2) : pr ? 3 : o ? 4 : 5;
#pragma unroll
      for (int c = 0; c < 6; ++c) ag[c] += col == c;
    }
  });
  __syncthreads();

  if (with_pred) {
#pragma unroll
    for (int c = 0; c < 6; ++c) ag[c] = wave_sum(ag[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) agree_o[(size_t)blockIdx.x * 6 + c] = ag[c];
    }
  }

  // ---- components, valence rule, counts, status (mol_screen_core.h) ------------------------------------------------------------
  mol_screen_finish(s, lane, n, arow, n_kept, n_bond, bad_pos, masked, info, max_valence2, status, counts, val2_o, comp_o);
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_screen_dist(const float* node_scores, int64_t node_fs, const float* pos, int64_t pos_fs, const float* edge_scores,
                                  int64_t edge_fs, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig, int n_bond,
                                  int max_n, const uint8_t* max_valence2, const float* thresholds, int* status, int* counts, int8_t* cls,
                                  int16_t* compact, uint8_t* valence2, int16_t* comp, int8_t* order, int* agree, void* stream) {
  const int rc = mol_check_batch("pg_mol_screen_dist", B, F, n_lig, n_bond, max_n);
  if (rc != PG_OK && rc != kMolNothing) return rc;
  if (!max_valence2 || !thresholds) {
    set_error("pg_mol_screen_dist: max_valence2 and thresholds must not be null");
    return PG_ERR_ARG;
  }
  if (edge_scores && !agree) {
    set_error("pg_mol_screen_dist: edge_scores without an agree output");
    return PG_ERR_ARG;
  }
  if (((uintptr_t)node_scores & 15) || (node_fs & 3) || ((uintptr_t)counts & 15) ||
      (edge_scores && (((uintptr_t)edge_scores & 7) || (edge_fs & 1)))) {
    set_error("pg_mol_screen_dist: node_scores / node_fs must be 16-byte, edge_scores / edge_fs 8-byte, counts 16-byte aligned");
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  hipLaunchKernelGGL(mol_screen_dist_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, node_scores, (long)node_fs, pos,
                     (long)pos_fs, edge_scores, (long)edge_fs, g_lig_off, g_bond_off, B, n_lig, n_bond / 2, max_valence2, thresholds,
                     status, counts, cls, compact, valence2, comp, order, agree);
  return check_launch("pg_mol_screen_dist");
}
