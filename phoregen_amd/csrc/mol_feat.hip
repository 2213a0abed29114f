// Pharmacophore feature typing of the molecules the screen decoded, and the typed match against their feature points (pg_mol_feat,
// include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Features").  Reads the screen's outputs (cls, order,
// compact), the Kekulé form (kekule_order, hcount, charge, status), the rings' ring_size and the coordinates.  One wave per
// (frame, graph) (mol_common.h); the divergent loops below (pair rows, an atom's neighbours, points) hold no barrier or vote.  Typing
// is integer work (feature_core.h) and exact; the only floating point is a point's distance to an atom, which is mol_geom.hip's
// (mol_nearest_atom).
#include "mol_common.h"
#include "wave_prims.h"
#include "feature_core.h"

namespace pg {

constexpr int kFeatMax = kMolMax, kFeatCh = kMolCh;
constexpr int kFeatPairs = kFeatMax * (kFeatMax - 1) / 2;
static_assert(kFeatMax <= 255, "a degree fits one byte");

__global__ __launch_bounds__(64) void mol_feat_kernel(
    const float* __restrict__ pos, long pos_fs, const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
    const int16_t* __restrict__ compact_i, const int8_t* __restrict__ kek_i, const uint8_t* __restrict__ hcount_i,
    const int8_t* __restrict__ charge_i, const int* __restrict__ kek_status, const uint8_t* __restrict__ ring_size_i,
    const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B, int n_lig, int n_half,
    const float* __restrict__ point_pos, const int8_t* __restrict__ point_kind, int n_point, const int* __restrict__ g_point_range,
    const int* __restrict__ g_point_out_off, int n_out, float feat_cut, int max_unmatched, uint8_t* __restrict__ atom_fp,
    float* __restrict__ point_dist, int16_t* __restrict__ point_atom, int* __restrict__ counts, int* __restrict__ status) {
  __shared__ float4 s_atom[kFeatMax];                              // x, y, z, compact index as bits (-1 = dropped or non-finite)
  __shared__ MolAdjRow s_adj[kFeatMax];                            // kept bonds of an atom
  __shared__ uint8_t s_pair[kFeatPairs];                           // feature_core.h's byte per pair row
  __shared__ int8_t s_el[kFeatMax];
  __shared__ uint8_t s_h[kFeatMax], s_q[kFeatMax], s_deg[kFeatMax], s_flags[kFeatMax], s_fp[kFeatMax];
  __shared__ uint16_t s_v[kFeatMax];

  const int lane = threadIdx.x;
  MolFrame m;
  MolPoints pt;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  if (!mol_points(pt, m, g_point_range, g_point_out_off, n_point, n_out)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  const float* prow = pos + (size_t)m.f * pos_fs + (size_t)m.a0 * 3;
  const float inf = __builtin_inff();
  const bool kek_ok = (kek_status[blockIdx.x] & PG_KEKULE_FAILED) == 0;

  // ---- atoms: class, hydrogens, charge, coordinates; empty masks ----------------------------------------------------------------
  bool bad = false;
#pragma unroll
  for (int c = 0; c < kFeatCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      const int k = mol_class(cls_i[arow + i]);
      float x = 0.f, y = 0.f, z = 0.f;
      int ci = -1;
      if (k >= 0) {
        const float* p = prow + (size_t)i * 3;
        x = p[0], y = p[1], z = p[2];
        const bool fin = !(mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z));
        bad |= !fin;
        ci = fin ? (int)compact_i[arow + i] : -1;
      }
      s_el[i] = (int8_t)k;
      s_h[i] = k >= 0 ? hcount_i[arow + i] : (uint8_t)0;
      s_q[i] = (uint8_t)((k >= 0 && charge_i[arow + i] > 0) ? 1 : 0);
      s_atom[i] = make_float4(x, y, z, __int_as_float(ci));
      s_fp[i] = 0;
#pragma unroll
      for (int w = 0; w < kFeatCh; ++w) s_adj[i].w[w] = 0ull;
    }
  }
  __syncthreads();

  int n_atoms_t[kFeatTypes];
#pragma unroll
  for (int t = 0; t < kFeatTypes; ++t) n_atoms_t[t] = 0;

  if (kek_ok) {                                                    // (wave-uniform: one status word per block)
    // ---- bonds ----------------------------------------------------------------------------------------------------------------
    for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
      const int o = order_i[hrow + p];
      int pb = 0;
      if (mol_is_bond(o) && s_el[a] >= 0 && s_el[b] >= 0) {
        const int k = kek_i[hrow + p];
        pb = ((k >= 1 && k <= 3) ? k : 1) | (o == 4 ? kPairArom : 0) | (ring_size_i[hrow + p] > 0 ? kPairRing : 0);
        mol_adj_set(s_adj, a, b);
      }
      s_pair[p] = (uint8_t)pb;
    });
    __syncthreads();

    const FeatGraph fg = {n, s_el, s_h, s_q, mol_adj_words(s_adj), s_pair, s_deg, s_v, s_flags};
    // ---- per atom: degree, valence, arom; then the double-bond flags, which read every neighbour's arom ------------------------
#pragma unroll
    for (int c = 0; c < kFeatCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n) {
        int deg, v, arom;
        feat_atom_sums(fg, i, &deg, &v, &arom);
        s_deg[i] = (uint8_t)deg;
        s_v[i] = (uint16_t)v;
        s_flags[i] = (uint8_t)(arom ? kAtomArom : 0);
      }
    }
    __syncthreads();
    int dbl[kFeatCh];
#pragma unroll
    for (int c = 0; c < kFeatCh; ++c) {
      const int i = c * 64 + lane;
      dbl[c] = i < n ? feat_atom_dbl(fg, i) : 0;
    }
    __syncthreads();                                               // (every read of the arom flags is done before they are rewritten)
#pragma unroll
    for (int c = 0; c < kFeatCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n) s_flags[i] = (uint8_t)(s_flags[i] | dbl[c]);
    }
    __syncthreads();
    // ---- the atoms' bytes ---------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < kFeatCh; ++c) {
      const int i = c * 64 + lane;
      const int bits = i < n ? feat_atom_bits(fg, i) : 0;
      if (i < n) s_fp[i] = (uint8_t)bits;
#pragma unroll
      for (int t = 0; t < kFeatTypes; ++t) n_atoms_t[t] += __popcll(__ballot((bits >> t) & 1));
    }
  }
#pragma unroll
  for (int c = 0; c < kFeatCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) atom_fp[arow + i] = s_fp[i];                        // (its own lane wrote s_fp[i])
  }
  __syncthreads();

  // ---- points, lane-strided: every lane walks all atoms for its own points (one LDS address per step: a broadcast) -------------
  int n_points_t[kFeatTypes], n_matched_t[kFeatTypes], n_untyped = 0;
#pragma unroll
  for (int t = 0; t < kFeatTypes; ++t) n_points_t[t] = n_matched_t[t] = 0;
  for (int q = pt.ps + lane; q < pt.pe; q += 64) {
    const float* pp = point_pos + (size_t)q * 3;
    const float x = pp[0], y = pp[1], z = pp[2];
    const int kind = point_kind[q];
    float best = inf;
    int best_i = -1;
    if (kind >= -1 && kind < kFeatTypes) {                         // (anything else is an exclusion sphere or to be ignored)
      if (mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z)) {
        bad = true;                                                // left out of everything but its own two outputs
      } else if (kind < 0) {
        ++n_untyped;
      } else {
        int close = 0;                                             // (not asked for: with clear = 0 no d < clear, the count is dead code)
        mol_nearest_atom(s_atom, n, x, y, z, 0.f, [&](int i) { return (s_fp[i] >> kind) & 1; }, best, best_i, close);
        const bool hit = best < feat_cut;
#pragma unroll
        for (int t = 0; t < kFeatTypes; ++t) {                     // (constant indices: the counters stay in registers)
          n_points_t[t] += kind == t;
          n_matched_t[t] += kind == t && hit;
        }
      }
    }
    point_dist[pt.orow + (q - pt.ps)] = best;
    point_atom[pt.orow + (q - pt.ps)] = (int16_t)best_i;
  }

  // ---- the wave's totals (all lanes are back together here), then lane 0 writes the graph's row --------------------------------
  int n_typed = 0, n_matched = 0;
#pragma unroll
  for (int t = 0; t < kFeatTypes; ++t) {
    n_points_t[t] = wave_sum(n_points_t[t]);
    n_matched_t[t] = wave_sum(n_matched_t[t]);
    n_typed += n_points_t[t];
    n_matched += n_matched_t[t];
  }
  n_untyped = wave_sum(n_untyped);
  const bool any_bad = __any(bad);
  if (lane != 0) return;
  int* crow = counts + (size_t)blockIdx.x * PG_FEAT_N_COUNTS;
  crow[0] = n_typed, crow[1] = n_matched, crow[2] = n_typed - n_matched, crow[3] = n_untyped;
#pragma unroll
  for (int t = 0; t < kFeatTypes; ++t) {
    crow[4 + t] = n_atoms_t[t];
    crow[4 + kFeatTypes + t] = n_points_t[t];
    crow[4 + 2 * kFeatTypes + t] = n_matched_t[t];
  }
  int st = 0;
  st |= kek_ok ? 0 : PG_FEAT_NO_KEKULE;
  st |= n_typed - n_matched > max_unmatched ? PG_FEAT_UNMATCHED : 0;
  st |= n_untyped > 0 ? PG_FEAT_HAS_UNTYPED : 0;
  st |= any_bad ? PG_FEAT_NONFINITE : 0;
  status[blockIdx.x] = st;
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_feat(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int16_t* compact,
                           const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge, const int* kekule_status,
                           const uint8_t* ring_size, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig, int n_bond,
                           int max_n, const float* point_pos, const int8_t* point_kind, int n_point, const int* g_point_range,
                           const int* g_point_out_off, int n_point_out, float feat_cut, int max_unmatched, uint8_t* atom_fp,
                           float* point_dist, int16_t* point_atom, int* counts, int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_feat", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (n_point < 0 || n_point_out < 0 || max_unmatched < 0) {
    set_error("pg_mol_feat: n_point %d, n_point_out %d, max_unmatched %d", n_point, n_point_out, max_unmatched);
    return PG_ERR_ARG;
  }
  if (!(feat_cut == feat_cut)) {
    set_error("pg_mol_feat: feat_cut is not a number");
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  if (!pos || !cls || !order || !compact || !kekule_order || !hcount || !charge || !kekule_status || !ring_size || !g_lig_off ||
      !g_bond_off || !g_point_range || !g_point_out_off || !atom_fp || !counts || !status ||
      (n_point > 0 && (!point_pos || !point_kind)) || (n_point_out > 0 && (!point_dist || !point_atom))) {
    set_error("pg_mol_feat: an array is null (the screen's cls / order / compact, the Kekulé form's kekule_order / hcount / charge / "
              "status, ring_size, the offsets and ranges, the points and the outputs are all device memory)");
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_feat_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, pos, (long)pos_fs, cls, order, compact,
                     kekule_order, hcount, charge, kekule_status, ring_size, g_lig_off, g_bond_off, B, n_lig, n_bond / 2, point_pos,
                     point_kind, n_point, g_point_range, g_point_out_off, n_point_out, feat_cut, max_unmatched, atom_fp, point_dist,
                     point_atom, counts, status);
  return check_launch("pg_mol_feat");
}
