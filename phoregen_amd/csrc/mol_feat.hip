// Pharmacophore feature typing of the molecules the screen decoded, and the typed match against their feature points (pg_mol_feat,
// include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Features").  Reads the screen's outputs (cls, order,
// compact), the Kekulé form (kekule_order, hcount, charge, status), the rings' ring_size and the coordinates.  One wave per
// (frame, graph); a workgroup IS one wave, so __syncthreads() orders the wave's LDS traffic, and every loop that holds one (or a vote)
// has a wave-uniform trip count: the divergent loops below (pair rows, an atom's neighbours, points) hold neither.  Typing is integer
// work (feature_core.h) and exact; the only floating point is a point's distance to an atom, the fp32 expression of mol_geom.hip.
#include "common.h"
#include "wave_prims.h"
#include "feature_core.h"
#include "../../include/phoregen_hip.h"

namespace pg {

constexpr int kFeatMax = PG_MOL_MAX_ATOMS;   // atoms of the largest graph
constexpr int kFeatCh = kFeatMax / 64;       // atoms per lane = 64-bit adjacency words per atom
constexpr int kFeatPairs = kFeatMax * (kFeatMax - 1) / 2;
static_assert(kFeatCh == 2 && kFeatMax <= 255, "feature_core.h walks two mask words per atom; a degree fits one byte");

__device__ __forceinline__ bool feat_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(64) void mol_feat_kernel(
    const float* __restrict__ pos, long pos_fs, const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
    const int16_t* __restrict__ compact_i, const int8_t* __restrict__ kek_i, const uint8_t* __restrict__ hcount_i,
    const int8_t* __restrict__ charge_i, const int* __restrict__ kek_status, const uint8_t* __restrict__ ring_size_i,
    const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B, int n_lig, int n_half,
    const float* __restrict__ point_pos, const int8_t* __restrict__ point_kind, int n_point, const int* __restrict__ g_point_range,
    const int* __restrict__ g_point_out_off, int n_out, float feat_cut, int max_unmatched, uint8_t* __restrict__ atom_fp,
    float* __restrict__ point_dist, int16_t* __restrict__ point_atom, int* __restrict__ counts, int* __restrict__ status) {
  __shared__ float4 s_atom[kFeatMax];                              // x, y, z, compact index as bits (-1 = dropped or non-finite)
  __shared__ __align__(16) unsigned long long s_adj[kFeatMax * kFeatCh];   // kept bonds of an atom, a bit per local index
  __shared__ uint8_t s_pair[kFeatPairs];                           // feature_core.h's byte per pair row
  __shared__ int8_t s_el[kFeatMax];
  __shared__ uint8_t s_h[kFeatMax], s_q[kFeatMax], s_deg[kFeatMax], s_flags[kFeatMax], s_fp[kFeatMax];
  __shared__ uint16_t s_v[kFeatMax];

  const int lane = threadIdx.x;
  const int f = blockIdx.x / B, g = blockIdx.x - f * B;
  const int a0 = g_lig_off[g], n = g_lig_off[g + 1] - a0;
  if (n > kFeatMax || n < 0) return;                               // (the host wrapper has refused such a batch: never index LDS past its end)
  const int h0 = g_bond_off[g] >> 1, n_pair = n * (n - 1) / 2;
  if (a0 < 0 || a0 + n > n_lig || h0 < 0 || h0 + n_pair > n_half) return;   // (offsets that leave the frame: never read or write past it)
  const int ps = g_point_range[2 * g], pe = g_point_range[2 * g + 1], o0 = g_point_out_off[g];
  if (ps < 0 || pe < ps || pe > n_point || o0 < 0 || g_point_out_off[g + 1] - o0 != pe - ps || o0 + (pe - ps) > n_out) return;
  const float* prow = pos + (size_t)f * pos_fs + (size_t)a0 * 3;
  const size_t arow = (size_t)f * n_lig + a0, hrow = (size_t)f * n_half + h0, orow = (size_t)f * n_out + o0;
  const float inf = __builtin_inff();
  const bool kek_ok = (kek_status[blockIdx.x] & PG_KEKULE_FAILED) == 0;

  // ---- atoms: class, hydrogens, charge, coordinates; empty masks ----------------------------------------------------------------
  bool bad = false;
#pragma unroll
  for (int c = 0; c < kFeatCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      int k = cls_i[arow + i];
      k = (k >= 0 && k < 11) ? k : -1;
      float x = 0.f, y = 0.f, z = 0.f;
      int ci = -1;
      if (k >= 0) {
        const float* p = prow + (size_t)i * 3;
        x = p[0], y = p[1], z = p[2];
        const bool fin = !(feat_nonfinite(x) || feat_nonfinite(y) || feat_nonfinite(z));
        bad |= !fin;
        ci = fin ? (int)compact_i[arow + i] : -1;
      }
      s_el[i] = (int8_t)k;
      s_h[i] = k >= 0 ? hcount_i[arow + i] : (uint8_t)0;
      s_q[i] = (uint8_t)((k >= 0 && charge_i[arow + i] > 0) ? 1 : 0);
      s_atom[i] = make_float4(x, y, z, __int_as_float(ci));
      s_fp[i] = 0;
#pragma unroll
      for (int w = 0; w < kFeatCh; ++w) s_adj[i * kFeatCh + w] = 0ull;
    }
  }
  __syncthreads();

  int n_atoms_t[kFeatTypes];
#pragma unroll
  for (int t = 0; t < kFeatTypes; ++t) n_atoms_t[t] = 0;

  if (kek_ok) {                                                    // (wave-uniform: one status word per block)
    // ---- bonds: the pairs a < b in row-major order, dealt to lanes (pair p is lane p mod 64's) ---------------------------------
    {
      int a = 0, b = 1 + lane;
      for (int p = lane; p < n_pair; p += 64, b += 64) {
        while (b >= n) {                                           // next row of the triangle (p < n_pair: ends with a < n - 1)
          ++a;
          b = b - n + a + 1;
        }
        const int o = order_i[hrow + p];
        int pb = 0;
        if (o >= 1 && o <= 4 && s_el[a] >= 0 && s_el[b] >= 0) {
          const int k = kek_i[hrow + p];
          pb = ((k >= 1 && k <= 3) ? k : 1) | (o == 4 ? kPairArom : 0) | (ring_size_i[hrow + p] > 0 ? kPairRing : 0);
          atomicOr(&s_adj[a * kFeatCh + (b >> 6)], 1ull << (b & 63));
          atomicOr(&s_adj[b * kFeatCh + (a >> 6)], 1ull << (a & 63));
        }
        s_pair[p] = (uint8_t)pb;
      }
    }
    __syncthreads();

    const FeatGraph fg = {n, s_el, s_h, s_q, s_adj, s_pair, s_deg, s_v, s_flags};
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
  for (int q = ps + lane; q < pe; q += 64) {
    const float* pp = point_pos + (size_t)q * 3;
    const float x = pp[0], y = pp[1], z = pp[2];
    const int kind = point_kind[q];
    float best = inf;
    int best_i = -1;
    if (kind >= -1 && kind < kFeatTypes) {                         // (anything else is an exclusion sphere or to be ignored)
      if (feat_nonfinite(x) || feat_nonfinite(y) || feat_nonfinite(z)) {
        bad = true;                                                // left out of everything but its own two outputs
      } else if (kind < 0) {
        ++n_untyped;
      } else {
        for (int i = 0; i < n; ++i) {
          const float4 pa = s_atom[i];
          const int ci = __float_as_int(pa.w);
          if (ci < 0 || !((s_fp[i] >> kind) & 1)) continue;
          const float dx = pa.x - x, dy = pa.y - y, dz = pa.z - z;
          const float d = sqrtf(dx * dx + dy * dy + dz * dz);
          best_i = d < best ? ci : best_i;                         // (strict: the first minimum in atom order stays)
          best = fminf(best, d);
        }
        const bool hit = best < feat_cut;
#pragma unroll
        for (int t = 0; t < kFeatTypes; ++t) {                     // (constant indices: the counters stay in registers)
          n_points_t[t] += kind == t;
          n_matched_t[t] += kind == t && hit;
        }
      }
    }
    point_dist[orow + (q - ps)] = best;
    point_atom[orow + (q - ps)] = (int16_t)best_i;
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
  if (B < 0 || F < 0 || n_lig < 0 || n_bond < 0 || (n_bond & 1) || max_n < 0 || n_point < 0 || n_point_out < 0 || max_unmatched < 0) {
    set_error("pg_mol_feat: B %d, F %d, n_lig %d, n_bond %d, max_n %d, n_point %d, n_point_out %d, max_unmatched %d (n_bond counts both "
              "directions of every pair)", B, F, n_lig, n_bond, max_n, n_point, n_point_out, max_unmatched);
    return PG_ERR_ARG;
  }
  if (max_n > PG_MOL_MAX_ATOMS) {
    set_error("pg_mol_feat: a graph of %d atoms, the kernel holds at most PG_MOL_MAX_ATOMS = %d", max_n, PG_MOL_MAX_ATOMS);
    return PG_ERR_ARG;
  }
  if (!(feat_cut == feat_cut)) {
    set_error("pg_mol_feat: feat_cut is not a number");
    return PG_ERR_ARG;
  }
  if (B == 0 || F == 0) return PG_OK;
  if ((long long)B * F > 0x7fffffffLL) {
    set_error("pg_mol_feat: %d frames x %d graphs exceed one launch", F, B);
    return PG_ERR_ARG;
  }
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
