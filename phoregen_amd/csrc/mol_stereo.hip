// Stereo perception of the molecules the screen decoded: the parity of every tetrahedral centre, cis / trans of every double bond, their
// numbering-invariant labels and a key that tells stereoisomers apart (pg_mol_stereo, include/phoregen_hip.h;
// phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Stereo").  Reads the coordinates, the screen's cls and order, the Kekulé form,
// the rings' ring_size and the key's colours.  One wave per (frame, graph) (mol_common.h): the atoms are dealt two per lane, the
// pairs by for_each_pair; the rules and the arithmetic are stereo_core.h's.  No loop here but the pair walk and the two passes over a
// lane's atoms; no barrier inside either.
#include "mol_common.h"
#include "wave_prims.h"
#include "stereo_core.h"

namespace pg {

constexpr int kStMax = kMolMax, kStCh = kMolCh;

// the lowest set bit of a row, struck from it; -1 (and the row unchanged) if it is empty
__device__ __forceinline__ int stereo_take_lowest(MolAdjRow& r) {
  if (r.w[0]) {
    const int j = __builtin_ctzll(r.w[0]);
    r.w[0] &= r.w[0] - 1ull;
    return j;
  }
  if (r.w[1]) {
    const int j = 64 + __builtin_ctzll(r.w[1]);
    r.w[1] &= r.w[1] - 1ull;
    return j;
  }
  return -1;
}

// atom j struck from a row (written without an index into the row, which would put it into memory)
__device__ __forceinline__ void stereo_strike(MolAdjRow& r, int j) {
  const unsigned long long bit = 1ull << (j & 63);
  r.w[0] &= ~(j < 64 ? bit : 0ull);
  r.w[1] &= ~(j < 64 ? 0ull : bit);
}

__device__ __forceinline__ StereoVec stereo_pos(const float4* s_pos, int i) {
  const float4 p = s_pos[i];
  return {p.x, p.y, p.z};
}

__global__ __launch_bounds__(64) void mol_stereo_kernel(const float* __restrict__ pos_i, long long pos_fs, const int8_t* __restrict__ cls_i,
                                                        const int8_t* __restrict__ order_i, const int8_t* __restrict__ kek_i,
                                                        const uint8_t* __restrict__ hcount_i, const int* __restrict__ kstatus_i,
                                                        const uint8_t* __restrict__ ring_size_i, const long long* __restrict__ colour_i,
                                                        const long long* __restrict__ key_i, const int* __restrict__ g_lig_off,
                                                        const int* __restrict__ g_bond_off, int B, int n_lig, int n_half, float vol_min,
                                                        float planar_min, int max_undefined, int8_t* __restrict__ parity_o,
                                                        int8_t* __restrict__ alabel_o, int8_t* __restrict__ bstereo_o,
                                                        int8_t* __restrict__ blabel_o, long long* __restrict__ skey_o,
                                                        int* __restrict__ counts_o, int* __restrict__ status_o) {
  __shared__ int s_cls[kStMax];                                   // atom class, -1 = dropped
  __shared__ MolAdjRow s_adj[kStMax];                             // kept bonds of an atom (the screen's order 1..4)
  __shared__ unsigned int s_multi[kStMax];                        // its bonds of Kekulé order >= 2
  __shared__ int s_h[kStMax];                                     // its hydrogens
  __shared__ float4 s_pos[kStMax];
  __shared__ unsigned long long s_col[kStMax];

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  int* const cnt = counts_o + (size_t)blockIdx.x * PG_STEREO_N_COUNTS;

  // ---- a graph without a Kekulé structure has no stereo (wave-uniform) -----------------------------------------------------------
  if (kstatus_i[blockIdx.x] & PG_KEKULE_FAILED) {
    for (int i = lane; i < n; i += 64) parity_o[arow + i] = alabel_o[arow + i] = 0;
    for (int p = lane; p < m.n_pair; p += 64) bstereo_o[hrow + p] = blabel_o[hrow + p] = 0;
    if (lane < PG_STEREO_N_COUNTS) cnt[lane] = 0;
    if (lane == 0) {
      skey_o[blockIdx.x] = key_i[blockIdx.x];
      status_o[blockIdx.x] = PG_STEREO_NO_KEKULE;
    }
    return;
  }

  // ---- atoms ---------------------------------------------------------------------------------------------------------------------
  const float* pos = pos_i + (size_t)m.f * (size_t)pos_fs + (size_t)m.a0 * 3;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < kStCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      const int k = mol_class(cls_i[arow + i]);
      const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
      s_cls[i] = k;
      s_multi[i] = 0u;
      s_h[i] = hcount_i[arow + i];
      s_pos[i] = make_float4(x, y, z, 0.0f);
      s_col[i] = (unsigned long long)colour_i[arow + i];
#pragma unroll
      for (int w = 0; w < kStCh; ++w) s_adj[i].w[w] = 0ull;
      bad |= k >= 0 && (mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z));
    }
  }
  __syncthreads();

  // ---- bonds ---------------------------------------------------------------------------------------------------------------------
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    if (mol_is_bond(order_i[hrow + p]) && s_cls[a] >= 0 && s_cls[b] >= 0) {
      mol_adj_set(s_adj, a, b);
      if (kek_i[hrow + p] >= 2) {
        atomicAdd(&s_multi[a], 1u);
        atomicAdd(&s_multi[b], 1u);
      }
    }
  });
  __syncthreads();

  // ---- centres: one atom per lane and pass ---------------------------------------------------------------------------------------
  int c_cand = 0, c_gen = 0, c_def = 0, c_undef = 0;
  unsigned long long sum = 0ull;
#pragma unroll
  for (int c = 0; c < kStCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      int parity = 0, label = 0;
      MolAdjRow row = s_adj[i];
      const int degree = __popcll(row.w[0]) + __popcll(row.w[1]), h = s_h[i];
      if (s_cls[i] >= 0 && stereo_centre_candidate(s_cls[i], degree, h)) {
        ++c_cand;
        const int n0 = stereo_take_lowest(row), n1 = stereo_take_lowest(row), n2 = stereo_take_lowest(row);
        const bool four = degree == 4;
        const int n3 = four ? stereo_take_lowest(row) : n2;        // (degree 3: never read as a fourth neighbour)
        const int sign = stereo_sort_sign(s_col[n0], s_col[n1], s_col[n2], s_col[n3], four ? 4 : 3);
        if (sign != 0) {
          ++c_gen;
          parity = stereo_centre_parity(stereo_pos(s_pos, i), stereo_pos(s_pos, n0), stereo_pos(s_pos, n1), stereo_pos(s_pos, n2),
                                        stereo_pos(s_pos, n3), four, vol_min);
          label = parity == kStereoUndefined ? kStereoUndefined : parity * sign;
          if (parity == kStereoUndefined) {
            ++c_undef;
          } else {
            ++c_def;
            sum += stereo_centre_word(s_col[i], label);
          }
        }
      }
      parity_o[arow + i] = (int8_t)parity;
      alabel_o[arow + i] = (int8_t)label;
    }
  }

  // ---- double bonds: the pairs as they were dealt; every pair row is written -----------------------------------------------------
  int b_cand = 0, b_gen = 0, b_def = 0, b_undef = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    int stereo = 0, label = 0;
    const int o = order_i[hrow + p];
    if (o >= 1 && o <= 3 && kek_i[hrow + p] == 2 && ring_size_i[hrow + p] == 0 && s_cls[a] >= 0 && s_cls[b] >= 0) {
      MolAdjRow ra = s_adj[a], rb = s_adj[b];
      const int deg_a = __popcll(ra.w[0]) + __popcll(ra.w[1]), deg_b = __popcll(rb.w[0]) + __popcll(rb.w[1]);
      if (stereo_bond_end(deg_a, (int)s_multi[a], s_h[a]) && stereo_bond_end(deg_b, (int)s_multi[b], s_h[b])) {
        ++b_cand;
        stereo_strike(ra, b);                                      // the substituents: the neighbours other than the partner
        stereo_strike(rb, a);
        const int a0 = stereo_take_lowest(ra), a1 = stereo_take_lowest(ra), b0 = stereo_take_lowest(rb), b1 = stereo_take_lowest(rb);
        const unsigned long long ca0 = s_col[a0], ca1 = a1 >= 0 ? s_col[a1] : 0ull, cb0 = s_col[b0], cb1 = b1 >= 0 ? s_col[b1] : 0ull;
        if ((a1 < 0 || ca0 != ca1) && (b1 < 0 || cb0 != cb1)) {
          ++b_gen;
          stereo = stereo_bond_side(stereo_pos(s_pos, a), stereo_pos(s_pos, b), stereo_pos(s_pos, a0), stereo_pos(s_pos, b0), planar_min);
          if (stereo == kStereoUndefined) {
            ++b_undef;
            label = kStereoUndefined;
          } else {
            ++b_def;
            label = stereo * stereo_end_factor(ca0, a1 >= 0, ca1, s_h[a]) * stereo_end_factor(cb0, b1 >= 0, cb1, s_h[b]);
            sum += stereo_bond_word(s_col[a], s_col[b], label);
          }
        }
      }
    }
    bstereo_o[hrow + p] = (int8_t)stereo;
    blabel_o[hrow + p] = (int8_t)label;
  });

  // ---- counts, status, key -------------------------------------------------------------------------------------------------------
  c_cand = wave_sum(c_cand), c_gen = wave_sum(c_gen), c_def = wave_sum(c_def), c_undef = wave_sum(c_undef);
  b_cand = wave_sum(b_cand), b_gen = wave_sum(b_gen), b_def = wave_sum(b_def), b_undef = wave_sum(b_undef);
  sum = wave_sum(sum);
  const bool nonfinite = __any(bad);
  if (lane == 0) {
    int st = 0;
    st |= c_undef + b_undef > max_undefined ? PG_STEREO_UNDEFINED : 0;
    st |= c_def > 0 ? PG_STEREO_HAS_CENTRE : 0;
    st |= b_def > 0 ? PG_STEREO_HAS_BOND : 0;
    st |= nonfinite ? PG_STEREO_NONFINITE : 0;
    status_o[blockIdx.x] = st;
    const unsigned long long key = (unsigned long long)key_i[blockIdx.x];
    skey_o[blockIdx.x] = (long long)(c_def + b_def > 0 ? stereo_key(key, sum) : key);
    cnt[0] = c_cand, cnt[1] = c_gen, cnt[2] = c_def, cnt[3] = c_undef;
    cnt[4] = b_cand, cnt[5] = b_gen, cnt[6] = b_def, cnt[7] = b_undef;
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_stereo(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int8_t* kekule_order,
                             const uint8_t* hcount, const int8_t* charge, const int* kekule_status, const uint8_t* ring_size,
                             const int64_t* colour, const int64_t* key, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig,
                             int n_bond, int max_n, float vol_min, float planar_min, int max_undefined, int8_t* atom_parity,
                             int8_t* atom_label, int8_t* bond_stereo, int8_t* bond_label, int64_t* stereo_key, int* counts, int* status,
                             void* stream) {
  const int rc = mol_check_batch("pg_mol_stereo", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (!(vol_min > 0.0f) || !(planar_min > 0.0f) || !(vol_min < INFINITY) || !(planar_min < INFINITY) || max_undefined < 0) {
    set_error("pg_mol_stereo: vol_min %g, planar_min %g, max_undefined %d (finite thresholds above 0, a count of at least 0)", (double)vol_min,
              (double)planar_min, max_undefined);
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  if (!pos || !cls || !order || !kekule_order || !hcount || !charge || !kekule_status || !ring_size || !colour || !key || !g_lig_off ||
      !g_bond_off || !atom_parity || !atom_label || !bond_stereo || !bond_label || !stereo_key || !counts || !status) {
    set_error("pg_mol_stereo: an array is null (pos, cls, order, kekule_order, hcount, charge, kekule_status, ring_size, colour, key, the "
              "offsets and the seven outputs)");
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_stereo_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, pos, (long long)pos_fs, cls, order,
                     kekule_order, hcount, kekule_status, ring_size, (const long long*)colour, (const long long*)key, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, vol_min, planar_min, max_undefined, atom_parity, atom_label, bond_stereo, bond_label,
                     (long long*)stereo_key, counts, status);
  return check_launch("pg_mol_stereo");
}
