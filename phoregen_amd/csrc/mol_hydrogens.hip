// 3D hydrogens of the molecules the screen decoded: every hydrogen `kekulize` counted gets a position from the ideal local geometry
// of its parent (pg_mol_hydrogens, include/phoregen_hip.h; phoregen_amd/hydrogens.py; definition: DESIGN.md 2.9 "Hydrogens").  Reads
// the coordinates, the screen's cls and order and the Kekulé form.  One wave per (frame, graph) (mol_common.h): positions, classes and
// adjacency rows are staged in LDS once, the atoms are dealt two per lane, the pairs by for_each_pair; the shape rule and the
// direction arithmetic are hydrogen_core.h's.  The placed hydrogens are packed into LDS in (parent, slot) order and the contact pass
// walks them, a hydrogen per lane, against the atoms (one LDS address for the whole wave per step) and the hydrogens after it
// (consecutive addresses).  No barrier inside a lane-dependent loop.
#include "mol_common.h"
#include "wave_prims.h"
#include "hydrogen_core.h"

namespace pg {

constexpr int kHydN = PG_HYD_N_COUNTS;

__device__ __forceinline__ void hyd_store(float* __restrict__ h_pos, size_t atom, const HydOut& o) {
  float4* dst = reinterpret_cast<float4*>(h_pos + atom * (size_t)(3 * kHydMaxH));   // 48 bytes per atom: 16-byte aligned with the array
  dst[0] = make_float4(o.h0.x, o.h0.y, o.h0.z, o.h1.x);
  dst[1] = make_float4(o.h1.y, o.h1.z, o.h2.x, o.h2.y);
  dst[2] = make_float4(o.h2.z, o.h3.x, o.h3.y, o.h3.z);
}

__global__ __launch_bounds__(64) void mol_hydrogens_kernel(const float* __restrict__ pos_i, long long pos_fs, const int8_t* __restrict__ cls_i,
                                                           const int8_t* __restrict__ order_i, const int8_t* __restrict__ kek_i,
                                                           const uint8_t* __restrict__ hcount_i, const int* __restrict__ kstatus_i,
                                                           const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B, int n_lig,
                                                           int n_half, const float* __restrict__ xh_i, float clash_min, int max_contacts,
                                                           float* __restrict__ h_pos_o, uint8_t* __restrict__ placed_o,
                                                           uint8_t* __restrict__ shape_o, float* __restrict__ minc_o, int* __restrict__ counts_o,
                                                           int* __restrict__ status_o) {
  __shared__ HydAtom s_atom[kMolMax];                             // position and what the core reads of the atom
  __shared__ MolAdjRow s_adj[kMolMax];                            // heavy neighbours: pair rows of Kekulé order 1..3 between kept atoms
  __shared__ unsigned int s_bond[kMolMax];                        // the bond part of HydAtom::info, gathered by the pair walk
  __shared__ float4 s_h[kHydMaxH * kMolMax];                      // placed hydrogens, packed: x, y, z, the parent's local index as bits
  __shared__ float s_len[16];                                     // X-H length per class

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  int* const cnt = counts_o + (size_t)blockIdx.x * kHydN;
  const HydVec zero = {0.0f, 0.0f, 0.0f};
  const HydOut none = {zero, zero, zero, zero};

  // ---- a graph without a Kekulé structure has no hydrogen counts to place (wave-uniform) -------------------------------------------------
  if (kstatus_i[blockIdx.x] & PG_KEKULE_FAILED) {
    for (int i = lane; i < n; i += 64) {
      hyd_store(h_pos_o, arow + i, none);
      placed_o[arow + i] = shape_o[arow + i] = 0;
    }
    if (lane < kHydN) cnt[lane] = 0;
    if (lane == 0) {
      minc_o[blockIdx.x] = 0.0f;
      status_o[blockIdx.x] = PG_HYD_NO_KEKULE;
    }
    return;
  }

  // ---- atoms ---------------------------------------------------------------------------------------------------------------------------
  const float* pos = pos_i + (size_t)m.f * (size_t)pos_fs + (size_t)m.a0 * 3;
  bool bad = false, too = false;
  int kept = 0;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      const int k = mol_class(cls_i[arow + i]);
      const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
      const bool nonfinite = k >= 0 && (mol_nonfinite(x) || mol_nonfinite(y) || mol_nonfinite(z));
      const unsigned h = k >= 0 ? hcount_i[arow + i] : 0u;
      s_atom[i] = {x, y, z, (k >= 0 ? (unsigned)k : kHydDropped) | (nonfinite ? kHydNonfinite : 0u) | h << kHydHShift};
      s_bond[i] = 0u;
#pragma unroll
      for (int w = 0; w < kMolCh; ++w) s_adj[i].w[w] = 0ull;
      bad |= nonfinite;
      too |= h > (unsigned)kHydMaxH;
      kept += k >= 0;
    }
  }
  if (lane < 16) s_len[lane] = lane < 11 ? xh_i[lane] : 0.0f;
  __syncthreads();

  // ---- bonds ---------------------------------------------------------------------------------------------------------------------------
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    if ((s_atom[a].info & 15u) == kHydDropped || (s_atom[b].info & 15u) == kHydDropped) return;
    const int ko = kek_i[hrow + p];
    unsigned add = order_i[hrow + p] == 4 ? kHydArom : 0u;
    if (ko >= 1 && ko <= 3) {
      mol_adj_set(s_adj, a, b);
      add |= ko == 3 ? kHydTriple : 0u;
    }
    if (add) {
      atomicOr(&s_bond[a], add);
      atomicOr(&s_bond[b], add);
    }
    if (ko == 2) {                                                 // (at most 127 bonds per atom: the count stays in its byte)
      atomicAdd(&s_bond[a], 1u << kHydDoubleShift);
      atomicAdd(&s_bond[b], 1u << kHydDoubleShift);
    }
  });
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) s_atom[i].info |= s_bond[i];
  }
  __syncthreads();

  // ---- sites: one atom per lane and pass; the hydrogens go to memory slot by slot and to LDS packed --------------------------------------
  const bool too_many = __any(too);                                // (the tables cannot give more than four; the kernel does not trust them)
  const unsigned long long below = (1ull << lane) - 1ull;
  int n_h = 0, c_h = 0, c_site = 0, c_tet = 0, c_trig = 0, c_lin = 0, c_gen = 0;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    HydOut o = none;
    int placed = 0, shape = 0;
    if (i < n && !too_many) placed = hyd_site(s_atom, mol_adj_words(s_adj), i, s_len, o, shape);
    if (i < n) {
      hyd_store(h_pos_o, arow + i, o);
      placed_o[arow + i] = (uint8_t)placed;
      shape_o[arow + i] = (uint8_t)shape;
    }
    c_h += placed, c_site += placed > 0;
    c_tet += shape == kHydTet, c_trig += shape == kHydTrig, c_lin += shape == kHydLin, c_gen += shape == kHydGeneric;
    const float parent = __int_as_float(i);
    int at = n_h;                                                 // this lane's first packed slot: the hydrogens of the lanes below first
    {
      int mine = 0;
#pragma unroll
      for (int k = 0; k < kHydMaxH; ++k) {
        const unsigned long long has = __ballot(k < placed);
        mine += __popcll(has & below);
        n_h += __popcll(has);
      }
      at += mine;
    }
    if (placed > 0) s_h[at] = make_float4(o.h0.x, o.h0.y, o.h0.z, parent);
    if (placed > 1) s_h[at + 1] = make_float4(o.h1.x, o.h1.y, o.h1.z, parent);
    if (placed > 2) s_h[at + 2] = make_float4(o.h2.x, o.h2.y, o.h2.z, parent);
    if (placed > 3) s_h[at + 3] = make_float4(o.h3.x, o.h3.y, o.h3.z, parent);
  }
  __syncthreads();

  // ---- contacts: a hydrogen per lane against every kept atom but its parent and every later hydrogen of another parent -------------------
  int contacts = 0;
  float minc = INFINITY;
  for (int q = lane; q < n_h; q += 64) {
    const float4 hq = s_h[q];
    const int parent = __float_as_int(hq.w);
    const HydVec ph = {hq.x, hq.y, hq.z};
    for (int j = 0; j < n; ++j) {
      const HydAtom a = s_atom[j];
      if ((a.info & 15u) == kHydDropped || j == parent) continue;
      const float d = hyd_dist(ph, hv_of(a));
      contacts += d < clash_min;
      minc = fminf(minc, d);                                       // (a non-finite atom gives NaN or +inf: neither moves the minimum)
    }
    for (int r = q + 1; r < n_h; ++r) {
      const float4 hr = s_h[r];
      if (__float_as_int(hr.w) == parent) continue;
      const float d = hyd_dist(ph, HydVec{hr.x, hr.y, hr.z});
      contacts += d < clash_min;
      minc = fminf(minc, d);
    }
  }

  // ---- counts, status --------------------------------------------------------------------------------------------------------------------
  c_h = wave_sum(c_h), c_site = wave_sum(c_site), c_tet = wave_sum(c_tet), c_trig = wave_sum(c_trig), c_lin = wave_sum(c_lin);
  c_gen = wave_sum(c_gen), contacts = wave_sum(contacts), kept = wave_sum(kept);
  minc = wave_min(minc);
  const bool nonfinite = __any(bad);
  if (lane == 0) {
    int st = 0;
    st |= nonfinite ? PG_HYD_NONFINITE : 0;
    st |= too_many ? PG_HYD_TOO_MANY : 0;
    st |= contacts > max_contacts ? PG_HYD_CONTACTS : 0;
    st |= c_gen > 0 ? PG_HYD_GENERIC : 0;
    st |= c_h > 0 ? PG_HYD_HAS_HYDROGEN : 0;
    status_o[blockIdx.x] = st;
    minc_o[blockIdx.x] = minc;
    cnt[0] = c_h, cnt[1] = c_site, cnt[2] = c_tet, cnt[3] = c_trig, cnt[4] = c_lin, cnt[5] = c_gen, cnt[6] = contacts, cnt[7] = kept;
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_hydrogens(const float* pos, int64_t pos_fs, const int8_t* cls, const int8_t* order, const int8_t* kekule_order,
                                const uint8_t* hcount, const int8_t* charge, const int* kekule_status, const int* g_lig_off,
                                const int* g_bond_off, int B, int F, int n_lig, int n_bond, int max_n, const float* xh_length, float clash_min,
                                int max_contacts, float* h_pos, uint8_t* h_placed, uint8_t* site_shape, float* min_contact, int* counts,
                                int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_hydrogens", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (!(clash_min >= 0.0f) || !(clash_min < INFINITY) || max_contacts < 0) {
    set_error("pg_mol_hydrogens: clash_min %g, max_contacts %d (a finite distance of at least 0, a count of at least 0)", (double)clash_min,
              max_contacts);
    return PG_ERR_ARG;
  }
  if (!xh_length) {
    set_error("pg_mol_hydrogens: the table of X-H lengths is null");
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  // (an array without elements may be null: a batch of single atoms has no pair rows, one of empty graphs no atom rows)
  const bool atoms_null = !pos || !cls || !hcount || !charge || !h_pos || !h_placed || !site_shape, pairs_null = !order || !kekule_order;
  if ((n_lig > 0 && atoms_null) || (n_bond > 0 && pairs_null) || !kekule_status || !g_lig_off || !g_bond_off || !min_contact || !counts ||
      !status) {
    set_error("pg_mol_hydrogens: an array is null (pos, cls, order, kekule_order, hcount, charge, kekule_status, the offsets and the six "
              "outputs)");
    return PG_ERR_ARG;
  }
  if ((uintptr_t)h_pos & 15u) {
    set_error("pg_mol_hydrogens: h_pos must be 16-byte aligned");
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_hydrogens_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, pos, (long long)pos_fs, cls, order,
                     kekule_order, hcount, kekule_status, g_lig_off, g_bond_off, B, n_lig, n_bond / 2, xh_length, clash_min, max_contacts, h_pos,
                     h_placed, site_shape, min_contact, counts, status);
  return check_launch("pg_mol_hydrogens");
}
