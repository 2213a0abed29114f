// Ring perception of the molecules the screen decoded: smallest ring through every bond and atom, ring systems, and the counts users
// filter on (pg_mol_rings, include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Rings").  Reads the screen's
// outputs (cls, order), not the scores.  One wave per (frame, graph) (mol_common.h); the divergent loops below (bond rows, the search
// of a bond's ring, ring_search.h) hold no barrier or vote.  Integer work only, no floating point anywhere, so every output is exact.
#include "ring_search.h"
#include "wave_prims.h"

namespace pg {

constexpr int kRingMax = kMolMax, kRingCh = kMolCh;
static_assert(kRingMax <= 255, "a ring size fits one byte");

struct RingLimits {
  int ring_min, ring_max, system_max, rotatable_max;
};

__global__ __launch_bounds__(64) void mol_rings_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                       const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
                                                       int n_lig, int n_half, RingLimits lim, uint8_t* __restrict__ ring_size_o,
                                                       uint8_t* __restrict__ atom_ring_o, int16_t* __restrict__ ring_sys_o,
                                                       int* __restrict__ counts_o, int* __restrict__ status_o) {
  __shared__ int s_cls[kRingMax];                                 // atom class, -1 = dropped
  __shared__ MolAdjRow s_adj[kRingMax];                           // kept bonds of an atom
  __shared__ MolAdjRow s_radj[kRingMax];                          // its ring bonds
  __shared__ unsigned int s_stat[kRingMax];                       // degree | bonds of order 4 << 16
  __shared__ unsigned int s_aring[kRingMax];                      // smallest ring_size among the atom's ring bonds, ~0 = none
  __shared__ int s_comp[kRingMax];                                // component label over all bonds (a local atom index)
  __shared__ int s_sys[kRingMax];                                 // ring-system label over ring bonds
  __shared__ unsigned int s_size[kRingMax];                       // atoms of the ring system whose label this index is

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;

  // ---- atoms: class; empty masks, counters and labels -------------------------------------------------------------------------
  int n_kept = 0;
#pragma unroll
  for (int c = 0; c < kRingCh; ++c) {
    const int i = c * 64 + lane;
    int k = -1;
    if (i < n) {
      s_cls[i] = k = mol_class(cls_i[arow + i]);
      s_stat[i] = 0u, s_size[i] = 0u;
      s_aring[i] = ~0u;
      s_comp[i] = s_sys[i] = i;
#pragma unroll
      for (int w = 0; w < kRingCh; ++w) s_adj[i].w[w] = s_radj[i].w[w] = 0ull;
    }
    n_kept += __popcll(__ballot(k >= 0));
  }
  __syncthreads();

  // ---- bonds ------------------------------------------------------------------------------------------------------------------
  int n_bond = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    if (mol_is_bond(o) && s_cls[a] >= 0 && s_cls[b] >= 0) {
      ++n_bond;
      const unsigned int inc = 1u | (o == 4 ? 1u << 16 : 0u);
      atomicAdd(&s_stat[a], inc);
      atomicAdd(&s_stat[b], inc);
      mol_adj_set(s_adj, a, b);
    }
  });
  __syncthreads();

  // ---- rings: the same deal; a lane searches the ring of each of its bonds and writes the row of every one of its pairs ------
  int n_ringb = 0, rmin = 255, rmax = 0, n_rot = 0, n_arom_out = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    int rs = 0;
    if (mol_is_bond(o) && s_cls[a] >= 0 && s_cls[b] >= 0) {
      rs = ring_through(s_adj, a, b);
      if (rs > 0) {
        ++n_ringb;
        rmin = min(rmin, rs);
        rmax = max(rmax, rs);
        mol_adj_set(s_radj, a, b);
        atomicMin(&s_aring[a], (unsigned int)rs);
        atomicMin(&s_aring[b], (unsigned int)rs);
      } else {
        n_rot += (o == 1 && (s_stat[a] & 0xffffu) >= 2u && (s_stat[b] & 0xffffu) >= 2u) ? 1 : 0;
        n_arom_out += o == 4 ? 1 : 0;
      }
    }
    ring_size_o[hrow + p] = (uint8_t)rs;
  });
  __syncthreads();

  // ---- components (all bonds) and ring systems (ring bonds): every atom takes the smallest label among itself and its neighbours,
  // then its label's label, until a wave-wide vote sees no change in either.  Labels only decrease and stay inside their class, so
  // reading a neighbour's label of either round is fine; at the fixed point a class holds one label, the index of its first atom. ----
  bool changed;
  do {
    changed = false;
#pragma unroll
    for (int c = 0; c < kRingCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && s_cls[i] >= 0) {
        const int c0 = s_comp[i], y0 = s_sys[i];
        int lc = c0, ly = y0;
        const MolAdjRow all = s_adj[i], ring = s_radj[i];
#pragma unroll
        for (int w = 0; w < kRingCh; ++w) {                         // (both rows are on their way before either is walked)
          for_each_bit(all.w[w], w * 64, [&](int j) { lc = min(lc, s_comp[j]); });
          for_each_bit(ring.w[w], w * 64, [&](int j) { ly = min(ly, s_sys[j]); });
        }
        lc = min(lc, s_comp[lc]);
        ly = min(ly, s_sys[ly]);
        if (lc < c0) s_comp[i] = lc;
        if (ly < y0) s_sys[i] = ly;
        changed |= lc < c0 || ly < y0;
      }
    }
    __syncthreads();
  } while (__any(changed));

  // ---- per-atom outputs, system sizes, counts --------------------------------------------------------------------------------
  int n_comp = 0, n_sys = 0, n_ringa = 0, n_lone = 0;
#pragma unroll
  for (int c = 0; c < kRingCh; ++c) {
    const int i = c * 64 + lane;
    bool comp_root = false, sys_root = false, in_ring = false, lone = false;
    if (i < n) {
      const bool kept = s_cls[i] >= 0;
      const unsigned int ar = s_aring[i];
      in_ring = kept && ar != ~0u;
      comp_root = kept && s_comp[i] == i;
      sys_root = in_ring && s_sys[i] == i;
      lone = kept && (s_stat[i] >> 16) == 1u;
      if (in_ring) atomicAdd(&s_size[s_sys[i]], 1u);
      atom_ring_o[arow + i] = (uint8_t)(in_ring ? ar : 0u);
      ring_sys_o[arow + i] = (int16_t)(in_ring ? s_sys[i] : -1);
    }
    n_comp += __popcll(__ballot(comp_root));
    n_sys += __popcll(__ballot(sys_root));
    n_ringa += __popcll(__ballot(in_ring));
    n_lone += __popcll(__ballot(lone));
  }
  __syncthreads();
  int largest = 0;
#pragma unroll
  for (int c = 0; c < kRingCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) largest = max(largest, (int)s_size[i]);
  }
  largest = wave_imax(largest);
  n_bond = wave_sum(n_bond);
  n_ringb = wave_sum(n_ringb);
  n_rot = wave_sum(n_rot);
  n_arom_out = wave_sum(n_arom_out);
  rmin = wave_imin(rmin);
  rmax = wave_imax(rmax);
  rmin = n_ringb > 0 ? rmin : 0;
  int st = 0;
  st |= n_arom_out > 0 ? PG_RING_AROMATIC_OUTSIDE : 0;
  st |= (rmin > 0 && rmin < lim.ring_min) ? PG_RING_SMALL : 0;
  st |= rmax > lim.ring_max ? PG_RING_LARGE : 0;
  st |= largest > lim.system_max ? PG_RING_SYSTEM_LARGE : 0;
  st |= n_rot > lim.rotatable_max ? PG_RING_ROTATABLE : 0;
  st |= n_lone > 0 ? PG_RING_AROMATIC_LONE : 0;
  if (lane == 0) {
    status_o[blockIdx.x] = st;
    int* cnt = counts_o + (size_t)blockIdx.x * PG_RING_N_COUNTS;
    cnt[0] = n_bond - n_kept + n_comp;
    cnt[1] = n_ringb;
    cnt[2] = n_ringa;
    cnt[3] = n_sys;
    cnt[4] = rmin;
    cnt[5] = rmax;
    cnt[6] = largest;
    cnt[7] = n_rot;
    cnt[8] = n_arom_out;
    cnt[9] = n_lone;
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_rings(const int8_t* cls, const int8_t* order, const int* g_lig_off, const int* g_bond_off, int B, int F,
                            int n_lig, int n_bond, int max_n, const int* limits, uint8_t* ring_size, uint8_t* atom_ring,
                            int16_t* ring_sys, int* counts, int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_rings", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (!limits) {
    set_error("pg_mol_rings: limits is null (four ints in host memory)");
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  const RingLimits lim = {limits[0], limits[1], limits[2], limits[3]};
  hipLaunchKernelGGL(mol_rings_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, lim, ring_size, atom_ring, ring_sys, counts, status);
  return check_launch("pg_mol_rings");
}
