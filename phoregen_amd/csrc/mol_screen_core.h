// The phases of the molecule screen that do not depend on where a pair's bond order comes from: the atoms (class, compact index),
// a bond's bookkeeping, and everything after the bonds (components, valence rule, counts, status).  mol_screen.hip takes the order of
// a pair from the argmax of its edge scores, mol_screen_dist.hip from the distance of its two atoms; both write the same outputs.
// One wave per (frame, graph) (mol_common.h).  Integer work only.
#pragma once
#include "mol_common.h"
#include "wave_prims.h"

namespace pg {

static_assert(kMolMax <= 256, "per-atom counters below hold a degree in 8 bits");

// torch.argmax: first maximum, a NaN counts as the largest
template <int K>
__device__ __forceinline__ int first_argmax(const float* v) {
  int best = 0;
  float bv = v[0];
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const bool up = v[k] > bv || (v[k] != v[k] && bv == bv);
    best = up ? k : best;
    bv = up ? v[k] : bv;
  }
  return best;
}

// the LDS arrays of one graph
struct MolScreenLds {
  int cls[kMolMax];                                       // atom class, -1 = dropped
  MolAdjRow adj[kMolMax];                                 // kept bonds of an atom
  unsigned int stat[kMolMax];                             // valence2 | degree << 16 | aromatic bonds << 24
  int label[kMolMax];                                     // component label (a local atom index)
  unsigned int size[kMolMax];                             // atoms of the component whose label this index is
};

// ---- atoms: class = argmax of the 12 scores at nrow, compact index; writes cls_o / compact_o and clears the graph's LDS rows.
// each(i, k) is called for every atom i < n with its argmax k (kept iff k < 11).  Ends with a barrier.  Returns the kept atoms;
// masked: the lane saw an atom of class 11.
template <class Each>
__device__ __forceinline__ int mol_screen_atoms(MolScreenLds& s, int lane, int n, const float* nrow, size_t arow, int8_t* cls_o,
                                                int16_t* compact_o, bool& masked, Each&& each) {
  int n_kept = 0;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    int k = 11;
    if (i < n) {
      float v[12];
      const float4* r = reinterpret_cast<const float4*>(nrow + (size_t)i * 12);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float4 t = r[q];
        v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
      }
      k = first_argmax<12>(v);
      masked |= k == 11;
    }
    const bool keep = k < 11;
    const unsigned long long km = __ballot(keep);
    const int compact = n_kept + __popcll(km & ((1ull << lane) - 1ull));
    n_kept += __popcll(km);
    if (i < n) {
      s.cls[i] = keep ? k : -1;
      s.label[i] = keep ? i : -1;
      s.stat[i] = 0u, s.size[i] = 0u;
#pragma unroll
      for (int w = 0; w < kMolCh; ++w) s.adj[i].w[w] = 0ull;
      cls_o[arow + i] = (int8_t)(keep ? k : -1);
      compact_o[arow + i] = (int16_t)(keep ? compact : -1);
      each(i, k);
    }
  }
  __syncthreads();
  return n_kept;
}

// the kept bond a - b of order o (1..4), from any lane (LDS atomics)
__device__ __forceinline__ void mol_screen_bond(MolScreenLds& s, int a, int b, int o) {
  const unsigned int inc = (o == 4 ? 3u : 2u * o) | (1u << 16) | (o == 4 ? 1u << 24 : 0u);
  atomicAdd(&s.stat[a], inc);
  atomicAdd(&s.stat[b], inc);
  mol_adj_set(s.adj, a, b);
}

// ---- everything after the bonds (a barrier lies between the last mol_screen_bond and this call): components, per-atom outputs,
// valence rule, counts, status.  n_bond: the lane's kept bonds; info: the lane's further status bits (any lane's bit is set).
__device__ __forceinline__ void mol_screen_finish(MolScreenLds& s, int lane, int n, size_t arow, int n_kept, int n_bond, bool bad_pos,
                                                  bool masked, int info, const uint8_t* __restrict__ max_valence2,
                                                  int* __restrict__ status, int* __restrict__ counts, uint8_t* __restrict__ val2_o,
                                                  int16_t* __restrict__ comp_o) {
  // components: every atom takes the smallest label among itself and its neighbours, then its label's label; until a wave-wide
  // vote sees no change.  Labels only decrease and stay inside the component, so reading a neighbour's label of either round is
  // fine; at the fixed point a component holds one label, the index of its first atom.
  MolAdjRow adj[kMolCh];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) adj[c].w[w] = (i < n && s.cls[i] >= 0) ? s.adj[i].w[w] : 0ull;
  }
  bool changed;
  do {
    changed = false;
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && s.cls[i] >= 0) {
        const int l0 = s.label[i];
        int l = l0;
        for_each_neighbour(adj[c], [&](int j) { l = min(l, s.label[j]); });
        l = min(l, s.label[l]);
        if (l < l0) {
          s.label[i] = l;
          changed = true;
        }
      }
    }
    __syncthreads();
  } while (__any(changed));

  // per-atom outputs, valence rule, component sizes
  int n_comp = 0;
  bool over = false;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    bool root = false;
    if (i < n) {
      const int k = s.cls[i];
      if (k >= 0) {
        const int l = s.label[i];
        const unsigned int st = s.stat[i], v2 = st & 0xffffu;
        atomicAdd(&s.size[l], 1u);
        root = l == i;
        over |= v2 > (unsigned int)max_valence2[k] + ((st >> 24) ? 1u : 0u);
        val2_o[arow + i] = (uint8_t)min(v2, 255u);
        comp_o[arow + i] = (int16_t)l;
      } else {
        val2_o[arow + i] = 0;
        comp_o[arow + i] = -1;
      }
    }
    n_comp += __popcll(__ballot(root));
  }
  __syncthreads();
  int largest = 0;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) largest = max(largest, (int)s.size[i]);
  }
  largest = wave_imax(largest);
  n_bond = wave_sum(n_bond);
  int st = 0;
  st |= n_kept == 0 ? PG_MOL_NO_ATOMS : 0;
  st |= n_comp > 1 ? PG_MOL_DISCONNECTED : 0;
  st |= __any(over) ? PG_MOL_VALENCE : 0;
  st |= __any(bad_pos) ? PG_MOL_NONFINITE : 0;
  st |= __any(masked) ? PG_MOL_HAD_MASKED_ATOM : 0;
  st |= __any((info & PG_MOL_HAD_ABSORBING_BOND) != 0) ? PG_MOL_HAD_ABSORBING_BOND : 0;
  st |= __any((info & PG_MOL_DIST_UNMAPPED_ELEMENT) != 0) ? PG_MOL_DIST_UNMAPPED_ELEMENT : 0;
  if (lane == 0) {
    status[blockIdx.x] = st;
    *reinterpret_cast<int4*>(counts + (size_t)blockIdx.x * 4) = make_int4(n_kept, n_bond, n_comp, largest);
  }
}

}  // namespace pg
