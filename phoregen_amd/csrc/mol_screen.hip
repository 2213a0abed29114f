// From sampler output to molecules: decode, connectivity and valence screen of every (frame, graph) in one launch
// (pg_mol_screen, include/phoregen_hip.h; phoregen_amd/molecule.py).  One wave per (frame, graph) (mol_common.h).
// Integer work only (the scores are compared, never added), so every output is exact.
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

__global__ __launch_bounds__(64) void mol_screen_kernel(
    const float* __restrict__ node_scores, long node_fs, const float* __restrict__ edge_scores, long edge_fs,
    const float* __restrict__ pos, long pos_fs, const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
    int n_lig, int n_half, const uint8_t* __restrict__ max_valence2, int* __restrict__ status, int* __restrict__ counts,
    int8_t* __restrict__ cls_o, int16_t* __restrict__ compact_o, uint8_t* __restrict__ val2_o, int16_t* __restrict__ comp_o,
    int8_t* __restrict__ order_o) {
  __shared__ int s_cls[kMolMax];                          // atom class, -1 = dropped
  __shared__ MolAdjRow s_adj[kMolMax];                    // kept bonds of an atom
  __shared__ unsigned int s_stat[kMolMax];                // valence2 | degree << 16 | aromatic bonds << 24
  __shared__ int s_label[kMolMax];                        // component label (a local atom index)
  __shared__ unsigned int s_size[kMolMax];                // atoms of the component whose label this index is

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  const float* nrow = node_scores + (size_t)m.f * node_fs + (size_t)m.a0 * 12;
  const float* erow = edge_scores + (size_t)m.f * edge_fs + (size_t)m.h0 * 12;   // first half of the graph's rows, 6 floats each
  const float* prow = pos + (size_t)m.f * pos_fs + (size_t)m.a0 * 3;

  // ---- atoms: class, compact index, coordinates -------------------------------------------------------------------------------
  int n_kept = 0;
  bool bad_pos = false, masked = false;
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
      s_cls[i] = keep ? k : -1;
      s_label[i] = keep ? i : -1;
      s_stat[i] = 0u, s_size[i] = 0u;
#pragma unroll
      for (int w = 0; w < kMolCh; ++w) s_adj[i].w[w] = 0ull;
      cls_o[arow + i] = (int8_t)(keep ? k : -1);
      compact_o[arow + i] = (int16_t)(keep ? compact : -1);
      if (keep) {
        const float* p = prow + (size_t)i * 3;
        bad_pos |= mol_nonfinite(p[0]) || mol_nonfinite(p[1]) || mol_nonfinite(p[2]);
      }
    }
  }
  __syncthreads();

  // ---- bonds ------------------------------------------------------------------------------------------------------------------
  int n_bond = 0;
  bool absorbing = false;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    float v[6];
    const float2* r = reinterpret_cast<const float2*>(erow + (size_t)p * 6);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float2 t = r[q];
      v[2 * q] = t.x, v[2 * q + 1] = t.y;
    }
    const int o = first_argmax<6>(v);
    absorbing |= o == 5;
    const bool bond = mol_is_bond(o) && s_cls[a] >= 0 && s_cls[b] >= 0;
    order_o[hrow + p] = (int8_t)(bond ? o : 0);
    if (bond) {
      ++n_bond;
      const unsigned int inc = (o == 4 ? 3u : 2u * o) | (1u << 16) | (o == 4 ? 1u << 24 : 0u);
      atomicAdd(&s_stat[a], inc);
      atomicAdd(&s_stat[b], inc);
      mol_adj_set(s_adj, a, b);
    }
  });
  __syncthreads();

  // ---- components: every atom takes the smallest label among itself and its neighbours, then its label's label; until a
  // wave-wide vote sees no change.  Labels only decrease and stay inside the component, so reading a neighbour's label of
  // either round is fine; at the fixed point a component holds one label, the index of its first atom. ------------------------
  MolAdjRow adj[kMolCh];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) adj[c].w[w] = (i < n && s_cls[i] >= 0) ? s_adj[i].w[w] : 0ull;
  }
  bool changed;
  do {
    changed = false;
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && s_cls[i] >= 0) {
        const int l0 = s_label[i];
        int l = l0;
        for_each_neighbour(adj[c], [&](int j) { l = min(l, s_label[j]); });
        l = min(l, s_label[l]);
        if (l < l0) {
          s_label[i] = l;
          changed = true;
        }
      }
    }
    __syncthreads();
  } while (__any(changed));

  // ---- per-atom outputs, valence rule, component sizes ----------------------------------------------------------------------
  int n_comp = 0;
  bool over = false;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    bool root = false;
    if (i < n) {
      const int k = s_cls[i];
      if (k >= 0) {
        const int l = s_label[i];
        const unsigned int st = s_stat[i], v2 = st & 0xffffu;
        atomicAdd(&s_size[l], 1u);
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
    if (i < n) largest = max(largest, (int)s_size[i]);
  }
  largest = wave_imax(largest);
  n_bond = wave_sum(n_bond);
  int st = 0;
  st |= n_kept == 0 ? PG_MOL_NO_ATOMS : 0;
  st |= n_comp > 1 ? PG_MOL_DISCONNECTED : 0;
  st |= __any(over) ? PG_MOL_VALENCE : 0;
  st |= __any(bad_pos) ? PG_MOL_NONFINITE : 0;
  st |= __any(masked) ? PG_MOL_HAD_MASKED_ATOM : 0;
  st |= __any(absorbing) ? PG_MOL_HAD_ABSORBING_BOND : 0;
  if (lane == 0) {
    status[blockIdx.x] = st;
    *reinterpret_cast<int4*>(counts + (size_t)blockIdx.x * 4) = make_int4(n_kept, n_bond, n_comp, largest);
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_screen(const float* node_scores, int64_t node_fs, const float* edge_scores, int64_t edge_fs, const float* pos,
                             int64_t pos_fs, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig, int n_bond,
                             int max_n, const uint8_t* max_valence2, int* status, int* counts, int8_t* cls, int16_t* compact,
                             uint8_t* valence2, int16_t* comp, int8_t* order, void* stream) {
  const int rc = mol_check_batch("pg_mol_screen", B, F, n_lig, n_bond, max_n);
  if (rc != PG_OK) return rc == kMolNothing ? PG_OK : rc;
  if (((uintptr_t)node_scores & 15) || (node_fs & 3) || ((uintptr_t)edge_scores & 7) || (edge_fs & 1) || ((uintptr_t)counts & 15)) {
    set_error("pg_mol_screen: node_scores / node_fs must be 16-byte, edge_scores / edge_fs 8-byte, counts 16-byte aligned");
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_screen_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, node_scores, (long)node_fs,
                     edge_scores, (long)edge_fs, pos, (long)pos_fs, g_lig_off, g_bond_off, B, n_lig, n_bond / 2, max_valence2,
                     status, counts, cls, compact, valence2, comp, order);
  return check_launch("pg_mol_screen");
}
