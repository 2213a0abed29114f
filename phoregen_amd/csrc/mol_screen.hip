// From sampler output to molecules: decode, connectivity and valence screen of every (frame, graph) in one launch
// (pg_mol_screen, include/phoregen_hip.h; phoregen_amd/molecule.py).  One wave per (frame, graph) (mol_common.h).
// Integer work only (the scores are compared, never added), so every output is exact.
#include "mol_screen_core.h"

namespace pg {

__global__ __launch_bounds__(64) void mol_screen_kernel(
    const float* __restrict__ node_scores, long node_fs, const float* __restrict__ edge_scores, long edge_fs,
    const float* __restrict__ pos, long pos_fs, const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
    int n_lig, int n_half, const uint8_t* __restrict__ max_valence2, int* __restrict__ status, int* __restrict__ counts,
    int8_t* __restrict__ cls_o, int16_t* __restrict__ compact_o, uint8_t* __restrict__ val2_o, int16_t* __restrict__ comp_o,
    int8_t* __restrict__ order_o) {
  __shared__ MolScreenLds s;

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  const float* nrow = node_scores + (size_t)m.f * node_fs + (size_t)m.a0 * 12;
  const float* erow = edge_scores + (size_t)m.f * edge_fs + (size_t)m.h0 * 12;   // first half of the graph's rows, 6 floats each
  const float* prow = pos + (size_t)m.f * pos_fs + (size_t)m.a0 * 3;

  // ---- atoms: class, compact index, coordinates -------------------------------------------------------------------------------
  bool bad_pos = false, masked = false;
  const int n_kept = mol_screen_atoms(s, lane, n, nrow, arow, cls_o, compact_o, masked, [&](int i, int k) {
    if (k < 11) {
      const float* p = prow + (size_t)i * 3;
      bad_pos |= mol_nonfinite(p[0]) || mol_nonfinite(p[1]) || mol_nonfinite(p[2]);
    }
  });

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
    const bool bond = mol_is_bond(o) && s.cls[a] >= 0 && s.cls[b] >= 0;
    order_o[hrow + p] = (int8_t)(bond ? o : 0);
    if (bond) {
      ++n_bond;
      mol_screen_bond(s, a, b, o);
    }
  });
  __syncthreads();

  // ---- components, valence rule, counts, status (mol_screen_core.h) ------------------------------------------------------------
  mol_screen_finish(s, lane, n, arow, n_kept, n_bond, bad_pos, masked, absorbing ? PG_MOL_HAD_ABSORBING_BOND : 0, max_valence2, status,
                    counts, val2_o, comp_o);
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
