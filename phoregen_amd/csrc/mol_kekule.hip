// Kekulé form, hydrogens and charges of the molecules the screen decoded (pg_mol_kekule, include/phoregen_hip.h;
// phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Kekulé form").  Reads the screen's outputs (cls, order), not the scores.  One
// wave per (frame, graph) (mol_common.h).  The wave deals the pairs, builds the aromatic adjacency, classifies the atoms, computes
// the per-atom results and the counts and writes kekule_order; the matching itself (Edmonds' algorithm with blossom contraction,
// kekule_core.h) runs on lane 0 over arrays in LDS.  Integer work only, no floating point anywhere, so every output is exact.
#include "mol_common.h"
#include "wave_prims.h"
#include "kekule_core.h"

namespace pg {

constexpr int kKekMax = kMolMax, kKekCh = kMolCh;
constexpr int kKekEl = 11;                  // elements (atom classes 0..10)
constexpr int kKekN = 2;                    // the class of N
constexpr int kKekO = 3;                    // the class of O

struct KekuleTables {
  uint8_t dbl_neutral[kKekEl], dbl_charged[kKekEl], must[kKekEl], hval[kKekEl][4];
};

__global__ __launch_bounds__(64) void mol_kekule_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                        const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
                                                        int n_lig, int n_half, const uint8_t* __restrict__ t_neutral,
                                                        const uint8_t* __restrict__ t_charged, const uint8_t* __restrict__ t_must,
                                                        const uint8_t* __restrict__ t_hval, int allow_charged,
                                                        int8_t* __restrict__ kek_o, uint8_t* __restrict__ hcount_o,
                                                        int8_t* __restrict__ charge_o, int* __restrict__ counts_o,
                                                        int* __restrict__ status_o) {
  __shared__ int s_cls[kKekMax];                                  // atom class, -1 = dropped
  __shared__ unsigned int s_sa[kKekMax];                          // s | a << 16
  __shared__ MolAdjRow s_arom[kKekMax];                           // bonds of order 4 of an atom
  __shared__ MolAdjRow s_allow[kKekMax];                          // the pass's allowed graph
  __shared__ uint8_t s_kind[kKekMax];
  __shared__ int16_t s_match[2 * kKekMax], s_parent[2 * kKekMax], s_base[kKekMax], s_queue[kKekMax];
  __shared__ uint8_t s_flags[kKekMax];
  __shared__ KekuleTables s_tab;
  __shared__ int s_feasible;

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;

  // ---- tables and atoms ------------------------------------------------------------------------------------------------------
  if (lane < kKekEl) {
    s_tab.dbl_neutral[lane] = t_neutral[lane];
    s_tab.dbl_charged[lane] = t_charged[lane];
    s_tab.must[lane] = t_must[lane];
  }
  if (lane < kKekEl * 4) s_tab.hval[lane >> 2][lane & 3] = t_hval[lane];
  int n_kept = 0;
#pragma unroll
  for (int c = 0; c < kKekCh; ++c) {
    const int i = c * 64 + lane;
    int k = -1;
    if (i < n) {
      s_cls[i] = k = mol_class(cls_i[arow + i]);
      s_sa[i] = 0u;
#pragma unroll
      for (int w = 0; w < kKekCh; ++w) s_arom[i].w[w] = 0ull;
    }
    n_kept += __popcll(__ballot(k >= 0));
  }
  __syncthreads();

  // ---- bonds ------------------------------------------------------------------------------------------------------------------
  int n_arom_bond = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    if (mol_is_bond(o) && s_cls[a] >= 0 && s_cls[b] >= 0) {
      const unsigned int inc = o == 4 ? 1u << 16 : (unsigned int)o;
      atomicAdd(&s_sa[a], inc);
      atomicAdd(&s_sa[b], inc);
      if (o == 4) {
        ++n_arom_bond;
        mol_adj_set(s_arom, a, b);
      }
    }
  });
  __syncthreads();

  // ---- the passes: classify, restrict the aromatic graph to the atoms that may carry a double bond, match ---------------------
  int feasible = 1, pass_used = 0, n_arom = 0, n_must = 0;
  for (int pass = 0; pass < 2; ++pass) {
    unsigned long long ok[kKekCh];
    n_arom = n_must = 0;
#pragma unroll
    for (int c = 0; c < kKekCh; ++c) {
      const int i = c * 64 + lane;
      int kind = kKekNone;
      if (i < n && s_cls[i] >= 0) {
        const int el = s_cls[i];
        const unsigned int sa = s_sa[i];
        const int neutral = s_tab.dbl_neutral[el];
        const int cap = pass == 0 ? neutral : max(neutral, (int)s_tab.dbl_charged[el]);
        kind = kekule_kind((int)(sa & 0xffffu), (int)(sa >> 16), cap, s_tab.must[el]);
      }
      if (i < n) s_kind[i] = (uint8_t)kind;
      ok[c] = __ballot(kind >= kKekMay);
      n_arom += __popcll(__ballot(kind != kKekNone));
      n_must += __popcll(__ballot(kind == kKekMust));
    }
#pragma unroll
    for (int c = 0; c < kKekCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n) {
        const bool in = (ok[c] >> lane) & 1ull;
#pragma unroll
        for (int w = 0; w < kKekCh; ++w) s_allow[i].w[w] = in ? s_arom[i].w[w] & ok[w] : 0ull;
      }
    }
    for (int i = lane; i < 2 * n; i += 64) s_match[i] = -1;
    __syncthreads();
    if (lane == 0) s_feasible = (ok[0] | ok[1]) == 0ull ? (n_must == 0) : kekule_match(n, mol_adj_words(s_allow), s_kind, s_match, s_parent, s_base, s_queue, s_flags);
    __syncthreads();
    feasible = s_feasible;
    pass_used = pass;
    __syncthreads();                                              // (s_feasible and s_kind are rewritten by the next pass)
    if (feasible || !allow_charged) break;
  }

  // ---- per-atom results and the counts -----------------------------------------------------------------------------------------
  int n_dbl2 = 0, n_may = 0, n_h = 0, n_q = 0, n_hbd = 0, n_hba = 0;
#pragma unroll
  for (int c = 0; c < kKekCh; ++c) {
    const int i = c * 64 + lane;
    int h = 0, q = 0, d = 0, el = -1;
    if (i < n && s_cls[i] >= 0) {
      el = s_cls[i];
      const unsigned int sa = s_sa[i];
      d = (feasible && s_match[i] >= 0) ? 1 : 0;
      kekule_atom(el == kKekN, (int)(sa & 0xffffu), (int)(sa >> 16), d, s_tab.dbl_neutral[el], s_tab.hval[el], &h, &q);
    }
    if (i < n) {
      hcount_o[arow + i] = (uint8_t)h;
      charge_o[arow + i] = (int8_t)q;
    }
    const bool no = el == kKekN || el == kKekO;
    n_dbl2 += __popcll(__ballot(d == 1));
    n_may += __popcll(__ballot(d == 1 && s_kind[min(i, kKekMax - 1)] == kKekMay));
    n_hbd += __popcll(__ballot(no && h >= 1));
    n_hba += __popcll(__ballot(no));
    n_h += h;
    n_q += q;
  }
  n_h = wave_sum(n_h);
  n_q = wave_sum(n_q);
  n_arom_bond = wave_sum(n_arom_bond);

  // ---- kekule_order: the same deal of the pairs ----------------------------------------------------------------------------------
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    int o = order_i[hrow + p];
    if (feasible && o == 4 && s_cls[a] >= 0 && s_cls[b] >= 0) o = s_match[a] == b ? 2 : 1;
    kek_o[hrow + p] = (int8_t)o;
  });

  if (lane == 0) {
    int st = 0;
    st |= feasible ? 0 : PG_KEKULE_FAILED;
    st |= (feasible && pass_used == 1) ? PG_KEKULE_CHARGED : 0;
    st |= n_arom > 0 ? PG_KEKULE_HAS_AROMATIC : 0;
    st |= n_q != 0 ? PG_KEKULE_CATION : 0;
    status_o[blockIdx.x] = st;
    int* cnt = counts_o + (size_t)blockIdx.x * PG_KEKULE_N_COUNTS;
    cnt[0] = n_arom;
    cnt[1] = n_arom_bond;
    cnt[2] = n_dbl2 >> 1;
    cnt[3] = n_must;
    cnt[4] = n_may;
    cnt[5] = n_h;
    cnt[6] = n_q;
    cnt[7] = n_hbd;
    cnt[8] = n_hba;
    cnt[9] = n_kept;
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_kekule(const int8_t* cls, const int8_t* order, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig,
                             int n_bond, int max_n, const uint8_t* dbl_neutral, const uint8_t* dbl_charged, const uint8_t* must,
                             const uint8_t* h_valences, int allow_charged, int8_t* kekule_order, uint8_t* hcount, int8_t* charge,
                             int* counts, int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_kekule", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (!dbl_neutral || !dbl_charged || !must || !h_valences) {
    set_error("pg_mol_kekule: a table is null (dbl_neutral, dbl_charged, must: uint8 [11]; h_valences: uint8 [11][4], device memory)");
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  hipLaunchKernelGGL(mol_kekule_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, dbl_neutral, dbl_charged, must, h_valences, allow_charged, kekule_order, hcount, charge, counts,
                     status);
  return check_launch("pg_mol_kekule");
}
