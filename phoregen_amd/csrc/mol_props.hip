// Property descriptors and drug-likeness limits of the molecules the screen decoded (pg_mol_props, include/phoregen_hip.h;
// phoregen_amd/properties.py; definition: DESIGN.md 2.9 "Properties").  Reads the screen's outputs (cls, order), the Kekulé form
// (kekule_order, hcount, charge, status) and the rings' ring_size and atom_ring; no coordinates.  One wave per (frame, graph)
// (mol_common.h); the divergent loops below (pair rows, an atom's neighbours, the rows of a table) hold no barrier or vote.  Integer
// work only (props_core.h): every result is exact, and the graph's totals are integer wave sums, so no order of the atoms moves them.
#include "mol_common.h"
#include "wave_prims.h"
#include "props_core.h"

namespace pg {

constexpr int kPropPairs = kMolMax * (kMolMax - 1) / 2;
constexpr int kPropTableInts = PG_PROP_MAX_TABLES * PG_PROP_MAX_ROWS * PG_PROP_ROW_INTS;
static_assert(PG_PROP_MAX_ROWS <= 255, "a row index fits a byte next to 255 = none");

// what the launch hands over by value: the tables' row counts and the limits
struct PropArgs {
  int n_tables, max_violations;
  int rows[PG_PROP_MAX_TABLES];
  int lim[2 * PG_PROP_N_LIMITS];
};

__global__ __launch_bounds__(64) void mol_props_kernel(
    const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i, const int8_t* __restrict__ kek_i,
    const uint8_t* __restrict__ hcount_i, const int8_t* __restrict__ charge_i, const int* __restrict__ kek_status,
    const uint8_t* __restrict__ ring_size_i, const uint8_t* __restrict__ atom_ring_i, const int* __restrict__ g_lig_off,
    const int* __restrict__ g_bond_off, int B, int n_lig, int n_half, const int* __restrict__ tables, const int* __restrict__ weights,
    const PropArgs args, int* __restrict__ atom_env, uint8_t* __restrict__ atom_row, int* __restrict__ sums_o, int* __restrict__ counts_o,
    int* __restrict__ weight_o, int* __restrict__ violated_o, int* __restrict__ status_o) {
  __shared__ MolAdjRow s_adj[kMolMax];                               // kept bonds of an atom
  __shared__ uint8_t s_pair[kPropPairs];                             // props_core.h's byte per pair row
  __shared__ int s_tab[kPropTableInts];                              // the tables' rows, one table after the other
  __shared__ int s_env[kMolMax];
  __shared__ int s_w[PG_PROP_N_WEIGHTS];
  __shared__ int8_t s_el[kMolMax], s_q[kMolMax];
  __shared__ uint8_t s_h[kMolMax], s_aring[kMolMax];

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  const bool kek_ok = (kek_status[blockIdx.x] & PG_KEKULE_FAILED) == 0;

  // ---- the tables and the weights, once per block (the host wrapper bounds n_tables and every row count) ----------------------------
  int t_off[PG_PROP_MAX_TABLES], n_rows_all = 0;
#pragma unroll
  for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) {
    t_off[t] = n_rows_all * PG_PROP_ROW_INTS;
    n_rows_all += t < args.n_tables ? min(max(args.rows[t], 0), PG_PROP_MAX_ROWS) : 0;
  }
  for (int k = lane; k < n_rows_all * PG_PROP_ROW_INTS; k += 64) s_tab[k] = tables[k];
  if (lane < PG_PROP_N_WEIGHTS) s_w[lane] = weights[lane];

  // ---- atoms: class, hydrogens, charge, ring membership; empty masks --------------------------------------------------------------
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      const int k = mol_class(cls_i[arow + i]);
      s_el[i] = (int8_t)k;
      s_h[i] = k >= 0 ? hcount_i[arow + i] : (uint8_t)0;
      s_q[i] = k >= 0 ? charge_i[arow + i] : (int8_t)0;
      s_aring[i] = k >= 0 ? atom_ring_i[arow + i] : (uint8_t)0;
      s_env[i] = -1;
#pragma unroll
      for (int w = 0; w < kMolCh; ++w) s_adj[i].w[w] = 0ull;
    }
  }
  __syncthreads();

  int cnt[PG_PROP_N_COUNTS], sum[PG_PROP_MAX_TABLES], weight = 0;
#pragma unroll
  for (int k = 0; k < PG_PROP_N_COUNTS; ++k) cnt[k] = 0;
#pragma unroll
  for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) sum[t] = 0;
  int env[kMolCh];
  uint8_t row[kMolCh][PG_PROP_MAX_TABLES];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    env[c] = -1;
#pragma unroll
    for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) row[c][t] = 255;
  }

  if (kek_ok) {                                                      // (wave-uniform: one status word per block)
    // ---- bonds ------------------------------------------------------------------------------------------------------------------
    for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
      const int o = order_i[hrow + p];
      int pb = 0;
      if (mol_is_bond(o) && s_el[a] >= 0 && s_el[b] >= 0) {
        pb = prop_pair_byte(o, kek_i[hrow + p], ring_size_i[hrow + p]);
        mol_adj_set(s_adj, a, b);
      }
      s_pair[p] = (uint8_t)pb;
    });
    __syncthreads();

    const PropGraph pg = {n, s_el, s_h, s_q, s_aring, mol_adj_words(s_adj), s_pair, s_env};
    // ---- the word's first pass; then the two fields that read every neighbour's flags -----------------------------------------------
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n) s_env[i] = env[c] = prop_env_own(pg, i);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && env[c] >= 0) env[c] |= prop_env_nbr(pg, i);
    }
    __syncthreads();                                                 // (every read of the first pass's words is done before they are rewritten)
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n) s_env[i] = env[c];
    }
    __syncthreads();

    // ---- per atom: the counts, the weight and the row of every table ---------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && env[c] >= 0) {
        const int h = s_h[i];
        prop_atom_counts(env[c], h, s_q[i], cnt);
        weight += s_w[prop_el(env[c])] + h * s_w[PG_PROP_N_WEIGHTS - 1];
#pragma unroll
        for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) {
          if (t < args.n_tables) {
            const int r = prop_match(s_tab + t_off[t], args.rows[t], env[c]);
            if (r >= 0) {
              sum[t] += prop_contribution(s_tab + t_off[t] + PG_PROP_ROW_INTS * r, h);
              row[c][t] = (uint8_t)r;
            } else {
              ++cnt[PG_PROP_C_UNTYPED];
            }
          }
        }
      }
    }
    // ---- per bond: rotatable and amide bonds ---------------------------------------------------------------------------------------
    for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
      const int pb = s_pair[p];
      if (pb & kPropBond) {
        const int kind = prop_bond_kind(pb, s_env[a], s_env[b]);
        cnt[PG_PROP_C_ROTATABLE] += kind == 1;
        cnt[PG_PROP_C_AMIDE_BONDS] += kind == 2;
      }
    });
  }

  // ---- per-atom outputs (its own lane computed them) -----------------------------------------------------------------------------------
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      atom_env[arow + i] = env[c];
#pragma unroll
      for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) atom_row[((size_t)m.f * PG_PROP_MAX_TABLES + t) * n_lig + m.a0 + i] = row[c][t];
    }
  }

  // ---- the wave's totals (all lanes are back together here), then lane 0 writes the graph's rows ------------------------------------
#pragma unroll
  for (int k = 0; k < PG_PROP_N_COUNTS; ++k) cnt[k] = wave_sum(cnt[k]);
#pragma unroll
  for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) sum[t] = wave_sum(sum[t]);
  weight = wave_sum(weight);
  if (lane != 0) return;
  int viol = 0;
  if (kek_ok) {
    int v[PG_PROP_N_LIMITS];
    v[PG_PROP_L_WEIGHT] = weight, v[PG_PROP_L_HEAVY_ATOMS] = cnt[PG_PROP_C_HEAVY_ATOMS], v[PG_PROP_L_NHOH] = cnt[PG_PROP_C_NHOH];
    v[PG_PROP_L_NO_COUNT] = cnt[PG_PROP_C_NO_COUNT], v[PG_PROP_L_ROTATABLE] = cnt[PG_PROP_C_ROTATABLE];
#pragma unroll
    for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) v[PG_PROP_L_SUM0 + t] = sum[t];
    viol = prop_violated(v, args.lim);
    cnt[PG_PROP_C_VIOLATIONS] = prop_popc((unsigned int)viol);
  }
  int* crow = counts_o + (size_t)blockIdx.x * PG_PROP_N_COUNTS;
#pragma unroll
  for (int k = 0; k < PG_PROP_N_COUNTS; ++k) crow[k] = cnt[k];
#pragma unroll
  for (int t = 0; t < PG_PROP_MAX_TABLES; ++t) sums_o[(size_t)blockIdx.x * PG_PROP_MAX_TABLES + t] = sum[t];
  weight_o[blockIdx.x] = weight;
  violated_o[blockIdx.x] = viol;
  status_o[blockIdx.x] = prop_status(kek_ok, viol, args.max_violations, cnt[PG_PROP_C_UNTYPED]);
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_props(const int8_t* cls, const int8_t* order, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                            const int* kekule_status, const uint8_t* ring_size, const uint8_t* atom_ring, const int* g_lig_off,
                            const int* g_bond_off, int B, int F, int n_lig, int n_bond, int max_n, const int* tables, const int* table_rows,
                            int n_tables, const int* weights, const int* limits, int max_violations, int* atom_env, uint8_t* atom_row,
                            int* sums, int* counts, int* weight_milli, int* violated, int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_props", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (n_tables < 0 || n_tables > PG_PROP_MAX_TABLES || (n_tables > 0 && !table_rows)) {
    set_error("pg_mol_props: %d tables, at most PG_PROP_MAX_TABLES = %d go in one call (table_rows is a host array)", n_tables,
              PG_PROP_MAX_TABLES);
    return PG_ERR_ARG;
  }
  PropArgs args = {};
  args.n_tables = n_tables, args.max_violations = max_violations;
  int n_rows_all = 0;
  for (int t = 0; t < n_tables; ++t) {
    if (table_rows[t] < 0 || table_rows[t] > PG_PROP_MAX_ROWS) {
      set_error("pg_mol_props: table %d has %d rows, a table holds at most PG_PROP_MAX_ROWS = %d", t, table_rows[t], PG_PROP_MAX_ROWS);
      return PG_ERR_ARG;
    }
    args.rows[t] = table_rows[t];
    n_rows_all += table_rows[t];
  }
  if (max_violations < 0 || !limits) {
    set_error("pg_mol_props: max_violations %d, limits %s (a host array of PG_PROP_N_LIMITS = %d lo / hi pairs)", max_violations,
              limits ? "given" : "null", PG_PROP_N_LIMITS);
    return PG_ERR_ARG;
  }
  for (int k = 0; k < 2 * PG_PROP_N_LIMITS; ++k) args.lim[k] = limits[k];
  if (rc == kMolNothing) return PG_OK;
  if (!cls || !order || !kekule_order || !hcount || !charge || !kekule_status || !ring_size || !atom_ring || !g_lig_off || !g_bond_off ||
      !weights || (n_rows_all > 0 && !tables) || !atom_env || !atom_row || !sums || !counts || !weight_milli || !violated || !status) {
    set_error("pg_mol_props: an array is null (the screen's cls / order, the Kekulé form's kekule_order / hcount / charge / status, "
              "ring_size, atom_ring, the offsets, the tables, the weights and the outputs are all device memory)");
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_props_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, kekule_order, hcount, charge,
                     kekule_status, ring_size, atom_ring, g_lig_off, g_bond_off, B, n_lig, n_bond / 2, tables, weights, args, atom_env,
                     atom_row, sums, counts, weight_milli, violated, status);
  return check_launch("pg_mol_props");
}
