// Murcko scaffold of the molecules the screen decoded, written as the arrays of a screen of its own, so that every analysis that takes
// a screen works on scaffolds unchanged (pg_mol_scaffold, include/phoregen_hip.h; phoregen_amd/scaffold.py; definition: DESIGN.md 2.9
// "Scaffolds").  Reads the screen's outputs (cls, order), not the scores.  One wave per (frame, graph) (mol_common.h).  The sets of
// atoms (kept, core, scaffold) are two mask words that every lane holds, made by wave-wide votes: the pruning loop's trip count is
// wave-uniform.  The divergent loops (pair rows, the search of a bond's ring) hold no barrier or vote.  The selection rules are
// scaffold_core.h's, the ring search is ring_search.h's.  Integer work only, so every output is exact.
#include "ring_search.h"
#include "scaffold_core.h"
#include "wave_prims.h"

namespace pg {

static_assert(kScafWords == kMolCh, "a set of atoms has one word per adjacency word");

__global__ __launch_bounds__(64) void mol_scaffold_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                          const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
                                                          int n_lig, int n_half, int flags, uint8_t* __restrict__ part_o,
                                                          int* __restrict__ counts_o, int* __restrict__ status_o,
                                                          int* __restrict__ scounts_o, int8_t* __restrict__ cls_o,
                                                          int16_t* __restrict__ compact_o, uint8_t* __restrict__ val2_o,
                                                          int16_t* __restrict__ comp_o, int8_t* __restrict__ order_o) {
  __shared__ MolAdjRow s_adj[kMolMax];                            // kept bonds of an atom
  __shared__ MolAdjRow s_dbl[kMolMax];                            // those of order exactly 2
  __shared__ MolAdjRow s_radj[kMolMax];                           // the ring bonds of the core
  __shared__ unsigned int s_val[kMolMax];                         // twice the valence over scaffold bonds
  __shared__ int s_comp[kMolMax];                                 // scaffold component label (a local atom index)
  __shared__ int s_sys[kMolMax];                                  // ring-system label over ring bonds
  __shared__ unsigned int s_size[kMolMax];                        // atoms of the component whose label this index is

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;

  // ---- atoms: class, the set of kept atoms; empty masks, counters and labels --------------------------------------------------
  int cls[kMolCh];
  unsigned long long kept[kMolCh];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    cls[c] = -1;
    if (i < n) {
      cls[c] = mol_class(cls_i[arow + i]);
      s_val[i] = 0u, s_size[i] = 0u;
      s_comp[i] = s_sys[i] = i;
#pragma unroll
      for (int w = 0; w < kMolCh; ++w) s_adj[i].w[w] = s_dbl[i].w[w] = s_radj[i].w[w] = 0ull;
    }
    kept[c] = __ballot(cls[c] >= 0);
  }
  __syncthreads();

  // ---- bonds ------------------------------------------------------------------------------------------------------------------
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    if (mol_is_bond(o) && scaf_has(kept, a) && scaf_has(kept, b)) {
      mol_adj_set(s_adj, a, b);
      if (o == 2) mol_adj_set(s_dbl, a, b);
    }
  });
  __syncthreads();

  // ---- core: rounds of leaf removal until a round removes nothing (at most n / 2 rounds for a chain, n - 3 for a tail on a ring).
  // `core` is the same in every lane, so every lane leaves the loop in the same round. -------------------------------------------
  MolAdjRow row[kMolCh];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) row[c].w[w] = i < n ? s_adj[i].w[w] : 0ull;
  }
  unsigned long long core[kMolCh];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) core[c] = kept[c];
  for (int round = 0; round < kMolMax; ++round) {                 // (the bound is never reached: a round that removes takes an atom)
    unsigned long long leaf[kMolCh];
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) leaf[c] = __ballot(scaf_is_leaf(row[c].w, core, c * 64 + lane));
    unsigned long long any = 0ull;
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      core[c] &= ~leaf[c];
      any |= leaf[c];
    }
    if (any == 0ull) break;
  }

  // ---- ring bonds of the core: a lane searches the ring of each of its core bonds; a bond outside the core is a bridge ----------
  int n_linkb = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    if (mol_is_bond(o) && scaf_has(core, a) && scaf_has(core, b)) {
      if (ring_through(s_adj, a, b) > 0)
        mol_adj_set(s_radj, a, b);
      else
        ++n_linkb;
    }
  });
  __syncthreads();

  // ---- parts, the set of scaffold atoms, per-atom outputs -------------------------------------------------------------------------
  MolAdjRow ring[kMolCh];
  unsigned long long ringm[kMolCh], exom[kMolCh], sel[kMolCh];
  int part[kMolCh];
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    MolAdjRow dbl;
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) ring[c].w[w] = i < n ? s_radj[i].w[w] : 0ull, dbl.w[w] = i < n ? s_dbl[i].w[w] : 0ull;
    const bool k = cls[c] >= 0, in_core = scaf_has(core, i);
    const bool exo = (flags & PG_SCAF_EXOCYCLIC) && scaf_is_exocyclic(dbl.w, core, k, in_core);
    part[c] = scaf_part(k, in_core, ring[c].w, exo);
    ringm[c] = __ballot(part[c] == PG_SCAF_PART_RING);
    exom[c] = __ballot(exo);
    sel[c] = core[c] | exom[c];
  }
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      const bool in = scaf_has(sel, i);
      part_o[arow + i] = (uint8_t)part[c];
      cls_o[arow + i] = (int8_t)(in ? scaf_class(cls[c], flags) : -1);
      compact_o[arow + i] = (int16_t)(in ? scaf_compact(sel, i) : -1);
    }
  }

  // ---- scaffold bonds: the order of every pair row, the valence of the scaffold atoms -----------------------------------------------
  int n_sbond = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    int so = 0;
    if (mol_is_bond(o) && scaf_has(sel, a) && scaf_has(sel, b)) {
      so = scaf_order(o, flags);
      ++n_sbond;
      const unsigned int v = scaf_valence2(so);
      atomicAdd(&s_val[a], v);
      atomicAdd(&s_val[b], v);
    }
    order_o[hrow + p] = (int8_t)so;
  });

  // ---- scaffold components (scaffold bonds = an atom's bonds inside the set) and ring systems (ring bonds), as mol_rings.hip's:
  // a label step per atom and round until a wave-wide vote sees no change in either -------------------------------------------------
  const unsigned long long all[kMolCh] = {~0ull, ~0ull};
  bool changed;
  do {
    changed = false;
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && scaf_has(sel, i)) {
        const int c0 = s_comp[i], y0 = s_sys[i];
        const int lc = scaf_min_label(row[c].w, sel, s_comp, c0), ly = scaf_min_label(ring[c].w, all, s_sys, y0);
        if (lc < c0) s_comp[i] = lc;
        if (ly < y0) s_sys[i] = ly;
        changed |= lc < c0 || ly < y0;
      }
    }
    __syncthreads();
  } while (__any(changed));

  // ---- per-atom outputs, component sizes, counts, status ---------------------------------------------------------------------------
  int n_comp = 0, n_sys = 0;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    bool comp_root = false, sys_root = false;
    if (i < n) {
      const bool in = scaf_has(sel, i);
      if (in) atomicAdd(&s_size[s_comp[i]], 1u);
      comp_root = in && s_comp[i] == i;
      sys_root = part[c] == PG_SCAF_PART_RING && s_sys[i] == i;
      val2_o[arow + i] = (uint8_t)(in ? min(s_val[i], 255u) : 0u);
      comp_o[arow + i] = (int16_t)(in ? s_comp[i] : -1);
    }
    n_comp += __popcll(__ballot(comp_root));
    n_sys += __popcll(__ballot(sys_root));
  }
  __syncthreads();
  int largest = 0;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) largest = max(largest, (int)s_size[i]);
  }
  largest = wave_imax(largest);
  n_sbond = wave_sum(n_sbond);
  n_linkb = wave_sum(n_linkb);
  const int n_sel = scaf_count(sel), n_ring = scaf_count(ringm), n_exo = scaf_count(exom);
  if (lane == 0) {
    status_o[blockIdx.x] = (n_sel == 0 ? PG_MOL_NO_ATOMS : 0) | (n_comp > 1 ? PG_MOL_DISCONNECTED : 0);
    int* sc = scounts_o + (size_t)blockIdx.x * 4;
    sc[0] = n_sel, sc[1] = n_sbond, sc[2] = n_comp, sc[3] = largest;
    int* cnt = counts_o + (size_t)blockIdx.x * PG_SCAF_N_COUNTS;
    cnt[0] = n_sel;
    cnt[1] = n_sbond;
    cnt[2] = n_ring;
    cnt[3] = scaf_count(core) - n_ring;
    cnt[4] = n_exo;
    cnt[5] = scaf_count(kept) - n_sel;
    cnt[6] = n_sys;
    cnt[7] = n_linkb;
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_scaffold(const int8_t* cls, const int8_t* order, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig,
                               int n_bond, int max_n, int flags, uint8_t* part, int* counts, int* s_status, int* s_counts, int8_t* s_cls,
                               int16_t* s_compact, uint8_t* s_valence2, int16_t* s_comp, int8_t* s_order, void* stream) {
  const int rc = mol_check_batch("pg_mol_scaffold", B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (flags & ~(PG_SCAF_EXOCYCLIC | PG_SCAF_GENERIC)) {
    set_error("pg_mol_scaffold: flags %d (PG_SCAF_EXOCYCLIC = 1, PG_SCAF_GENERIC = 2)", flags);
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  hipLaunchKernelGGL(mol_scaffold_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, flags, part, counts, s_status, s_counts, s_cls, s_compact, s_valence2, s_comp, s_order);
  return check_launch("pg_mol_scaffold");
}
