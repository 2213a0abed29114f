// Substructure search: the embeddings of every pattern of a table in every decoded (frame, graph) (pg_mol_sub, include/phoregen_hip.h;
// phoregen_amd/substructure.py; definition: DESIGN.md 2.9 "Substructure").  Reads the screen's, the rings' and the Kekulé outputs.  One
// wave per (frame, graph, pattern): block (f * B + g) * P + p (mol_common.h).  The wave builds, in the screen's compact numbering, one
// adjacency bit matrix per bond class and one property word per atom in LDS, then a 128-bit compatibility mask per query atom; the
// roots (the atoms compatible with query atom 0) are dealt to the lanes, root r to lane r mod 64, and every lane runs its own depth-
// first search (sub_core.h) with its stack in LDS.  The searches are lane-dependent loops: they hold no barrier, vote or cross-lane
// move; the lanes' results meet in LDS atomics after them.  Integer work only, so every output is exact.
#include "mol_common.h"
#include "sub_core.h"

namespace pg {

constexpr int kSubWords = PG_SUB_PATTERN_BYTES / 4;

// the search state of one lane: the stack and the partial embedding live in LDS ([level][lane]: the lanes of a wave read neighbouring
// 16-byte rows), the pattern's tables are shared by the wave (every lane reads one address: a broadcast)
struct SubLaneStore {
  int lane;
  MolAdjRow (*adj_)[kSubTargetMax];              // [class][atom]
  MolAdjRow (*stack_)[64];                       // [level][lane]
  unsigned char (*map_)[64], (*first_)[64];      // [level][lane]
  const MolAdjRow* compat_;                      // [level]
  const unsigned* back_;                         // [level]
  unsigned char (*classes_)[kSubMaxAtoms];       // [level][earlier level]

  __device__ __forceinline__ SubMask compat(int d) const {
    const MolAdjRow r = compat_[d & 15];
    return SubMask{{r.w[0], r.w[1]}};
  }
  __device__ __forceinline__ unsigned back(int d) const { return back_[d & 15]; }
  __device__ __forceinline__ unsigned classes(int d, int e) const { return classes_[d & 15][e & 15]; }
  __device__ __forceinline__ SubMask adj(int c, int t) const {
    const MolAdjRow r = adj_[c & 7][t & (kSubTargetMax - 1)];
    return SubMask{{r.w[0], r.w[1]}};
  }
  __device__ __forceinline__ int image(int d) const { return map_[d & 15][lane]; }
  __device__ __forceinline__ void set_image(int d, int t) { map_[d & 15][lane] = (unsigned char)t; }
  __device__ __forceinline__ SubMask cand(int d) const {
    const MolAdjRow r = stack_[d & 15][lane];
    return SubMask{{r.w[0], r.w[1]}};
  }
  __device__ __forceinline__ void set_cand(int d, const SubMask& m) {
    MolAdjRow r;
    r.w[0] = m.w[0], r.w[1] = m.w[1];
    stack_[d & 15][lane] = r;
  }
  __device__ __forceinline__ void save_first(int k, int last) {
    for (int d = 0; d + 1 < k; ++d) first_[d & 15][lane] = map_[d & 15][lane];
    first_[(k - 1) & 15][lane] = (unsigned char)last;
  }
};

__global__ __launch_bounds__(64) void mol_sub_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                     const int16_t* __restrict__ compact_i, const uint8_t* __restrict__ ring_size_i,
                                                     const uint8_t* __restrict__ atom_ring_i, const uint8_t* __restrict__ hcount_i,
                                                     const int8_t* __restrict__ charge_i, const int* __restrict__ kek_status_i,
                                                     const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B, int P,
                                                     int n_lig, int n_half, const uint32_t* __restrict__ table, unsigned max_steps,
                                                     int* __restrict__ emb_o, int* __restrict__ anc_o, long long* __restrict__ mask_o,
                                                     int16_t* __restrict__ first_o, int* __restrict__ status_o) {
  __shared__ MolAdjRow s_adj[kSubClasses][kSubTargetMax];         // bonds of a class, compact numbering
  __shared__ MolAdjRow s_stack[kSubMaxAtoms][64];                 // a lane's untried candidates per level
  __shared__ MolAdjRow s_compat[kSubMaxAtoms];                    // atoms that meet the query atom at a position
  __shared__ unsigned int s_stat[kSubTargetMax];                  // degree | aromatic bonds << 16, compact numbering
  __shared__ int s_cidx[kSubTargetMax];                           // local atom -> compact index, -1 = dropped
  __shared__ unsigned char s_map[kSubMaxAtoms][64], s_first[kSubMaxAtoms][64];
  __shared__ __align__(16) uint32_t s_row[kSubWords];             // the pattern row
  __shared__ unsigned char s_classes[kSubMaxAtoms][kSubMaxAtoms]; // by position: the classes the bond (d, e) accepts
  __shared__ unsigned int s_back[kSubMaxAtoms];
  __shared__ unsigned long long s_emb, s_anchor[kMolCh], s_mask[kMolCh];
  __shared__ unsigned int s_min_root, s_flags;                    // s_flags: 1 = a root was abandoned

  const int lane = threadIdx.x;
  const unsigned fg = blockIdx.x / (unsigned)P, p = blockIdx.x - fg * (unsigned)P;
  for (int i = lane; i < kSubWords; i += 64) s_row[i] = table[(size_t)p * kSubWords + i];
  if (lane < kSubMaxAtoms) s_compat[lane].w[0] = s_compat[lane].w[1] = 0ull, s_back[lane] = 0u;
  if (lane < kMolCh) s_anchor[lane] = s_mask[lane] = 0ull;
  if (lane == 0) s_emb = 0ull, s_min_root = 0xffffffffu, s_flags = 0u;
#pragma unroll
  for (int c = 0; c < kMolCh; ++c) {
    const int i = c * 64 + lane;
    s_stat[i] = 0u, s_cidx[i] = -1;
#pragma unroll
    for (int b = 0; b < kSubClasses; ++b) s_adj[b][i].w[0] = s_adj[b][i].w[1] = 0ull;
  }
  MolFrame m;
  const bool ok = mol_frame(m, fg, B, g_lig_off, g_bond_off, n_lig, n_half);   // (wave-uniform)
  __syncthreads();

  const uint8_t* row = reinterpret_cast<const uint8_t*>(s_row);
  const int k = sub_row_k(row);                                                // (wave-uniform, as all that is read from the row)
  const bool row_ok = k >= 1 && k <= kSubMaxAtoms;                             // (the entry point refuses any other row)
  const bool uses_kekule = row_ok && sub_row_uses_kekule(row, k);
  const bool no_kekule = ok && uses_kekule && (kek_status_i[(size_t)m.f * B + m.g] & 1) != 0;
  const bool search = ok && row_ok && !no_kekule;
  if (search) {
    const int n = m.n;
    const size_t arow = m.arow, hrow = m.hrow;
    if (lane >= 1 && lane < k) {                                               // position d: its bonds to the earlier positions
      const int q = sub_row_order(row, lane);
      unsigned back = 0u;
      for (int e = 0; e < lane; ++e) {
        const unsigned classes = sub_class_mask(sub_row_bond(row, q, sub_row_order(row, e)));
        s_classes[lane][e] = (unsigned char)classes;
        back |= classes ? 1u << e : 0u;
      }
      s_back[lane] = back;
    }
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && mol_class(cls_i[arow + i]) >= 0) {
        const int ci = compact_i[arow + i];
        s_cidx[i] = (ci >= 0 && ci < kSubTargetMax) ? ci : -1;
      }
    }
    __syncthreads();

    for_each_pair(lane, n, m.n_pair, [&](int pr, int a, int b) {
      const int o = order_i[hrow + pr];
      const int ca = s_cidx[a], cb = s_cidx[b];
      if (mol_is_bond(o) && ca >= 0 && cb >= 0 && ca != cb) {
        const unsigned inc = 1u | (o == 4 ? 1u << 16 : 0u);
        atomicAdd(&s_stat[ca], inc);
        atomicAdd(&s_stat[cb], inc);
        mol_adj_set(s_adj[sub_bond_class(o, ring_size_i[hrow + pr] > 0)], ca, cb);
      }
    });
    __syncthreads();

    // the compatibility masks: every kept atom against every query atom
#pragma unroll
    for (int c = 0; c < kMolCh; ++c) {
      const int i = c * 64 + lane;
      const int ci = i < n ? s_cidx[i] : -1;
      if (ci >= 0) {
        const unsigned st = s_stat[ci];
        const int h = uses_kekule ? hcount_i[arow + i] : 0;
        const bool charged = uses_kekule && charge_i[arow + i] != 0;
        const uint32_t prop = sub_prop_pack(cls_i[arow + i], (int)(st & 0xffffu), h, charged, atom_ring_i[arow + i] > 0, (st >> 16) != 0);
        for (int d = 0; d < k; ++d)
          if (sub_atom_ok(sub_row_atom(row, sub_row_order(row, d)), prop)) atomicOr(&s_compat[d].w[ci >> 6], 1ull << (ci & 63));
      }
    }
    __syncthreads();

    // the searches: lane-dependent, no barrier inside
    SubLaneStore st = {lane, s_adj, s_stack, s_map, s_first, s_compat, s_back, s_classes};
    SubFound found = {0ull, {{0ull, 0ull}}, false, false};
    unsigned first_root = 0xffffffffu;
#pragma unroll 1
    for (int c = 0; c < kMolCh; ++c) {
      const int root = c * 64 + lane;
      if (s_compat[0].w[c] >> lane & 1ull) {
        const bool had = found.have_first;
        if (sub_search_root(st, k, root, (sub_u64)max_steps, found)) atomicOr(&s_anchor[c], 1ull << lane);
        if (!had && found.have_first) first_root = (unsigned)root;
      }
    }
    if (found.embeddings) atomicAdd(&s_emb, found.embeddings);
    if (found.atoms.w[0]) atomicOr(&s_mask[0], found.atoms.w[0]);
    if (found.atoms.w[1]) atomicOr(&s_mask[1], found.atoms.w[1]);
    if (found.have_first) atomicMin(&s_min_root, first_root);
    if (found.truncated) atomicOr(&s_flags, 1u);
  }
  __syncthreads();

  // a graph the kernel must not touch (the entry point refuses such a batch) still gets whole rows: no embedding
  const size_t out = blockIdx.x;
  const unsigned min_root = s_min_root;
  if (lane < kSubMaxAtoms) {
    int v = -1;
    if (search && min_root != 0xffffffffu) {
      // the lane that holds the smallest root with a find: its first find is that root's (its other root is 64 above or had none)
      for (int d = 0; d < k; ++d)
        if (sub_row_order(row, d) == lane) v = s_first[d][min_root & 63u];
    }
    first_o[out * kSubMaxAtoms + lane] = (int16_t)v;
  }
  if (lane < kMolCh) mask_o[out * kMolCh + lane] = (long long)s_mask[lane];
  if (lane == 0) {
    const int anchors = __popcll(s_anchor[0]) + __popcll(s_anchor[1]);
    emb_o[out] = sub_saturate(s_emb);
    anc_o[out] = anchors;
    status_o[out] = row_ok ? sub_status(s_emb, anchors, no_kekule, (s_flags & 1u) != 0, sub_row_int(row, PG_SUB_OFF_MIN),
                                        sub_row_int(row, PG_SUB_OFF_MAX))
                           : 0;
  }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_sub(const int8_t* cls, const int8_t* order, const int16_t* compact, const uint8_t* ring_size, const uint8_t* atom_ring,
                          const uint8_t* hcount, const int8_t* charge, const int* kekule_status, const int* g_lig_off, const int* g_bond_off,
                          int B, int F, int n_lig, int n_bond, int max_n, const uint8_t* table, const uint8_t* table_host, int P, int max_steps,
                          int* embeddings, int* anchors, int64_t* atom_mask, int16_t* first, int* status, void* stream) {
  const int rc = mol_check_batch("pg_mol_sub", B, F, n_lig, n_bond, max_n);
  if (rc != PG_OK && rc != kMolNothing) return rc;
  if (P < 1 || P > PG_SUB_MAX_PATTERNS) {
    set_error("pg_mol_sub: %d patterns, a table holds 1 .. PG_SUB_MAX_PATTERNS = %d", P, PG_SUB_MAX_PATTERNS);
    return PG_ERR_ARG;
  }
  if (max_steps < 1 || max_steps > PG_SUB_MAX_STEPS) {
    set_error("pg_mol_sub: max_steps %d, the work bound is 1 .. %d", max_steps, PG_SUB_MAX_STEPS);
    return PG_ERR_ARG;
  }
  if (!table_host) {
    set_error("pg_mol_sub: no host copy of the pattern table to check the %d rows from", P);
    return PG_ERR_ARG;
  }
  for (int p = 0; p < P; ++p) {
    const int e = sub_row_check(table_host + (size_t)p * PG_SUB_PATTERN_BYTES);
    if (e != kSubRowOk) {
      set_error("pg_mol_sub: pattern %d is malformed: %s", p, sub_row_error_text(e));
      return PG_ERR_ARG;
    }
  }
  if ((long long)B * F * P > 0x7fffffffLL) {
    set_error("pg_mol_sub: %d frames x %d graphs x %d patterns exceed one launch", F, B, P);
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  if ((n_lig > 0 && (!cls || !compact || !atom_ring || !hcount || !charge)) || (n_bond > 0 && (!order || !ring_size)) || !kekule_status ||
      !g_lig_off || !g_bond_off || !table || !embeddings || !anchors || !atom_mask || !first || !status) {
    set_error("pg_mol_sub: a null array with %d frames x %d graphs", F, B);
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_sub_kernel, dim3((unsigned)(B * F * P)), dim3(64), 0, (hipStream_t)stream, cls, order, compact, ring_size,
                     atom_ring, hcount, charge, kekule_status, g_lig_off, g_bond_off, B, P, n_lig, n_bond / 2,
                     reinterpret_cast<const uint32_t*>(table), (unsigned)max_steps, embeddings, anchors,
                     reinterpret_cast<long long*>(atom_mask), first, status);
  return check_launch("pg_mol_sub");
}
