// SMILES text of the molecules the screen decoded (pg_mol_smiles, include/phoregen_hip.h; phoregen_amd/molecule.py; definition:
// DESIGN.md 2.9 "SMILES").  Reads the screen's cls and the Kekulé form's kekule_order, hcount, charge and status.  One wave per
// (frame, graph) (mol_common.h).  The wave deals the pairs and builds the two bit planes of the bonds; the depth-first traversal and
// the ring-closure labels (smiles_core.h) run on lane 0 over arrays in LDS; then every lane formats its own atoms twice -- once to
// count the bytes, once, after a prefix sum of the counts in preorder, to write them -- so the length is known, and held against
// the capacity, before the first byte of text is written.  Integer work only.
//
// pg_mol_smiles_stereo is the same kernel with kStereo set (DESIGN.md 2.9 "Stereo"): it reads pg_mol_stereo's atom_parity and
// bond_stereo, finds the double bonds whose cis / trans the text can express while the pairs are dealt, has lane 0 decide the '/' and
// '\\' of the single bonds next to them after the labels, and the atoms' texts carry them and '@' / '@@'.  Without kStereo none of
// that is compiled in.
#include "mol_common.h"
#include "wave_prims.h"
#include "smiles_core.h"

namespace pg {

constexpr int kSmiMax = kMolMax, kSmiCh = kMolCh;
constexpr int kSmiPairs = kSmiMax * (kSmiMax - 1) / 2;

// zeros from byte `from` of the row to its end
__device__ __forceinline__ void smiles_write_row(int lane, uint8_t* text, int capacity, int from) {
  for (int i = from + lane; i < capacity; i += 64) text[i] = 0;
}

template <bool kStereo>
__global__ __launch_bounds__(64) void mol_smiles_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ kek_i,
                                                        const uint8_t* __restrict__ hcount_i, const int8_t* __restrict__ charge_i,
                                                        const int* __restrict__ kstatus_i, const int8_t* __restrict__ parity_i,
                                                        const int8_t* __restrict__ bstereo_i, const int* __restrict__ g_lig_off,
                                                        const int* __restrict__ g_bond_off, int B, int n_lig, int n_half,
                                                        const uint8_t* __restrict__ t_val, int capacity, uint8_t* __restrict__ text_o,
                                                        int* __restrict__ length_o, int16_t* __restrict__ rank_o,
                                                        int* __restrict__ counts_o, int* __restrict__ status_o,
                                                        int* __restrict__ scounts_o) {
  __shared__ MolAdjRow s_p0[kSmiMax], s_p1[kSmiMax];               // the bonds: odd order / order >= 2 (smiles_core.h)
  __shared__ int s_cls[kSmiMax];                                    // atom class, -1 = dropped
  __shared__ int16_t s_rank[kSmiMax], s_order[kSmiMax], s_parent[kSmiMax], s_stack[kSmiMax];
  __shared__ uint8_t s_flags[kSmiMax];
  __shared__ uint8_t s_label[kSmiPairs];                            // ring-closure label at the bond's pair row
  __shared__ int s_len[kSmiMax];                                    // bytes of the atom of rank k, then their exclusive prefix sum
  __shared__ uint8_t s_val[kSmiEl][4];
  __shared__ int s_tree[4];                                         // components, branches, largest label (or overflow), ring closures
  // kStereo only (not allocated otherwise): groups of marks dropped, marked bonds, double bonds expressed; the mark at the bond's pair
  // row; the other end and the value of an atom's stereo double bond
  __shared__ int s_marks[3];
  __shared__ uint8_t s_mark[kSmiPairs];
  __shared__ int16_t s_partner[kSmiMax];
  __shared__ int8_t s_sval[kSmiMax];

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;
  uint8_t* const text = text_o + (size_t)blockIdx.x * (size_t)capacity;
  int* const cnt = counts_o + (size_t)blockIdx.x * PG_SMILES_N_COUNTS;

  // ---- a graph without a Kekulé structure has no text (wave-uniform) ------------------------------------------------------------
  if (kstatus_i[blockIdx.x] & PG_KEKULE_FAILED) {
    smiles_write_row(lane, text, capacity, 0);
    for (int i = lane; i < n; i += 64) rank_o[arow + i] = -1;
    if (lane < PG_SMILES_N_COUNTS) cnt[lane] = 0;
    if (kStereo && lane < PG_SMILES_N_STEREO_COUNTS) scounts_o[(size_t)blockIdx.x * PG_SMILES_N_STEREO_COUNTS + lane] = 0;
    if (lane == 0) {
      length_o[blockIdx.x] = 0;
      status_o[blockIdx.x] = PG_SMILES_NO_KEKULE;
    }
    return;
  }

  // ---- table and atoms -------------------------------------------------------------------------------------------------------------
  if (lane < kSmiEl * 4) s_val[lane >> 2][lane & 3] = t_val[lane];
  unsigned long long kept[kSmiCh];
#pragma unroll
  for (int c = 0; c < kSmiCh; ++c) {
    const int i = c * 64 + lane;
    int k = -1;
    if (i < n) {
      s_cls[i] = k = mol_class(cls_i[arow + i]);
      s_rank[i] = -1;
      s_parent[i] = -1;
      s_flags[i] = 0;
      if (kStereo) s_partner[i] = -1, s_sval[i] = 0;
#pragma unroll
      for (int w = 0; w < kSmiCh; ++w) s_p0[i].w[w] = s_p1[i].w[w] = 0ull;
    }
    kept[c] = __ballot(k >= 0);
  }
  const int n_kept = __popcll(kept[0]) + __popcll(kept[1]);
  __syncthreads();

  // ---- bonds -----------------------------------------------------------------------------------------------------------------------
  int n_bond = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = kek_i[hrow + p];
    if (o >= 1 && o <= 3 && s_cls[a] >= 0 && s_cls[b] >= 0) {
      ++n_bond;
      if (o & 1) mol_adj_set(s_p0, a, b);
      if (o & 2) mol_adj_set(s_p1, a, b);
    }
  });
  n_bond = wave_sum(n_bond);
  __syncthreads();
  bool any_marks = false;                                            // (wave-uniform) a double bond whose stereo the text can express
  if (kStereo) {                                                     // ... their ends are disjoint: an atom has one partner at most
    bool found = false;
    for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
      const int s = bstereo_i[hrow + p];
      if (s_cls[a] >= 0 && s_cls[b] >= 0 && smi_stereo_bond_ok(s, mol_adj_words(s_p0), mol_adj_words(s_p1), a, b)) {
        s_partner[a] = (int16_t)b, s_partner[b] = (int16_t)a;
        s_sval[a] = s_sval[b] = (int8_t)s;
        found = true;
      }
    });
    any_marks = __any(found);
    if (any_marks)                                                   // without one the marks are neither settled nor read
      for (int p = lane; p < m.n_pair; p += 64) s_mark[p] = 0;
    __syncthreads();
  }

  // ---- the traversal and the labels, on one lane ------------------------------------------------------------------------------------
  if (lane == 0) {
    int comps = 0, branches = 0, closures = 0;
    const int seen = smiles_tree(n, mol_adj_words(s_p0), mol_adj_words(s_p1), kept[0], kept[1], s_rank, s_order, s_parent, s_flags, s_stack,
                                 &comps, &branches);
    s_tree[0] = comps;
    s_tree[1] = branches;
    s_tree[2] = smiles_labels(n, seen, mol_adj_words(s_p0), mol_adj_words(s_p1), s_rank, s_order, s_parent, s_label, &closures);
    s_tree[3] = closures;
    if (kStereo) s_marks[0] = s_marks[1] = s_marks[2] = 0;
    if (kStereo && any_marks && s_tree[2] != kSmiLabelOverflow) {
      int marked = 0, expressed = 0;
      s_marks[0] = smiles_stereo_marks(n, seen, mol_adj_words(s_p0), mol_adj_words(s_p1), s_rank, s_order, s_parent, s_partner, s_sval, s_mark,
                                      s_stack, &marked, &expressed);
      s_marks[1] = marked;
      s_marks[2] = expressed;
    }
  }
  __syncthreads();
  const int n_comp = s_tree[0], n_branch = s_tree[1], max_label = s_tree[2], n_closure = s_tree[3];

  if (max_label == kSmiLabelOverflow) {                              // (wave-uniform)
    smiles_write_row(lane, text, capacity, 0);
    for (int i = lane; i < n; i += 64) rank_o[arow + i] = -1;
    if (lane < PG_SMILES_N_COUNTS) cnt[lane] = 0;
    if (kStereo && lane < PG_SMILES_N_STEREO_COUNTS) scounts_o[(size_t)blockIdx.x * PG_SMILES_N_STEREO_COUNTS + lane] = 0;
    if (lane == 0) {
      length_o[blockIdx.x] = 0;
      status_o[blockIdx.x] = PG_SMILES_RING_LABELS;
    }
    return;
  }

  // ---- the bytes of every atom, and where they start: a prefix sum in preorder --------------------------------------------------------
  const uint8_t* const mark = kStereo && any_marks ? s_mark : nullptr;
  int n_bracket = 0, n_centre = 0, n_clockwise = 0;
#pragma unroll
  for (int c = 0; c < kSmiCh; ++c) {
    const int i = c * 64 + lane;
    int what = 0;
    if (i < n && s_cls[i] >= 0) {
      int len = 0;
      what = smiles_atom_text_stereo(i, n, s_cls[i], hcount_i[arow + i], charge_i[arow + i], s_val[s_cls[i]], mol_adj_words(s_p0),
                                     mol_adj_words(s_p1), s_rank, s_parent, s_flags, s_label, kStereo ? parity_i[arow + i] : 0, mark,
                                     [&](char) { ++len; });
      s_len[s_rank[i]] = len;
    }
    n_bracket += __popcll(__ballot(what & kSmiBracket));
    if (kStereo) n_centre += __popcll(__ballot(what & kSmiCentre)), n_clockwise += __popcll(__ballot(what & kSmiClockwise));
  }
  __syncthreads();
  int carry = 0;
#pragma unroll
  for (int c = 0; c < kSmiCh; ++c) {
    const int k = c * 64 + lane;
    const int len = k < n_kept ? s_len[k] : 0;
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      incl += lane >= o ? up : 0;
    }
    if (k < n_kept) s_len[k] = carry + incl - len;
    carry += __shfl(incl, 63);
  }
  const int need = carry;
  __syncthreads();
  const bool fits = need <= capacity;

  // ---- the text, the zero fill, the ranks ------------------------------------------------------------------------------------------------
#pragma unroll
  for (int c = 0; c < kSmiCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) rank_o[arow + i] = fits ? s_rank[i] : (int16_t)-1;
    if (fits && i < n && s_cls[i] >= 0) {
      uint8_t* at = text + s_len[s_rank[i]];                        // (need <= capacity: every byte lies inside the row)
      smiles_atom_text_stereo(i, n, s_cls[i], hcount_i[arow + i], charge_i[arow + i], s_val[s_cls[i]], mol_adj_words(s_p0),
                              mol_adj_words(s_p1), s_rank, s_parent, s_flags, s_label, kStereo ? parity_i[arow + i] : 0, mark,
                              [&](char ch) { *at++ = (uint8_t)ch; });
    }
  }
  smiles_write_row(lane, text, capacity, fits ? need : 0);

  if (lane == 0) {
    int st = fits ? 0 : PG_SMILES_TOO_LONG;
    st |= n_comp > 1 ? PG_SMILES_DISCONNECTED : 0;
    st |= n_kept == 0 ? PG_SMILES_EMPTY : 0;
    st |= n_bracket > 0 ? PG_SMILES_BRACKET : 0;
    if (kStereo) {
      st |= s_marks[0] > 0 ? PG_SMILES_STEREO_DROPPED : 0;
      int* const sc = scounts_o + (size_t)blockIdx.x * PG_SMILES_N_STEREO_COUNTS;
      sc[0] = n_centre, sc[1] = n_clockwise, sc[2] = s_marks[1], sc[3] = s_marks[2];
    }
    status_o[blockIdx.x] = st;
    length_o[blockIdx.x] = fits ? need : 0;
    cnt[0] = need;
    cnt[1] = n_kept;
    cnt[2] = n_bond;
    cnt[3] = n_comp;
    cnt[4] = n_closure;
    cnt[5] = n_branch;
    cnt[6] = max_label;
    cnt[7] = n_bracket;
  }
}

}  // namespace pg

using namespace pg;

// the checks and the launch of both entry points
template <bool kStereo>
static int smiles_launch(const char* name, const int8_t* cls, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                         const int* kekule_status, const int8_t* atom_parity, const int8_t* bond_stereo, const int* g_lig_off,
                         const int* g_bond_off, int B, int F, int n_lig, int n_bond, int max_n, const uint8_t* valences, int capacity,
                         uint8_t* text, int* length, int16_t* atom_rank, int* counts, int* status, int* stereo_counts, void* stream) {
  const int rc = mol_check_batch(name, B, F, n_lig, n_bond, max_n);
  if (rc == PG_ERR_ARG) return rc;
  if (capacity < 1) {
    set_error("%s: capacity %d, a text row holds at least one byte", name, capacity);
    return PG_ERR_ARG;
  }
  if (!valences) {
    set_error("%s: the table is null (valences: uint8 [11][4], device memory)", name);
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  if (!cls || !kekule_order || !hcount || !charge || !kekule_status || !g_lig_off || !g_bond_off || !text || !length || !atom_rank ||
      !counts || !status || (kStereo && (!atom_parity || !bond_stereo || !stereo_counts))) {
    set_error("%s: an array is null (cls, kekule_order, hcount, charge, kekule_status, %sthe offsets and the %s outputs)", name,
              kStereo ? "atom_parity, bond_stereo, " : "", kStereo ? "six" : "five");
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_smiles_kernel<kStereo>, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, kekule_order, hcount,
                     charge, kekule_status, atom_parity, bond_stereo, g_lig_off, g_bond_off, B, n_lig, n_bond / 2, valences, capacity, text,
                     length, atom_rank, counts, status, stereo_counts);
  return check_launch(name);
}

extern "C" int pg_mol_smiles(const int8_t* cls, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                             const int* kekule_status, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig, int n_bond,
                             int max_n, const uint8_t* valences, int capacity, uint8_t* text, int* length, int16_t* atom_rank, int* counts,
                             int* status, void* stream) {
  return smiles_launch<false>("pg_mol_smiles", cls, kekule_order, hcount, charge, kekule_status, nullptr, nullptr, g_lig_off, g_bond_off, B, F,
                              n_lig, n_bond, max_n, valences, capacity, text, length, atom_rank, counts, status, nullptr, stream);
}

extern "C" int pg_mol_smiles_stereo(const int8_t* cls, const int8_t* kekule_order, const uint8_t* hcount, const int8_t* charge,
                                    const int* kekule_status, const int8_t* atom_parity, const int8_t* bond_stereo, const int* g_lig_off,
                                    const int* g_bond_off, int B, int F, int n_lig, int n_bond, int max_n, const uint8_t* valences,
                                    int capacity, uint8_t* text, int* length, int16_t* atom_rank, int* counts, int* status,
                                    int* stereo_counts, void* stream) {
  return smiles_launch<true>("pg_mol_smiles_stereo", cls, kekule_order, hcount, charge, kekule_status, atom_parity, bond_stereo, g_lig_off,
                             g_bond_off, B, F, n_lig, n_bond, max_n, valences, capacity, text, length, atom_rank, counts, status,
                             stereo_counts, stream);
}
