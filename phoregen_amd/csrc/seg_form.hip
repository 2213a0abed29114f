// Which kernel serves a pg_seg_attn / pg_seg_attn_bwd call: the one place that decides it (PgSegForm, include/phoregen_hip.h).
// Host arithmetic on the arguments only -- no HIP runtime call, nothing dereferenced -- so it answers without a GPU.  The entry points
// (seg_attn.hip, seg_attn_bwd.hip) resolve first and then launch what the form names; every refusal by argument lives here.
#include "seg_common.h"

using namespace pg;

static int g_seg_debug = 0;      // pg_debug_force_generic_seg: bit 0 the generic kernel for the node modes, bit 2 the staged triplet kernel on 8 waves
extern "C" int pg_debug_force_generic_seg(int mask) {
  const int old = g_seg_debug;
  g_seg_debug = mask;
  return old;
}

static int row_tiles(int rows) { return (rows + PG_SEG_ROW_TILE - 1) / PG_SEG_ROW_TILE; }
static int clamp_tiles(int tiles, int lo) { return tiles < lo ? lo : tiles; }
static bool pos_mode(int mode) { return mode == PG_SEG_KNN_POS || mode == PG_SEG_BOND_POS; }
static bool knn_mode(int mode) { return mode == PG_SEG_KNN_NODE || mode == PG_SEG_KNN_POS; }

// the fused form of the node modes is asked for: q and W2k_l given (and, for the node-update modes, W2v_l, b2v, out)
static bool fused_request(const PgSegAttn* p) {
  return p->mode <= PG_SEG_BOND_POS && p->q && p->W2k_l && (pos_mode(p->mode) || (p->W2v_l && p->b2v && p->out));
}

// node modes in the kernels of node_attn.hip; false: the shape is outside what they hold in registers
static bool node_form(const PgTopo* t, const PgSegAttn* p, PgSegForm* f) {
  const bool knn = knn_mode(p->mode), fused = fused_request(p);
  const int tiles = knn ? row_tiles(PG_SEG_KNN_MAX_K) : row_tiles(t->max_nlig);
  if (knn ? p->knn_k > PG_SEG_KNN_MAX_K : tiles > PG_SEG_NODE_MAX_TILES) return false;
  // the tiled form serves the fused sampler calls of the position modes: no second target list, no training outputs
  if (fused && p->pos_tiled && pos_mode(p->mode) && !p->alpha && p->n_seg2 <= 0 && tiles <= PG_SEG_POS_TILED_MAX_TILES) {
    f->family = PG_FORM_POS_TILED;
    f->tiles = clamp_tiles(tiles, PG_SEG_POS_TILED_MIN_TILES);
    f->threads = 768;
    return true;
  }
  f->family = fused ? PG_FORM_NODE_FUSED : PG_FORM_NODE_TWO_PASS;
  f->tiles = knn ? tiles : clamp_tiles(tiles, PG_SEG_NODE_MIN_TILES);
  f->threads = fused ? 768 : 256;
  f->record_floats = !p->alpha ? 0 : pos_mode(p->mode) ? 32 : 16;
  return true;
}

// triplet in the staged kernel (triplet2.hip): the caller provides the source-atom groups (tri_iters) and P is one [n_bond, 256] =
// [P_k | P_v] tensor, for the sampling form (out = resid + update) and for the training form (S, swn and optionally the record)
static bool staged_form(const PgTopo* t, const PgSegAttn* p, PgSegForm* f) {
  if (!p->tri_iters || !p->tri_counter || p->n_tri_iters <= 0) return false;
  const bool train = p->S != nullptr;
#ifdef PG_T2_PROF
  if (train || !p->out || !p->resid) return false;
#else
  if (train ? (!p->swn || !p->q || !p->W2k_l || (p->alpha && p->alpha_rows < t->max_nlig)) : (p->alpha || !p->out || !p->resid)) return false;
#endif
  if (p->Csrc_v != p->Csrc_k + 128 || p->ld_csrc != PG_SEG_TRI_STAGED_LD || ((size_t)p->Csrc_k & 15) || !p->Cdst_k || !p->Cdst_v) return false;
  if (t->max_nlig - 1 > PG_SEG_TRI_STAGED_ROWS || t->max_nlig > PG_SEG_TRI_STAGED_ATOMS) return false;
  const int maxn = (p->tri_max_nlig > 0 && p->tri_max_nlig < t->max_nlig) ? p->tri_max_nlig : t->max_nlig;     // largest ligand among this queue's entries
  f->family = train ? PG_FORM_TRI_STAGED_TRAIN : PG_FORM_TRI_STAGED;
  f->tiles = clamp_tiles(row_tiles(maxn - 2), PG_SEG_TRI_MIN_TILES);      // rows a segment visits: every atom but its source and its target
  f->threads = 64 * ((g_seg_debug & 4) && !train ? PG_SEG_TRI_WAVES_DEBUG : PG_SEG_TRI_WAVES);
  f->record_floats = train && p->alpha ? 16 : 0;
  return true;
}

// one target list
static int one_list_form(const PgTopo* t, const PgSegAttn* p, PgSegForm* f) {
  if (p->mode <= PG_SEG_BOND_POS && !(g_seg_debug & 1)) {
    // the weight tables go to LDS in 16-byte pieces
    if ((((size_t)p->Wf_k | (size_t)p->Wf_v | (size_t)p->Wf_k2 | (size_t)p->Wf_v2 | (size_t)p->W2xv_l) & 15) != 0) {
      set_error("pg_seg_attn: Wf_k / Wf_v / W2xv_l must be 16-byte aligned");
      return PG_ERR_ARG;
    }
    if (node_form(t, p, f)) return PG_OK;
  }
  if (fused_request(p)) {
    // the fused form was asked for but the one-pass kernel runs (shape outside the node kernels, or forced): fold, attend and
    // unfold as separate launches through the caller's U / S / swn scratch
    if (!p->U || !p->seg_ids || (!pos_mode(p->mode) && (!p->S || !p->swn))) {
      set_error("pg_seg_attn: the fused node form needs U (and S, swn) scratch and seg_ids for the one-pass kernel");
      return PG_ERR_ARG;
    }
    f->compose |= PG_FORM_FOLD_UNFOLD;
  }
  if (p->mode == PG_SEG_TRIPLET && staged_form(t, p, f)) return PG_OK;
  f->family = PG_FORM_GENERIC;
  f->threads = 256;
  f->record_floats = p->mode == PG_SEG_PHORE && p->alpha ? 16 : 0;
  return PG_OK;
}

extern "C" int pg_seg_attn_form(const PgTopo* t, const PgSegAttn* p, PgSegForm* out) {
  if (!t || !p || !out) { set_error("pg_seg_attn: null argument"); return PG_ERR_ARG; }
  *out = PgSegForm{};
  out->mode = p->mode;
  if (p->n_seg == 0 && p->n_seg2 <= 0) return PG_OK;
  if (p->mode < PG_SEG_KNN_NODE || p->mode > PG_SEG_PHORE) { set_error("pg_seg_attn: unknown mode %d", p->mode); return PG_ERR_ARG; }
  if (p->n_seg2 <= 0) return one_list_form(t, p, out);
  // two target lists in one call (fused knn form): one launch when the fused node kernel takes it, else list after list
  if (!knn_mode(p->mode) || !p->seg_ids || !p->seg_ids2 || !p->Wf_k2 || !p->Wf_v2) {
    set_error("pg_seg_attn: a second target list needs a knn mode, seg_ids, seg_ids2 and Wf_k2 / Wf_v2");
    return PG_ERR_ARG;
  }
  if (p->n_seg > 0 && fused_request(p) && !(g_seg_debug & 1) && p->knn_k <= PG_SEG_KNN_MAX_K) return one_list_form(t, p, out);
  PgSegAttn one = *p;                    // (both lists resolve alike: they differ in the ids and the feature weights only)
  one.n_seg2 = 0;
  out->compose |= PG_FORM_TWO_LISTS;
  return one_list_form(t, &one, out);
}

// ---- adjoint ----
static size_t bwd_lds_bytes(int mode, int nw, int split, int max_nlig) {
  switch (mode) {
    case PG_SEG_KNN_NODE: return bwd_lds_floats<PG_SEG_KNN_NODE>(nw, split, max_nlig) * sizeof(float);
    case PG_SEG_KNN_POS: return bwd_lds_floats<PG_SEG_KNN_POS>(nw, split, max_nlig) * sizeof(float);
    case PG_SEG_BOND_NODE: return bwd_lds_floats<PG_SEG_BOND_NODE>(nw, split, max_nlig) * sizeof(float);
    case PG_SEG_BOND_POS: return bwd_lds_floats<PG_SEG_BOND_POS>(nw, split, max_nlig) * sizeof(float);
    case PG_SEG_TRIPLET: return bwd_lds_floats<PG_SEG_TRIPLET>(nw, split, max_nlig) * sizeof(float);
    default: return bwd_lds_floats<PG_SEG_PHORE>(nw, split, max_nlig) * sizeof(float);
  }
}
static_assert(bwd_lds_floats<PG_SEG_TRIPLET>(2, 0, 17) == PG_SEG_BWD_TRI_BASE_FLOATS + 2 * PG_SEG_BWD_TRI_WAVE_FLOATS + 32 * PG_SEG_BWD_TRI_ROW_FLOATS,
              "the header's numbers for the triplet adjoint's LDS");

// waves per workgroup of the seg_attn_bwd.hip forms.  One wave per tile: the triplet's per-source-atom rows (max_nlig x 259 floats)
// share the LDS with the per-wave tiles, 4 waves up to 64 atoms, 2 waves up to the reference's maximum of 78 (and beyond, to 96).
// Two passes (profiles/r04_adjoint_codegen_fences.txt): a wave that holds ONE path fits 512 registers without spilling, and that is
// worth more than a second wave per SIMD at 256 registers -- except for the triplet value pass, the lightest, which runs best as 8.
static int one_wave_nw(int mode, int max_nlig) { return mode == PG_SEG_TRIPLET && max_nlig > PG_SEG_BWD_TRI_MAX_ATOMS ? 2 : 4; }
static int value_pass_nw(int mode) { return mode == PG_SEG_TRIPLET ? 8 : 4; }
static const int kKeyPassNw = 4;

// (the one-pass kernels do not touch the row buffer today; sizing it for them anyway keeps a later change from writing past it)
extern "C" int pg_seg_attn_bwd_waves(int mode) {
  const int a = one_wave_nw(mode, 0), b = value_pass_nw(mode);
  return a > b ? a : b;
}

extern "C" int pg_seg_attn_bwd_form(const PgTopo* t, const PgSegAttn* p, const PgSegAttnGrad* gr, PgSegForm* out) {
  if (!t || !p || !gr || !out) { set_error("pg_seg_attn_bwd: null argument"); return PG_ERR_ARG; }
  *out = PgSegForm{};
  out->mode = p->mode;
  if (p->n_seg == 0) return PG_OK;
  if (!p->U || !p->Cdst_k || !p->Cdst_v || gr->grid < 1) {
    set_error("pg_seg_attn_bwd: U, Cdst_k/v and a grid are required");
    return PG_ERR_ARG;
  }
  // the row buffer: every form but the triplet's channel-split one (its rows live in LDS) -- a launch that needs it and has none is refused
  const bool small = t->max_nlig <= PG_SEG_BWD_TRI_MAX_ATOMS;
  const bool channel_split = p->mode == PG_SEG_TRIPLET && gr->tri_form && small && p->Cdst_v == p->Cdst_k + 128;   // (Cdst k | v: one 1 KB row)
  if (!gr->rowbuf && !channel_split) {
    set_error("pg_seg_attn_bwd: mode %d in this form needs PgSegAttnGrad.rowbuf (grid x pg_seg_attn_bwd_waves x rows x 48 floats)", p->mode);
    return PG_ERR_ARG;
  }
  if (p->mode < PG_SEG_KNN_NODE || p->mode > PG_SEG_PHORE) { set_error("pg_seg_attn_bwd: unknown mode %d", p->mode); return PG_ERR_ARG; }
  if (channel_split) {
    // tri_form 1: 4 waves x 32 channels (up to 512 registers, one wave per SIMD).  tri_form 2: ligands of up to 32 atoms on 8 waves x 16
    // channels (two waves per SIMD at 256 registers, no spills: the fastest form), the larger ones of the batch in a second launch of the
    // 4-wave form.  (The 8-wave instances for 3 / 4 row tiles need more than 256 registers; they are not built.)
    const int nt = clamp_tiles(row_tiles(t->max_nlig), 2);
    out->family = PG_FORM_BWD_CHANNEL_SPLIT;
    if (gr->tri_form == 2) {
      out->tiles = row_tiles(PG_SEG_BWD_TRI_FORM2_ATOMS);
      out->threads = 512;
      if (nt > out->tiles) { out->compose = PG_FORM_SECOND_LAUNCH; out->tiles2 = nt; out->threads2 = 256; }
    } else {
      out->tiles = nt;
      out->threads = 256;
    }
    return PG_OK;
  }
  // the forward's record: softmax weights with S / swn (one pass instead of two; the position modes have no such kernel), and for two
  // passes the scratch on top (the position update redoes the softmax adjoint from the logits / value scalars of the record)
  const bool pos = pos_mode(p->mode);
  const bool record = pos ? gr->alpha != nullptr : gr->alpha && gr->S && gr->swn;
  const bool two_pass = record && gr->dlogit && gr->gfeat_v &&
                        (knn_mode(p->mode) || (p->mode == PG_SEG_TRIPLET && small));
  int nw;
  if (two_pass) {
    out->family = PG_FORM_BWD_TWO_PASS;
    nw = value_pass_nw(p->mode);
    out->threads = 64 * nw;
    out->threads2 = 64 * kKeyPassNw;
    out->record_floats = pos ? 32 : 16;
  } else {
    out->family = PG_FORM_BWD_ONE_WAVE;
    nw = one_wave_nw(p->mode, t->max_nlig);
    out->threads = 64 * nw;
    out->record_floats = record && !pos ? 16 : 0;
  }
  out->rowbuf_waves = nw > kKeyPassNw || !two_pass ? nw : kKeyPassNw;
  const size_t lds = bwd_lds_bytes(p->mode, nw, two_pass ? 1 : 0, t->max_nlig);
  const size_t lds2 = two_pass ? bwd_lds_bytes(p->mode, kKeyPassNw, 2, t->max_nlig) : 0;
  if (lds > PG_SEG_BWD_LDS_BYTES || lds2 > PG_SEG_BWD_LDS_BYTES) {
    set_error("pg_seg_attn_bwd: %zu B of LDS needed (ligand of %d atoms is too large)", lds > PG_SEG_BWD_LDS_BYTES ? lds : lds2, t->max_nlig);
    return PG_ERR_ARG;
  }
  return PG_OK;
}
