// Gaussian shape and colour overlap of molecules where they lie: packing a screened batch into a set, the self overlaps, the all-pairs
// similarity matrix and the nearest neighbour with row sums (pg_shape_pack, pg_shape_self, pg_shape_similarity, pg_shape_nearest,
// include/phoregen_hip.h; phoregen_amd/shape.py; definition: DESIGN.md 2.9 "Shape").  fp32 throughout; a term is one fma into
// v_exp_f32 (shape_core.h), so a shape and a colour term cost one exponential each beside the three differences and three fmas of d^2.
//
// Matrix and nearest share one sweep, after csrc/fp_sim.hip: a workgroup of kShapeWaves waves owns kShapeTileA rows of set A, the
// other set passes through LDS in tiles of kShapeTileB molecules (their kept atoms, 16 bytes each, 2 KiB per molecule).  A wave takes
// one pair of molecules at a time: lane l holds atoms l and l + 64 of the A row in registers and walks the staged atoms of the B
// molecule in order, every lane reading the same LDS address (a broadcast).  The tile loop holds the barriers and has a
// workgroup-uniform trip count; the loops inside it hold none.
//
// The summation order of a pair is fixed and depends on the two molecules alone: every lane adds the terms of its atom i against
// the B atoms j = 0, 1, .. in packed order (one fp32 accumulator for atom l, one for atom l + 64, added as low + high), then the 64 lane
// sums go through wave_sum's butterfly (offsets 32, 16, .. 1).  A is always the set in registers, so a value does not depend on where
// the two molecules sit in their sets, on the tiling or the split, or on whether the matrix, the nearest search or the self overlap
// asks for it.  V(A, B) and V(B, A) are different orders and may differ in the last bits.
//
// Utilisation: molecules are ragged and a wave is 64 atoms wide.  A row of 30 atoms keeps 30 of 64 lanes busy (47 %); the second
// register atom costs nothing below 65 atoms (its half of the loop body is skipped by a wave-uniform branch).  Rows above 64 atoms
// run both halves at (n - 64) / 64 of the second one.
#include "shape_core.h"
#include "../../include/phoregen_hip.h"
#include "common.h"
#include "wave_prims.h"

namespace pg {

struct ShapeTile {
  float4 atom[kShapeTileB][kShapeMaxAtoms];
  ShapePair pair[kShapeClasses * kShapeClasses];
  int count[kShapeTileB];
  float self_v[kShapeTileB], self_c[kShapeTileB];
};

// the atoms of row `row` (-1: none) that lane `lane` holds; the row's atom count
struct ShapeOwn {
  float x[2], y[2], z[2], m[2];             // m: 1 for an atom, 0 for none
  int cls[2], fp[2], n;
};

__device__ __forceinline__ void shape_own_row(ShapeOwn& o, const float4* __restrict__ atoms, int n_atoms, const int* __restrict__ mol,
                                              int row, int lane) {
  int start = 0;
  o.n = 0;
  if (row >= 0) {
    start = mol[2 * (size_t)row];
    o.n = shape_atom_count(start, mol[2 * (size_t)row + 1], n_atoms);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    int w = -1;
    if (i < o.n) {
      v = atoms[(size_t)start + i];
      w = __float_as_int(v.w);
    }
    const bool have = w >= 0 && shape_word_class(w) < kShapeClasses;
    o.x[h] = v.x, o.y[h] = v.y, o.z[h] = v.z, o.m[h] = have ? 1.f : 0.f;
    o.cls[h] = have ? shape_word_class(w) : 0, o.fp[h] = have ? shape_word_fp(w) : 0;
  }
}

// molecules j0 .. j0 + cnt (cnt <= kShapeTileB) of a set into the tile; slots past a molecule's atoms are not written and not read.
// Every lane of the workgroup calls it.
__device__ __forceinline__ void shape_stage(ShapeTile& t, const float4* __restrict__ atoms, int n_atoms, const int* __restrict__ mol,
                                            const float* __restrict__ self_v, const float* __restrict__ self_c, int j0, int cnt, int tid) {
  constexpr int kThreads = 64 * kShapeWaves;
#pragma unroll
  for (int p = 0; p < kShapeTileB * kShapeMaxAtoms / kThreads; ++p) {
    const int slot = p * kThreads + tid, m = slot / kShapeMaxAtoms, k = slot % kShapeMaxAtoms;
    if (m < cnt) {
      const int start = mol[2 * ((size_t)j0 + m)];
      const int n = shape_atom_count(start, mol[2 * ((size_t)j0 + m) + 1], n_atoms);
      if (k < n) t.atom[m][k] = atoms[(size_t)start + k];
      if (k == 0) {
        t.count[m] = n;
        t.self_v[m] = self_v[(size_t)j0 + m];
        t.self_c[m] = self_c ? self_c[(size_t)j0 + m] : 0.f;
      }
    }
  }
}

// V and C of the lane's row against the n_b staged atoms at s: the whole wave calls it, every lane returns the totals
template <bool COLOUR>
__device__ __forceinline__ void shape_pair_overlap(const ShapeOwn& o, const float4* s, int n_b, const ShapePair* pair, ShapePair colour,
                                                   float& v_out, float& c_out) {
  float v0 = 0.f, v1 = 0.f, c0 = 0.f, c1 = 0.f;
  const bool high = o.n > 64;                                       // (wave-uniform)
  for (int k = 0; k < n_b; ++k) {                                   // (wave-uniform)
    const float4 q = s[k];
    const int w = __float_as_int(q.w);
    if (w < 0) continue;                                            // (wave-uniform: a broadcast value; packed sets hold no such atom)
    const int cj = min(shape_word_class(w), kShapeClasses - 1), fj = shape_word_fp(w);
    const ShapePair* row = pair + cj * kShapeClasses;
    {
      const float d2 = shape_dist2(o.x[0], o.y[0], o.z[0], q.x, q.y, q.z);
      v0 = fmaf(o.m[0], shape_term(d2, row[o.cls[0]]), v0);
      if (COLOUR) c0 = fmaf((float)__popc(o.fp[0] & fj), shape_term(d2, colour), c0);
    }
    if (high) {
      const float d2 = shape_dist2(o.x[1], o.y[1], o.z[1], q.x, q.y, q.z);
      v1 = fmaf(o.m[1], shape_term(d2, row[o.cls[1]]), v1);
      if (COLOUR) c1 = fmaf((float)__popc(o.fp[1] & fj), shape_term(d2, colour), c1);
    }
  }
  v_out = wave_sum(v0 + v1);
  c_out = COLOUR ? wave_sum(c0 + c1) : 0.f;
}

__device__ __forceinline__ void shape_table_to_lds(ShapeTile& t, const ShapeTable& tab, int tid) {
  for (int i = tid; i < kShapeClasses * kShapeClasses; i += 64 * kShapeWaves) t.pair[i] = tab.pair[i];
}

// ---- pack: one wave per (frame, graph) --------------------------------------------------------------------------------------------
// The kept atoms (class 0..10) of graph g of frame f in their order, compacted to the front of the graph's span of atom rows; the rest
// of the span reads as dropped.  mol = (first atom row, atoms); a row with a status bit has no atoms.
__global__ __launch_bounds__(64) void shape_pack_kernel(const int8_t* __restrict__ cls, const int* __restrict__ g_lig_off,
                                                        const float* __restrict__ pos, long long pos_fs,
                                                        const uint8_t* __restrict__ atom_fp, const uint8_t* __restrict__ select, int B,
                                                        int n_lig, float4* __restrict__ atoms, int* __restrict__ mol,
                                                        int* __restrict__ status) {
  const int lane = threadIdx.x;
  const unsigned block = blockIdx.x;
  const int f = (int)(block / (unsigned)B), g = (int)(block - (unsigned)f * (unsigned)B);
  const int a0 = g_lig_off[g], a1 = g_lig_off[g + 1];
  if (a0 < 0 || a1 < a0 || a1 - a0 > kShapeMaxAtoms || a1 > n_lig) {          // (the entry point's callers hand in no such graph)
    if (lane == 0) mol[2 * (size_t)block] = 0, mol[2 * (size_t)block + 1] = 0, status[block] = kShapeEmpty;
    return;
  }
  const int n = a1 - a0;
  const size_t arow = (size_t)f * n_lig + a0;
  float4 v[2];
  bool keep[2], bad[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    v[h] = float4{0.f, 0.f, 0.f, __int_as_float(-1)};
    keep[h] = bad[h] = false;
    if (i < n) {
      const int c = cls[arow + i];
      const float* p = pos + (size_t)f * pos_fs + 3 * ((size_t)a0 + i);
      const int w = shape_atom_word(c, atom_fp ? atom_fp[arow + i] : 0);
      if (w >= 0) {
        v[h] = float4{p[0], p[1], p[2], __int_as_float(w)};
        keep[h] = true;
        bad[h] = !(fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY);
      }
    }
  }
  const unsigned long long lo = __ballot(keep[0]), hi = __ballot(keep[1]), below = (1ull << lane) - 1ull;
  const int n_lo = __popcll(lo), kept = n_lo + __popcll(hi);
  int st = (kept == 0 ? kShapeEmpty : 0) | (__ballot(bad[0] || bad[1]) ? kShapeNonfinite : 0);
  if (select && !select[block]) st |= kShapeUnselected;
  // every row of the span is written once: the kept atoms first, dropped ones behind them
  const int before_lo = __popcll(lo & below), before_hi = __popcll(hi & below);
  const int at[2] = {keep[0] ? before_lo : kept + (lane - before_lo),
                     keep[1] ? n_lo + before_hi : kept + (64 - n_lo) + (lane - before_hi)};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    if (i < n && at[h] < n) atoms[arow + at[h]] = v[h];
  }
  if (lane == 0) mol[2 * (size_t)block] = (int)arow, mol[2 * (size_t)block + 1] = st ? 0 : kept, status[block] = st;
}

// ---- self overlaps: one wave per row ------------------------------------------------------------------------------------------------
template <bool COLOUR>
__global__ __launch_bounds__(64) void shape_self_kernel(const float4* __restrict__ atoms, int n_atoms, const int* __restrict__ mol, int n,
                                                        ShapeTable tab, float* __restrict__ self_v, float* __restrict__ self_c) {
  __shared__ float4 s_atom[kShapeMaxAtoms];
  __shared__ ShapePair s_pair[kShapeClasses * kShapeClasses];
  const int lane = threadIdx.x, row = blockIdx.x;
  for (int i = lane; i < kShapeClasses * kShapeClasses; i += 64) s_pair[i] = tab.pair[i];
  ShapeOwn o;
  shape_own_row(o, atoms, n_atoms, mol, row, lane);
  const int start = mol[2 * (size_t)row];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (lane + 64 * h < o.n) s_atom[lane + 64 * h] = atoms[(size_t)start + lane + 64 * h];
  __syncthreads();
  float v, c;
  shape_pair_overlap<COLOUR>(o, s_atom, o.n, s_pair, tab.colour, v, c);
  if (lane == 0) {
    self_v[row] = v;
    if (self_c) self_c[row] = c;
  }
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------------------
struct ShapeSetArg {
  const float4* atoms;
  const int* mol;
  const float* self_v;
  const float* self_c;
  int n_atoms, n;
};

// Block (x, y): rows x * kShapeTileA .. of A, run y of B's tiles.  MATRIX: st_o / ct_o [na][nb].  Else the nearest search: with
// part_best == null the block has all of B and writes the rows' results; else it writes its part to [y][na].
template <bool COLOUR, bool MATRIX>
__global__ __launch_bounds__(64 * kShapeWaves) void shape_sweep_kernel(ShapeSetArg a, ShapeSetArg b, ShapeTable tab, int tiles_per_split,
                                                                       int same, float w, float* __restrict__ st_o,
                                                                       float* __restrict__ ct_o, int* __restrict__ index_o,
                                                                       double* __restrict__ sum_o, fp_u64* __restrict__ part_best,
                                                                       double* __restrict__ part_sum) {
  __shared__ ShapeTile tile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  shape_table_to_lds(tile, tab, tid);
  fp_u64 best[kShapeRowsPerWave];
  double sum[kShapeRowsPerWave];
#pragma unroll
  for (int r = 0; r < kShapeRowsPerWave; ++r) best[r] = kFpMaxNone, sum[r] = 0.0;
  int j0, j1;
  shape_split_rows((int)blockIdx.y, tiles_per_split, b.n, j0, j1);
  for (int base = j0; base < j1; base += kShapeTileB) {               // (workgroup-uniform)
    const int cnt = min(kShapeTileB, j1 - base);
    __syncthreads();
    shape_stage(tile, b.atoms, b.n_atoms, b.mol, b.self_v, b.self_c, base, cnt, tid);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kShapeRowsPerWave; ++r) {
      const int ia = shape_wave_row(blockIdx.x, wave, r, a.n);      // (wave-uniform)
      if (ia < 0) continue;
      ShapeOwn o;
      shape_own_row(o, a.atoms, a.n_atoms, a.mol, ia, lane);
      const float aa_v = a.self_v[ia], aa_c = COLOUR ? a.self_c[ia] : 0.f;
      float st_mine = 0.f, ct_mine = 0.f;
      for (int m = 0; m < cnt; ++m) {                               // (wave-uniform)
        float v = 0.f, c = 0.f;
        if (o.n > 0) shape_pair_overlap<COLOUR>(o, tile.atom[m], tile.count[m], tile.pair, tab.colour, v, c);
        const float st = shape_tanimoto(v, aa_v, tile.self_v[m]);
        const float ct = COLOUR ? shape_tanimoto(c, aa_c, tile.self_c[m]) : 0.f;
        if (MATRIX) {
          if (lane == m) st_mine = st, ct_mine = ct;
        } else if (!(same && base + m == ia)) {
          const float s = shape_score(st, ct, w);
          const fp_u64 p = fp_pack_max(s, base + m);
          best[r] = p > best[r] ? p : best[r];
          sum[r] += (double)s;
        }
      }
      if (MATRIX && lane < cnt) {
        const size_t at = fp_matrix_at(ia, base + lane, b.n);
        st_o[at] = st_mine;
        if (COLOUR) ct_o[at] = ct_mine;
      }
    }
  }
  if (MATRIX || lane != 0) return;
#pragma unroll
  for (int r = 0; r < kShapeRowsPerWave; ++r) {
    const int ia = shape_wave_row(blockIdx.x, wave, r, a.n);
    if (ia < 0) continue;
    if (part_best) {
      part_best[(size_t)blockIdx.y * a.n + ia] = best[r];
      part_sum[(size_t)blockIdx.y * a.n + ia] = sum[r];
    } else {
      st_o[ia] = fp_max_sim(best[r]), index_o[ia] = fp_max_index(best[r]), sum_o[ia] = sum[r];
    }
  }
}

// the parts of a row in the order of the runs: the maximum does not depend on the cut, the sum is added in one fixed order
__global__ void shape_nearest_combine_kernel(const fp_u64* __restrict__ part_best, const double* __restrict__ part_sum, int na, int n_split,
                                             float* __restrict__ sim_o, int* __restrict__ index_o, double* __restrict__ sum_o) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= na) return;
  fp_u64 best = kFpMaxNone;
  double sum = 0.0;
  for (int s = 0; s < n_split; ++s) {
    const fp_u64 w = part_best[(size_t)s * na + i];
    best = w > best ? w : best;
    sum += part_sum[(size_t)s * na + i];
  }
  sim_o[i] = fp_max_sim(best), index_o[i] = fp_max_index(best), sum_o[i] = sum;
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------------
static int shape_check_table(const char* name, const float* alpha, ShapeTable& tab) {
  if (!alpha) {
    set_error("%s: a null alpha table", name);
    return PG_ERR_ARG;
  }
  if (!shape_table(alpha, tab)) {
    set_error("%s: every alpha of the table (%d elements, then the colour alpha) must be positive and finite", name, kShapeClasses);
    return PG_ERR_ARG;
  }
  return PG_OK;
}

static int shape_check_set(const char* name, const char* which, const float* atoms, int n_atoms, const int* mol, const float* self_v,
                           const float* self_c, int n, bool need_self, bool colour) {
  if (n < 0 || n_atoms < 0) {
    set_error("%s: set %s has %d rows and %d atom rows", name, which, n, n_atoms);
    return PG_ERR_ARG;
  }
  if (n > 0 && (!mol || (n_atoms > 0 && !atoms) || (need_self && (!self_v || (colour && !self_c))))) {
    set_error("%s: set %s has %d rows and a null array", name, which, n);
    return PG_ERR_ARG;
  }
  return PG_OK;
}

}  // namespace pg

using namespace pg;

extern "C" int pg_shape_pack(const int8_t* cls, const int* g_lig_off, const float* pos, int64_t pos_fs, const uint8_t* atom_fp,
                             const uint8_t* select, int B, int F, int n_lig, int max_n, const float* alpha, float* atoms, int* mol,
                             int* status, void* stream) {
  if (B < 0 || F < 0 || n_lig < 0 || max_n < 0 || pos_fs < 0) {
    set_error("pg_shape_pack: B %d, F %d, n_lig %d, max_n %d, frame stride %lld", B, F, n_lig, max_n, (long long)pos_fs);
    return PG_ERR_ARG;
  }
  if (max_n > PG_MOL_MAX_ATOMS) {
    set_error("pg_shape_pack: a graph of %d atoms, the kernel holds at most PG_MOL_MAX_ATOMS = %d", max_n, PG_MOL_MAX_ATOMS);
    return PG_ERR_ARG;
  }
  if ((long long)B * F > 0x7fffffffLL || (long long)F * n_lig > 0x7fffffffLL) {
    set_error("pg_shape_pack: %d frames x %d graphs / %d atom rows exceed one set", F, B, n_lig);
    return PG_ERR_ARG;
  }
  ShapeTable tab;
  const int rc = shape_check_table("pg_shape_pack", alpha, tab);
  if (rc != PG_OK) return rc;
  if (B == 0 || F == 0) return PG_OK;
  if (!g_lig_off || !mol || !status || (n_lig > 0 && (!cls || !pos || !atoms))) {
    set_error("pg_shape_pack: a null array with %d frames x %d graphs, %d atom rows", F, B, n_lig);
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(shape_pack_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, g_lig_off, pos, (long long)pos_fs,
                     atom_fp, select, B, n_lig, reinterpret_cast<float4*>(atoms), mol, status);
  return check_launch("pg_shape_pack");
}

extern "C" int pg_shape_self(const float* atoms, int n_atoms, const int* mol, int n, const float* alpha, float* self_shape,
                             float* self_colour, void* stream) {
  int rc = shape_check_set("pg_shape_self", "a", atoms, n_atoms, mol, nullptr, nullptr, n, false, false);
  if (rc != PG_OK) return rc;
  ShapeTable tab;
  rc = shape_check_table("pg_shape_self", alpha, tab);
  if (rc != PG_OK) return rc;
  if (n == 0) return PG_OK;
  if (!self_shape) {
    set_error("pg_shape_self: a null output for %d rows", n);
    return PG_ERR_ARG;
  }
  const float4* at = reinterpret_cast<const float4*>(atoms);
  if (self_colour)
    hipLaunchKernelGGL(shape_self_kernel<true>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, at, n_atoms, mol, n, tab, self_shape,
                       self_colour);
  else
    hipLaunchKernelGGL(shape_self_kernel<false>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, at, n_atoms, mol, n, tab, self_shape,
                       self_colour);
  return check_launch("pg_shape_self");
}

extern "C" int pg_shape_similarity(const float* a_atoms, int a_n_atoms, const int* a_mol, const float* a_self_shape,
                                   const float* a_self_colour, int na, const float* b_atoms, int b_n_atoms, const int* b_mol,
                                   const float* b_self_shape, const float* b_self_colour, int nb, const float* alpha, float* shape_out,
                                   float* colour_out, void* stream) {
  const bool colour = colour_out != nullptr;
  int rc = shape_check_set("pg_shape_similarity", "a", a_atoms, a_n_atoms, a_mol, a_self_shape, a_self_colour, na, true, colour);
  if (rc == PG_OK) rc = shape_check_set("pg_shape_similarity", "b", b_atoms, b_n_atoms, b_mol, b_self_shape, b_self_colour, nb, true, colour);
  if (rc != PG_OK) return rc;
  if ((long long)na * nb > 0x7fffffffLL) {
    set_error("pg_shape_similarity: %d x %d elements exceed 2^31 - 1; use pg_shape_nearest, or cut the sets", na, nb);
    return PG_ERR_ARG;
  }
  ShapeTable tab;
  rc = shape_check_table("pg_shape_similarity", alpha, tab);
  if (rc != PG_OK) return rc;
  if (na == 0 || nb == 0) return PG_OK;
  if (!shape_out) {
    set_error("pg_shape_similarity: a null output for %d x %d elements", na, nb);
    return PG_ERR_ARG;
  }
  const ShapeSetArg a = {reinterpret_cast<const float4*>(a_atoms), a_mol, a_self_shape, a_self_colour, a_n_atoms, na};
  const ShapeSetArg b = {reinterpret_cast<const float4*>(b_atoms), b_mol, b_self_shape, b_self_colour, b_n_atoms, nb};
  const FpSplit sp = shape_split(na, nb, 8 * kNumCU);
  const dim3 grid((unsigned)fp_tiles(na, kShapeTileA), (unsigned)sp.n_split), block(64 * kShapeWaves);
  if (colour)
    hipLaunchKernelGGL((shape_sweep_kernel<true, true>), grid, block, 0, (hipStream_t)stream, a, b, tab, sp.tiles_per_split, 0, 0.f, shape_out,
                       colour_out, (int*)nullptr, (double*)nullptr, (fp_u64*)nullptr, (double*)nullptr);
  else
    hipLaunchKernelGGL((shape_sweep_kernel<false, true>), grid, block, 0, (hipStream_t)stream, a, b, tab, sp.tiles_per_split, 0, 0.f, shape_out,
                       colour_out, (int*)nullptr, (double*)nullptr, (fp_u64*)nullptr, (double*)nullptr);
  return check_launch("pg_shape_similarity");
}

extern "C" int pg_shape_nearest(const float* a_atoms, int a_n_atoms, const int* a_mol, const float* a_self_shape,
                                const float* a_self_colour, int na, const float* b_atoms, int b_n_atoms, const int* b_mol,
                                const float* b_self_shape, const float* b_self_colour, int nb, int same, int has_colour, float w,
                                const float* alpha, float* sim, int* index, double* sum, void* stream) {
  const bool colour = has_colour != 0;
  int rc = shape_check_set("pg_shape_nearest", "a", a_atoms, a_n_atoms, a_mol, a_self_shape, a_self_colour, na, true, colour);
  if (rc == PG_OK) rc = shape_check_set("pg_shape_nearest", "b", b_atoms, b_n_atoms, b_mol, b_self_shape, b_self_colour, nb, true, colour);
  if (rc != PG_OK) return rc;
  if (!shape_weight_ok(w)) {
    set_error("pg_shape_nearest: the colour weight %g is not a number in [0, 1]", (double)w);
    return PG_ERR_ARG;
  }
  if (same && (a_mol != b_mol || na != nb)) {
    set_error("pg_shape_nearest: same is set, but the two sets differ (%d and %d rows)", na, nb);
    return PG_ERR_ARG;
  }
  ShapeTable tab;
  rc = shape_check_table("pg_shape_nearest", alpha, tab);
  if (rc != PG_OK) return rc;
  if (na == 0) return PG_OK;
  if (!sim || !index || !sum) {
    set_error("pg_shape_nearest: a null output for %d rows", na);
    return PG_ERR_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;
  const ShapeSetArg a = {reinterpret_cast<const float4*>(a_atoms), a_mol, a_self_shape, a_self_colour, a_n_atoms, na};
  const ShapeSetArg b = {reinterpret_cast<const float4*>(b_atoms), b_mol, b_self_shape, b_self_colour, b_n_atoms, nb};
  const FpSplit sp = shape_split(na, nb, 8 * kNumCU);
  const dim3 grid((unsigned)fp_tiles(na, kShapeTileA), (unsigned)sp.n_split), block(64 * kShapeWaves);
  fp_u64* part_best = nullptr;
  double* part_sum = nullptr;
  void* ws = nullptr;
  if (sp.n_split > 1) {                                             // the parts of the runs: stream-ordered memory, no host synchronisation
    const size_t cells = (size_t)sp.n_split * na;
    const hipError_t e = hipMallocAsync(&ws, cells * 16, st);
    if (e != hipSuccess) {
      set_error("pg_shape_nearest: %zu bytes for the parts of %d runs: %s", cells * 16, sp.n_split, hipGetErrorString(e));
      return PG_ERR_HIP;
    }
    part_best = static_cast<fp_u64*>(ws);
    part_sum = reinterpret_cast<double*>(part_best + cells);
  }
  if (colour)
    hipLaunchKernelGGL((shape_sweep_kernel<true, false>), grid, block, 0, st, a, b, tab, sp.tiles_per_split, same, w, sim, (float*)nullptr,
                       index, sum, part_best, part_sum);
  else
    hipLaunchKernelGGL((shape_sweep_kernel<false, false>), grid, block, 0, st, a, b, tab, sp.tiles_per_split, same, w, sim, (float*)nullptr,
                       index, sum, part_best, part_sum);
  int out = check_launch("pg_shape_nearest");
  if (ws) {
    if (out == PG_OK) {
      hipLaunchKernelGGL(shape_nearest_combine_kernel, dim3((unsigned)fp_tiles(na, 256)), dim3(256), 0, st, part_best, part_sum, na,
                         sp.n_split, sim, index, sum);
      out = check_launch("pg_shape_nearest (combine)");
    }
    const hipError_t e = hipFreeAsync(ws, st);
    if (e != hipSuccess && out == PG_OK) {
      set_error("pg_shape_nearest: %s", hipGetErrorString(e));
      out = PG_ERR_HIP;
    }
  }
  return out;
}
