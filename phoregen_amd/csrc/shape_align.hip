// Rigid overlay of molecule pairs: the frames of a set and the overlay optimiser (pg_shape_frames, pg_shape_align,
// include/phoregen_hip.h; phoregen_amd/shape.py; definition: DESIGN.md 2.9 "Shape alignment").  fp32 after the frames; a term is
// shape_sim.hip's (one fma into v_exp_f32) plus one product and three fmas for its share of the gradient.
//
// One workgroup per pair, one wave per enabled start.  A is fixed: lane l holds atoms l and l + 64 of A's row in registers, and B's
// atoms l and l + 64 as stored.  An evaluation re-poses B into the wave's own LDS slice (R (y - c_B) + p; start 0 reads the stored
// coordinates until its first accepted step, so its first evaluation is shape_sim.hip's bit for bit) and walks B's atoms in order by
// broadcast reads.  Per lane and register atom it accumulates the overlap and a = sum_j 2 k g (x_i - y'_j), the force its atom exerts
// on B; then F = sum_i a_i and tau = sum_i (x_i - p) x a_i -- which is the issue's s (x - p) - u form with a = s (x - p) - u, one fma
// less per term and free of its cancellation.  An evaluation ends in seven wave_sum butterflies per objective (V, F, tau; the same
// for colour).  Every value the loop branches on comes out of a butterfly, so trip count and accept / reject / stop are wave-uniform.
// The waves of a pair meet once, after their loops, at the barrier before the winner is chosen: the largest final score, ties to
// the lowest start.
//
// Summation order of an evaluation (fixed; depends on the two molecules and the pose alone): shape_sim.hip's for V and C; the six
// gradient sums the same way (atom l over j ascending, atom l + 64 over j ascending, low + high, wave_sum's butterfly).
#include "shape_align_core.h"
#include "../../include/phoregen_hip.h"
#include "common.h"
#include "wave_prims.h"

namespace pg {

struct AlignSetArg {
  const float4* atoms;
  const int* mol;
  const float* self_v;
  const float* self_c;
  const float* frame;
  int n_atoms, n;
};

struct AlignResult {                         // of one start
  float v, c, st, ct, score, r[9], t[3];
  int steps;
};

struct AlignShared {
  float4 atom[kAlignStarts][kShapeMaxAtoms];
  ShapePair pair[kShapeClasses * kShapeClasses];
  AlignResult result[kAlignStarts];
};

// the atoms of A's row that the lane holds (shape_sim.hip's ShapeOwn)
struct AlignOwn {
  float x[2], y[2], z[2], m[2];
  int cls[2], fp[2], n;
};

struct AlignEval {
  float v, c, st, ct, f, force[3], torque[3];
};

__device__ __forceinline__ void align_own_row(AlignOwn& o, const float4* __restrict__ atoms, int start, int n, int lane) {
  o.n = n;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    float4 v = {0.f, 0.f, 0.f, 0.f};
    int w = -1;
    if (i < n) {
      v = atoms[(size_t)start + i];
      w = __float_as_int(v.w);
    }
    const bool have = w >= 0 && shape_word_class(w) < kShapeClasses;
    o.x[h] = v.x, o.y[h] = v.y, o.z[h] = v.z, o.m[h] = have ? 1.f : 0.f;
    o.cls[h] = have ? shape_word_class(w) : 0, o.fp[h] = have ? shape_word_fp(w) : 0;
  }
}

// One evaluation: B (the lane's stored atoms mine[0], mine[1] of its n_b) posed by (q, p) into s, then f and its gradient.  The whole
// wave calls it; every lane returns the same values.
template <bool COLOUR>
__device__ __forceinline__ void align_evaluate(const AlignOwn& o, const float4 (&mine)[2], int n_b, float4* s, const ShapePair* pair,
                                               ShapePair colour, AlignQuat q, const float (&p)[3], bool stored, const float* cb, float aa_v,
                                               float bb_v, float aa_c, float bb_c, float w, int lane, AlignEval& e) {
  float r[9];
  align_quat_matrix(q, r);
  wave_lds_sync();                                                  // the walk of the evaluation before is over
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    if (i < n_b) {
      float4 y = mine[h];
      if (!stored) align_apply(r, cb, p, mine[h].x, mine[h].y, mine[h].z, y.x, y.y, y.z);
      s[i] = y;
    }
  }
  wave_lds_sync();
  float v[2] = {0.f, 0.f}, c[2] = {0.f, 0.f}, av[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, ac[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  const bool high = o.n > 64;                                       // (wave-uniform)
  for (int k = 0; k < n_b; ++k) {                                   // (wave-uniform)
    const float4 b = s[k];
    const int wd = __float_as_int(b.w);
    if (wd < 0) continue;                                           // (wave-uniform: a broadcast value; packed sets hold no such atom)
    const int cj = min(shape_word_class(wd), kShapeClasses - 1), fj = shape_word_fp(wd);
    const ShapePair* row = pair + cj * kShapeClasses;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !high) continue;
      const float dx = o.x[h] - b.x, dy = o.y[h] - b.y, dz = o.z[h] - b.z;
      const float d2 = shape_dist2(o.x[h], o.y[h], o.z[h], b.x, b.y, b.z);
      const ShapePair pe = row[o.cls[h]];
      const float g = shape_term(d2, pe);
      v[h] = fmaf(o.m[h], g, v[h]);
      const float gt = (o.m[h] * g) * pe.t1;
      av[h][0] = fmaf(gt, dx, av[h][0]), av[h][1] = fmaf(gt, dy, av[h][1]), av[h][2] = fmaf(gt, dz, av[h][2]);
      if (COLOUR) {
        const float pop = (float)__popc(o.fp[h] & fj), gc = shape_term(d2, colour);
        c[h] = fmaf(pop, gc, c[h]);
        const float gp = pop * gc;
        ac[h][0] = fmaf(gp, dx, ac[h][0]), ac[h][1] = fmaf(gp, dy, ac[h][1]), ac[h][2] = fmaf(gp, dz, ac[h][2]);
      }
    }
  }
  // the lane's share of F = sum_i a_i and tau = sum_i (x_i - p) x a_i, still without the factor 2 k = -t1 (2 / log2 e)
  float fv[3], tv[3], fc[3] = {0.f, 0.f, 0.f}, tc[3] = {0.f, 0.f, 0.f};
  {
    const float x0 = o.x[0] - p[0], y0 = o.y[0] - p[1], z0 = o.z[0] - p[2], x1 = o.x[1] - p[0], y1 = o.y[1] - p[1], z1 = o.z[1] - p[2];
    fv[0] = av[0][0] + av[1][0], fv[1] = av[0][1] + av[1][1], fv[2] = av[0][2] + av[1][2];
    tv[0] = (y0 * av[0][2] - z0 * av[0][1]) + (y1 * av[1][2] - z1 * av[1][1]);
    tv[1] = (z0 * av[0][0] - x0 * av[0][2]) + (z1 * av[1][0] - x1 * av[1][2]);
    tv[2] = (x0 * av[0][1] - y0 * av[0][0]) + (x1 * av[1][1] - y1 * av[1][0]);
    if (COLOUR) {
      fc[0] = ac[0][0] + ac[1][0], fc[1] = ac[0][1] + ac[1][1], fc[2] = ac[0][2] + ac[1][2];
      tc[0] = (y0 * ac[0][2] - z0 * ac[0][1]) + (y1 * ac[1][2] - z1 * ac[1][1]);
      tc[1] = (z0 * ac[0][0] - x0 * ac[0][2]) + (z1 * ac[1][0] - x1 * ac[1][2]);
      tc[2] = (x0 * ac[0][1] - y0 * ac[0][0]) + (x1 * ac[1][1] - y1 * ac[1][0]);
    }
  }
  e.v = wave_sum(v[0] + v[1]);
  e.c = COLOUR ? wave_sum(c[0] + c[1]) : 0.f;
  e.st = shape_tanimoto(e.v, aa_v, bb_v);
  e.ct = COLOUR ? shape_tanimoto(e.c, aa_c, bb_c) : 0.f;
  e.f = shape_score(e.st, e.ct, w);
  const float wv = -kAlignTwoOverLog2e * (1.0f - w) * align_tanimoto_slope(e.v, aa_v, bb_v);
  const float wc = COLOUR ? -kAlignTwoOverLog2e * colour.t1 * w * align_tanimoto_slope(e.c, aa_c, bb_c) : 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e.force[d] = wv * wave_sum(fv[d]);
    e.torque[d] = wv * wave_sum(tv[d]);
    if (COLOUR) {
      e.force[d] = fmaf(wc, wave_sum(fc[d]), e.force[d]);
      e.torque[d] = fmaf(wc, wave_sum(tc[d]), e.torque[d]);
    }
  }
}

// ---- frames: one wave per row ---------------------------------------------------------------------------------------------------------
// Every lane runs the same serial sums over the row's atoms (broadcast loads; at most 128 atoms, in double), lane 0 writes.
__global__ __launch_bounds__(64) void shape_frames_kernel(const float4* __restrict__ atoms, int n_atoms, const int* __restrict__ mol, int n,
                                                          float* __restrict__ frame) {
  const int row = blockIdx.x;
  const int start = mol[2 * (size_t)row];
  const int cnt = shape_atom_count(start, mol[2 * (size_t)row + 1], n_atoms);
  float out[kAlignFrame];
  align_frame(atoms + (cnt > 0 ? (size_t)start : 0), cnt, out);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kAlignFrame; ++k) frame[(size_t)row * kAlignFrame + k] = out[k];
  }
}

// ---- the optimiser: one workgroup per pair, wave k takes the k-th enabled start -----------------------------------------------------------
template <bool COLOUR>
__global__ __launch_bounds__(64 * kAlignStarts) void shape_align_kernel(AlignSetArg a, AlignSetArg b, ShapeTable tab,
                                                                        const int* __restrict__ pairs, int starts, int max_steps,
                                                                        float first_step, float min_step, float w, float* __restrict__ values,
                                                                        float* __restrict__ transform, int* __restrict__ start_o,
                                                                        int* __restrict__ steps_o) {
  __shared__ AlignShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const size_t pair = blockIdx.x;
  int ia, ib;
  if (pairs) {
    ia = pairs[2 * pair], ib = pairs[2 * pair + 1];
  } else {
    ia = (int)(pair / (unsigned)b.n), ib = (int)(pair - (size_t)ia * (unsigned)b.n);
  }
  int a0 = 0, na = 0, b0 = 0, nb = 0;
  if (ia >= 0 && ia < a.n && ib >= 0 && ib < b.n) {                 // (the entry point refuses any other pair)
    a0 = a.mol[2 * (size_t)ia], na = shape_atom_count(a0, a.mol[2 * (size_t)ia + 1], a.n_atoms);
    b0 = b.mol[2 * (size_t)ib], nb = shape_atom_count(b0, b.mol[2 * (size_t)ib + 1], b.n_atoms);
  }
  if (na == 0 || nb == 0) {                                         // (workgroup-uniform) an empty row: zeros, the identity, no start
    if (tid < 5) values[5 * pair + tid] = 0.f;
    if (tid < 12) transform[12 * pair + tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.f : 0.f;
    if (tid == 0) start_o[pair] = -1, steps_o[pair] = 0;
    return;
  }
  for (int i = tid; i < kShapeClasses * kShapeClasses; i += blockDim.x) sh.pair[i] = tab.pair[i];
  int k = -1;                                                       // the wave's start: the wave-th set bit of the mask
  for (int bit = 0, seen = 0; bit < kAlignStarts; ++bit)
    if (starts >> bit & 1) {
      if (seen == wave) k = bit;
      ++seen;
    }
  float fa[kAlignFrame], fb[kAlignFrame];
#pragma unroll
  for (int i = 0; i < kAlignFrame; ++i) fa[i] = a.frame[(size_t)ia * kAlignFrame + i], fb[i] = b.frame[(size_t)ib * kAlignFrame + i];
  const float rho = fb[12];
  const float aa_v = a.self_v[ia], bb_v = b.self_v[ib], aa_c = COLOUR ? a.self_c[ia] : 0.f, bb_c = COLOUR ? b.self_c[ib] : 0.f;
  AlignOwn o;
  align_own_row(o, a.atoms, a0, na, lane);
  float4 mine[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) mine[h] = lane + 64 * h < nb ? b.atoms[(size_t)b0 + lane + 64 * h] : float4{0.f, 0.f, 0.f, __int_as_float(-1)};
  __syncthreads();                                                  // the table is staged
  AlignQuat q;
  float p[3];
  align_start(k < 0 ? 0 : k, fa, fb, q, p);
  bool stored = k == 0;
  float4* s = sh.atom[wave];
  AlignEval cur;
  align_evaluate<COLOUR>(o, mine, nb, s, sh.pair, tab.colour, q, p, stored, fb, aa_v, bb_v, aa_c, bb_c, w, lane, cur);
  int evaluations = 1;
  float step = first_step;
  while (!align_stop(step, evaluations, min_step, max_steps)) {     // (wave-uniform: every operand is a butterfly's result or an argument)
    float d[6];
    if (!align_direction(cur.force, cur.torque, rho, d)) break;
    AlignQuat qt;
    float pt[3];
    align_trial(q, p, d, step, rho, qt, pt);
    AlignEval trial;
    align_evaluate<COLOUR>(o, mine, nb, s, sh.pair, tab.colour, qt, pt, false, fb, aa_v, bb_v, aa_c, bb_c, w, lane, trial);
    ++evaluations;
    if (align_accept(trial.f, cur.f, step)) {
      cur = trial, q = qt, p[0] = pt[0], p[1] = pt[1], p[2] = pt[2];
      stored = false;
    }
  }
  if (lane == 0) {
    AlignResult& res = sh.result[wave];
    res.v = cur.v, res.c = cur.c, res.st = cur.st, res.ct = cur.ct, res.score = cur.f, res.steps = evaluations;
    align_quat_matrix(q, res.r);
    align_translation(res.r, fb, p, res.t);
  }
  __syncthreads();
  if (wave != 0) return;
  int best = 0;
  for (int i = 1; i < n_waves; ++i)
    if (sh.result[i].score > sh.result[best].score) best = i;       // (strictly: ties go to the lowest start)
  const AlignResult& res = sh.result[best];
  if (lane == 0) {
    values[5 * pair] = res.v, values[5 * pair + 1] = res.c, values[5 * pair + 2] = res.st, values[5 * pair + 3] = res.ct;
    values[5 * pair + 4] = res.score;
    int seen = 0, which = -1;
    for (int bit = 0; bit < kAlignStarts; ++bit)
      if (starts >> bit & 1) {
        if (seen == best) which = bit;
        ++seen;
      }
    start_o[pair] = which, steps_o[pair] = res.steps;
  }
  if (lane < 9) transform[12 * pair + lane] = res.r[lane];
  else if (lane < 12) transform[12 * pair + lane] = res.t[lane - 9];
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------------
static int align_check_set(const char* name, const char* which, const float* atoms, int n_atoms, const int* mol, const float* self_v,
                           const float* self_c, const float* frames, int n, bool need_all, bool colour) {
  if (n < 0 || n_atoms < 0) {
    set_error("%s: set %s has %d rows and %d atom rows", name, which, n, n_atoms);
    return PG_ERR_ARG;
  }
  if (n > 0 && (!mol || !frames || (n_atoms > 0 && !atoms) || (need_all && (!self_v || (colour && !self_c))))) {
    set_error("%s: set %s has %d rows and a null array", name, which, n);
    return PG_ERR_ARG;
  }
  return PG_OK;
}

}  // namespace pg

using namespace pg;

extern "C" int pg_shape_frames(const float* atoms, int n_atoms, const int* mol, int n, float* frames, void* stream) {
  const int rc = align_check_set("pg_shape_frames", "a", atoms, n_atoms, mol, nullptr, nullptr, frames, n, false, false);
  if (rc != PG_OK) return rc;
  if (n == 0) return PG_OK;
  hipLaunchKernelGGL(shape_frames_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(atoms), n_atoms,
                     mol, n, frames);
  return check_launch("pg_shape_frames");
}

extern "C" int pg_shape_align(const float* a_atoms, int a_n_atoms, const int* a_mol, const float* a_self_shape, const float* a_self_colour,
                              const float* a_frames, int na, const float* b_atoms, int b_n_atoms, const int* b_mol,
                              const float* b_self_shape, const float* b_self_colour, const float* b_frames, int nb, const int* pairs,
                              int n_pairs, int has_colour, float w, const float* alpha, int max_steps, float first_step, float min_step,
                              int starts, float* values, float* transform, int* start, int* steps, void* stream) {
  const char* name = "pg_shape_align";
  const hipStream_t st = (hipStream_t)stream;
  if (!(w >= 0.0f && w <= 1.0f)) {
    set_error("%s: the colour weight %g is not a number in [0, 1]", name, (double)w);
    return PG_ERR_ARG;
  }
  const bool colour = has_colour != 0 && w > 0.0f;                  // w = 0: CT = 0 and the colour terms are skipped
  int rc = align_check_set(name, "a", a_atoms, a_n_atoms, a_mol, a_self_shape, a_self_colour, a_frames, na, true, colour);
  if (rc == PG_OK) rc = align_check_set(name, "b", b_atoms, b_n_atoms, b_mol, b_self_shape, b_self_colour, b_frames, nb, true, colour);
  if (rc != PG_OK) return rc;
  if (n_pairs < 0) {
    set_error("%s: %d pairs", name, n_pairs);
    return PG_ERR_ARG;
  }
  if (!pairs && n_pairs > 0 && (long long)na * nb != (long long)n_pairs) {
    set_error("%s: without a pair list the pairs are the grid of %d x %d rows, not %d", name, na, nb, n_pairs);
    return PG_ERR_ARG;
  }
  if (!align_options_ok(max_steps, first_step, min_step, starts)) {
    set_error("%s: max_steps %d (1 .. %d), first step %g and least step %g (positive, finite, least <= first), starts mask 0x%x (bits 0 .. 4, "
              "not empty)", name, max_steps, kAlignMaxSteps, (double)first_step, (double)min_step, starts);
    return PG_ERR_ARG;
  }
  ShapeTable tab;
  if (!alpha) {
    set_error("%s: a null alpha table", name);
    return PG_ERR_ARG;
  }
  if (!shape_table(alpha, tab)) {
    set_error("%s: every alpha of the table (%d elements, then the colour alpha) must be positive and finite", name, kShapeClasses);
    return PG_ERR_ARG;
  }
  if (n_pairs == 0) return PG_OK;
  if (!values || !transform || !start || !steps) {
    set_error("%s: a null output for %d pairs", name, n_pairs);
    return PG_ERR_ARG;
  }
  if (pairs) {
    // A listed pair must name a row of each set, and the list lives on the device: it is read back once, before anything is launched
    // (the one host read of this entry point; the full grid, pairs = null, needs none).
    int* host = static_cast<int*>(malloc((size_t)n_pairs * 2 * sizeof(int)));
    if (!host) {
      set_error("%s: no host memory to check %d pairs", name, n_pairs);
      return PG_ERR_HIP;
    }
    hipError_t e = hipMemcpyAsync(host, pairs, (size_t)n_pairs * 2 * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    long long bad = -1;
    if (e == hipSuccess)
      for (long long i = 0; i < n_pairs && bad < 0; ++i)
        if (host[2 * i] < 0 || host[2 * i] >= na || host[2 * i + 1] < 0 || host[2 * i + 1] >= nb) bad = i;
    if (e != hipSuccess) {
      free(host);
      set_error("%s: reading the pair list: %s", name, hipGetErrorString(e));
      return PG_ERR_HIP;
    }
    if (bad >= 0) {
      set_error("%s: pair %lld is (%d, %d), the sets have %d and %d rows", name, bad, host[2 * bad], host[2 * bad + 1], na, nb);
      free(host);
      return PG_ERR_ARG;
    }
    free(host);
  }
  const AlignSetArg a = {reinterpret_cast<const float4*>(a_atoms), a_mol, a_self_shape, a_self_colour, a_frames, a_n_atoms, na};
  const AlignSetArg b = {reinterpret_cast<const float4*>(b_atoms), b_mol, b_self_shape, b_self_colour, b_frames, b_n_atoms, nb};
  const dim3 grid((unsigned)n_pairs), block(64u * (unsigned)__builtin_popcount((unsigned)starts));
  if (colour)
    hipLaunchKernelGGL(shape_align_kernel<true>, grid, block, 0, st, a, b, tab, pairs, starts, max_steps, first_step, min_step, w, values,
                       transform, start, steps);
  else
    hipLaunchKernelGGL(shape_align_kernel<false>, grid, block, 0, st, a, b, tab, pairs, starts, max_steps, first_step, min_step, w, values,
                       transform, start, steps);
  return check_launch(name);
}
