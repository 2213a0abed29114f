// Bit-vector Tanimoto over sets of 2048-bit fingerprints: the all-pairs matrix, the nearest neighbour with row sums, and MaxMin
// diverse-subset picking (pg_fp_tanimoto, pg_fp_nearest, pg_fp_maxmin, include/phoregen_hip.h; phoregen_amd/similarity.py;
// definition: DESIGN.md 2.9 "Fingerprints and similarity").  Integer work and one correctly rounded division per pair (fp_core.h), so
// every similarity is exact; only the fp64 row sums depend on the order of their terms.
//
// Matrix and nearest share one sweep: a workgroup of kFpTileA lanes holds one row each in 64 registers, the other set passes through
// LDS in tiles of kFpTileB rows, and every lane reads a staged row at one address (a broadcast: 16 ds_read_b128 per row, four LDS
// cycles each, against 128 VALU operations of the wave on it).  A pair costs 64 v_and_b32 and 64 accumulating v_bcnt_u32_b32.  No
// barrier stands inside a lane-dependent loop: the tile loop and the row loop have workgroup-uniform trip counts.
#include "fp_core.h"
#include "common.h"

namespace pg {

struct FpTile {
  uint4 row[kFpTileB][kFpDwords / 4];       // 256 bytes per row: a row is one LDS bank row
  int pop[kFpTileB];
};

// rows j0 .. j0 + cnt (cnt <= kFpTileB) of y and their popcounts; 16 lanes per row, 16 bytes each: a wave reads 1 KiB in a piece.
// Rows past cnt are zero.  Every lane of the workgroup calls it.
__device__ __forceinline__ void fp_stage(FpTile& t, const uint4* __restrict__ y, int j0, int cnt, int tid) {
  constexpr int kRowsPerPass = kFpTileA / kFpRowLanes;
#pragma unroll
  for (int p = 0; p < kFpTileB / kRowsPerPass; ++p) {
    const int r = p * kRowsPerPass + (tid >> 4), q = tid & 15;
    uint4 v = {0u, 0u, 0u, 0u};
    if (r < cnt) v = y[((size_t)j0 + r) * kFpRowLanes + q];
    t.row[r][q] = v;
    int pc = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    pc += __shfl_xor(pc, 8);
    pc += __shfl_xor(pc, 4);
    pc += __shfl_xor(pc, 2);
    pc += __shfl_xor(pc, 1);
    if (q == 0) t.pop[r] = pc;
  }
}

// popcount(x & staged row j): the lane's row in registers against a broadcast row
__device__ __forceinline__ int fp_common_bits(const uint32_t (&x)[kFpDwords], const FpTile& t, int j) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < kFpDwords / 4; ++q) {
    const uint4 v = t.row[j][q];
    c += __popc(x[4 * q] & v.x);
    c += __popc(x[4 * q + 1] & v.y);
    c += __popc(x[4 * q + 2] & v.z);
    c += __popc(x[4 * q + 3] & v.w);
  }
  return c;
}

// The lane's row i (-1: none, all zero) into registers; returns its popcount.
__device__ __forceinline__ int fp_own_row(uint32_t (&x)[kFpDwords], const uint4* __restrict__ rows, int i) {
  int px = 0;
#pragma unroll
  for (int q = 0; q < kFpDwords / 4; ++q) {
    uint4 v = {0u, 0u, 0u, 0u};
    if (i >= 0) v = rows[(size_t)i * kFpRowLanes + q];
    x[4 * q] = v.x, x[4 * q + 1] = v.y, x[4 * q + 2] = v.z, x[4 * q + 3] = v.w;
    px += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  return px;
}

// out [na][nb]: the lanes hold rows of B (so a wave writes 64 neighbouring elements of an output row), A passes through LDS.
// Block (x, y): B rows x * kFpTileA .., run y of A's tiles.
__global__ __launch_bounds__(kFpTileA) void fp_tanimoto_kernel(const uint4* __restrict__ a, int na, const uint4* __restrict__ b, int nb,
                                                               int tiles_per_split, float* __restrict__ out) {
  __shared__ FpTile tile;
  const int tid = threadIdx.x;
  const int jb = fp_lane_row(blockIdx.x, tid, nb);
  uint32_t x[kFpDwords];
  const int px = fp_own_row(x, b, jb);
  int i0, i1;
  fp_split_rows((int)blockIdx.y, tiles_per_split, na, i0, i1);
  for (int base = i0; base < i1; base += kFpTileB) {             // (workgroup-uniform)
    const int cnt = min(kFpTileB, i1 - base);
    __syncthreads();
    fp_stage(tile, a, base, cnt, tid);
    __syncthreads();
    for (int r = 0; r < cnt; ++r) {                               // (workgroup-uniform)
      const int c = fp_common_bits(x, tile, r);
      const float s = fp_tanimoto(c, px + tile.pop[r] - c);
      if (jb >= 0) out[fp_matrix_at(base + r, jb, nb)] = s;
    }
  }
}

// The lanes hold rows of A, B passes through LDS.  Block (x, y): A rows x * kFpTileA .., run y of B's tiles.  With part_best == null
// the block has all of B and writes the row's result; else it writes its part to [y][na].
__global__ __launch_bounds__(kFpTileA) void fp_nearest_kernel(const uint4* __restrict__ a, int na, const uint4* __restrict__ b, int nb,
                                                              int tiles_per_split, int same, float* __restrict__ sim_o,
                                                              int* __restrict__ index_o, double* __restrict__ sum_o,
                                                              fp_u64* __restrict__ part_best, double* __restrict__ part_sum) {
  __shared__ FpTile tile;
  const int tid = threadIdx.x;
  const int ia = fp_lane_row(blockIdx.x, tid, na);
  uint32_t x[kFpDwords];
  const int px = fp_own_row(x, a, ia);
  const int skip = same ? ia : -1;
  fp_u64 best = kFpMaxNone;
  double sum = 0.0;
  int j0, j1;
  fp_split_rows((int)blockIdx.y, tiles_per_split, nb, j0, j1);
  for (int base = j0; base < j1; base += kFpTileB) {             // (workgroup-uniform)
    const int cnt = min(kFpTileB, j1 - base);
    __syncthreads();
    fp_stage(tile, b, base, cnt, tid);
    __syncthreads();
    for (int r = 0; r < cnt; ++r) {                               // (workgroup-uniform)
      const int c = fp_common_bits(x, tile, r);
      const float s = fp_tanimoto(c, px + tile.pop[r] - c);
      if (base + r != skip) {
        const fp_u64 w = fp_pack_max(s, base + r);
        best = w > best ? w : best;
        sum += (double)s;
      }
    }
  }
  if (ia < 0) return;
  if (part_best) {
    part_best[(size_t)blockIdx.y * na + ia] = best;
    part_sum[(size_t)blockIdx.y * na + ia] = sum;
  } else {
    sim_o[ia] = fp_max_sim(best), index_o[ia] = fp_max_index(best), sum_o[ia] = sum;
  }
}

// the parts of a row in the order of the runs: the maximum does not depend on the cut, the sum is added in one fixed order
__global__ void fp_nearest_combine_kernel(const fp_u64* __restrict__ part_best, const double* __restrict__ part_sum, int na, int n_split,
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

// ---- MaxMin: one launch per pick, no host read between them -----------------------------------------------------------------------------
// work[i]: the largest similarity of row i to the rows picked so far (-1 before the first step), kFpPicked once i is picked.
// slots[t]: the packed (pick_sim, index) of pick t; step t reads slot t - 1 and reduces into slot t with a 64-bit atomicMin.
constexpr float kFpPicked = 2.0f;

__global__ void fp_maxmin_init_kernel(float* __restrict__ work, int n, fp_u64* __restrict__ slots, int k, int first) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) work[i] = -1.0f;
  if (i < k) slots[i] = i == 0 ? fp_pack_min(0.0f, first) : kFpMinNone;
}

// 16 lanes share a row, 16 bytes each (a wave reads four whole rows in a piece); the rows of a block are blockIdx.x * 16 + (tid >> 4),
// then on by the grid, kFpMaxMinFlight of them loaded before the first is used.  The loops' trip counts depend on the block alone.  One
// atomic per workgroup: thousands of 64-bit atomics on one address would cost more than the sweep.
constexpr int kFpMaxMinFlight = 4;

__global__ __launch_bounds__(256) void fp_maxmin_step_kernel(const uint4* __restrict__ fp, int n, float* __restrict__ work,
                                                             const fp_u64* __restrict__ prev_slot, fp_u64* __restrict__ slot) {
  constexpr int kRows = 256 / kFpRowLanes;
  __shared__ fp_u64 s_best[256 / 64];
  const int tid = threadIdx.x, q = tid & 15, sub = tid >> 4;
  const int p = fp_min_index(*prev_slot);
  if (p < 0 || p >= n) return;                                    // (grid-uniform; cannot happen for k <= n: every step has a candidate)
  const uint4 pv = fp[(size_t)p * kFpRowLanes + q];
  const long long stride = (long long)gridDim.x * kRows;
  fp_u64 best = kFpMinNone;
  for (long long base = (long long)blockIdx.x * kRows; base < n; base += kFpMaxMinFlight * stride) {
    uint4 v[kFpMaxMinFlight];
#pragma unroll
    for (int f = 0; f < kFpMaxMinFlight; ++f) {
      const long long i = base + f * stride + sub;
      v[f] = uint4{0u, 0u, 0u, 0u};
      if (i < n) v[f] = fp[(size_t)i * kFpRowLanes + q];
    }
#pragma unroll
    for (int f = 0; f < kFpMaxMinFlight; ++f) {
      const long long i = base + f * stride + sub;
      int cu = (__popc(v[f].x & pv.x) + __popc(v[f].y & pv.y) + __popc(v[f].z & pv.z) + __popc(v[f].w & pv.w))
               | (__popc(v[f].x | pv.x) + __popc(v[f].y | pv.y) + __popc(v[f].z | pv.z) + __popc(v[f].w | pv.w)) << 16;   // both at most 2048
      cu += __shfl_xor(cu, 8);
      cu += __shfl_xor(cu, 4);
      cu += __shfl_xor(cu, 2);
      cu += __shfl_xor(cu, 1);
      if (i < n && q == 0) {
        const float w = work[i];
        if (i == p) {
          work[i] = kFpPicked;
        } else if (w != kFpPicked) {
          const float m = fmaxf(w, fp_tanimoto(cu & 0xffff, cu >> 16));
          work[i] = m;
          const fp_u64 cand = fp_pack_min(m, (int)i);
          best = cand < best ? cand : best;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const fp_u64 other = __shfl_xor(best, o);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < 256 / 64; ++w) best = s_best[w] < best ? s_best[w] : best;
    if (best != kFpMinNone) atomicMin(slot, best);
  }
}

__global__ void fp_maxmin_unpack_kernel(const fp_u64* __restrict__ slots, int k, int* __restrict__ picked, float* __restrict__ pick_sim) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k) return;
  picked[t] = fp_min_index(slots[t]);
  pick_sim[t] = t == 0 ? -1.0f : fp_packed_sim(slots[t]);
}

static int fp_check_sets(const char* name, const void* a, int na, const void* b, int nb) {
  if (na < 0 || nb < 0) {
    set_error("%s: %d and %d rows", name, na, nb);
    return PG_ERR_ARG;
  }
  if ((na > 0 && !a) || (nb > 0 && !b)) {
    set_error("%s: a null set with %d and %d rows", name, na, nb);
    return PG_ERR_ARG;
  }
  return PG_OK;
}

}  // namespace pg

using namespace pg;

extern "C" int pg_fp_tanimoto(const uint64_t* a, int na, const uint64_t* b, int nb, float* out, void* stream) {
  const int rc = fp_check_sets("pg_fp_tanimoto", a, na, b, nb);
  if (rc != PG_OK) return rc;
  if ((long long)na * nb > 0x7fffffffLL) {
    set_error("pg_fp_tanimoto: %d x %d elements exceed 2^31 - 1; use pg_fp_nearest, or cut the sets", na, nb);
    return PG_ERR_ARG;
  }
  if (na == 0 || nb == 0) return PG_OK;
  if (!out) {
    set_error("pg_fp_tanimoto: a null output for %d x %d elements", na, nb);
    return PG_ERR_ARG;
  }
  const FpSplit sp = fp_split(nb, na, 8 * kNumCU);                // (the rows in registers are B's: fp_core.h)
  hipLaunchKernelGGL(fp_tanimoto_kernel, dim3((unsigned)fp_tiles(nb, kFpTileA), (unsigned)sp.n_split), dim3(kFpTileA), 0,
                     (hipStream_t)stream, reinterpret_cast<const uint4*>(a), na, reinterpret_cast<const uint4*>(b), nb,
                     sp.tiles_per_split, out);
  return check_launch("pg_fp_tanimoto");
}

extern "C" int pg_fp_nearest(const uint64_t* a, int na, const uint64_t* b, int nb, int same, float* sim, int* index, double* sum,
                             void* stream) {
  const int rc = fp_check_sets("pg_fp_nearest", a, na, b, nb);
  if (rc != PG_OK) return rc;
  if (same && (a != b || na != nb)) {
    set_error("pg_fp_nearest: same is set, but the two sets differ (%d and %d rows)", na, nb);
    return PG_ERR_ARG;
  }
  if (na == 0) return PG_OK;
  if (!sim || !index || !sum) {
    set_error("pg_fp_nearest: a null output for %d rows", na);
    return PG_ERR_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;
  const FpSplit sp = fp_split(na, nb, 8 * kNumCU);
  const dim3 grid((unsigned)fp_tiles(na, kFpTileA), (unsigned)sp.n_split);
  const uint4 *a4 = reinterpret_cast<const uint4*>(a), *b4 = reinterpret_cast<const uint4*>(b);
  if (sp.n_split == 1) {
    hipLaunchKernelGGL(fp_nearest_kernel, grid, dim3(kFpTileA), 0, st, a4, na, b4, nb, sp.tiles_per_split, same, sim, index, sum,
                       (fp_u64*)nullptr, (double*)nullptr);
    return check_launch("pg_fp_nearest");
  }
  // the parts of the runs: stream-ordered memory, so no host synchronisation
  const size_t cells = (size_t)sp.n_split * na;
  void* ws = nullptr;
  hipError_t e = hipMallocAsync(&ws, cells * 16, st);
  if (e != hipSuccess) {
    set_error("pg_fp_nearest: %zu bytes for the parts of %d runs: %s", cells * 16, sp.n_split, hipGetErrorString(e));
    return PG_ERR_HIP;
  }
  fp_u64* part_best = static_cast<fp_u64*>(ws);
  double* part_sum = reinterpret_cast<double*>(part_best + cells);
  hipLaunchKernelGGL(fp_nearest_kernel, grid, dim3(kFpTileA), 0, st, a4, na, b4, nb, sp.tiles_per_split, same, sim, index, sum,
                     part_best, part_sum);
  int out = check_launch("pg_fp_nearest");
  if (out == PG_OK) {
    hipLaunchKernelGGL(fp_nearest_combine_kernel, dim3((unsigned)fp_tiles(na, 256)), dim3(256), 0, st, part_best, part_sum, na,
                       sp.n_split, sim, index, sum);
    out = check_launch("pg_fp_nearest (combine)");
  }
  e = hipFreeAsync(ws, st);
  if (e != hipSuccess && out == PG_OK) {
    set_error("pg_fp_nearest: %s", hipGetErrorString(e));
    out = PG_ERR_HIP;
  }
  return out;
}

extern "C" int pg_fp_maxmin(const uint64_t* fp, int n, int k, int first, int* picked, float* pick_sim, float* work, uint64_t* slots,
                            void* stream) {
  if (n < 0 || k < 0 || k > n || (n > 0 && (first < 0 || first >= n))) {
    set_error("pg_fp_maxmin: %d picks from %d rows, first %d (0 <= k <= n, 0 <= first < n)", k, n, first);
    return PG_ERR_ARG;
  }
  if (k == 0) return PG_OK;
  if (!fp || !picked || !pick_sim || !work || !slots) {
    set_error("pg_fp_maxmin: a null array with %d picks from %d rows", k, n);
    return PG_ERR_ARG;
  }
  const hipStream_t st = (hipStream_t)stream;
  fp_u64* sl = reinterpret_cast<fp_u64*>(slots);
  hipLaunchKernelGGL(fp_maxmin_init_kernel, dim3((unsigned)fp_tiles(n, 256)), dim3(256), 0, st, work, n, sl, k, first);
  const int rows_per_block = 256 / kFpRowLanes;
  const int want = fp_tiles(n, rows_per_block), cap = 4 * kNumCU;
  const dim3 grid((unsigned)(want < cap ? want : cap));
  for (int t = 1; t < k; ++t)
    hipLaunchKernelGGL(fp_maxmin_step_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint4*>(fp), n, work, sl + t - 1, sl + t);
  hipLaunchKernelGGL(fp_maxmin_unpack_kernel, dim3((unsigned)fp_tiles(k, 256)), dim3(256), 0, st, sl, k, picked, pick_sim);
  return check_launch("pg_fp_maxmin");
}
