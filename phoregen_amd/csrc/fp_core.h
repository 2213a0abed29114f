// The core of the fingerprints and of the set kernels over them (DESIGN.md 2.9 "Fingerprints and similarity"): where an identifier's
// bit lies, the Tanimoto value of two popcounts, the 64-bit words whose unsigned order is the order the nearest-neighbour search and
// the MaxMin picker reduce by, and the index arithmetic of the tiles.  Plain functions over values, compiled for the device by
// mol_fp.hip and fp_sim.hip and for the host by tools/fp_host_check.cpp (the same text under the host sanitizers).  No arrays, no
// loops: nothing here can index out of bounds.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FP_HD __host__ __device__ inline
#else
#define PG_FP_HD inline
#endif

namespace pg {

typedef unsigned long long fp_u64;

constexpr int kFpBits = 2048;               // bits of a fingerprint (FP_BITS of molecule.py)
constexpr int kFpWords = kFpBits / 64;      // 64-bit words of a row (FP_WORDS)
constexpr int kFpDwords = kFpBits / 32;     // 32-bit words: what a lane of the set kernels holds in registers
constexpr int kFpMaxRadius = 4;             // FP_MAX_RADIUS
// The set kernels: a workgroup of kFpTileA lanes holds one row each in registers and sweeps the other set in LDS tiles of kFpTileB
// rows (similarity.TILE_A / TILE_B).  In pg_fp_nearest the rows in registers are A's, in pg_fp_tanimoto they are B's, so that the
// lanes of a wave write neighbouring elements of an output row.
constexpr int kFpTileA = 256;
constexpr int kFpTileB = 64;
constexpr int kFpRowLanes = 16;             // MaxMin: the lanes that share a row, 16 bytes each
static_assert(kFpTileA % 64 == 0 && kFpTileB % (kFpTileA / kFpRowLanes) == 0, "a workgroup stages kFpTileA / 16 rows per pass");

// ---- fingerprint ------------------------------------------------------------------------------------------------------------------------
// the bit of an identifier: bit (b & 63) of word (b >> 6)
PG_FP_HD int fp_bit(fp_u64 id) { return (int)(id & (fp_u64)(kFpBits - 1)); }
PG_FP_HD int fp_bit_word(int b) { return b >> 6; }
PG_FP_HD fp_u64 fp_bit_mask(int b) { return 1ull << (b & 63); }

// ---- Tanimoto ---------------------------------------------------------------------------------------------------------------------------
// c = popcount(x & y), u = popcount(x | y), 0 <= c <= u <= kFpBits: the fp32 value nearest to c / u (ties to even), 1 for two empty
// rows.  Written as a double division rounded once more: the double quotient is within 2^-52 of c / u, and c / u is either an fp32
// value itself (u a power of two) or at least 1 / (u 2^24) > 2^-37 (relative) away from every midpoint between two fp32 values, so
// the second rounding sees what a single one would.  That holds for any double division that is good to a few ulp, so the value does
// not depend on how the build treats fp32 division.
PG_FP_HD float fp_tanimoto(int c, int u) { return u > 0 ? (float)((double)c / (double)u) : 1.0f; }

// ---- packed (similarity, index) ---------------------------------------------------------------------------------------------------------
// Similarities are fp32 values in [0, 1]: their bit patterns order as the values do.
PG_FP_HD uint32_t fp_float_bits(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return b;
}
PG_FP_HD float fp_bits_float(uint32_t b) {
  float x;
  __builtin_memcpy(&x, &b, 4);
  return x;
}
// MaxMin: the unsigned MINIMUM of these words is the lowest similarity, and among equal ones the lowest index.  kFpMinNone: no candidate.
constexpr fp_u64 kFpMinNone = ~0ull;
PG_FP_HD fp_u64 fp_pack_min(float sim, int index) { return (fp_u64)fp_float_bits(sim) << 32 | (fp_u64)(uint32_t)index; }
PG_FP_HD int fp_min_index(fp_u64 w) { return (int)(uint32_t)(w & 0xffffffffull); }
// Nearest: the unsigned MAXIMUM of these words is the highest similarity, and among equal ones the lowest index.  kFpMaxNone (below
// every word of a candidate, whose low half is at least 2^31): no candidate, read back as similarity -1 and index -1.
constexpr fp_u64 kFpMaxNone = 0ull;
PG_FP_HD fp_u64 fp_pack_max(float sim, int index) { return (fp_u64)fp_float_bits(sim) << 32 | (fp_u64)(0xffffffffu - (uint32_t)index); }
PG_FP_HD int fp_max_index(fp_u64 w) { return w == kFpMaxNone ? -1 : (int)(0xffffffffu - (uint32_t)(w & 0xffffffffull)); }
PG_FP_HD float fp_max_sim(fp_u64 w) { return w == kFpMaxNone ? -1.0f : fp_bits_float((uint32_t)(w >> 32)); }
PG_FP_HD float fp_packed_sim(fp_u64 w) { return fp_bits_float((uint32_t)(w >> 32)); }

// ---- tiles ------------------------------------------------------------------------------------------------------------------------------
PG_FP_HD int fp_tiles(int n, int tile) { return n / tile + (n % tile != 0); }   // (no n + tile - 1: n may be 2^31 - 1)

// The sweep over the n_b rows of the set in LDS is cut into n_split runs of tiles_per_split tiles, one workgroup each per tile of
// the rows in registers, so that about `target` workgroups exist even where that set is small.  Every run has at least one tile;
// n_b = 0 gives one empty run.
struct FpSplit {
  int n_split, tiles_per_split;
};
PG_FP_HD FpSplit fp_split(int n_a, int n_b, int target) {
  const int ta = fp_tiles(n_a, kFpTileA), tb = fp_tiles(n_b, kFpTileB);
  int want = ta > 0 ? target / ta + (target % ta != 0) : 1;
  want = want < 1 ? 1 : want > tb ? tb : want;
  FpSplit s = {1, tb};
  if (want > 1) {
    s.tiles_per_split = tb / want + (tb % want != 0);
    s.n_split = tb / s.tiles_per_split + (tb % s.tiles_per_split != 0);
  }
  return s;
}
// rows [j0, j1) of run `split`
PG_FP_HD void fp_split_rows(int split, int tiles_per_split, int n_b, int& j0, int& j1) {
  const long long lo = (long long)split * tiles_per_split * kFpTileB, hi = lo + (long long)tiles_per_split * kFpTileB;
  j0 = (int)(lo < n_b ? lo : n_b), j1 = (int)(hi < n_b ? hi : n_b);
}
// the row a lane holds, -1 past the end of its set
PG_FP_HD int fp_lane_row(unsigned block, int lane, int n) {
  const long long i = (long long)block * kFpTileA + lane;
  return i < n ? (int)i : -1;
}
// element (i, j) of the [n_a][n_b] matrix
PG_FP_HD size_t fp_matrix_at(int i, int j, int n_b) { return (size_t)i * (size_t)n_b + (size_t)j; }

}  // namespace pg
