// Molecule identity keys: a 64-bit key per (frame, graph) that does not depend on the numbering of the atoms, and the per-atom
// colour it is built from (pg_mol_key, include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Identity").
// Reads the screen's outputs (cls, order), not the scores.  One wave per (frame, graph); a workgroup IS one wave, so __syncthreads()
// orders the wave's LDS traffic, and every loop that holds one (or a vote) has a wave-uniform trip count: the divergent loops below
// (bond rows, frontier expansion) hold neither.  Integer work only, sums wrap at 64 bits, so every output is exact.
#include "common.h"
#include "../../include/phoregen_hip.h"

namespace pg {

constexpr int kKeyMax = PG_MOL_MAX_ATOMS;   // atoms of the largest graph
constexpr int kKeyCh = kKeyMax / 64;        // atoms per lane = 64-bit adjacency words per atom
constexpr int kKeyRow = kKeyMax + 8;        // bytes per row of the pair table: 34 dwords, so the 64-bit reads of 32 lanes (one row each) hit 32 distinct bank pairs
constexpr int kKeyRounds = 3;               // refinement rounds (KEY_ROUNDS of molecule.py)
static_assert(kKeyMax % 64 == 0 && kKeyMax <= 128, "a pair code holds a hop distance below 128 or 128 + bond order in one byte");

// the splitmix64 step: add the golden gamma, then the finaliser
__device__ __forceinline__ unsigned long long key_mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long wave_usum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(64) void mol_key_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                     const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
                                                     int n_lig, int n_half, long long* __restrict__ key_o,
                                                     long long* __restrict__ colour_o) {
  __shared__ int s_cls[kKeyMax];                                  // atom class, -1 = dropped
  __shared__ unsigned long long s_adj[kKeyMax][kKeyCh];           // kept bonds of an atom as a bit per local atom index
  __shared__ unsigned int s_stat[kKeyMax];                        // valence2 | degree << 16 | aromatic bonds << 24 (the screen's word)
  // pair code of (i, j): 128 + order for a bond (hop distance 1), the hop distance 2..127 otherwise, 255 = no path
  __shared__ __align__(8) unsigned char s_pair[kKeyMax][kKeyRow];
  __shared__ unsigned long long s_word[256];                      // pair code -> mix(distance | order << 8)
  __shared__ unsigned long long s_col[2][kKeyMax];                // colours of the previous / the current round

  const int lane = threadIdx.x;
  const int f = blockIdx.x / B, g = blockIdx.x - f * B;
  const int a0 = g_lig_off[g], n = g_lig_off[g + 1] - a0;
  if (n > kKeyMax || n < 0) return;                               // (the host wrapper has refused such a batch: never index LDS past its end)
  const int h0 = g_bond_off[g] >> 1, n_pair = n * (n - 1) / 2;
  if (a0 < 0 || a0 + n > n_lig || h0 < 0 || h0 + n_pair > n_half) return;   // (offsets that leave the frame: never read past it)
  const size_t arow = (size_t)f * n_lig + a0, hrow = (size_t)f * n_half + h0;

  // ---- atoms: class; empty adjacency, counters and pair rows; the table of pair words ----------------------------------------
  int n_kept = 0;
#pragma unroll
  for (int c = 0; c < kKeyCh; ++c) {
    const int i = c * 64 + lane;
    int k = -1;
    if (i < n) {
      k = cls_i[arow + i];
      k = (k >= 0 && k < 11) ? k : -1;
      s_cls[i] = k;
      s_stat[i] = 0u;
#pragma unroll
      for (int w = 0; w < kKeyCh; ++w) s_adj[i][w] = 0ull;
      unsigned long long* row = reinterpret_cast<unsigned long long*>(&s_pair[i][0]);
#pragma unroll
      for (int q = 0; q < kKeyRow / 8; ++q) row[q] = ~0ull;
    }
    n_kept += __popcll(__ballot(k >= 0));
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned int e = q * 64 + lane;
    s_word[e] = key_mix((e > 128u && e <= 132u) ? (1u | (e - 128u) << 8) : e);
  }
  __syncthreads();

  // ---- bonds: the pairs a < b in row-major order, lane-strided (a wave reads 64 consecutive rows) ---------------------------
  int n_bond = 0;
  {
    int a = 0, b = 1 + lane;
    for (int p = lane; p < n_pair; p += 64, b += 64) {
      while (b >= n) {                                            // next row of the triangle (p < n_pair: ends with a < n - 1)
        ++a;
        b = b - n + a + 1;
      }
      const int o = order_i[hrow + p];
      if (o >= 1 && o <= 4 && s_cls[a] >= 0 && s_cls[b] >= 0) {
        ++n_bond;
        const unsigned int inc = (o == 4 ? 3u : 2u * o) | (1u << 16) | (o == 4 ? 1u << 24 : 0u);
        atomicAdd(&s_stat[a], inc);
        atomicAdd(&s_stat[b], inc);
        atomicOr(&s_adj[a][b >> 6], 1ull << (b & 63));
        atomicOr(&s_adj[b][a >> 6], 1ull << (a & 63));
        s_pair[a][b] = s_pair[b][a] = (unsigned char)(128 + o);
      }
    }
  }
  __syncthreads();

  // ---- hop distances: a lane expands the frontier of its own atoms over the adjacency masks and writes its own rows --------
#pragma unroll
  for (int c = 0; c < kKeyCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n && s_cls[i] >= 0) {
      unsigned long long seen[kKeyCh], front[kKeyCh];
      bool more = false;
#pragma unroll
      for (int w = 0; w < kKeyCh; ++w) {
        front[w] = s_adj[i][w];
        seen[w] = front[w] | (w == (i >> 6) ? 1ull << (i & 63) : 0ull);
        more |= front[w] != 0ull;
      }
      for (int d = 2; more; ++d) {
        unsigned long long next[kKeyCh];
#pragma unroll
        for (int w = 0; w < kKeyCh; ++w) next[w] = 0ull;
#pragma unroll
        for (int w = 0; w < kKeyCh; ++w) {
          unsigned long long m = front[w];
          while (m) {
            const int j = w * 64 + __builtin_ctzll(m);
            m &= m - 1ull;
#pragma unroll
            for (int v = 0; v < kKeyCh; ++v) next[v] |= s_adj[j][v];
          }
        }
        more = false;
#pragma unroll
        for (int w = 0; w < kKeyCh; ++w) {
          next[w] &= ~seen[w];
          seen[w] |= next[w];
          front[w] = next[w];
          more |= next[w] != 0ull;
          unsigned long long m = next[w];
          while (m) {
            const int j = w * 64 + __builtin_ctzll(m);
            m &= m - 1ull;
            s_pair[i][j] = (unsigned char)d;                      // d <= n - 1 < 128
          }
        }
      }
    }
  }

  // ---- colours: the initial one from the atom's own counters, then kKeyRounds rounds over all pairs ------------------------
#pragma unroll
  for (int c = 0; c < kKeyCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) s_col[0][i] = s_cls[i] >= 0 ? key_mix((unsigned long long)s_cls[i] | (unsigned long long)s_stat[i] << 8) : 0ull;
  }
  __syncthreads();
  for (int r = 0; r < kKeyRounds; ++r) {
    const unsigned long long* cur = s_col[r & 1];
#pragma unroll
    for (int c = 0; c < kKeyCh; ++c) {
      if (c * 64 < n) {                                           // (wave-uniform)
        const int i = c * 64 + lane;
        const bool active = i < n && s_cls[i] >= 0;
        const int ir = active ? i : 0;                            // idle lanes read row 0 and drop the result
        unsigned long long sum = 0ull;
        for (int j0 = 0; j0 < n; j0 += 8) {
          const unsigned long long e8 = *reinterpret_cast<const unsigned long long*>(&s_pair[ir][j0]);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int j = j0 + q;
            if (j < n && s_cls[j] >= 0) {                         // (wave-uniform)
              const unsigned long long t = key_mix(cur[j] ^ s_word[(e8 >> (8 * q)) & 255ull]);
              sum += j != ir ? t : 0ull;
            }
          }
        }
        if (i < n) s_col[(r & 1) ^ 1][i] = active ? key_mix(cur[i] ^ key_mix(sum)) : 0ull;
      }
    }
    __syncthreads();
  }

  // ---- outputs ---------------------------------------------------------------------------------------------------------------
  const unsigned long long* fin = s_col[kKeyRounds & 1];
  unsigned long long acc = 0ull;
#pragma unroll
  for (int c = 0; c < kKeyCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n) {
      const bool kept = s_cls[i] >= 0;
      acc += kept ? key_mix(fin[i]) : 0ull;
      if (colour_o) colour_o[arow + i] = (long long)(kept ? fin[i] : 0ull);
    }
  }
  acc = wave_usum64(acc);
  const unsigned long long nb = wave_usum64((unsigned long long)n_bond);
  if (lane == 0) key_o[blockIdx.x] = (long long)key_mix(acc ^ ((unsigned long long)n_kept | nb << 16));
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_key(const int8_t* cls, const int8_t* order, const int* g_lig_off, const int* g_bond_off, int B, int F,
                          int n_lig, int n_bond, int max_n, int64_t* key, int64_t* colour, void* stream) {
  if (B < 0 || F < 0 || n_lig < 0 || n_bond < 0 || (n_bond & 1) || max_n < 0) {
    set_error("pg_mol_key: B %d, F %d, n_lig %d, n_bond %d, max_n %d (n_bond counts both directions of every pair)", B, F, n_lig,
              n_bond, max_n);
    return PG_ERR_ARG;
  }
  if (max_n > PG_MOL_MAX_ATOMS) {
    set_error("pg_mol_key: a graph of %d atoms, the kernel holds at most PG_MOL_MAX_ATOMS = %d", max_n, PG_MOL_MAX_ATOMS);
    return PG_ERR_ARG;
  }
  if (B == 0 || F == 0) return PG_OK;
  if ((long long)B * F > 0x7fffffffLL) {
    set_error("pg_mol_key: %d frames x %d graphs exceed one launch", F, B);
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_key_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, reinterpret_cast<long long*>(key), reinterpret_cast<long long*>(colour));
  return check_launch("pg_mol_key");
}
