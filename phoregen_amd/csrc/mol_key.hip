// Molecule identity keys: a 64-bit key per (frame, graph) that does not depend on the numbering of the atoms, and the per-atom
// colour it is built from (pg_mol_key, include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Identity").
// Reads the screen's outputs (cls, order), not the scores.  One wave per (frame, graph) (mol_common.h); the divergent loops below
// (bond rows, frontier expansion) hold no barrier or vote.  Integer work only, sums wrap at 64 bits, so every output is exact.
#include "mol_common.h"
#include "wave_prims.h"

namespace pg {

constexpr int kKeyMax = kMolMax, kKeyCh = kMolCh;
constexpr int kKeyRow = kKeyMax + 8;        // bytes per row of the pair table: 34 dwords, so the 64-bit reads of 32 lanes (one row each) hit 32 distinct bank pairs
constexpr int kKeyRounds = 3;               // refinement rounds (KEY_ROUNDS of molecule.py)
static_assert(kKeyMax % 64 == 0 && kKeyMax <= 128, "a pair code holds a hop distance below 128 or 128 + bond order in one byte");

__global__ __launch_bounds__(64) void mol_key_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                     const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
                                                     int n_lig, int n_half, long long* __restrict__ key_o,
                                                     long long* __restrict__ colour_o) {
  __shared__ int s_cls[kKeyMax];                                  // atom class, -1 = dropped
  __shared__ MolAdjRow s_adj[kKeyMax];                            // kept bonds of an atom
  __shared__ unsigned int s_stat[kKeyMax];                        // valence2 | degree << 16 | aromatic bonds << 24 (the screen's word)
  // pair code of (i, j): 128 + order for a bond (hop distance 1), the hop distance 2..127 otherwise, 255 = no path
  __shared__ __align__(8) unsigned char s_pair[kKeyMax][kKeyRow];
  __shared__ unsigned long long s_word[256];                      // pair code -> mix(distance | order << 8)
  __shared__ unsigned long long s_col[2][kKeyMax];                // colours of the previous / the current round

  const int lane = threadIdx.x;
  MolFrame m;
  if (!mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half)) return;
  const int n = m.n;
  const size_t arow = m.arow, hrow = m.hrow;

  // ---- atoms: class; empty adjacency, counters and pair rows; the table of pair words ----------------------------------------
  int n_kept = 0;
#pragma unroll
  for (int c = 0; c < kKeyCh; ++c) {
    const int i = c * 64 + lane;
    int k = -1;
    if (i < n) {
      s_cls[i] = k = mol_class(cls_i[arow + i]);
      s_stat[i] = 0u;
#pragma unroll
      for (int w = 0; w < kKeyCh; ++w) s_adj[i].w[w] = 0ull;
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

  // ---- bonds ------------------------------------------------------------------------------------------------------------------
  int n_bond = 0;
  for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
    const int o = order_i[hrow + p];
    if (mol_is_bond(o) && s_cls[a] >= 0 && s_cls[b] >= 0) {
      ++n_bond;
      const unsigned int inc = (o == 4 ? 3u : 2u * o) | (1u << 16) | (o == 4 ? 1u << 24 : 0u);
      atomicAdd(&s_stat[a], inc);
      atomicAdd(&s_stat[b], inc);
      mol_adj_set(s_adj, a, b);
      s_pair[a][b] = s_pair[b][a] = (unsigned char)(128 + o);
    }
  });
  __syncthreads();

  // ---- hop distances: a lane expands the frontier of its own atoms over the adjacency masks and writes its own rows --------
#pragma unroll
  for (int c = 0; c < kKeyCh; ++c) {
    const int i = c * 64 + lane;
    if (i < n && s_cls[i] >= 0) {
      MolAdjRow front = s_adj[i];
      unsigned long long seen[kKeyCh];
      bool more = false;
#pragma unroll
      for (int w = 0; w < kKeyCh; ++w) {
        seen[w] = front.w[w] | (w == (i >> 6) ? 1ull << (i & 63) : 0ull);
        more |= front.w[w] != 0ull;
      }
      for (int d = 2; more; ++d) {
        MolAdjRow next = {};
        for_each_neighbour(front, [&](int j) {
#pragma unroll
          for (int v = 0; v < kKeyCh; ++v) next.w[v] |= s_adj[j].w[v];
        });
        more = false;
#pragma unroll
        for (int w = 0; w < kKeyCh; ++w) {
          next.w[w] &= ~seen[w];
          seen[w] |= next.w[w];
          more |= next.w[w] != 0ull;
        }
        for_each_neighbour(next, [&](int j) { s_pair[i][j] = (unsigned char)d; });   // d <= n - 1 < 128
        front = next;
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
  acc = wave_sum(acc);
  const unsigned long long nb = wave_sum((unsigned long long)n_bond);
  if (lane == 0) key_o[blockIdx.x] = (long long)key_mix(acc ^ ((unsigned long long)n_kept | nb << 16));
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_key(const int8_t* cls, const int8_t* order, const int* g_lig_off, const int* g_bond_off, int B, int F,
                          int n_lig, int n_bond, int max_n, int64_t* key, int64_t* colour, void* stream) {
  const int rc = mol_check_batch("pg_mol_key", B, F, n_lig, n_bond, max_n);
  if (rc != PG_OK) return rc == kMolNothing ? PG_OK : rc;
  hipLaunchKernelGGL(mol_key_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, reinterpret_cast<long long*>(key), reinterpret_cast<long long*>(colour));
  return check_launch("pg_mol_key");
}
