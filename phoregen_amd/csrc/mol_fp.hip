// Circular fingerprints: 2048 bits per (frame, graph), one for every (kept atom, radius 0..R) environment identifier (pg_mol_fp,
// include/phoregen_hip.h; phoregen_amd/molecule.py; definition: DESIGN.md 2.9 "Fingerprints and similarity").  Reads the screen's
// outputs (cls, order) as mol_key.hip does.  One wave per (frame, graph) (mol_common.h); the divergent loops below (bond rows, an
// atom's neighbours) hold no barrier or vote.  Integer work only, sums wrap at 64 bits, so every output is exact.
#include "fp_core.h"
#include "mol_common.h"
#include "wave_prims.h"

namespace pg {

constexpr int kFpAtomMax = kMolMax, kFpCh = kMolCh;
constexpr int kFpOrdRow = kFpAtomMax + 4;   // bytes per row of the bond-order table: 33 dwords, so a column walk moves one bank per row

__global__ __launch_bounds__(64) void mol_fp_kernel(const int8_t* __restrict__ cls_i, const int8_t* __restrict__ order_i,
                                                    const int* __restrict__ g_lig_off, const int* __restrict__ g_bond_off, int B,
                                                    int n_lig, int n_half, int radius, unsigned long long* __restrict__ fp_o,
                                                    int* __restrict__ bits_o) {
  __shared__ int s_cls[kFpAtomMax];                               // atom class, -1 = dropped
  __shared__ MolAdjRow s_adj[kFpAtomMax];                         // kept bonds of an atom
  __shared__ unsigned int s_stat[kFpAtomMax];                     // valence2 | degree << 16 | aromatic bonds << 24 (the key's word)
  __shared__ unsigned char s_ord[kFpAtomMax][kFpOrdRow];          // order of the kept bond (i, j); read only where s_adj has the bit
  __shared__ unsigned long long s_id[2][kFpAtomMax];              // identifiers of the previous / the current radius
  __shared__ unsigned long long s_fp[kFpWords];

  const int lane = threadIdx.x;
  if (lane < kFpWords) s_fp[lane] = 0ull;
  MolFrame m;
  const bool ok = mol_frame(m, blockIdx.x, B, g_lig_off, g_bond_off, n_lig, n_half);   // (wave-uniform)
  if (ok) {
    const int n = m.n;
    const size_t arow = m.arow, hrow = m.hrow;
#pragma unroll
    for (int c = 0; c < kFpCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n) {
        s_cls[i] = mol_class(cls_i[arow + i]);
        s_stat[i] = 0u;
#pragma unroll
        for (int w = 0; w < kFpCh; ++w) s_adj[i].w[w] = 0ull;
      }
    }
    __syncthreads();

    for_each_pair(lane, n, m.n_pair, [&](int p, int a, int b) {
      const int o = order_i[hrow + p];
      if (mol_is_bond(o) && s_cls[a] >= 0 && s_cls[b] >= 0) {
        const unsigned int inc = (o == 4 ? 3u : 2u * o) | (1u << 16) | (o == 4 ? 1u << 24 : 0u);
        atomicAdd(&s_stat[a], inc);
        atomicAdd(&s_stat[b], inc);
        mol_adj_set(s_adj, a, b);
        s_ord[a][b] = s_ord[b][a] = (unsigned char)o;
      }
    });
    __syncthreads();

    // radius 0: the key's initial colour word
#pragma unroll
    for (int c = 0; c < kFpCh; ++c) {
      const int i = c * 64 + lane;
      if (i < n && s_cls[i] >= 0) {
        const unsigned long long id = key_mix((unsigned long long)s_cls[i] | (unsigned long long)s_stat[i] << 8);
        s_id[0][i] = id;
        const int b = fp_bit(id);
        atomicOr(&s_fp[fp_bit_word(b)], fp_bit_mask(b));
      }
    }
    __syncthreads();

    for (int r = 1; r <= radius; ++r) {                           // (wave-uniform)
      const unsigned long long* cur = s_id[(r - 1) & 1];
#pragma unroll
      for (int c = 0; c < kFpCh; ++c) {
        const int i = c * 64 + lane;
        if (i < n && s_cls[i] >= 0) {
          unsigned long long sum = 0ull;
          for_each_neighbour(s_adj[i], [&](int j) { sum += key_mix(cur[j] ^ key_mix((unsigned long long)s_ord[i][j])); });
          const unsigned long long id = key_mix(cur[i] ^ key_mix(sum));
          s_id[r & 1][i] = id;
          const int b = fp_bit(id);
          atomicOr(&s_fp[fp_bit_word(b)], fp_bit_mask(b));
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  // a graph the kernel must not touch (the entry point refuses such a batch) still gets a whole row: all zero
  const unsigned long long w = lane < kFpWords ? s_fp[lane] : 0ull;
  if (lane < kFpWords) fp_o[(size_t)blockIdx.x * kFpWords + lane] = w;
  const int bits = wave_sum(__popcll(w));
  if (lane == 0) bits_o[blockIdx.x] = bits;
}

}  // namespace pg

using namespace pg;

extern "C" int pg_mol_fp(const int8_t* cls, const int8_t* order, const int* g_lig_off, const int* g_bond_off, int B, int F, int n_lig,
                         int n_bond, int max_n, int radius, uint64_t* fp, int* bits, void* stream) {
  const int rc = mol_check_batch("pg_mol_fp", B, F, n_lig, n_bond, max_n);
  if (rc != PG_OK && rc != kMolNothing) return rc;
  if (radius < 0 || radius > kFpMaxRadius) {
    set_error("pg_mol_fp: radius %d, the fingerprint takes 0 .. %d", radius, kFpMaxRadius);
    return PG_ERR_ARG;
  }
  if (rc == kMolNothing) return PG_OK;
  if ((n_lig > 0 && !cls) || !g_lig_off || !g_bond_off || !fp || !bits || (n_bond > 0 && !order)) {
    set_error("pg_mol_fp: a null array with %d frames x %d graphs", F, B);
    return PG_ERR_ARG;
  }
  hipLaunchKernelGGL(mol_fp_kernel, dim3((unsigned)(B * F)), dim3(64), 0, (hipStream_t)stream, cls, order, g_lig_off, g_bond_off, B,
                     n_lig, n_bond / 2, radius, reinterpret_cast<unsigned long long*>(fp), bits);
  return check_launch("pg_mol_fp");
}
