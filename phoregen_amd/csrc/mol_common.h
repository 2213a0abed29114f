// What the molecule kernels (mol_screen, mol_key, mol_geom, mol_rings, mol_kekule, mol_feat .hip) share: where a block's graph lies in
// its frame, the walk over the graph's pairs, the kept-bond predicate and adjacency rows, the nearest atom of a point, and the
// argument checks of the entry points.
//
// All six kernels run one wave per (frame, graph): block f * B + g.  A workgroup IS one wave, so __syncthreads() orders the wave's LDS
// traffic, and every loop that holds one (or a vote, or a cross-lane move) must have a wave-uniform trip count: the lane-dependent
// loops here (the pair walk, an atom's neighbours, the points) hold none, and what a kernel passes into them must hold none either.
//
// The index arithmetic (MolFrame, MolPoints, for_each_pair) also compiles for the host: tools/mol_common_host_check.cpp runs the same
// text under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/phoregen_hip.h"

#if defined(__HIPCC__)
#include "common.h"
#define PG_MOL_HD __host__ __device__ __forceinline__
#else
#define PG_MOL_HD inline
#endif

namespace pg {

constexpr int kMolMax = PG_MOL_MAX_ATOMS;   // atoms of the largest graph
constexpr int kMolCh = kMolMax / 64;        // atoms per lane = 64-bit adjacency words per atom
static_assert(kMolCh == 2, "an adjacency row is one 16-byte LDS read; kekule_core.h and feature_core.h walk two mask words per atom");

// ---- the graph of a block ---------------------------------------------------------------------------------------------------------------
// Frame f, graph g; atoms a0 .. a0 + n of the frame's n_lig atom rows, pair rows (a < b, row-major) h0 .. h0 + n_pair of its n_half;
// arow / hrow: the graph's first element in an [F, n_lig] / [F, n_half] array.
struct MolFrame {
  int f, g, a0, n, h0, n_pair;
  size_t arow, hrow;
};

// False for a graph the kernel must not touch: more atoms than the LDS arrays hold, or offsets that leave the frame (the host wrappers
// refuse such a batch; a kernel returns, so that it never indexes past LDS or the frame).  n_lig, n_half >= 0.
PG_MOL_HD bool mol_frame(MolFrame& m, unsigned block, int B, const int* g_lig_off, const int* g_bond_off, int n_lig, int n_half) {
  m.f = (int)(block / (unsigned)B), m.g = (int)(block - (unsigned)m.f * (unsigned)B);
  const int a1 = g_lig_off[m.g + 1];
  m.a0 = g_lig_off[m.g];
  if (m.a0 < 0 || a1 < m.a0) return false;               // (tested before the subtraction: 0 <= a0 <= a1 cannot overflow it)
  m.n = a1 - m.a0;
  if (m.n > kMolMax || m.a0 > n_lig - m.n) return false;
  m.h0 = g_bond_off[m.g] >> 1, m.n_pair = m.n * (m.n - 1) / 2;
  if (m.h0 < 0 || m.h0 > n_half - m.n_pair) return false;
  m.arow = (size_t)m.f * n_lig + m.a0, m.hrow = (size_t)m.f * n_half + m.h0;
  return true;
}

// The graph's points: rows ps .. pe of the n_point points, written to o0 .. o0 + (pe - ps) of the frame's n_out point outputs; orow: the
// first of them in an [F, n_out] array.
struct MolPoints {
  int ps, pe, o0;
  size_t orow;
};

// False for a range that leaves the points, or an output span of another length or outside the frame.  n_point, n_out >= 0.
PG_MOL_HD bool mol_points(MolPoints& q, const MolFrame& m, const int* g_point_range, const int* g_point_out_off, int n_point, int n_out) {
  q.ps = g_point_range[2 * m.g], q.pe = g_point_range[2 * m.g + 1], q.o0 = g_point_out_off[m.g];
  if (q.ps < 0 || q.pe < q.ps || q.pe > n_point || q.o0 < 0 || q.o0 > n_out - (q.pe - q.ps)) return false;
  if (g_point_out_off[m.g + 1] != q.o0 + (q.pe - q.ps)) return false;
  q.orow = (size_t)m.f * n_out + q.o0;
  return true;
}

// ---- the pairs a < b in row-major order, dealt to the lanes: pair p is lane p mod 64's (a wave reads 64 consecutive rows) ---------------
// fn(p, a, b) for p = lane, lane + 64, .. below n_pair = n (n - 1) / 2, with p = a n - a (a + 1) / 2 + (b - a - 1).  The order is part
// of the contract: mol_geom.hip's per-lane floating-point partial sums depend on it.
template <class Fn>
PG_MOL_HD void for_each_pair(int lane, int n, int n_pair, Fn&& fn) {
  int a = 0, b = 1 + lane;
  for (int p = lane; p < n_pair; p += 64, b += 64) {
    while (b >= n) {                                     // next row of the triangle (p < n_pair: ends with a < n - 1)
      ++a;
      b = b - n + a + 1;
    }
    fn(p, a, b);
  }
}

// atom class 0..10, anything else is a dropped atom
PG_MOL_HD int mol_class(int k) { return (k >= 0 && k < 11) ? k : -1; }
// a pair row's order that is a bond (4 = aromatic); the bond is kept if both its atoms are
PG_MOL_HD bool mol_is_bond(int o) { return o >= 1 && o <= 4; }

// the splitmix64 step of the identity key and the fingerprint (`mix` of DESIGN.md 2.9): add the golden gamma, then the finaliser
PG_MOL_HD unsigned long long key_mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

#if defined(__HIPCC__)

__device__ __forceinline__ bool mol_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// An atom's bonds as a bit per local atom index.  Rows are 16 bytes and dense: one row is one 128-bit LDS read, 16 consecutive rows
// fill the 256-byte bank row exactly, so the 16 lanes that share a read cycle collide only where their row indices agree mod 16; the
// searches read rows at data-dependent indices, and for those any padded stride is a permutation of the same residues or worse.
// kekule_core.h and feature_core.h read an array of rows as unsigned long long [2 n] (mol_adj_words).
struct __align__(16) MolAdjRow {
  unsigned long long w[kMolCh];
};
static_assert(sizeof(MolAdjRow) == 16, "dense rows");

__device__ __forceinline__ const unsigned long long* mol_adj_words(const MolAdjRow* adj) { return &adj[0].w[0]; }

// the bond a - b, from any lane (LDS atomics)
__device__ __forceinline__ void mol_adj_set(MolAdjRow* adj, int a, int b) {
  atomicOr(&adj[a].w[b >> 6], 1ull << (b & 63));
  atomicOr(&adj[b].w[a >> 6], 1ull << (a & 63));
}

// fn(j) for every set bit of one mask word, ascending: j = base + the bit's index
template <class Fn>
__device__ __forceinline__ void for_each_bit(unsigned long long m, int base, Fn&& fn) {
  while (m) {
    const int j = base + __builtin_ctzll(m);
    m &= m - 1ull;
    fn(j);
  }
}

// fn(j) for every atom j of a row, ascending
template <class Fn>
__device__ __forceinline__ void for_each_neighbour(const MolAdjRow row, Fn&& fn) {   // (by value: one 16-byte read of an LDS row)
#pragma unroll
  for (int w = 0; w < kMolCh; ++w) for_each_bit(row.w[w], w * 64, fn);
}

// The atom nearest to the point (x, y, z) among s_atom[0 .. n) = (x, y, z, compact index as bits; negative = not kept) for which
// keep(i) holds: its distance (+inf: none) and compact index (-1), and the number of such atoms closer than `clear`.  fp32; the first
// minimum in atom order stays.  Every lane reads one LDS address per step: a broadcast.
template <class Keep>
__device__ __forceinline__ void mol_nearest_atom(const float4* s_atom, int n, float x, float y, float z, float clear, Keep&& keep,
                                                 float& best, int& best_i, int& close) {
  for (int i = 0; i < n; ++i) {
    const float4 pa = s_atom[i];
    const int ci = __float_as_int(pa.w);
    if (ci < 0 || !keep(i)) continue;
    const float dx = pa.x - x, dy = pa.y - y, dz = pa.z - z;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    best_i = d < best ? ci : best_i;                     // (strict: the first minimum in atom order stays)
    best = fminf(best, d);
    close += d < clear;
  }
}

// ---- the entry points' common argument checks -------------------------------------------------------------------------------------------
constexpr int kMolNothing = -1;   // a batch without a frame or a graph: nothing to launch, the entry point returns PG_OK

// PG_OK, PG_ERR_ARG (the message begins with `name`) or kMolNothing.  n_bond counts the directed rows; max_n = the largest graph.
inline int mol_check_batch(const char* name, int B, int F, int n_lig, int n_bond, int max_n) {
  if (B < 0 || F < 0 || n_lig < 0 || n_bond < 0 || (n_bond & 1) || max_n < 0) {
    set_error("%s: B %d, F %d, n_lig %d, n_bond %d, max_n %d (n_bond counts both directions of every pair)", name, B, F, n_lig, n_bond,
              max_n);
    return PG_ERR_ARG;
  }
  if (max_n > PG_MOL_MAX_ATOMS) {
    set_error("%s: a graph of %d atoms, the kernel holds at most PG_MOL_MAX_ATOMS = %d", name, max_n, PG_MOL_MAX_ATOMS);
    return PG_ERR_ARG;
  }
  if ((long long)B * F > 0x7fffffffLL) {
    set_error("%s: %d frames x %d graphs exceed one launch", name, F, B);
    return PG_ERR_ARG;
  }
  return (B == 0 || F == 0) ? kMolNothing : PG_OK;
}

#endif  // __HIPCC__

}  // namespace pg
