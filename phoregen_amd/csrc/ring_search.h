// The search of the smallest ring through a bond, the one copy that mol_rings.hip (every bond's ring size) and mol_scaffold.hip (ring
// bond or bridge) share.  Written over rows of kMolCh mask words (MolAdjRow on the device), so that it also compiles for the host:
// tools/scaffold_host_check.cpp runs the same text under the host sanitizers.  It is lane-dependent and holds no barrier or vote.
#pragma once
#include "mol_common.h"

namespace pg {

// Atoms of the smallest ring through the bond (a, b), 0 if the bond is a bridge: breadth-first from a over the masks with b struck
// from a's own row (a is never expanded again, so the bond itself is never walked); the frontier at step d holds the atoms d bonds
// from a, and the first of them that has b as a neighbour closes a ring of d + 2 atoms.  (The walk over the frontier's bits is written
// out: it returns from inside.)  Row: kMolCh words `w`, bit j & 63 of w[j >> 6] = a bond to atom j.
template <class Row>
PG_MOL_HD int ring_through(const Row* adj, int a, int b) {
  const int bw = b >> 6;
  const unsigned long long bbit = 1ull << (b & 63);
  unsigned long long seen[kMolCh], front[kMolCh];
  const Row ra = adj[a];
  bool more = false;
#pragma unroll
  for (int w = 0; w < kMolCh; ++w) {
    front[w] = ra.w[w] & ~(w == bw ? bbit : 0ull);
    seen[w] = front[w] | (w == (a >> 6) ? 1ull << (a & 63) : 0ull);
    more |= front[w] != 0ull;
  }
  for (int d = 1; more; ++d) {                                    // (d <= n - 2: every step adds an atom to `seen`)
    unsigned long long next[kMolCh];
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) next[w] = 0ull;
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) {
      unsigned long long m = front[w];
      while (m) {
        const int j = w * 64 + __builtin_ctzll(m);
        m &= m - 1ull;
        const Row rj = adj[j];
#pragma unroll
        for (int v = 0; v < kMolCh; ++v) next[v] |= rj.w[v];
        if ((bw ? next[kMolCh - 1] : next[0]) & bbit) return d + 2;
      }
    }
    more = false;
#pragma unroll
    for (int w = 0; w < kMolCh; ++w) {
      next[w] &= ~seen[w];
      seen[w] |= next[w];
      front[w] = next[w];
      more |= next[w] != 0ull;
    }
  }
  return 0;
}

}  // namespace pg
