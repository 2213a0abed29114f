// The stereo cores (phoregen_amd/csrc/stereo_core.h: the rules and the arithmetic the kernel of csrc/mol_stereo.hip compiles for the
// device; csrc/smiles_core.h: the stereo marks and the atom text of pg_mol_smiles_stereo) compiled for the host together with
// mol_common.h's host part, so that they can run under the host sanitizers and be held against the tests' restatement without a GPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stereo_host_check.cpp -o stereo_host_check
//   ./stereo_host_check cases.txt > results.txt
//
// (tests/stereo_reference.py writes the cases and reads the results; tests/test_molstereo_host.py does all three steps.)
//
// cases.txt: one line with the notation's valence table (44 numbers), one line `vol_min planar_min max_undefined` (the floats in C's
// hexadecimal form), then per case a line `n capacity kekule_status n_rows key given`, n lines `class hydrogens charge colour x y z
// parity` and n_rows lines `a b order kekule_order ring_size stereo` (a < b).  With given = 0 the text is written from what the
// program perceived; with given = 1 from the parity and stereo columns.  Per case six lines come out: `status stereo_key` and the
// eight counts; the n pairs `atom_parity atom_label`; the n_rows pairs `bond_stereo bond_label`; `status length`, the eight counts
// and the four stereo counts of the text; the text; the n ranks.  The program follows the kernels step by step: atoms one by one,
// the pairs dealt by for_each_pair lane by lane; the work arrays are exactly as large as the cores' contracts say.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phoregen_amd/csrc/mol_common.h"
#include "../phoregen_amd/csrc/smiles_core.h"
#include "../phoregen_amd/csrc/stereo_core.h"

typedef unsigned long long u64;

static bool read_float(std::FILE* fh, float* x) {
  char word[64];
  if (std::fscanf(fh, "%63s", word) != 1) return false;
  *x = std::strtof(word, nullptr);
  return true;
}

// the lowest neighbour of a row, struck from it; -1 if it is empty
static int take_lowest(u64* row) {
  const int j = pg::smi_lowest(row[0], row[1]);
  if (j >= 0) row[j >> 6] &= ~(1ull << (j & 63));
  return j;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> val(4 * pg::kSmiEl);
  for (auto& t : val) {
    int x;
    if (std::fscanf(fh, "%d", &x) != 1 || x < 0 || x > 255) return 3;
    t = (uint8_t)x;
  }
  float vol_min, planar_min;
  int max_undefined;
  if (!read_float(fh, &vol_min) || !read_float(fh, &planar_min) || std::fscanf(fh, "%d", &max_undefined) != 1) return 3;
  int n, capacity, kstatus, n_rows, given;
  u64 key;
  while (std::fscanf(fh, "%d %d %d %d %llu %d", &n, &capacity, &kstatus, &n_rows, &key, &given) == 6) {
    if (n < 0 || n > pg::kMolMax || capacity < 1 || n_rows < 0) return 3;
    const int n_pair = n * (n - 1) / 2;
    std::vector<int> cls(n), h(n), q(n), parity_in(n);
    std::vector<u64> col(n);
    std::vector<pg::StereoVec> pos(n);
    for (int i = 0; i < n; ++i) {
      if (std::fscanf(fh, "%d %d %d %llu", &cls[i], &h[i], &q[i], &col[i]) != 4 || cls[i] < -1 || cls[i] > 10 || h[i] < 0 || h[i] > 255) return 3;
      if (!read_float(fh, &pos[i].x) || !read_float(fh, &pos[i].y) || !read_float(fh, &pos[i].z)) return 3;
      if (std::fscanf(fh, "%d", &parity_in[i]) != 1) return 3;
    }
    std::vector<int8_t> order(n_pair, 0), kek(n_pair, 0), stereo_in(n_pair, 0);
    std::vector<uint8_t> ring(n_pair, 0);
    std::vector<int> listed(n_rows);
    for (int r = 0; r < n_rows; ++r) {
      int a, b, o, k, rs, s;
      if (std::fscanf(fh, "%d %d %d %d %d %d", &a, &b, &o, &k, &rs, &s) != 6 || a < 0 || a >= b || b >= n || rs < 0 || rs > 255) return 3;
      const int p = listed[r] = pg::smi_pair(n, a, b);
      order[p] = (int8_t)o, kek[p] = (int8_t)k, ring[p] = (uint8_t)rs, stereo_in[p] = (int8_t)s;
    }

    // ==== perception, as mol_stereo.hip does it ====
    std::vector<int8_t> parity(n, 0), alabel(n, 0), bstereo(n_pair, 0), blabel(n_pair, 0);
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, status = 0;
    u64 skey = key;
    if (kstatus & PG_KEKULE_FAILED) {
      status = PG_STEREO_NO_KEKULE;
    } else {
      std::vector<u64> adj(2 * n, 0ull);
      std::vector<int> multi(n, 0);
      bool bad = false;
      for (int i = 0; i < n; ++i) bad |= cls[i] >= 0 && !(pos[i].x - pos[i].x == 0.0f && pos[i].y - pos[i].y == 0.0f && pos[i].z - pos[i].z == 0.0f);
      for (int lane = 0; lane < 64; ++lane)
        pg::for_each_pair(lane, n, n_pair, [&](int p, int a, int b) {
          if (pg::mol_is_bond(order[p]) && cls[a] >= 0 && cls[b] >= 0) {
            adj[2 * a + (b >> 6)] |= 1ull << (b & 63), adj[2 * b + (a >> 6)] |= 1ull << (a & 63);
            if (kek[p] >= 2) ++multi[a], ++multi[b];
          }
        });
      u64 sum = 0ull;
      for (int i = 0; i < n; ++i) {
        u64 row[2] = {adj[2 * i], adj[2 * i + 1]};
        const int degree = pg::smi_popc64(row[0]) + pg::smi_popc64(row[1]);
        if (cls[i] < 0 || !pg::stereo_centre_candidate(cls[i], degree, h[i])) continue;
        ++cnt[0];
        const int n0 = take_lowest(row), n1 = take_lowest(row), n2 = take_lowest(row);
        const bool four = degree == 4;
        const int n3 = four ? take_lowest(row) : n2;
        const int sign = pg::stereo_sort_sign(col[n0], col[n1], col[n2], col[n3], four ? 4 : 3);
        if (sign == 0) continue;
        ++cnt[1];
        const int par = pg::stereo_centre_parity(pos[i], pos[n0], pos[n1], pos[n2], pos[n3], four, vol_min);
        parity[i] = (int8_t)par;
        alabel[i] = (int8_t)(par == pg::kStereoUndefined ? par : par * sign);
        if (par == pg::kStereoUndefined) {
          ++cnt[3];
        } else {
          ++cnt[2];
          sum += pg::stereo_centre_word(col[i], alabel[i]);
        }
      }
      for (int lane = 0; lane < 64; ++lane)
        pg::for_each_pair(lane, n, n_pair, [&](int p, int a, int b) {
          const int o = order[p];
          if (!(o >= 1 && o <= 3 && kek[p] == 2 && ring[p] == 0 && cls[a] >= 0 && cls[b] >= 0)) return;
          u64 ra[2] = {adj[2 * a], adj[2 * a + 1]}, rb[2] = {adj[2 * b], adj[2 * b + 1]};
          const int deg_a = pg::smi_popc64(ra[0]) + pg::smi_popc64(ra[1]), deg_b = pg::smi_popc64(rb[0]) + pg::smi_popc64(rb[1]);
          if (!pg::stereo_bond_end(deg_a, multi[a], h[a]) || !pg::stereo_bond_end(deg_b, multi[b], h[b])) return;
          ++cnt[4];
          ra[b >> 6] &= ~(1ull << (b & 63));
          rb[a >> 6] &= ~(1ull << (a & 63));
          const int a0 = take_lowest(ra), a1 = take_lowest(ra), b0 = take_lowest(rb), b1 = take_lowest(rb);
          const u64 ca0 = col[a0], ca1 = a1 >= 0 ? col[a1] : 0ull, cb0 = col[b0], cb1 = b1 >= 0 ? col[b1] : 0ull;
          if (!((a1 < 0 || ca0 != ca1) && (b1 < 0 || cb0 != cb1))) return;
          ++cnt[5];
          const int st = pg::stereo_bond_side(pos[a], pos[b], pos[a0], pos[b0], planar_min);
          bstereo[p] = (int8_t)st;
          if (st == pg::kStereoUndefined) {
            ++cnt[7];
            blabel[p] = (int8_t)st;
          } else {
            ++cnt[6];
            blabel[p] = (int8_t)(st * pg::stereo_end_factor(ca0, a1 >= 0, ca1, h[a]) * pg::stereo_end_factor(cb0, b1 >= 0, cb1, h[b]));
            sum += pg::stereo_bond_word(col[a], col[b], blabel[p]);
          }
        });
      status |= cnt[3] + cnt[7] > max_undefined ? PG_STEREO_UNDEFINED : 0;
      status |= cnt[2] > 0 ? PG_STEREO_HAS_CENTRE : 0;
      status |= cnt[6] > 0 ? PG_STEREO_HAS_BOND : 0;
      status |= bad ? PG_STEREO_NONFINITE : 0;
      if (cnt[2] + cnt[6] > 0) skey = pg::stereo_key(key, sum);
    }
    std::printf("%d %llu", status, skey);
    for (int c : cnt) std::printf(" %d", c);
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%d %d ", (int)parity[i], (int)alabel[i]);
    std::printf("\n");
    for (int p : listed) std::printf("%d %d ", (int)bstereo[p], (int)blabel[p]);
    std::printf("\n");

    // ==== the isomeric text, as mol_smiles.hip does it with kStereo ====
    const std::vector<int8_t>& bs = given ? stereo_in : bstereo;
    std::vector<int> par(n);
    for (int i = 0; i < n; ++i) par[i] = given ? parity_in[i] : (int)parity[i];
    std::vector<uint8_t> text(capacity, 0xAA);
    std::vector<int16_t> rank(n, -1), ord(n), parent(n, -1), stack(n), partner(n, -1);
    std::vector<int8_t> sval(n, 0);
    std::vector<uint8_t> flags(n, 0), label(n_pair), mark(n_pair, 0);
    std::vector<int> len(n, 0), scnt(8, 0), stc(4, 0);
    int sstatus = 0, length = 0;
    if (kstatus & PG_KEKULE_FAILED) {
      sstatus = PG_SMILES_NO_KEKULE;
      for (auto& t : text) t = 0;
    } else {
      std::vector<u64> p0(2 * n, 0ull), p1(2 * n, 0ull);
      u64 kept[2] = {0ull, 0ull};
      int n_kept = 0, n_bond = 0;
      for (int i = 0; i < n; ++i)
        if (pg::mol_class(cls[i]) >= 0) {
          kept[i >> 6] |= 1ull << (i & 63);
          ++n_kept;
        }
      for (int lane = 0; lane < 64; ++lane)
        pg::for_each_pair(lane, n, n_pair, [&](int p, int a, int b) {
          const int o = kek[p];
          if (o >= 1 && o <= 3 && cls[a] >= 0 && cls[b] >= 0) {
            ++n_bond;
            if (o & 1) p0[2 * a + (b >> 6)] |= 1ull << (b & 63), p0[2 * b + (a >> 6)] |= 1ull << (a & 63);
            if (o & 2) p1[2 * a + (b >> 6)] |= 1ull << (b & 63), p1[2 * b + (a >> 6)] |= 1ull << (a & 63);
          }
        });
      for (int lane = 0; lane < 64; ++lane)
        pg::for_each_pair(lane, n, n_pair, [&](int p, int a, int b) {
          if (cls[a] >= 0 && cls[b] >= 0 && pg::smi_stereo_bond_ok(bs[p], p0.data(), p1.data(), a, b)) {
            partner[a] = (int16_t)b, partner[b] = (int16_t)a;
            sval[a] = sval[b] = bs[p];
          }
        });
      int comps = 0, branches = 0, closures = 0;
      const int seen = pg::smiles_tree(n, p0.data(), p1.data(), kept[0], kept[1], rank.data(), ord.data(), parent.data(), flags.data(),
                                       stack.data(), &comps, &branches);
      if (seen != n_kept) return 4;
      const int max_label = pg::smiles_labels(n, seen, p0.data(), p1.data(), rank.data(), ord.data(), parent.data(), label.data(), &closures);
      if (max_label == pg::kSmiLabelOverflow) {
        sstatus = PG_SMILES_RING_LABELS;
        for (auto& t : text) t = 0;
        for (auto& r : rank) r = -1;
      } else {
        int marked = 0, expressed = 0;
        const int dropped = pg::smiles_stereo_marks(n, seen, p0.data(), p1.data(), rank.data(), ord.data(), parent.data(), partner.data(),
                                                    sval.data(), mark.data(), stack.data(), &marked, &expressed);
        int n_bracket = 0, n_centre = 0, n_clockwise = 0;
        for (int i = 0; i < n; ++i) {
          if (cls[i] < 0) continue;
          int k = 0;
          const int what = pg::smiles_atom_text_stereo(i, n, cls[i], h[i], q[i], &val[4 * cls[i]], p0.data(), p1.data(), rank.data(),
                                                       parent.data(), flags.data(), label.data(), par[i], mark.data(), [&](char) { ++k; });
          n_bracket += (what & pg::kSmiBracket) != 0, n_centre += (what & pg::kSmiCentre) != 0, n_clockwise += (what & pg::kSmiClockwise) != 0;
          len[rank[i]] = k;
        }
        int need = 0;
        for (int k = 0; k < n_kept; ++k) {
          const int l = len[k];
          len[k] = need;
          need += l;
        }
        const bool fits = need <= capacity;
        if (fits)
          for (int i = 0; i < n; ++i) {
            if (cls[i] < 0) continue;
            uint8_t* at = text.data() + len[rank[i]];
            pg::smiles_atom_text_stereo(i, n, cls[i], h[i], q[i], &val[4 * cls[i]], p0.data(), p1.data(), rank.data(), parent.data(),
                                        flags.data(), label.data(), par[i], mark.data(), [&](char ch) { *at++ = (uint8_t)ch; });
          }
        else
          for (auto& r : rank) r = -1;
        for (int i = fits ? need : 0; i < capacity; ++i) text[i] = 0;
        sstatus = (fits ? 0 : PG_SMILES_TOO_LONG) | (comps > 1 ? PG_SMILES_DISCONNECTED : 0) | (n_kept == 0 ? PG_SMILES_EMPTY : 0) |
                  (n_bracket > 0 ? PG_SMILES_BRACKET : 0) | (dropped > 0 ? PG_SMILES_STEREO_DROPPED : 0);
        length = fits ? need : 0;
        scnt = {need, n_kept, n_bond, comps, closures, branches, max_label, n_bracket};
        stc = {n_centre, n_clockwise, marked, expressed};
      }
    }
    std::printf("%d %d", sstatus, length);
    for (int c : scnt) std::printf(" %d", c);
    for (int c : stc) std::printf(" %d", c);
    std::printf("\n");
    for (int i = 0; i < capacity; ++i) {
      if (i < length && (text[i] < 0x21 || text[i] > 0x7e)) return 5;
      if (i >= length && text[i] != 0) return 6;
      if (i < length) std::fputc(text[i], stdout);
    }
    std::printf("\n");
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)rank[i]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
