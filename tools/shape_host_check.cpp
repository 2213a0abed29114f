// Stand-alone host program over phoregen_amd/csrc/shape_core.h: the text the device compiles, run under the host sanitizers
// (tests/mol_support.build_host_check compiles it with g++ -fsanitize=address,undefined; tests/test_molshape_host.py runs it).
//
//   shape_host_check pairs FILE      FILE: "alpha" and 12 floats; "w" and the colour weight; "mols" and n; per molecule "mol" and
//                                    its atom count (kept atoms only, at most 128), then one line "x y z class fp" per atom.
//       prints   self i V C          every row's self overlaps
//                pair i j V C ST CT score
//                near i sim index    the packed maximum of row i's scores over all j, ties to the lowest index
//   shape_host_check split NA NB TARGET
//       prints   n_split tiles_per_split, then "run j0 j1" per run, then "row" and the rows of block 0's waves
//
// Floats are read and written as C99 hexadecimal text.  The summation order is the kernel's (csrc/shape_sim.hip): per lane the terms
// of atom l, then of atom l + 64, over the other molecule's atoms in order; low + high; then the butterfly over the 64 lanes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../phoregen_amd/csrc/shape_core.h"

using namespace pg;

struct Atom {
  float x, y, z;
  int word;
};
typedef std::vector<Atom> Mol;

static float butterfly(float (&v)[64]) {
  for (int o = 32; o >= 1; o >>= 1) {
    float next[64];
    for (int l = 0; l < 64; ++l) next[l] = v[l] + v[l ^ o];
    memcpy(v, next, sizeof(next));
  }
  return v[0];
}

static void overlap(const Mol& a, const Mol& b, const ShapeTable& t, float& v_out, float& c_out) {
  float v[64], c[64];
  const int na = (int)a.size();
  for (int l = 0; l < 64; ++l) {
    float acc_v[2] = {0.f, 0.f}, acc_c[2] = {0.f, 0.f};
    for (int h = 0; h < 2; ++h) {
      const int i = l + 64 * h;
      if (i >= na || (h == 1 && na <= 64)) continue;
      for (size_t k = 0; k < b.size(); ++k) {
        const float d2 = shape_dist2(a[i].x, a[i].y, a[i].z, b[k].x, b[k].y, b[k].z);
        const ShapePair e = t.pair[shape_word_class(b[k].word) * kShapeClasses + shape_word_class(a[i].word)];
        acc_v[h] = fmaf(1.0f, shape_term(d2, e), acc_v[h]);
        acc_c[h] = fmaf((float)__builtin_popcount(shape_word_fp(a[i].word) & shape_word_fp(b[k].word)), shape_term(d2, t.colour), acc_c[h]);
      }
    }
    v[l] = acc_v[0] + acc_v[1], c[l] = acc_c[0] + acc_c[1];
  }
  v_out = butterfly(v), c_out = butterfly(c);
}

static int fail(const char* what) {
  fprintf(stderr, "shape_host_check: %s\n", what);
  return 2;
}

static int run_pairs(const char* path) {
  FILE* fh = fopen(path, "r");
  if (!fh) return fail("cannot open the case file");
  char tag[16];
  float alpha[kShapeAlphas], w = 0.f;
  int n = 0;
  if (fscanf(fh, "%15s", tag) != 1 || strcmp(tag, "alpha")) return fail("alpha expected");
  for (int i = 0; i < kShapeAlphas; ++i)
    if (fscanf(fh, "%a", &alpha[i]) != 1) return fail("12 alphas expected");
  if (fscanf(fh, "%15s %a", tag, &w) != 2 || strcmp(tag, "w")) return fail("w expected");
  if (fscanf(fh, "%15s %d", tag, &n) != 2 || strcmp(tag, "mols") || n < 0 || n > 4096) return fail("mols expected");
  ShapeTable t;
  if (!shape_table(alpha, t)) return fail("an alpha is not positive and finite");
  if (!shape_weight_ok(w)) return fail("w outside [0, 1]");
  std::vector<Mol> mols((size_t)n);
  for (int m = 0; m < n; ++m) {
    int k = 0;
    if (fscanf(fh, "%15s %d", tag, &k) != 2 || strcmp(tag, "mol") || k < 0 || k > kShapeMaxAtoms) return fail("mol and its atom count expected");
    for (int i = 0; i < k; ++i) {
      Atom a;
      int cls = 0, fp = 0;
      if (fscanf(fh, "%a %a %a %d %d", &a.x, &a.y, &a.z, &cls, &fp) != 5) return fail("x y z class fp expected");
      a.word = shape_atom_word(cls, fp);
      if (a.word < 0) return fail("a class outside 0 .. 10");
      mols[(size_t)m].push_back(a);
    }
  }
  fclose(fh);
  std::vector<float> self_v((size_t)n), self_c((size_t)n);
  for (int i = 0; i < n; ++i) {
    overlap(mols[(size_t)i], mols[(size_t)i], t, self_v[(size_t)i], self_c[(size_t)i]);
    printf("self %d %a %a\n", i, self_v[(size_t)i], self_c[(size_t)i]);
  }
  for (int i = 0; i < n; ++i) {
    fp_u64 best = kFpMaxNone;
    for (int j = 0; j < n; ++j) {
      float v, c;
      overlap(mols[(size_t)i], mols[(size_t)j], t, v, c);
      const float st = shape_tanimoto(v, self_v[(size_t)i], self_v[(size_t)j]), ct = shape_tanimoto(c, self_c[(size_t)i], self_c[(size_t)j]);
      const float s = shape_score(st, ct, w);
      printf("pair %d %d %a %a %a %a %a\n", i, j, v, c, st, ct, s);
      const fp_u64 p = fp_pack_max(s, j);
      best = p > best ? p : best;
    }
    printf("near %d %a %d\n", i, fp_max_sim(best), fp_max_index(best));
  }
  return 0;
}

static int run_split(int na, int nb, int target) {
  if (na < 0 || nb < 0 || target < 1) return fail("split: NA, NB >= 0 and TARGET >= 1");
  const FpSplit sp = shape_split(na, nb, target);
  printf("%d %d\n", sp.n_split, sp.tiles_per_split);
  for (int s = 0; s < sp.n_split; ++s) {
    int j0, j1;
    shape_split_rows(s, sp.tiles_per_split, nb, j0, j1);
    printf("run %d %d\n", j0, j1);
  }
  printf("row");
  for (int wave = 0; wave < kShapeWaves; ++wave)
    for (int r = 0; r < kShapeRowsPerWave; ++r) printf(" %d", shape_wave_row(0u, wave, r, na));
  printf("\n%d %d %d\n", shape_atom_count(0, 128, 128), shape_atom_count(1, 128, 128), shape_atom_count(0x7fffffff, 1, 0x7fffffff));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "pairs")) return run_pairs(argv[2]);
  if (argc == 5 && !strcmp(argv[1], "split")) return run_split(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
  return fail("usage: shape_host_check pairs FILE | split NA NB TARGET");
}
