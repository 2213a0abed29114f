// Stand-alone host program over phoregen_amd/csrc/shape_align_core.h: the text the device compiles, run under the host sanitizers
// (tests/mol_support.build_host_check compiles it with g++ -fsanitize=address,undefined; tests/test_molshape_align_host.py runs it).
//
//   shape_align_host_check frames FILE   FILE: "mols" and n; per molecule "mol" and its atom count (at most 128), then one line
//                                        "x y z" per atom.
//       prints   frame i f0 .. f15       the frame of every molecule
//                start i k w x y z px py pz     for the molecules 2i (A) and 2i + 1 (B), k = 0 .. 4: the start's quaternion and p
//   shape_align_host_check quat FILE     FILE: lines "q w x y z" (a quaternion), "e rx ry rz" (a rotation vector),
//                                        "t w x y z px py pz d0 .. d5 s rho" (a pose, a direction, a step) and
//                                        "g fx fy fz tx ty tz rho" (a gradient)
//       prints   q: "matrix" r0 .. r8 of the normalised quaternion, then "back" w x y z from that matrix
//                e: "exp" w x y z            t: "trial" w x y z px py pz          g: "direction" ok d0 .. d5
//   shape_align_host_check steps FIRST MIN MAX F0 F1 ..     a scripted objective: F0 is the start's score, F1 .. the trials' scores
//       prints   one line "accept" or "reject" per trial the rule asks for, then "end evaluations step score"
//
// Floats are read and written as C99 hexadecimal text.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../phoregen_amd/csrc/shape_align_core.h"

using namespace pg;

struct Atom {
  float x, y, z;
};

static int fail(const char* what) {
  fprintf(stderr, "shape_align_host_check: %s\n", what);
  return 2;
}

static int run_frames(const char* path) {
  FILE* fh = fopen(path, "r");
  if (!fh) return fail("cannot open the case file");
  char tag[16];
  int n = 0;
  if (fscanf(fh, "%15s %d", tag, &n) != 2 || strcmp(tag, "mols") || n < 0 || n > 4096) return fail("mols expected");
  std::vector<std::vector<float> > frames((size_t)n, std::vector<float>(kAlignFrame));
  for (int m = 0; m < n; ++m) {
    int k = 0;
    if (fscanf(fh, "%15s %d", tag, &k) != 2 || strcmp(tag, "mol") || k < 0 || k > kShapeMaxAtoms) return fail("mol and its atom count expected");
    std::vector<Atom> atoms((size_t)k);
    for (int i = 0; i < k; ++i)
      if (fscanf(fh, "%a %a %a", &atoms[(size_t)i].x, &atoms[(size_t)i].y, &atoms[(size_t)i].z) != 3) return fail("x y z expected");
    align_frame(atoms.data(), k, frames[(size_t)m].data());
    printf("frame %d", m);
    for (int i = 0; i < kAlignFrame; ++i) printf(" %a", frames[(size_t)m][(size_t)i]);
    printf("\n");
  }
  fclose(fh);
  for (int i = 0; 2 * i + 1 < n; ++i)
    for (int k = 0; k < kAlignStarts; ++k) {
      AlignQuat q;
      float p[3];
      align_start(k, frames[(size_t)(2 * i)].data(), frames[(size_t)(2 * i + 1)].data(), q, p);
      printf("start %d %d %a %a %a %a %a %a %a\n", i, k, q.w, q.x, q.y, q.z, p[0], p[1], p[2]);
    }
  return 0;
}

static int run_quat(const char* path) {
  FILE* fh = fopen(path, "r");
  if (!fh) return fail("cannot open the case file");
  char tag[16];
  while (fscanf(fh, "%15s", tag) == 1) {
    if (!strcmp(tag, "q")) {
      AlignQuat q;
      if (fscanf(fh, "%a %a %a %a", &q.w, &q.x, &q.y, &q.z) != 4) return fail("q: w x y z expected");
      float r[9];
      align_quat_matrix(align_quat_normalised(q), r);
      printf("matrix");
      for (int i = 0; i < 9; ++i) printf(" %a", r[i]);
      const AlignQuat b = align_matrix_quat(r);
      printf("\nback %a %a %a %a\n", b.w, b.x, b.y, b.z);
    } else if (!strcmp(tag, "e")) {
      float v[3];
      if (fscanf(fh, "%a %a %a", &v[0], &v[1], &v[2]) != 3) return fail("e: rx ry rz expected");
      const AlignQuat q = align_quat_exp(v[0], v[1], v[2]);
      printf("exp %a %a %a %a\n", q.w, q.x, q.y, q.z);
    } else if (!strcmp(tag, "t")) {
      AlignQuat q, qt;
      float p[3], pt[3], d[6], s, rho;
      if (fscanf(fh, "%a %a %a %a %a %a %a", &q.w, &q.x, &q.y, &q.z, &p[0], &p[1], &p[2]) != 7) return fail("t: a pose expected");
      for (int i = 0; i < 6; ++i)
        if (fscanf(fh, "%a", &d[i]) != 1) return fail("t: a direction expected");
      if (fscanf(fh, "%a %a", &s, &rho) != 2) return fail("t: s rho expected");
      align_trial(q, p, d, s, rho, qt, pt);
      printf("trial %a %a %a %a %a %a %a\n", qt.w, qt.x, qt.y, qt.z, pt[0], pt[1], pt[2]);
    } else if (!strcmp(tag, "g")) {
      float f[3], t[3], rho, d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (fscanf(fh, "%a %a %a %a %a %a %a", &f[0], &f[1], &f[2], &t[0], &t[1], &t[2], &rho) != 7) return fail("g: a gradient and rho expected");
      const bool ok = align_direction(f, t, rho, d);
      printf("direction %d %a %a %a %a %a %a\n", ok ? 1 : 0, d[0], d[1], d[2], d[3], d[4], d[5]);
    } else {
      return fail("q, e, t or g expected");
    }
  }
  fclose(fh);
  return 0;
}

static int run_steps(int argc, char** argv) {
  float first = 0.f, least = 0.f;
  if (sscanf(argv[2], "%a", &first) != 1 || sscanf(argv[3], "%a", &least) != 1) return fail("steps: FIRST MIN expected");
  const int max_steps = atoi(argv[4]);
  if (!align_options_ok(max_steps, first, least, kAlignStartInPlace)) return fail("steps: options the entry point refuses");
  std::vector<float> score;
  for (int i = 5; i < argc; ++i) {
    float f;
    if (sscanf(argv[i], "%a", &f) != 1) return fail("steps: a score expected");
    score.push_back(f);
  }
  if (score.empty()) return fail("steps: the start's score expected");
  float f = score[0], s = first;
  int evaluations = 1;
  while (!align_stop(s, evaluations, least, max_steps)) {
    if ((size_t)evaluations >= score.size()) return fail("steps: the script is too short");
    const float trial = score[(size_t)evaluations++];
    const bool better = align_accept(trial, f, s);
    if (better) f = trial;
    printf("%s\n", better ? "accept" : "reject");
  }
  printf("end %d %a %a\n", evaluations, s, f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "frames")) return run_frames(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "quat")) return run_quat(argv[2]);
  if (argc >= 6 && !strcmp(argv[1], "steps")) return run_steps(argc, argv);
  return fail("usage: shape_align_host_check frames FILE | quat FILE | steps FIRST MIN MAX F0 F1 ..");
}
