// spsa_host_check.cpp - host check of csrc/spsa_m0.h, the code k_lds_minimize_spsa calls, without a GPU.
// tests/test_spsa_cpu.py builds it with g++ -fsanitize=address,undefined and runs it as a program.
//   argv[1]: a text file of commands, numbers as hexadecimal floating point:
//     run <maxiter> <a> <alpha> <stability> <c> <gamma> <beta_1> <beta_2> <lamda> <eps> <P> <hole>
//         then P values of x0, then per iteration P signs (+1, -1, 0) and the pair f+ f-
//       -> "point <k> x_0 .. x_{P-1}" for k = 0 .. maxiter (hexadecimal floating point), and "trial <k> <c_k>"
//     bad <maxiter> <a> <alpha> <stability> <c> <gamma> <beta_1> <beta_2> <lamda> <eps>
//       -> "bad <0 | 1> <message>": what the validator says
// The perturbation signs come from the test (the engine's counter hash is not part of this header).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spsa_m0.h"

using namespace vqe;

static bool read_opts(FILE* f, SpsaOpts& o) {
  int mi = 0;
  if (std::fscanf(f, "%d %la %la %la %la %la %la %la %la %la", &mi, &o.a, &o.alpha, &o.stability, &o.c, &o.gamma, &o.beta_1,
                  &o.beta_2, &o.lamda, &o.eps) != 10)
    return false;
  o.maxiter = mi;
  o.seed = 0;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: spsa_host_check <commands>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::perror(argv[1]); return 2; }
  {   // the defaults are the header's own
    const SpsaOpts d = spsa_default_opts();
    std::printf("defaults %d %a %a %a %a %a %a %a %a %a %llu\n", (int)d.maxiter, d.a, d.alpha, d.stability, d.c, d.gamma, d.beta_1,
                d.beta_2, d.lamda, d.eps, (unsigned long long)d.seed);
    if (spsa_bad_option(d)) { std::fprintf(stderr, "the defaults are refused\n"); return 1; }
  }
  char cmd[16];
  int run = 0;
  while (std::fscanf(f, "%15s", cmd) == 1) {
    SpsaOpts o{};
    if (!read_opts(f, o)) { std::fprintf(stderr, "bad options line\n"); return 2; }
    if (!std::strcmp(cmd, "bad")) {
      const char* why = spsa_bad_option(o);
      std::printf("bad %d %s\n", why ? 1 : 0, why ? why : "-");
      continue;
    }
    if (std::strcmp(cmd, "run")) { std::fprintf(stderr, "unknown command %s\n", cmd); return 2; }
    int P = 0, hole = -1;
    if (std::fscanf(f, "%d %d", &P, &hole) != 2 || P < 0) { std::fprintf(stderr, "bad run header\n"); return 2; }
    if (spsa_bad_option(o)) { std::fprintf(stderr, "run %d: options refused: %s\n", run, spsa_bad_option(o)); return 1; }
    std::vector<double> x(P), m(P, 0.0), v(P, 0.0), D(P);
    for (int j = 0; j < P; ++j)
      if (std::fscanf(f, "%la", &x[j]) != 1) { std::fprintf(stderr, "short x0\n"); return 2; }
    const auto print_point = [&](int k) {
      std::printf("point %d", k);
      for (int j = 0; j < P; ++j) std::printf(" %a", x[j]);
      std::printf("\n");
    };
    print_point(0);
    SpsaIter it = spsa_start();
    for (int k = 0; k < o.maxiter; ++k) {
      double fp = 0.0, fm = 0.0;
      for (int j = 0; j < P; ++j)
        if (std::fscanf(f, "%la", &D[j]) != 1) { std::fprintf(stderr, "short signs\n"); return 2; }
      if (std::fscanf(f, "%la %la", &fp, &fm) != 2) { std::fprintf(stderr, "short pair\n"); return 2; }
      if (hole >= 0 && D[hole] != 0.0) { std::fprintf(stderr, "the hole has a sign\n"); return 1; }
      spsa_begin_iteration(it, o, k);           // once per iteration, as the kernel
      std::printf("trial %d %a\n", k, it.c_k);
      spsa_close_iteration(it, o, fp, fm);
      for (int j = 0; j < P; ++j) spsa_update_element(it, o, D[j], x[j], m[j], v[j]);
      print_point(k + 1);
    }
    ++run;
  }
  std::fclose(f);
  return 0;
}
