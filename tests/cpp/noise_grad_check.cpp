// noise_grad_check.cpp - the host rules of csrc/noise_grad_host.h (vqe_set_noise_grad) without a GPU.
// A model handle (the fields the rules read, and the counter) is driven through sequences of calls; every line printed
// is "<call> <verdict> <eval_base>", which tests/test_noise_grad_cpu.py compares with the rules as include/vqe_hip.h
// states them.  Built with -fsanitize=address,undefined and run as a program.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "noise_grad_host.h"

using namespace vqe;

struct Model {
  NoiseGradState s{0, 0, false, true};
  bool hold = false;
  double shot = 0.0;
  int shard_world = 1;
  uint64_t eval_base = 0;
};

// The order of the refusal test of the adjoint entry points: the verdict, then mode 1, shot noise; for the L-BFGS the
// term shard.  A refused call changes nothing.  -> 0 served, else the number of the test that refused
static int call(Model& m, NoiseGradRun run) {
  const NoiseGradVerdict v = noise_grad_verdict(m.s);
  if (v == NG_REFUSED_OFF) return 1;
  if (v == NG_REFUSED_PATH) return 2;
  if (m.s.noise_mode == 1) return 3;
  if (m.shot != 0.0) return 4;
  if (run != NoiseGradRun::Gradient && m.shard_world > 1) return 5;
  if (v == NG_SERVED) m.eval_base += noise_grad_consumed(run, m.s.n_real, m.hold);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  Model m;
  char op[64];
  long a, b;
  // script: one "<op> <a> <b>" per line
  while (fscanf(f, "%63s %ld %ld", op, &a, &b) == 3) {
    int rc = 0;
    if (!strcmp(op, "new")) m = Model{};
    else if (!strcmp(op, "set")) {          // vqe_set_noise_grad(a, b)
      if (a < 0 || a > kNoiseGradMaxReal) rc = -22;
      else { m.s.n_real = (int)a; m.hold = b != 0; }
    }
    else if (!strcmp(op, "noise")) { m.s.pauli_on = a != 0; m.eval_base = 0; }      // vqe_set_noise resets the counter
    else if (!strcmp(op, "mode")) m.s.noise_mode = (int)a;
    else if (!strcmp(op, "qubits")) m.s.lds_path = a <= 13;
    else if (!strcmp(op, "shot")) m.shot = (double)a;
    else if (!strcmp(op, "shard")) m.shard_world = (int)a;
    else if (!strcmp(op, "grad")) rc = call(m, NoiseGradRun::Gradient);
    else if (!strcmp(op, "lbfgs")) rc = call(m, NoiseGradRun::Lbfgs);
    else if (!strcmp(op, "envstep")) rc = call(m, NoiseGradRun::EnvStepLbfgs);
    else if (!strcmp(op, "advance")) m.eval_base += (uint64_t)m.s.n_real;
    else { fclose(f); return 3; }
    printf("%s %d %llu\n", op, rc, (unsigned long long)m.eval_base);
  }
  fclose(f);
  puts("ok");
  return 0;
}
