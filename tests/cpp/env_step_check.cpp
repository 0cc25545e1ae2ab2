// CPU driver for the host halves of an environment step (tensorrl-qas_amd/csrc/env_step_host.h) and the rule they are
// built on (pre_action, vqe_geo.h; the fused kernel holds a hand-kept copy of it, which only the GPU tests see).
// Driven by tests/test_env_step_host_cpu.py, which computes every expected value itself and compares exactly.
//
//   env_step_check CASES
//
// CASES: per circuit "G P new_gate", then G lines "kind q0 q1 pidx", then P theta and P optimiser values as the hex
// bit patterns of the doubles (nothing is rounded in transit; the first P or P - 1 optimiser values are used).  The
// pre-action circuits of all cases are appended to ONE gate list and ONE x0, as the streaming path does, and each
// case's segment is printed:
//   case I skip skip_end hole / gates k q0 q1 pidx ... / x0 ... / xraw ... / x32 ... (env_step) / x64 ... (not)
// The gate behind the last one of every circuit's buffer is a channel that WOULD attach to the last gate: a rule that
// reads the follower without checking the gate count shows as a wrong skip_end.
#include "env_step_host.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace vqe;

namespace {

double from_bits(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
uint64_t to_bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
void print_doubles(const char* name, const double* v, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; ++i) std::printf(" %016" PRIx64, to_bits(v[i]));
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::vector<GateRec> gates2;
  std::vector<double> x0;
  int G, P, new_gate;
  for (int c = 0; std::fscanf(f, "%d %d %d", &G, &P, &new_gate) == 3; ++c) {
    std::vector<GateRec> g(G + 1);
    std::vector<double> theta(P), xopt(P);
    for (int i = 0; i < G; ++i)
      if (std::fscanf(f, "%d %d %d %d", &g[i].kind, &g[i].q0, &g[i].q1, &g[i].pidx) != 4) return 2;
    uint64_t u;
    for (int j = 0; j < P; ++j) { if (std::fscanf(f, "%" SCNx64, &u) != 1) return 2; theta[j] = from_bits(u); }
    for (int j = 0; j < P; ++j) { if (std::fscanf(f, "%" SCNx64, &u) != 1) return 2; xopt[j] = from_bits(u); }
    g[G] = G ? GateRec{g[G - 1].kind == G_CNOT ? G_DEPOL2 : G_DEPOL1, g[G - 1].q0, g[G - 1].q1, -1} : GateRec{G_DEPOL1, 0, -1, -1};

    const size_t g_at = gates2.size(), x_at = x0.size();
    const PreAction pa = pre_action_circuit(g.data(), G, new_gate, theta.data(), P, gates2, x0);
    const PreAction rule = pre_action(g.data(), G, new_gate);
    if (rule.skip != pa.skip || rule.skip_end != pa.skip_end || rule.hole != pa.hole) {
      std::printf("FAIL case %d: pre_action_circuit does not return what pre_action does\n", c);
      return 1;
    }
    std::printf("case %d %d %d %d\ngates", c, pa.skip, pa.skip_end, pa.hole);
    for (size_t i = g_at; i < gates2.size(); ++i)
      std::printf(" %d %d %d %d", gates2[i].kind, gates2[i].q0, gates2[i].q1, gates2[i].pidx);
    std::printf("\n");
    print_doubles("x0", x0.data() + x_at, x0.size() - x_at);
    std::vector<double> xraw(P), x32(P), xraw2(P), x64(P);
    merge_optimum(theta.data(), P, pa.hole, xopt.data(), true, x32.data(), xraw.data());
    merge_optimum(theta.data(), P, pa.hole, xopt.data(), false, x64.data(), xraw2.data());
    if (P && std::memcmp(xraw.data(), xraw2.data(), (size_t)P * 8) != 0) {
      std::printf("FAIL case %d: xraw depends on env_step\n", c);
      return 1;
    }
    print_doubles("xraw", xraw.data(), P);
    print_doubles("x32", x32.data(), P);
    print_doubles("x64", x64.data(), P);
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
