// Host program for tests/test_lanczos_cpu.py: the host logic of the device Lanczos solver (csrc/lanczos_host.h) on
// inputs the test generates.  Numbers travel as C99 hex floats, so nothing is rounded on the way.
//   tridiag  <file>                      file: which m / alpha[m] / beta[m-1]   ->  "theta <hex>" and "s <hex> x m"
//   decide   <file>                      file: which capacity max_matvec tol steps matvecs broke / alpha[steps] / beta[steps]
//                                        ->  "decision <name> dim <k> theta <hex>"
//   capacity <budget_bytes> <n> <max_basis>   ->  the number of basis vectors
#include "lanczos_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

using namespace vqe;

static bool read_doubles(std::ifstream& f, int count, std::vector<double>& out) {
  out.resize((size_t)count);
  std::string tok;
  for (int i = 0; i < count; ++i) {
    if (!(f >> tok)) return false;
    out[(size_t)i] = std::strtod(tok.c_str(), nullptr);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string what = argv[1];
  if (what == "capacity" && argc == 5) {
    std::printf("%d\n", lz_basis_capacity(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]), std::atoi(argv[4])));
    return 0;
  }
  if (argc != 3) return 2;
  std::ifstream f(argv[2]);
  if (!f) return 2;
  if (what == "tridiag") {
    int which = 0, m = 0;
    std::vector<double> alpha, beta;
    if (!(f >> which >> m) || m < 1 || !read_doubles(f, m, alpha) || !read_doubles(f, m - 1, beta)) return 2;
    std::vector<double> s((size_t)m);
    double theta = 0.0;
    if (!lz_tridiag_extreme(alpha.data(), beta.data(), m, which, &theta, s.data())) return 1;
    std::printf("theta %a\ns", theta);
    for (double v : s) std::printf(" %a", v);
    std::printf("\n");
    return 0;
  }
  if (what == "decide") {
    LzRule rule{};
    LzCounters c{};
    std::string tol;
    if (!(f >> rule.which >> rule.capacity >> rule.max_matvec >> tol >> c.steps >> c.matvecs >> c.broke)) return 2;
    rule.tol = std::strtod(tol.c_str(), nullptr);
    std::vector<double> alpha, beta;
    if (c.steps < 0 || !read_doubles(f, c.steps, alpha) || !read_doubles(f, c.steps, beta)) return 2;
    std::vector<double> s((size_t)c.steps + 1);
    double theta = 0.0;
    int dim = 0;
    const int d = lz_decide(alpha.data(), beta.data(), rule, c, &theta, s.data(), &dim);
    static const char* const names[] = {"continue", "converged", "restart", "breakdown", "budget"};
    std::printf("decision %s dim %d theta %a\n", names[d], dim, theta);
    return 0;
  }
  return 2;
}
