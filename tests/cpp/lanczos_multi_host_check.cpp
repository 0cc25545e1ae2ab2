// Host program for tests/test_lanczos_multi_cpu.py: the host logic of vqe_lanczos_multi (csrc/lanczos_host.h) without a
// GPU.  Numbers travel as C99 hex floats, so nothing is rounded on the way.
//   symeig <file>      file: n / a[n * n] row major        ->  "w <hex> x n" and "z <hex> x n*n" (row major, columns = vectors)
//   keep <capacity> <keep_option>                          ->  the number of Ritz vectors a thick restart keeps
//   slots <budget_bytes> <n> <max_basis> <n_eig>           ->  "<slots> <fits 0|1> <capacity of stage 0> .. <of stage n_eig-1>"
//   run <file>         file: n which n_eig max_basis max_matvec check_every keep tol seed slots / Re, Im of the dense
//                      Hermitian 2^n x 2^n matrix, row major.  The LzMulti state machine drives plain-loop vector
//                      arithmetic here - the commands the device driver executes with kernels.
//                      ->  "info <status> <matvecs> <restarts> <pairs>", "theta ..", "resid ..", "vec <e> <Re Im> x 2^n"
#include "lanczos_host.h"

#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

using namespace vqe;
typedef std::complex<double> cplx;
typedef std::vector<cplx> cvec;

static bool read_doubles(std::ifstream& f, size_t count, std::vector<double>& out) {
  out.resize(count);
  std::string tok;
  for (size_t i = 0; i < count; ++i) {
    if (!(f >> tok)) return false;
    out[i] = std::strtod(tok.c_str(), nullptr);
  }
  return true;
}

static uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static cplx dot(const cvec& a, const cvec& b) {      // <a|b>
  cplx acc = 0.0;
  for (size_t p = 0; p < a.size(); ++p) acc += std::conj(a[p]) * b[p];
  return acc;
}

static double norm(const cvec& a) { return std::sqrt(dot(a, a).real()); }

static cvec matvec(const cvec& H, const cvec& v) {
  const size_t dim = v.size();
  cvec out(dim, 0.0);
  for (size_t p = 0; p < dim; ++p)
    for (size_t q = 0; q < dim; ++q) out[p] += H[p * dim + q] * v[q];
  return out;
}

// two passes of classical Gram-Schmidt of w against slots[0 .. cnt)
static void orthogonalise(const std::vector<cvec>& slots, int cnt, cvec& w) {
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<cplx> c((size_t)cnt);
    for (int k = 0; k < cnt; ++k) c[(size_t)k] = dot(slots[(size_t)k], w);
    for (int k = 0; k < cnt; ++k)
      for (size_t p = 0; p < w.size(); ++p) w[p] -= c[(size_t)k] * slots[(size_t)k][p];
  }
}

static int run(std::ifstream& f) {
  int n = 0, slots_n = 0;
  LzMultiOptions o{};
  std::string tol;
  unsigned long long seed = 0;
  if (!(f >> n >> o.which >> o.n_eig >> o.max_basis >> o.max_matvec >> o.check_every >> o.keep >> tol >> seed >> slots_n)) return 2;
  o.tol = std::strtod(tol.c_str(), nullptr);
  o.seed = seed;
  const size_t dim = (size_t)1 << n;
  std::vector<double> raw;
  if (!read_doubles(f, 2 * dim * dim, raw)) return 2;
  cvec H(dim * dim);
  double hnorm = 0.0;
  for (size_t p = 0; p < dim; ++p) {
    double row = 0.0;
    for (size_t q = 0; q < dim; ++q) {
      H[p * dim + q] = cplx(raw[2 * (p * dim + q)], raw[2 * (p * dim + q) + 1]);
      row += std::abs(H[p * dim + q]);
    }
    hnorm = std::max(hnorm, row);
  }
  if (!lz_multi_fits(slots_n, n, o.max_basis, o.n_eig)) return 3;
  const double thresh = 1e-13 * hnorm;
  std::vector<cvec> slot((size_t)slots_n, cvec(dim));
  cvec w(dim);
  std::vector<double> alpha((size_t)o.max_basis), beta((size_t)o.max_basis);
  LzMulti M(o, n, slots_n);
  for (;;) {
    const LzMultiCmd c = M.cmd();
    if (c.op == LZM_DONE) break;
    const int e = c.stage;
    if (c.op == LZM_START) {
      for (size_t p = 0; p < dim; ++p) {
        const double re = (double)(mix(c.seed ^ (2 * p + 1)) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        const double im = (double)(mix(c.seed ^ (2 * p + 2)) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        w[p] = cplx(re, im);
      }
      orthogonalise(slot, e, w);
      const double b = norm(w);
      if (!(b > 0.0)) return 4;
      for (size_t p = 0; p < dim; ++p) slot[(size_t)e][p] = w[p] / b;
      M.started();
    } else if (c.op == LZM_STEPS) {
      int broke = -1;
      for (int j = c.j0; j < c.j1 && broke < 0; ++j) {
        const cvec& v = slot[(size_t)(e + j)];
        w = matvec(H, v);
        if (!(j == c.j0 && c.no_prev))
          for (size_t p = 0; p < dim; ++p) w[p] -= beta[(size_t)j - 1] * slot[(size_t)(e + j - 1)][p];
        alpha[(size_t)j] = dot(v, w).real();
        for (size_t p = 0; p < dim; ++p) w[p] -= alpha[(size_t)j] * v[p];
        orthogonalise(slot, e + j + 1, w);
        const double b = norm(w);
        beta[(size_t)j] = b;
        if (!(b > thresh)) {
          broke = j;
          break;
        }
        if (j + 1 < c.capacity) for (size_t p = 0; p < dim; ++p) slot[(size_t)(e + j + 1)][p] = w[p] / b;
        else for (size_t p = 0; p < dim; ++p) w[p] /= b;
      }
      M.steps_done(alpha.data(), beta.data(), broke);
    } else if (c.op == LZM_RESTART) {
      for (size_t p = 0; p < dim; ++p) {      // in place, amplitude by amplitude, sums over i ascending
        std::vector<cplx> col((size_t)c.m);
        for (int i = 0; i < c.m; ++i) col[(size_t)i] = slot[(size_t)(e + i)][p];
        for (int q = 0; q < c.r; ++q) {
          cplx acc = 0.0;
          for (int i = 0; i < c.m; ++i) acc += c.s[(size_t)i * c.ld + q] * col[(size_t)i];
          slot[(size_t)(e + q)][p] = acc;
        }
        if (c.with_resid) slot[(size_t)(e + c.r)][p] = w[p];
      }
      M.restarted();
    } else {      // LZM_LOCK
      cvec y(dim, 0.0);
      for (int i = 0; i < c.m; ++i)
        for (size_t p = 0; p < dim; ++p) y[p] += c.s[(size_t)i] * slot[(size_t)(e + i)][p];
      const double b = norm(y);
      for (size_t p = 0; p < dim; ++p) slot[(size_t)e][p] = y[p] / b;
      const cvec hy = matvec(H, slot[(size_t)e]);
      const double theta = dot(slot[(size_t)e], hy).real();
      double r2 = 0.0;
      for (size_t p = 0; p < dim; ++p) r2 += std::norm(hy[p] - theta * slot[(size_t)e][p]);
      M.locked(theta, std::sqrt(r2));
    }
  }
  std::printf("info %d %d %d %d\ntheta", M.status(), M.matvecs(), M.restarts(), M.pairs());
  for (int e = 0; e < M.pairs(); ++e) std::printf(" %a", M.theta(e));
  std::printf("\nresid");
  for (int e = 0; e < M.pairs(); ++e) std::printf(" %a", M.residual(e));
  std::printf("\n");
  for (int e = 0; e < M.pairs(); ++e) {
    std::printf("vec %d", e);
    for (size_t p = 0; p < dim; ++p) std::printf(" %a %a", slot[(size_t)e][p].real(), slot[(size_t)e][p].imag());
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string what = argv[1];
  if (what == "keep" && argc == 4) {
    std::printf("%d\n", lz_keep_count(std::atoi(argv[2]), std::atoi(argv[3])));
    return 0;
  }
  if (what == "slots" && argc == 6) {
    const int n = std::atoi(argv[3]), max_basis = std::atoi(argv[4]), n_eig = std::atoi(argv[5]);
    const int slots = lz_multi_slots(std::strtoull(argv[2], nullptr, 10), n, max_basis, n_eig);
    std::printf("%d %d", slots, lz_multi_fits(slots, n, max_basis, n_eig) ? 1 : 0);
    for (int e = 0; e < n_eig; ++e) std::printf(" %d", lz_stage_capacity(slots, n, max_basis, e));
    std::printf("\n");
    return 0;
  }
  if (argc != 3) return 2;
  std::ifstream f(argv[2]);
  if (!f) return 2;
  if (what == "symeig") {
    int n = 0;
    std::vector<double> a;
    if (!(f >> n) || n < 1 || !read_doubles(f, (size_t)n * n, a)) return 2;
    std::vector<double> w((size_t)n), z((size_t)n * n);
    if (!lz_sym_eig(a.data(), n, w.data(), z.data())) return 1;
    std::printf("w");
    for (double v : w) std::printf(" %a", v);
    std::printf("\nz");
    for (double v : z) std::printf(" %a", v);
    std::printf("\n");
    return 0;
  }
  if (what == "run") return run(f);
  return 2;
}
