// gicp_bfgs_main.cpp -- lv_slam_amd/csrc/gicp_bfgs.hpp on a 6-D test function, for tests/test_gicp_cpu.py (built with
// -fsanitize=address,undefined -ffp-contract=off).  The function uses + - * / only, so C++ and Python round alike.
// usage: gicp_bfgs_main <max_inner_iterations> <x0> ... <x5>
// output: one line per driver iteration -- inner, status, x[6], f, |gradient| as the 64-bit words in hex -- then "end <status> <inner> <evaluations>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gicp_bfgs.hpp"

static const double W[6] = {1.0, 2.5, 0.5, 4.0, 1.5, 3.0};
static const double C[6] = {0.5, -1.25, 2.0, 0.125, -0.75, 1.5};

struct Poly {
  int evaluations = 0;
  void fdf(const double* x, double& f, double* g) {
    evaluations++;
    double t[6];
    for (int i = 0; i < 6; i++) t[i] = x[i] - C[i];
    f = 0.0;
    for (int i = 0; i < 6; i++) { f = f + W[i] * (t[i] * t[i]); g[i] = 2.0 * W[i] * t[i]; }
    const double u = t[0] * t[1] + t[2] * t[3];
    f = f + 0.25 * (u * u);
    g[0] = g[0] + 0.5 * u * t[1]; g[1] = g[1] + 0.5 * u * t[0]; g[2] = g[2] + 0.5 * u * t[3]; g[3] = g[3] + 0.5 * u * t[2];
    const double d = 1.0 + t[5] * t[5], q = (t[4] * t[4]) / d;
    f = f + q;
    g[4] = g[4] + 2.0 * t[4] / d;
    g[5] = g[5] - 2.0 * t[5] * q / d;
  }
  double f(const double* x) { double v, g[6]; fdf(x, v, g); return v; }
  void df(const double* x, double* g) { double v; fdf(x, v, g); }
};

static unsigned long long word(double v) { std::uint64_t u; std::memcpy(&u, &v, 8); return (unsigned long long)u; }

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int max_inner = std::atoi(argv[1]);
  double x[6];
  for (int i = 0; i < 6; i++) x[i] = std::strtod(argv[2 + i], nullptr);
  Poly fn;
  gicp_bfgs::BFGS<Poly> bfgs(fn);
  // the driver loop of gicp_bfgs::minimize, with a line of output per iteration
  int inner = 0;
  int result = bfgs.minimizeInit(x);
  result = gicp_bfgs::Running;
  do {
    inner++;
    result = bfgs.minimizeOneStep(x);
    std::printf("%d %d", inner, result);
    for (int i = 0; i < 6; i++) std::printf(" %016llx", word(x[i]));
    std::printf(" %016llx %016llx\n", word(bfgs.f), word(gicp_bfgs::norm(bfgs.gradient)));
    if (result) break;
    result = bfgs.testGradient(1e-2);
  } while (result == gicp_bfgs::Running && inner < max_inner);
  std::printf("end %d %d %d %d\n", result, inner, fn.evaluations, gicp_bfgs::accepted(result, inner, max_inner) ? 1 : 0);
  // the same run through gicp_bfgs::minimize ends alike
  double y[6];
  for (int i = 0; i < 6; i++) y[i] = std::strtod(argv[2 + i], nullptr);
  Poly fn2;
  gicp_bfgs::BFGS<Poly> b2(fn2);
  int inner2 = 0;
  const int r2 = gicp_bfgs::minimize(b2, y, 1e-2, max_inner, &inner2);
  if (r2 != result || inner2 != inner || std::memcmp(x, y, sizeof x) != 0) return 3;
  return 0;
}
