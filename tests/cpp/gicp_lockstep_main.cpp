// gicp_lockstep_main.cpp -- lv_slam_amd/csrc/gicp_lockstep.hpp under lv_slam_amd/csrc/gicp_bfgs.hpp, for tests/test_gicp_batch_cpu.py (built
// with -fsanitize=thread -pthread -ffp-contract=off).  The 6-D function of gicp_bfgs_main.cpp is minimised from K = 1, 2, 5 and 64 starts
// twice: one start after the other with the function called directly, and in lockstep, one worker thread per start, every posted point
// evaluated by one serve callback per round.  The starts are the four of tests/test_gicp_cpu.py's BFGS_CASES (slot k takes case k % 4, with
// its max_inner_iterations) moved by k / 4 steps of 1/32, so the slots end in different rounds; zero_gradient ends before its first step.
// output: per K and slot "K k status inner evaluations x[6] f" (64-bit words in hex), then "K rounds <rounds>".
// exit status: 0 when both runs agree word for word, rounds == max_k requests[k], and a run whose callback fails in round 3 returns with
// every worker ended; 1 otherwise.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gicp_bfgs.hpp"
#include "gicp_lockstep.hpp"

static const double W[6] = {1.0, 2.5, 0.5, 4.0, 1.5, 3.0};
static const double C[6] = {0.5, -1.25, 2.0, 0.125, -0.75, 1.5};

static void poly(const double* x, double& f, double* g) {
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

struct Direct {
  int evaluations = 0;
  void fdf(const double* x, double& f, double* g) { evaluations++; poly(x, f, g); }
  double f(const double* x) { double v, g[6]; fdf(x, v, g); return v; }
  void df(const double* x, double* g) { double v; fdf(x, v, g); }
};

struct Req { double x[6]; };
struct Rec { double f, g[6]; };
typedef gicp_lockstep::Lockstep<Req, Rec> Steps;

struct Posted {
  Steps* ls; int k;
  void fdf(const double* x, double& f, double* g) {
    Req r;
    Rec o;
    std::memcpy(r.x, x, sizeof r.x);
    ls->post(k, r, &o);
    f = o.f;
    std::memcpy(g, o.g, sizeof o.g);
  }
  double f(const double* x) { double v, g[6]; fdf(x, v, g); return v; }
  void df(const double* x, double* g) { double v; fdf(x, v, g); }
};

struct Case { double x[6]; int max_inner; };
static const Case CASES[4] = {{{3.0, -2.0, 1.0, 2.0, -3.0, 0.5}, 50}, {{-1.0, 4.0, -2.0, 1.5, 2.0, -1.0}, 50},
                              {{0.5, -1.25, 2.0, 0.125, -0.75, 1.5}, 20}, {{3.0, -2.0, 1.0, 2.0, -3.0, 0.5}, 2}};
static Case start(int k) {
  Case c = CASES[k % 4];
  for (int i = 0; i < 6; i++) c.x[i] = c.x[i] + 0.03125 * (double)(k / 4) * ((i & 1) ? -1.0 : 1.0);
  return c;
}

struct Out { double x[6], f; int status, inner, evaluations; };

template <typename Fn>
static Out minimise(Fn& fn, int k) {
  Case c = start(k);
  Out o;
  gicp_bfgs::BFGS<Fn> bfgs(fn);
  o.status = gicp_bfgs::minimize(bfgs, c.x, 1e-2, c.max_inner, &o.inner);
  std::memcpy(o.x, c.x, sizeof o.x);
  o.f = bfgs.f;
  o.evaluations = 0;
  return o;
}

static unsigned long long word(double v) { std::uint64_t u; std::memcpy(&u, &v, 8); return (unsigned long long)u; }

static bool serve_all(const int* slots, int n, const Req* req, Rec* rec) {
  for (int j = 0; j < n; j++) poly(req[slots[j]].x, rec[slots[j]].f, rec[slots[j]].g);
  return true;
}

int main() {
  const int KS[4] = {1, 2, 5, 64};
  bool good = true;
  for (int K : KS) {
    std::vector<Out> one((size_t)K), many((size_t)K);
    for (int k = 0; k < K; k++) {
      Direct fn;
      one[(size_t)k] = minimise(fn, k);
      one[(size_t)k].evaluations = fn.evaluations;
    }
    Steps ls(K);
    const bool ok = ls.run([&](int k) { Posted fn{&ls, k}; many[(size_t)k] = minimise(fn, k); }, serve_all);
    int most = 0;
    for (int k = 0; k < K; k++) {
      Out& m = many[(size_t)k];
      const Out& o = one[(size_t)k];
      m.evaluations = ls.requests(k);
      most = m.evaluations > most ? m.evaluations : most;
      std::printf("%d %d %d %d %d", K, k, m.status, m.inner, m.evaluations);
      for (int i = 0; i < 6; i++) std::printf(" %016llx", word(m.x[i]));
      std::printf(" %016llx\n", word(m.f));
      if (std::memcmp(m.x, o.x, sizeof o.x) != 0 || word(m.f) != word(o.f) || m.status != o.status || m.inner != o.inner || m.evaluations != o.evaluations) {
        std::printf("slot %d differs from its sequential run: status %d inner %d evaluations %d f %016llx\n", k, o.status, o.inner, o.evaluations, word(o.f));
        good = false;
      }
    }
    std::printf("%d rounds %d\n", K, ls.rounds());
    if (!ok || ls.rounds() != most) good = false;
    if (K >= 5 && !(many[2].status == gicp_bfgs::NoProgress && many[2].inner == 1 && many[2].evaluations == 1)) good = false;   // zero_gradient
  }
  {                                                // the callback fails in round 3: every worker ends, run() returns false
    const int K = 5;
    Steps ls(K);
    std::vector<Out> many((size_t)K);
    int calls = 0;
    const bool ok = ls.run([&](int k) { Posted fn{&ls, k}; many[(size_t)k] = minimise(fn, k); },
                           [&](const int* slots, int n, const Req* req, Rec* rec) { return ++calls < 3 && serve_all(slots, n, req, rec); });
    std::printf("failure in round 3: returned %d after %d rounds\n", ok ? 1 : 0, ls.rounds());
    if (ok || ls.rounds() != 3 || calls != 3) good = false;
  }
  return good ? 0 : 1;
}
