// gicp_bfgs.hpp -- the optimiser of pclomp::GeneralizedIterativeClosestPoint::estimateRigidTransformationBFGS (gicp_omp_impl.hpp:189-252):
// PCL's BFGS<Functor> (pcl/registration/bfgs.h), which is GSL's vector_bfgs2 minimiser with Fletcher's line search (multimin/vector_bfgs2.c,
// multimin/linear_minimize.c, multimin/linear_wrapper.c) carried over to Eigen.
//
// RESTATED AS RECALLED.  Neither PCL nor GSL is in the reference tree or available to the build; the published algorithm is written down here
// from memory of those sources and is unpinned.  tools/gicp_ref.py holds the same statements in Python, and
// tests/test_gicp_cpu.py holds the two to each other word for word.  What is fixed here where the originals leave it to BLAS / Eigen:
//   dot(a, b)  = a[0]*b[0] + a[1]*b[1] + ... summed in index order;  norm(a) = sqrt(dot(a, a))
//   axpy       = y[i] + alpha * x[i], one rounding per operation (the build's -ffp-contract=off)
// The pieces:
//   * direction: the memoryless BFGS update  p' = g - A dx0 - B dg0,  B = dx0.g / dx0.dg0,  A = -(1 + dg0.dg0 / dx0.dg0) B + dg0.g / dx0.dg0
//     (A = B = 0 when dx0.dg0 == 0), normalised and pointed downhill;
//   * first trial step of a line search: min(1, 2 max(-delta_f, 10 eps |f0|) / (-fp0)) after a decrease, |step| otherwise;
//   * line search: bracketing (rho test, sigma test, extrapolation within [alpha + delta, alpha + tau1 delta]) then sectioning within
//     [a + tau2 (b - a), b - tau3 (b - a)], both choosing the trial point by cubic (order 3, when the far slope is known) or quadratic
//     interpolation; NoProgress when (a - alpha) fpa <= eps; one budget of 100 trials for the two phases together;
//   * the function along the line caches f, the gradient and the slope by their alpha, as linear_wrapper.c does -- the number and order of the
//     functor's evaluations are part of the restatement;
//   * NoProgress without a step when pnorm, g0norm or fp0 is zero.
// Nothing of HIP in this file: it compiles into the library's host side and into tests/cpp/gicp_bfgs_main.cpp.
//
// Functor:  double f(const double x[6]);  void df(const double x[6], double g[6]);  void fdf(const double x[6], double& f, double g[6]);
#pragma once
#include <cmath>
#include <cstring>

namespace gicp_bfgs {

enum Status { NegativeGradientEpsilon = -3, NotStarted = -2, Running = -1, Success = 0, NoProgress = 1 };   // BFGSSpace::Status
constexpr int N = 6;
constexpr double EPS = 2.2204460492503131e-16;   // GSL_DBL_EPSILON

struct Parameters {                              // as estimateRigidTransformationBFGS sets them (:222-227); step_size: PCL's default
  double sigma = 0.01, rho = 0.01, tau1 = 9, tau2 = 0.05, tau3 = 0.5, step_size = 1.0;
  int order = 3;
};

inline double dot(const double* a, const double* b) { double s = a[0] * b[0]; for (int i = 1; i < N; i++) s = s + a[i] * b[i]; return s; }
inline double norm(const double* a) { return std::sqrt(dot(a, a)); }
inline void copy(double* d, const double* s) { std::memcpy(d, s, N * sizeof(double)); }

// gsl_poly_solve_quadratic: real roots of a x^2 + b x + c, ascending
inline int solve_quadratic(double a, double b, double c, double* x0, double* x1) {
  if (a == 0) {
    if (b == 0) return 0;
    *x0 = -c / b;
    return 1;
  }
  const double disc = b * b - 4 * a * c;
  if (disc > 0) {
    if (b == 0) {
      const double r = std::sqrt(-c / a);
      *x0 = -r; *x1 = r;
    } else {
      const double sgnb = b > 0 ? 1.0 : -1.0;
      const double temp = -0.5 * (b + sgnb * std::sqrt(disc));
      const double r1 = temp / a, r2 = c / temp;
      if (r1 < r2) { *x0 = r1; *x1 = r2; } else { *x0 = r2; *x1 = r1; }
    }
    return 2;
  }
  if (disc == 0) { *x0 = -0.5 * b / a; *x1 = -0.5 * b / a; return 2; }
  return 0;
}

inline double interp_quad(double f0, double fp0, double f1, double zl, double zh) {
  const double fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0));
  const double fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0));
  const double c = 2 * (f1 - f0 - fp0);          // curvature
  double zmin = zl, fmin = fl;
  if (fh < fmin) { zmin = zh; fmin = fh; }
  if (c > 0) {                                   // positive curvature required for a minimum
    const double z = -fp0 / c;
    if (z > zl && z < zh) {
      const double f = f0 + z * (fp0 + z * (f1 - f0 - fp0));
      if (f < fmin) { zmin = z; fmin = f; }
    }
  }
  return zmin;
}

inline double cubic(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }
inline void check_extremum(double c0, double c1, double c2, double c3, double z, double* zmin, double* fmin) {
  const double y = cubic(c0, c1, c2, c3, z);
  if (y < *fmin) { *zmin = z; *fmin = y; }
}
inline double interp_cubic(double f0, double fp0, double f1, double fp1, double zl, double zh) {
  const double eta = 3 * (f1 - f0) - 2 * fp0 - fp1;
  const double xi = fp0 + fp1 - 2 * (f1 - f0);
  const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
  double zmin = zl, fmin = cubic(c0, c1, c2, c3, zl), z0 = 0, z1 = 0;
  check_extremum(c0, c1, c2, c3, zh, &zmin, &fmin);
  const int n = solve_quadratic(3 * c3, 2 * c2, c1, &z0, &z1);
  if (n == 2) {
    if (z0 > zl && z0 < zh) check_extremum(c0, c1, c2, c3, z0, &zmin, &fmin);
    if (z1 > zl && z1 < zh) check_extremum(c0, c1, c2, c3, z1, &zmin, &fmin);
  } else if (n == 1) {
    if (z0 > zl && z0 < zh) check_extremum(c0, c1, c2, c3, z0, &zmin, &fmin);
  }
  return zmin;
}
inline double interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax, int order) {
  double zmin = (xmin - a) / (b - a), zmax = (xmax - a) / (b - a);   // [a, b] -> [0, 1]
  if (zmin > zmax) { const double t = zmin; zmin = zmax; zmax = t; }
  const double z = (order > 2 && std::isfinite(fpb)) ? interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax)
                                                     : interp_quad(fa, fpa * (b - a), fb, zmin, zmax);
  return a + z * (b - a);
}

template <typename Functor>
struct BFGS {
  Functor& fn;
  Parameters parameters;
  int iter = 0;
  double step = 0, delta_f = 0, f = 0, fp0 = 0, g0norm = 0, pnorm = 0;
  double x0[N], g0[N], p[N], dx0[N], dg0[N], gradient[N], dx[N];
  // the function along the line x + alpha p (linear_wrapper.c)
  const double* wx = nullptr;
  double f_alpha = 0, df_alpha = 0, x_alpha[N], g_alpha[N], f_key = 0, df_key = 0, x_key = 0, g_key = 0;

  explicit BFGS(Functor& f_) : fn(f_) {}

  void moveto(double alpha) {
    if (alpha == x_key) return;
    for (int i = 0; i < N; i++) x_alpha[i] = wx[i] + alpha * p[i];
    x_key = alpha;
  }
  double slope() const { return dot(g_alpha, p); }
  double wrap_f(double alpha) {
    if (alpha == f_key) return f_alpha;
    moveto(alpha);
    f_alpha = fn.f(x_alpha);
    f_key = alpha;
    return f_alpha;
  }
  double wrap_df(double alpha) {
    if (alpha == df_key) return df_alpha;
    moveto(alpha);
    if (alpha != g_key) { fn.df(x_alpha, g_alpha); g_key = alpha; }
    df_alpha = slope();
    df_key = alpha;
    return df_alpha;
  }
  void wrap_fdf(double alpha, double* fo, double* dfo) {
    if (alpha == f_key && alpha == df_key) { *fo = f_alpha; *dfo = df_alpha; return; }
    if (alpha == f_key || alpha == df_key) { *fo = wrap_f(alpha); *dfo = wrap_df(alpha); return; }
    moveto(alpha);
    fn.fdf(x_alpha, f_alpha, g_alpha);
    f_key = alpha; g_key = alpha;
    df_alpha = slope();
    df_key = alpha;
    *fo = f_alpha; *dfo = df_alpha;
  }
  void reset_line(const double* x, const double* g) {   // prepare_wrapper / change_direction
    wx = x;
    copy(x_alpha, x); x_key = 0;
    f_key = 0;
    copy(g_alpha, g); g_key = 0;
    df_alpha = slope(); df_key = 0;
  }

  // Fletcher's line search; *alpha_new is written on Success at a trial point only
  Status line_search(double alpha1, double* alpha_new) {
    const double rho = parameters.rho, sigma = parameters.sigma, tau1 = parameters.tau1, tau2 = parameters.tau2, tau3 = parameters.tau3;
    const int order = parameters.order;
    double f0, fp0_, falpha, falpha_prev, fpalpha, fpalpha_prev, delta, alpha_next;
    double alpha = alpha1, alpha_prev = 0.0;
    double a = 0.0, b = alpha, fa, fb = 0.0, fpa, fpb = 0.0;
    const int bracket_iters = 100, section_iters = 100;
    int i = 0;
    wrap_fdf(0.0, &f0, &fp0_);
    falpha_prev = f0; fpalpha_prev = fp0_;
    fa = f0; fpa = fp0_;
    while (i++ < bracket_iters) {                 // bracketing
      falpha = wrap_f(alpha);
      if (falpha > f0 + alpha * rho * fp0_ || falpha >= falpha_prev) {      // Fletcher's rho test
        a = alpha_prev; fa = falpha_prev; fpa = fpalpha_prev;
        b = alpha; fb = falpha; fpb = NAN;
        break;
      }
      fpalpha = wrap_df(alpha);
      if (std::fabs(fpalpha) <= -sigma * fp0_) { *alpha_new = alpha; return Success; }   // Fletcher's sigma test
      if (fpalpha >= 0) {
        a = alpha; fa = falpha; fpa = fpalpha;
        b = alpha_prev; fb = falpha_prev; fpb = fpalpha_prev;
        break;
      }
      delta = alpha - alpha_prev;
      {
        const double lower = alpha + delta, upper = alpha + tau1 * delta;
        alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, lower, upper, order);
      }
      alpha_prev = alpha; falpha_prev = falpha; fpalpha_prev = fpalpha;
      alpha = alpha_next;
    }
    while (i++ < section_iters) {                 // sectioning of the bracket [a, b]
      delta = b - a;
      {
        const double lower = a + tau2 * delta, upper = b - tau3 * delta;
        alpha = interpolate(a, fa, fpa, b, fb, fpb, lower, upper, order);
      }
      falpha = wrap_f(alpha);
      if ((a - alpha) * fpa <= EPS) return NoProgress;   // roundoff prevents progress
      if (falpha > f0 + rho * alpha * fp0_ || falpha >= fa) {
        b = alpha; fb = falpha; fpb = NAN;
      } else {
        fpalpha = wrap_df(alpha);
        if (std::fabs(fpalpha) <= -sigma * fp0_) { *alpha_new = alpha; return Success; }
        if (((b - a) >= 0 && fpalpha >= 0) || ((b - a) <= 0 && fpalpha <= 0)) {
          b = a; fb = fa; fpb = fpa;
          a = alpha; fa = falpha; fpa = fpalpha;
        } else {
          a = alpha; fa = falpha; fpa = fpalpha;
        }
      }
    }
    return Success;
  }

  Status minimizeInit(double* x) {
    iter = 0;
    step = parameters.step_size;
    delta_f = 0;
    for (int i = 0; i < N; i++) dx[i] = dx0[i] = dg0[i] = 0.0;
    fn.fdf(x, f, gradient);
    copy(x0, x);
    copy(g0, gradient);
    g0norm = norm(g0);
    for (int i = 0; i < N; i++) p[i] = gradient[i] * (-1.0 / g0norm);
    pnorm = norm(p);
    fp0 = -g0norm;
    f_alpha = f;
    reset_line(x, gradient);
    return NotStarted;
  }

  Status minimizeOneStep(double* x) {
    double alpha = 0.0, alpha1;
    const double f0 = f;
    if (pnorm == 0.0 || g0norm == 0.0 || fp0 == 0) {
      for (int i = 0; i < N; i++) dx[i] = 0.0;
      return NoProgress;
    }
    if (delta_f < 0) {
      const double d = -delta_f, e = 10 * EPS * std::fabs(f0);
      const double del = d > e ? d : e;
      const double t = 2.0 * del / (-fp0);
      alpha1 = t < 1.0 ? t : 1.0;
    } else {
      alpha1 = std::fabs(step);
    }
    wx = x;
    const Status status = line_search(alpha1, &alpha);
    if (status != Success) return status;
    {                                              // update_position
      double fa_, dfa_;
      wrap_fdf(alpha, &fa_, &dfa_);
      f = fa_;
      copy(x, x_alpha);
      copy(gradient, g_alpha);
    }
    delta_f = f - f0;
    for (int i = 0; i < N; i++) { dx0[i] = x[i] - x0[i]; dx[i] = dx0[i]; dg0[i] = gradient[i] - g0[i]; }
    const double dxg = dot(dx0, gradient), dgg = dot(dg0, gradient), dxdg = dot(dx0, dg0), dgnorm = norm(dg0);
    double A, B;
    if (dxdg != 0) {
      B = dxg / dxdg;
      A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg;
    } else {
      B = 0; A = 0;
    }
    for (int i = 0; i < N; i++) p[i] = (gradient[i] - A * dx0[i]) - B * dg0[i];
    copy(g0, gradient);
    copy(x0, x);
    g0norm = norm(g0);
    pnorm = norm(p);
    const double pg = dot(p, gradient);
    const double dir = pg >= 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < N; i++) p[i] = p[i] * (dir / pnorm);
    pnorm = norm(p);
    fp0 = dot(p, g0);
    reset_line(x, gradient);
    iter++;
    return Success;
  }

  Status testGradient(double epsabs) const {
    if (epsabs < 0) return NegativeGradientEpsilon;
    return norm(gradient) < epsabs ? Success : Running;
  }
};

// the driver loop of estimateRigidTransformationBFGS (:229-241); returns the last status, *inner = inner_iterations_
template <typename Functor>
inline int minimize(BFGS<Functor>& bfgs, double* x, double gradient_tol, int max_inner_iterations, int* inner) {
  int inner_iterations = 0;
  int result = bfgs.minimizeInit(x);
  result = Running;
  do {
    inner_iterations++;
    result = bfgs.minimizeOneStep(x);
    if (result) break;
    result = bfgs.testGradient(gradient_tol);
  } while (result == Running && inner_iterations < max_inner_iterations);
  *inner = inner_iterations;
  return result;
}
// ... and its acceptance test (:242)
inline bool accepted(int result, int inner_iterations, int max_inner_iterations) {
  return result == NoProgress || result == Success || inner_iterations == max_inner_iterations;
}

}  // namespace gicp_bfgs
