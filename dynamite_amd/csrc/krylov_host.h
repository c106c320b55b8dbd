// The host arithmetic of the Krylov drivers (krylov.cpp): small dense matrices, tridiagonal eigenpairs, expansion
// coefficients, the re-orthogonalisation monitors and the choices the solvers make from a Lanczos probe.  Nothing
// here touches the device or the operator handle, so a plain C++ program checks it under the sanitizers
// (tests/krylov_host_check.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

namespace dnm {

typedef std::complex<double> zc;

// small dense helpers (column-major, leading dimension = n)
void zgemm(int n, const std::vector<zc> &A, const std::vector<zc> &B, std::vector<zc> &C);
int zsolve(int n, std::vector<zc> &A, std::vector<zc> &Bm);
int zexpm(int n, const std::vector<zc> &Ain, std::vector<zc> &E);
void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &w, std::vector<double> &Sv);
void hjacobi_eig(int n, std::vector<zc> &A, std::vector<double> &w, std::vector<zc> &Q);
// a symmetric tridiagonal matrix T (diagonal a[0..n), off-diagonal b[0..n-1))
int sturm_count(const std::vector<double> &a, const std::vector<double> &b, int n, double x);
double tridiag_eigpair(const std::vector<double> &a, const std::vector<double> &b, int n, int k, std::vector<double> &z);
void tridiag_ritz(const std::vector<double> &al, const std::vector<double> &be, std::vector<double> &w,
                  std::vector<double> &S);
// Chebyshev expansion of exp(-i t A) (cheb_coeffs returns 1 when the coefficients have not decayed); Expokit's rounding
int cheb_coeffs(double z, double cut, std::vector<double> &J, double *tail_out);
void cheb_steps(double ztot, int *nsteps, double *z);
double round2(double t);
double pro_threshold(double eps1, double tol, const char *forced);

// When a plain Lanczos run (plain_lanczos, krylov.cpp) stops: beta_{j+1} <= eps * scale, an invariant subspace.  Its
// three users measure against different scales, and differ in whether that last beta is still recorded.
struct StopRule {
  enum Scale { ALPHA, FIXED, RUNNING } scale;
  double eps, fixed;
  bool record_last;
  static StopRule alpha(double eps) { return {ALPHA, eps, 0.0, true}; }              // eps (|alpha_j| + 1)
  static StopRule norm(double eps, double nrm) { return {FIXED, eps, nrm, true}; }   // eps |H|
  static StopRule running(double eps) { return {RUNNING, eps, 0.0, false}; }         // eps max(1, max_i |alpha_i| + beta_i)
  // al: alpha_0..alpha_j; be: the betas recorded so far (beta_{j+1} not among them)
  double threshold(const std::vector<double> &al, const std::vector<double> &be) const {
    if (scale == ALPHA) return eps * (std::fabs(al.back()) + 1.0);
    if (scale == FIXED) return eps * fixed;
    double s = 0;
    for (size_t i = 0; i < al.size(); ++i) s = std::max(s, std::fabs(al[i]) + (i < be.size() ? be[i] : 0.0));
    return eps * std::max(1.0, s);
  }
};

// Simon's omega-recurrence: a running estimate of |v_{j+1}^H v_k| for a Lanczos
// process without re-orthogonalisation.  While every estimate stays below
// sqrt(eps) the three-term recurrence is kept (5 vector passes per step);
// when one crosses it the new vector and its successor are orthogonalised
// against the whole basis (partial re-orthogonalisation, Simon 1984; the trigger level: pro_threshold).
// OmegaRows is what the plain and the thick-restart recurrence share.
struct OmegaRows {
  std::vector<double> alpha, beta;      // alpha[j]; beta[j] = ||r_{j-1}|| (beta[0] = 0)
  std::vector<double> wprev, wcur;      // omega_{j-1,.}, omega_{j,.}
  double eps1 = 0, thresh = 0;
  bool force_next = false;
  int reorths = 0;
  void setup(int m, double n_global, double tol, const char *forced_thresh) {
    alpha.assign(m + 2, 0.0);
    beta.assign(m + 2, 0.0);
    wprev.assign(m + 2, 0.0);
    wcur.assign(m + 2, 0.0);
    const double eps = 2.220446049250313e-16;
    eps1 = eps * std::sqrt(n_global) / 2.0;
    if (eps1 > 1e-11) eps1 = 1e-11;
    thresh = pro_threshold(eps1, tol, forced_thresh);
  }
  // wnew = omega_{j+1,.}, `worst` its largest entry below j: it becomes the current row; true when v_{j+1} needs a full pass
  bool advance(int j, std::vector<double> &wnew, double worst) {
    wnew[j] = eps1;
    wnew[j + 1] = 1.0;
    wprev.swap(wcur);
    wcur.swap(wnew);
    const bool need = force_next || worst > thresh;
    if (need) {
      force_next = !force_next;          // the successor of a re-orthogonalised vector gets a pass too
      for (int k = 0; k <= j; ++k) wcur[k] = eps1;
      ++reorths;
    }
    return need;
  }
};

struct LanczosMonitor : OmegaRows {
  void reset(int m, double n_global, double tol, const char *forced_thresh) {
    setup(m, n_global, tol, forced_thresh);
    wcur[0] = 1.0;
    force_next = false;
  }
  // step j produced alpha_j and beta_{j+1}; returns true when v_{j+1} needs a full pass
  bool update(int j, double a_j, double b_next) {
    alpha[j] = a_j;
    beta[j + 1] = b_next;
    std::vector<double> wnew(wcur.size(), 0.0);
    double worst = 0.0;
    if (b_next > 0) {
      for (int k = 0; k < j; ++k) {
        double v = beta[k + 1] * wcur[k + 1] + (alpha[k] - a_j) * wcur[k] - beta[j] * wprev[k];
        if (k > 0) v += beta[k] * wcur[k - 1];
        v = (v + (v >= 0 ? eps1 : -eps1)) / b_next;
        wnew[k] = v;
        worst = std::max(worst, std::fabs(v));
      }
    }
    return advance(j, wnew, worst);
  }
};

// The same estimate for thick-restart Lanczos.  The basis of a cycle is
// q_0..q_{l-1} (kept Ritz vectors, H u_i = theta_i u_i + s_i q_l), then Lanczos vectors
// q_l, q_{l+1}, ...; with T the projected matrix (diag(theta) + spike row/column l +
// tridiagonal beyond), omega_{j+1,i} = q_{j+1}^H q_i obeys
//   beta_{j+1} omega_{j+1,i} = sum_k T_{k,i} omega_{j,k} - alpha_j omega_{j,i} - beta_j omega_{j-1,i}   (j > l),
// the step j = l being orthogonalised against the whole basis explicitly (it has to
// remove the spike components anyway).
struct RestartMonitor : OmegaRows {
  int l = 0, steps = 0;
  std::vector<double> th, sp;
  // start of a cycle: row_l[i] bounds |q_l^H u_i|
  void begin_cycle(int l_, const std::vector<double> &theta, const std::vector<double> &spike,
                   const std::vector<double> &row_l) {
    l = l_;
    th = theta;
    sp = spike;
    std::fill(wprev.begin(), wprev.end(), 0.0);
    std::fill(wcur.begin(), wcur.end(), 0.0);
    for (int i = 0; i < l; ++i) wcur[i] = std::max(eps1, i < (int)row_l.size() ? row_l[i] : eps1);
    wcur[l] = 1.0;
    force_next = false;
  }
  // step j = l was orthogonalised against q_0..q_l explicitly
  void first_step(double a_l, double b_next) {
    alpha[l] = a_l;
    beta[l + 1] = b_next;
    wprev = wcur;
    std::fill(wcur.begin(), wcur.end(), 0.0);
    for (int i = 0; i <= l; ++i) wcur[i] = eps1;
    wcur[l + 1] = 1.0;
  }
  // step j > l produced alpha_j, beta_{j+1} by the three-term recurrence; true: q_{j+1} needs a full pass
  bool update(int j, double a_j, double b_next) {
    alpha[j] = a_j;
    beta[j + 1] = b_next;
    ++steps;
    std::vector<double> wnew(wcur.size(), 0.0);
    double worst = 0.0;
    if (b_next > 0) {
      for (int i = 0; i < j; ++i) {
        double v;
        if (i < l) {
          v = th[i] * wcur[i] + sp[i] * wcur[l];
        } else if (i == l) {
          v = alpha[l] * wcur[l] + beta[l + 1] * wcur[l + 1];
          for (int k = 0; k < l; ++k) v += sp[k] * wcur[k];
        } else {
          v = beta[i] * wcur[i - 1] + alpha[i] * wcur[i] + beta[i + 1] * wcur[i + 1];
        }
        v -= a_j * wcur[i] + beta[j] * wprev[i];
        v = (v + (v >= 0 ? eps1 : -eps1)) / b_next;
        wnew[i] = v;
        worst = std::max(worst, std::fabs(v));
      }
    }
    return advance(j, wnew, worst);
  }
};

// The numbers of the Chebyshev filter p(A) = T_d((A - c) / h) / T_d((ref - c) / h) (ChebFilter, krylov.cpp).  2 A x is
// avoided by halving the recurrence: u_j = s_j / 2^(j-1)  =>  u_{j+1} = (A - c) u_j - (h/2)^2 u_{j-1},
// u_1 = (A - c) u_0, u_2 = (A - c) u_1 - (h^2/2) u_0
struct ChebPoly {
  int d = 0;
  double c = 0, h = 0, ref = 0;
  double log_tref() const {                // log |T_d((ref - c) / h)|
    const double at = std::fabs((ref - c) / h);
    return at > 1.0 ? d * std::log(at + std::sqrt(at * at - 1.0)) - std::log(2.0) : 0.0;
  }
  double step_b(int j) const { return j == 1 ? 0.0 : (j == 2 ? 0.5 * h * h : 0.25 * h * h); }    // factor of u_{j-2}
  // u_d = h^d T_d / 2^(d-1); normalise by the value at the reference point so that the wanted end is O(1..)
  double log_scale() const { return -(d * std::log(h) - (d - 1) * std::log(2.0)) - log_tref(); }
  // A Ritz pair (mu, absolute residual res_p) of p(A) seen from A: mu = p(lambda) inverted on the wanted side and
  // the residual divided by the slope |p'(lambda)| -- what the residual in A is when the error lies along
  // neighbouring eigenvectors (components deep inside the damped interval count with |mu| / 2h instead; the
  // measured residual decides in the end).  Returns the relative residual estimate, *lam the eigenvalue estimate.
  double seen_from_a(double mu, double res_p, bool low_side, double *lam) const {
    const double a = std::fabs(mu) * std::exp(log_tref());
    if (!(a > 1.0)) { *lam = c; return 1e300; }              // inside the damped interval: not a wanted pair
    const double th = std::acosh(a) / d;
    *lam = low_side ? c - h * std::cosh(th) : c + h * std::cosh(th);
    const double slope = d * std::tanh(d * th) / (h * std::sinh(th)) * std::fabs(mu);
    return res_p / slope / std::max(std::fabs(*lam), 1e-300);
  }
};

// ... and of the folded filter p(A) = T_d((G - c) / e) / T_d(-c / e), G = (A - sigma)^2 (FoldFilter, krylov.cpp)
struct FoldPoly {
  int d = 0;
  double sigma = 0, c = 0, e = 0;
  double theta0() const { return std::acosh(c / e); }
  double bound() const { return 1.0 / std::cosh(d * theta0()); }      // |p| on the unwanted part
  double step_b(int j) const { return j == 1 ? 0.0 : (j == 2 ? 0.5 * e * e : 0.25 * e * e); }
  // what brings u_d to p(A) x, `ltaken` the log of the growth taken out on the way; T_d(-c / e) = (-1)^d cosh(d acosh(c / e))
  double scale(double ltaken) const {
    const double dth = d * theta0();
    const double logT = dth - std::log(2.0) + std::log1p(std::exp(-2.0 * dth));
    const double logscale = ltaken - (d * std::log(e) - (d - 1) * std::log(2.0)) - logT;
    return ((d & 1) ? -1.0 : 1.0) * std::exp(logscale);
  }
};

// The end filter of dnm_eigsolve, from the probe's Ritz values wv (ascending, at least nev + end_filter_margin(nev) + 2
// of them), its last residual norm blast and nrmH >= |H|; lowest: the wanted end; degree_knob: DNM_EIGS_FILTER_DEGREE
struct EndFilterChoice {
  bool usable;                             // false: no usable gap estimate (degenerate Ritz values)
  ChebPoly p;
  double a_cut, far, near_t, gam;          // for the trace
};
int end_filter_margin(int nev);
EndFilterChoice end_filter_choice(const std::vector<double> &wv, double blast, double nrmH, int nev, bool lowest,
                                  const char *degree_knob);

// The window of dnm_eigsolve_interior from the probe's Ritz pairs (w, S) (tridiag_ritz) and its last residual norm;
// factor: DNM_EIGS_INTERIOR_WINDOW, 1 without the knob
struct InteriorWindow {
  double emin, emax, a, nwant;
};
InteriorWindow interior_window(const std::vector<double> &w, const std::vector<double> &S, double blast, double nrmH,
                               int64_t Nglob, int nev, double target, double factor);

}  // namespace dnm
