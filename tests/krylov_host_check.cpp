// Known answers for the host arithmetic of the Krylov drivers (dynamite_amd/csrc/krylov_host.cpp), as a plain C++
// program for the sanitizers: tests/test_krylov_host.py builds it with -fsanitize=address,undefined and runs it.
// Every floating-point bound is written 8 * m, m the value measured with the same functions before they left
// krylov.cpp, in this program (the Jacobi sweeps stop at a relative off-diagonal of 1e-16 and the residuals scale with
// n).  Two compilers were used, the larger value counts; where both gave exactly 0, m is one unit of rounding of the
// compared number (2.2e-16 times its size).  A bound of 0 is an exact comparison of exactly representable numbers.
#include <cstdio>

#include "../dynamite_amd/csrc/krylov_host.h"

using namespace dnm;

static int failures = 0;

static void check(const char *what, double measured, double bound) {
  const bool ok = measured <= bound;      // (false for a NaN)
  printf("%-52s %.3e  (bound %.1e)%s\n", what, measured, bound, ok ? "" : "   FAILED");
  if (!ok) ++failures;
}
static void check_true(const char *what, bool ok) {
  printf("%-52s %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

// exp(i t [[0, 1], [1, 0]]) = [[cos t, i sin t], [i sin t, cos t]]
static double expm_pauli_x(double t) {
  std::vector<zc> A = {zc(0), zc(0, t), zc(0, t), zc(0)}, E;
  if (zexpm(2, A, E)) return 1e300;
  const zc want[4] = {zc(std::cos(t)), zc(0, std::sin(t)), zc(0, std::sin(t)), zc(std::cos(t))};
  double err = 0;
  for (int i = 0; i < 4; ++i) err = std::max(err, std::abs(E[i] - want[i]));
  return err;
}

static void dense_checks() {
  check("zexpm: i 0.7 sigma_x against cos, sin", expm_pauli_x(0.7), 8 * 1.2e-16);
  check("zexpm: i 10 sigma_x (|A|_1 > 5.37: squaring)", expm_pauli_x(10.0), 8 * 5.6e-16);
  {
    const zc d[3] = {zc(0.3, -1.1), zc(-2.0, 0.4), zc(0.0, 2.5)};
    std::vector<zc> A(9, zc(0)), E;
    for (int i = 0; i < 3; ++i) A[(size_t)i * 3 + i] = d[i];
    double err = zexpm(3, A, E) ? 1e300 : 0.0;
    for (int j = 0; j < 3 && err < 1e300; ++j)
      for (int i = 0; i < 3; ++i)
        err = std::max(err, std::abs(E[(size_t)j * 3 + i] - (i == j ? std::exp(d[i]) : zc(0))));
    check("zexpm: diagonal matrix", err, 8 * 2.3e-16);
  }
  {
    // A = [[0, 2, 1], [1, 1, 0], [3, 0, 1]] (column-major below): the first pivot is zero
    const std::vector<zc> A0 = {zc(0), zc(1), zc(3), zc(2), zc(1), zc(0), zc(1), zc(0), zc(1, 0.5)};
    std::vector<zc> A = A0, X(9, zc(0)), P;
    for (int i = 0; i < 3; ++i) X[(size_t)i * 3 + i] = 1.0;
    double err = zsolve(3, A, X) ? 1e300 : 0.0;
    zgemm(3, A0, X, P);
    for (int j = 0; j < 3 && err < 1e300; ++j)
      for (int i = 0; i < 3; ++i) err = std::max(err, std::abs(P[(size_t)j * 3 + i] - (i == j ? zc(1) : zc(0))));
    check("zsolve: A A^-1 = 1 with a zero first pivot", err, 8 * 5.8e-17);
    std::vector<zc> Z(9, zc(0)), B(9, zc(1));
    check_true("zsolve: a singular matrix is refused", zsolve(3, Z, B) == 1);
  }
}

// the n = 12 second-difference matrix: eigenvalues 2 - 2 cos(k pi / 13), k = 1..12
static void tridiagonal_checks() {
  const int n = 12;
  std::vector<double> al(n, 2.0), be(n - 1, 1.0), want(n);
  for (int k = 1; k <= n; ++k) want[k - 1] = 2.0 - 2.0 * std::cos(k * M_PI / (n + 1));
  std::vector<double> A((size_t)n * n, 0.0), w, S;
  for (int i = 0; i < n; ++i) {
    A[(size_t)i * n + i] = 2.0;
    if (i + 1 < n) A[(size_t)(i + 1) * n + i] = A[(size_t)i * n + i + 1] = -1.0;
  }
  const std::vector<double> A0 = A;
  jacobi_eig(n, A, w, S);
  std::vector<double> ws = w;
  std::sort(ws.begin(), ws.end());
  double err = 0, res = 0;
  for (int k = 0; k < n; ++k) err = std::max(err, std::fabs(ws[k] - want[k]));
  for (int c = 0; c < n; ++c)
    for (int i = 0; i < n; ++i) {
      double r = -w[c] * S[(size_t)c * n + i];
      for (int k = 0; k < n; ++k) r += A0[(size_t)k * n + i] * S[(size_t)c * n + k];
      res = std::max(res, std::fabs(r));
    }
  check("jacobi_eig: eigenvalues of the second difference", err, 8 * 4.5e-15);
  check("jacobi_eig: max |A S - S w|", res, 8 * 2.5e-15);
  // (off-diagonal +1 instead of -1: the same spectrum)
  std::vector<double> z;
  double terr = 0, tres = 0;
  for (int k = 0; k < n; ++k) {
    const double th = tridiag_eigpair(al, be, n, k, z);
    terr = std::max(terr, std::fabs(th - want[k]));
    for (int i = 0; i < n; ++i) {
      const double r = (i > 0 ? z[i - 1] : 0.0) + (i + 1 < n ? z[i + 1] : 0.0) + (2.0 - th) * z[i];
      tres = std::max(tres, std::fabs(r));
    }
  }
  check("tridiag_eigpair: eigenvalues", terr, 8 * 8.9e-16);
  check("tridiag_eigpair: max |T z - theta z|", tres, 8 * 2.3e-16);
  bool counts = sturm_count(al, be, n, want[0] - 0.01) == 0 && sturm_count(al, be, n, want[n - 1] + 0.01) == n;
  for (int k = 0; k + 1 < n; ++k) counts = counts && sturm_count(al, be, n, 0.5 * (want[k] + want[k + 1])) == k + 1;
  check_true("sturm_count: between every two eigenvalues", counts);
  // tridiag_ritz is new with the move: Jacobi against bisection, each with the error measured above; the vectors to
  // the rounding of a 12-term inner product.  be one longer than needed, as the probes hand it over.
  std::vector<double> be1 = be, rw, rS, zlo, zhi;
  be1.push_back(0.37);
  tridiag_ritz(al, be1, rw, rS);
  const double lo = tridiag_eigpair(al, be, n, 0, zlo), hi = tridiag_eigpair(al, be, n, n - 1, zhi);
  const double rlo = *std::min_element(rw.begin(), rw.end()), rhi = *std::max_element(rw.begin(), rw.end());
  check("tridiag_ritz: lowest value against tridiag_eigpair", std::fabs(rlo - lo), 8 * (4.5e-15 + 8.9e-16));
  check("tridiag_ritz: highest value against tridiag_eigpair", std::fabs(rhi - hi), 8 * (4.5e-15 + 8.9e-16));
  const int ilo = (int)(std::min_element(rw.begin(), rw.end()) - rw.begin());
  double dots = 0;
  for (int i = 0; i < n; ++i) dots += rS[(size_t)ilo * n + i] * zlo[i];
  check("tridiag_ritz: lowest vector against tridiag_eigpair", std::fabs(std::fabs(dots) - 1.0), 8 * 12 * 2.3e-16);
}

static void hermitian_check() {
  const int n = 8;
  std::vector<zc> A((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = i; j < n; ++j) {
      const zc v = i == j ? zc(std::cos(1.0 + i), 0) : zc(std::sin(1.0 + 3 * i + j), std::cos(2.0 + i * j + 0.5 * j));
      A[(size_t)i * n + j] = v;
      A[(size_t)j * n + i] = std::conj(v);
    }
  const std::vector<zc> A0 = A;
  std::vector<double> w;
  std::vector<zc> Q;
  hjacobi_eig(n, A, w, Q);
  double res = 0, uni = 0;
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i < n; ++i) {
      zc r = -w[c] * Q[(size_t)c * n + i];
      for (int k = 0; k < n; ++k) r += A0[(size_t)i * n + k] * Q[(size_t)c * n + k];
      res = std::max(res, std::abs(r));
    }
    for (int c2 = 0; c2 < n; ++c2) {
      zc g = 0;
      for (int k = 0; k < n; ++k) g += std::conj(Q[(size_t)c * n + k]) * Q[(size_t)c2 * n + k];
      uni = std::max(uni, std::abs(g - (c == c2 ? zc(1) : zc(0))));
    }
  }
  check("hjacobi_eig: max |A q - w q|, 8 x 8 complex", res, 8 * 2.7e-15);
  check("hjacobi_eig: max |Q^H Q - 1|", uni, 8 * 2.3e-15);
}

static void expansion_checks() {
  for (double z : {0.5, 10.0, 64.0}) {
    std::vector<double> J;
    double tail = -1;
    const double cut = 1e-12;
    check_true("cheb_coeffs: the coefficients have decayed", cheb_coeffs(z, cut, J, &tail) == 0);
    double s = J[0] * J[0];
    for (size_t k = 1; k < J.size(); ++k) s += 2.0 * J[k] * J[k];
    // J_0^2 + 2 sum J_k^2 = 1: what the kept terms miss is 2 sum_{k > K} J_k^2 <= tail^2, the rest is rounding
    check("cheb_coeffs: |1 - J_0^2 - 2 sum_{k <= K} J_k^2| - tail^2", std::fabs(1.0 - s) - tail * tail, 8 * 5.6e-16);
    check_true("cheb_coeffs: 0 <= tail < cut", tail >= 0 && tail < cut);
  }
  int ns = 0;
  double zs = 0;
  cheb_steps(200.0, &ns, &zs);
  check_true("cheb_steps: 200 in four steps of 50", ns == 4 && zs == 50.0);
  check("round2: 0.0123456 -> 0.012", std::fabs(round2(0.0123456) - 0.012), 8 * 2.3e-16 * 0.012);
  check("round2: 3.78 -> 3.8", std::fabs(round2(3.78) - 3.8), 8 * 4.5e-16);
  check("round2: 0.95 -> 1.0", std::fabs(round2(0.95) - 1.0), 8 * 2.3e-16);
  check("round2: 1234.5 -> 1200", std::fabs(round2(1234.5) - 1200.0), 0.0);
}

// new with the move: no earlier version to measure, the bounds are reasoned
static void probe_choice_checks() {
  {
    // A flat synthetic spectrum: kk equally spaced Ritz values in [-1, 1] with equal weights stand for Nglob levels of
    // constant density Nglob (kk - 1) / (2 kk) between the outermost midpoints.  The bisection (60 halvings) finds the
    // half-width to rounding, so the levels counted in [target - a, target + a] are nev + max(4, nev / 2) to far
    // within the one level spacing allowed here.
    const int kk = 60, nev = 10;
    const int64_t Nglob = 1000;
    std::vector<double> w(kk), S((size_t)kk * kk, 0.0);
    for (int i = 0; i < kk; ++i) {
      w[(kk - 1 - i + 7) % kk] = -1.0 + 2.0 * i / (kk - 1);        // (unsorted, as jacobi_eig hands them over)
    }
    for (int i = 0; i < kk; ++i) S[(size_t)i * kk] = 1.0 / std::sqrt((double)kk);
    const InteriorWindow win = interior_window(w, S, 0.25, 5.0, Nglob, nev, 0.1, 1.0);
    const double density = (double)Nglob * (kk - 1) / (2.0 * kk);
    check_true("interior_window: nwant = nev + max(4, nev / 2)", win.nwant == 15.0);
    check("interior_window: levels in the window against nwant", std::fabs(2.0 * win.a * density - win.nwant), 1.0);
    // (last components zero: the ends move out by one per cent of the width alone)
    check("interior_window: emin = -1 - 0.01 width", std::fabs(win.emin + 1.02), 4 * 2.3e-16);
    check("interior_window: emax = +1 + 0.01 width", std::fabs(win.emax - 1.02), 4 * 2.3e-16);
    const InteriorWindow narrow = interior_window(w, S, 0.25, 5.0, Nglob, nev, 0.1, 0.2);
    check("interior_window: the knob's factor scales a", std::fabs(narrow.a - 0.2 * win.a), 4 * 2.3e-16 * win.a);
  }
  {
    // Ritz values with a known gap: the wanted three end at 0.2, the cut (margin 2) is at 0.3, the far end
    // min(|H|, 10 + 0.5): gam = 0.1 / 10.2, d = ceil(3.3 / (2 sqrt(gam))) = 17 (odd already)
    std::vector<double> wv = {0.0, 0.1, 0.2, 0.25, 0.3, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0};
    const int nev = 3;
    check_true("end_filter_margin(3) = 2", end_filter_margin(nev) == 2);
    const EndFilterChoice lo = end_filter_choice(wv, 0.5, 100.0, nev, true, nullptr);
    const double gam = (0.3 - 0.2) / (10.5 - 0.3);
    int d = (int)std::ceil(3.3 / (2.0 * std::sqrt(gam)));
    d = std::max(5, std::min(d, 49)) | 1;
    check_true("end_filter_choice: lowest, usable, degree 17", lo.usable && lo.p.d == d && d == 17);
    check_true("end_filter_choice: lowest, ref, c, h", lo.p.ref == 0.0 && lo.p.c == 0.5 * (0.3 + 10.5) &&
               lo.p.h == 0.5 * (10.5 - 0.3) && lo.a_cut == 0.3 && lo.near_t == 0.2 && lo.far == 10.5);
    // the norm bounds the far end; the degree is clamped to [5, 49]: gam = 0.1 / 0.7 gives 5
    const EndFilterChoice tight = end_filter_choice(wv, 0.5, 1.0, nev, true, nullptr);
    check_true("end_filter_choice: |H| bounds the far end, d >= 5", tight.usable && tight.far == 1.0 && tight.p.d == 5);
    const EndFilterChoice hi = end_filter_choice(wv, 0.5, 100.0, nev, false, nullptr);
    // highest: wanted 8, 9, 10, cut at 6, far end max(-|H|, 0 - 0.5): gam = 2 / 6.5 -> 3 -> clamped to 5
    check_true("end_filter_choice: highest", hi.usable && hi.p.ref == 10.0 && hi.a_cut == 6.0 && hi.near_t == 8.0 &&
               hi.far == -0.5 && hi.p.d == 5 && hi.p.c == 0.5 * (6.0 - 0.5) && hi.p.h == 0.5 * 6.5);
    check_true("end_filter_choice: the degree knob, made odd", end_filter_choice(wv, 0.5, 100.0, nev, true, "8").p.d == 9);
    std::vector<double> flat(15, 1.0);
    check_true("end_filter_choice: degenerate values are not usable",
               !end_filter_choice(flat, 0.0, 100.0, nev, true, nullptr).usable);
  }
  {
    const std::vector<double> al = {1.0, -3.0, 2.0}, be = {0.5, 4.0};
    check_true("StopRule: eps (|alpha_j| + 1)", StopRule::alpha(1e-12).threshold(al, be) == 1e-12 * 3.0);
    check_true("StopRule: eps |H|", StopRule::norm(1e-12, 7.0).threshold(al, be) == 1e-12 * 7.0);
    check_true("StopRule: eps max(1, max |alpha_i| + beta_i)", StopRule::running(1e-10).threshold(al, be) == 1e-10 * 7.0);
  }
}

int main() {
  dense_checks();
  tridiagonal_checks();
  hermitian_check();
  expansion_checks();
  probe_choice_checks();
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
