// Host arithmetic of the Krylov drivers: see krylov_host.h.  No device call, no operator handle.
#include "krylov_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace dnm {

// ---- small dense helpers (column-major, leading dimension = n) -----------------------------------------------------
void zgemm(int n, const std::vector<zc> &A, const std::vector<zc> &B, std::vector<zc> &C) {
  C.assign((size_t)n * n, zc(0));
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < n; ++k) {
      const zc b = B[(size_t)j * n + k];
      if (b == zc(0)) continue;
      for (int i = 0; i < n; ++i) C[(size_t)j * n + i] += A[(size_t)k * n + i] * b;
    }
}

// solve A X = B in place (B overwritten by X), partial pivoting; A destroyed
int zsolve(int n, std::vector<zc> &A, std::vector<zc> &Bm) {
  for (int c = 0; c < n; ++c) {
    int piv = c;
    double best = std::abs(A[(size_t)c * n + c]);
    for (int r = c + 1; r < n; ++r)
      if (std::abs(A[(size_t)c * n + r]) > best) { best = std::abs(A[(size_t)c * n + r]); piv = r; }
    if (best == 0.0) return 1;
    if (piv != c) {
      for (int j = 0; j < n; ++j) {
        std::swap(A[(size_t)j * n + c], A[(size_t)j * n + piv]);
        std::swap(Bm[(size_t)j * n + c], Bm[(size_t)j * n + piv]);
      }
    }
    const zc inv = zc(1) / A[(size_t)c * n + c];
    for (int r = c + 1; r < n; ++r) {
      const zc f = A[(size_t)c * n + r] * inv;
      if (f == zc(0)) continue;
      for (int j = c; j < n; ++j) A[(size_t)j * n + r] -= f * A[(size_t)j * n + c];
      for (int j = 0; j < n; ++j) Bm[(size_t)j * n + r] -= f * Bm[(size_t)j * n + c];
    }
  }
  for (int j = 0; j < n; ++j)
    for (int r = n - 1; r >= 0; --r) {
      zc s = Bm[(size_t)j * n + r];
      for (int k = r + 1; k < n; ++k) s -= A[(size_t)k * n + r] * Bm[(size_t)j * n + k];
      Bm[(size_t)j * n + r] = s / A[(size_t)r * n + r];
    }
  return 0;
}

// exp(A) by scaling and squaring with the diagonal Pade approximant of degree
// 13 (Higham 2005 coefficients), complex dense.
int zexpm(int n, const std::vector<zc> &Ain, std::vector<zc> &E) {
  static const double b[14] = {64764752532480000., 32382376266240000., 7771770303897600.,
                               1187353796428800.,  129060195264000.,   10559470521600.,
                               670442572800.,      33522128640.,       1323241920.,
                               40840800.,          960960.,            16380.,
                               182.,               1.};
  double nrm = 0;
  for (int j = 0; j < n; ++j) {
    double cs = 0;
    for (int i = 0; i < n; ++i) cs += std::abs(Ain[(size_t)j * n + i]);
    nrm = std::max(nrm, cs);
  }
  int s = 0;
  const double theta13 = 5.371920351148152;
  if (nrm > theta13) s = std::max(0, (int)std::ceil(std::log2(nrm / theta13)));
  std::vector<zc> A = Ain;
  const double sc = std::ldexp(1.0, -s);
  for (auto &v : A) v *= sc;
  std::vector<zc> A2, A4, A6, U, V, T1, T2;
  zgemm(n, A, A, A2);
  zgemm(n, A2, A2, A4);
  zgemm(n, A4, A2, A6);
  const size_t nn = (size_t)n * n;
  // U = A [A6 (b13 A6 + b11 A4 + b9 A2) + b7 A6 + b5 A4 + b3 A2 + b1 I]
  T1.assign(nn, zc(0));
  for (size_t i = 0; i < nn; ++i) T1[i] = b[13] * A6[i] + b[11] * A4[i] + b[9] * A2[i];
  zgemm(n, A6, T1, T2);
  for (size_t i = 0; i < nn; ++i) T2[i] += b[7] * A6[i] + b[5] * A4[i] + b[3] * A2[i];
  for (int i = 0; i < n; ++i) T2[(size_t)i * n + i] += b[1];
  zgemm(n, A, T2, U);
  // V = A6 (b12 A6 + b10 A4 + b8 A2) + b6 A6 + b4 A4 + b2 A2 + b0 I
  for (size_t i = 0; i < nn; ++i) T1[i] = b[12] * A6[i] + b[10] * A4[i] + b[8] * A2[i];
  zgemm(n, A6, T1, V);
  for (size_t i = 0; i < nn; ++i) V[i] += b[6] * A6[i] + b[4] * A4[i] + b[2] * A2[i];
  for (int i = 0; i < n; ++i) V[(size_t)i * n + i] += b[0];
  // (V - U) E = (V + U)
  std::vector<zc> P(nn), Q(nn);
  for (size_t i = 0; i < nn; ++i) { P[i] = V[i] + U[i]; Q[i] = V[i] - U[i]; }
  if (zsolve(n, Q, P)) return 1;
  E.swap(P);
  for (int k = 0; k < s; ++k) {
    zgemm(n, E, E, T1);
    E.swap(T1);
  }
  return 0;
}

// cyclic Jacobi for a dense real symmetric matrix: A = S diag(w) S^T
void jacobi_eig(int n, std::vector<double> &A, std::vector<double> &w, std::vector<double> &Sv) {
  Sv.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) Sv[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        if (i != j) off += A[(size_t)j * n + i] * A[(size_t)j * n + i];
        else diag += A[(size_t)j * n + i] * A[(size_t)j * n + i];
      }
    if (off <= 1e-32 * (diag + 1e-300)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)q * n + p];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < n; ++k) {   // columns p, q
          const double akp = A[(size_t)p * n + k], akq = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * akp - s * akq;
          A[(size_t)q * n + k] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {   // rows p, q
          const double apk = A[(size_t)k * n + p], aqk = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * apk - s * aqk;
          A[(size_t)k * n + q] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double skp = Sv[(size_t)p * n + k], skq = Sv[(size_t)q * n + k];
          Sv[(size_t)p * n + k] = c * skp - s * skq;
          Sv[(size_t)q * n + k] = s * skp + c * skq;
        }
      }
  }
  w.resize(n);
  for (int i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
}

// Eigen-decomposition of a small Hermitian matrix (row-major n x n, destroyed) by cyclic Jacobi rotations
// J = [[c, s ph], [-s conj(ph), c]], ph = a_pq / |a_pq|: w the eigenvalues (unsorted), Q[c * n + k] component k of
// eigenvector c -- the layout jacobi_eig uses.  The Rayleigh-Ritz step of the interior solver in H, whose projected
// matrix is complex for a complex operator.
void hjacobi_eig(int n, std::vector<zc> &A, std::vector<double> &w, std::vector<zc> &Q) {
  Q.assign((size_t)n * n, zc(0));
  for (int i = 0; i < n; ++i) Q[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int p = 0; p < n; ++p) {
      dg += std::norm(A[(size_t)p * n + p]);
      for (int q = p + 1; q < n; ++q) off += std::norm(A[(size_t)p * n + q]);
    }
    if (off <= 1e-34 * (dg + off)) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const zc apq = A[(size_t)p * n + q];
        const double g = std::abs(apq);
        const double app = A[(size_t)p * n + p].real(), aqq = A[(size_t)q * n + q].real();
        if (g <= 1e-300 || g <= 1e-20 * (std::fabs(app) + std::fabs(aqq))) continue;
        const zc ph = apq / g;
        const double tau = (aqq - app) / (2.0 * g);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        const zc sp = s * ph, spc = s * std::conj(ph);
        for (int k = 0; k < n; ++k) {           // columns p, q: A <- A J
          const zc akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - spc * akq;
          A[(size_t)k * n + q] = sp * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {           // rows p, q: A <- J^H A
          const zc apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - sp * aqk;
          A[(size_t)q * n + k] = spc * apk + c * aqk;
        }
        A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0;
        A[(size_t)p * n + p] = A[(size_t)p * n + p].real();
        A[(size_t)q * n + q] = A[(size_t)q * n + q].real();
        for (int k = 0; k < n; ++k) {           // eigenvectors: Q <- Q J (stored transposed)
          const zc vkp = Q[(size_t)p * n + k], vkq = Q[(size_t)q * n + k];
          Q[(size_t)p * n + k] = c * vkp - spc * vkq;
          Q[(size_t)q * n + k] = sp * vkp + c * vkq;
        }
      }
  }
  w.resize(n);
  for (int i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i].real();
}

// ---- symmetric tridiagonal matrices --------------------------------------------------------------------------------
int sturm_count(const std::vector<double> &a, const std::vector<double> &b, int n, double x) {
  int cnt = 0;
  double q = a[0] - x;
  if (q < 0) ++cnt;
  for (int i = 1; i < n; ++i) {
    const double den = std::fabs(q) > 1e-300 ? q : (q < 0 ? -1e-300 : 1e-300);
    q = a[i] - x - b[i - 1] * b[i - 1] / den;
    if (q < 0) ++cnt;
  }
  return cnt;
}

// k-th smallest eigenvalue of T by bisection, its eigenvector (unit norm) by inverse iteration
double tridiag_eigpair(const std::vector<double> &a, const std::vector<double> &b, int n, int k,
                              std::vector<double> &z) {
  double lo = a[0], hi = a[0], nrm = 0;
  for (int i = 0; i < n; ++i) {
    const double r = (i > 0 ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < n ? std::fabs(b[i]) : 0.0);
    lo = std::min(lo, a[i] - r);
    hi = std::max(hi, a[i] + r);
    nrm = std::max(nrm, std::fabs(a[i]) + r);
  }
  for (int it = 0; it < 200 && hi - lo > 4e-16 * std::max(nrm, 1e-300); ++it) {
    const double mid = 0.5 * (lo + hi);
    if (sturm_count(a, b, n, mid) > k) hi = mid; else lo = mid;
  }
  const double theta = 0.5 * (lo + hi);
  z.assign(n, 0.0);
  if (n == 1) { z[0] = 1.0; return theta; }
  // (T - theta') z = rhs by Gaussian elimination with partial pivoting on the tridiagonal (theta' a hair off the
  // eigenvalue); three sweeps from a generic start
  const double shift = theta + 1e-13 * std::max(nrm, 1e-300);
  std::vector<double> rhs(n);
  for (int i = 0; i < n; ++i) rhs[i] = 1.0 / std::sqrt((double)n) * ((i & 1) ? 0.7 : 1.0);
  std::vector<double> d(n), du(n), du2(n), dl(n);
  for (int sweep = 0; sweep < 3; ++sweep) {
    for (int i = 0; i < n; ++i) { d[i] = a[i] - shift; du[i] = i + 1 < n ? b[i] : 0.0; dl[i] = i + 1 < n ? b[i] : 0.0; du2[i] = 0.0; }
    z = rhs;
    for (int i = 0; i + 1 < n; ++i) {
      if (std::fabs(dl[i]) > std::fabs(d[i])) {          // swap rows i and i+1
        std::swap(d[i], dl[i]);
        const double t = du[i]; du[i] = d[i + 1]; d[i + 1] = t;
        du2[i] = du[i + 1]; du[i + 1] = 0.0;
        std::swap(z[i], z[i + 1]);
        // after the swap: row i = (d[i], du[i], du2[i]), row i+1 = (dl[i], d[i+1], du[i+1])
      }
      const double piv = std::fabs(d[i]) > 1e-300 ? d[i] : 1e-300;
      const double f = dl[i] / piv;
      d[i + 1] -= f * du[i];
      du[i + 1] -= f * du2[i];
      z[i + 1] -= f * z[i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double v = z[i];
      if (i + 1 < n) v -= du[i] * z[i + 1];
      if (i + 2 < n) v -= du2[i] * z[i + 2];
      const double piv = std::fabs(d[i]) > 1e-300 ? d[i] : 1e-300;
      z[i] = v / piv;
    }
    double nn = 0;
    for (int i = 0; i < n; ++i) nn += z[i] * z[i];
    nn = std::sqrt(nn);
    for (int i = 0; i < n; ++i) z[i] /= nn;
    rhs = z;
  }
  return theta;
}

void tridiag_ritz(const std::vector<double> &al, const std::vector<double> &be, std::vector<double> &w,
                  std::vector<double> &S) {
  const int kk = (int)al.size();
  std::vector<double> Tm((size_t)kk * kk, 0.0);
  for (int i = 0; i < kk; ++i) {
    Tm[(size_t)i * kk + i] = al[i];
    if (i + 1 < kk) Tm[(size_t)(i + 1) * kk + i] = Tm[(size_t)i * kk + i + 1] = be[i];
  }
  jacobi_eig(kk, Tm, w, S);
}

// ---- Chebyshev expansion, Expokit's rounding -----------------------------------------------------------------------
int cheb_coeffs(double z, double cut, std::vector<double> &J, double *tail_out) {
  const int kmax = (int)(z + 30.0 * std::cbrt(z + 1.0) + 80.0);
  J.resize((size_t)kmax + 1);
  for (int k = 0; k <= kmax; ++k) J[(size_t)k] = std::cyl_bessel_j((double)k, z);
  double tail = 0;
  int K = kmax;
  while (K > 1 && tail + 2.0 * std::fabs(J[(size_t)K]) < cut) { tail += 2.0 * std::fabs(J[(size_t)K]); --K; }
  if (!(K < kmax)) return 1;
  J.resize((size_t)K + 1);
  if (tail_out) *tail_out = tail;
  return 0;
}

// the coefficients J_k(z) die out super-exponentially beyond k = z
void cheb_steps(double ztot, int *nsteps, double *z) {
  *nsteps = std::max(1, (int)std::ceil(ztot / 64.0));
  *z = ztot / *nsteps;
}

double round2(double t) {
  const double sqr1 = std::sqrt(0.1);
  const double p1 = std::pow(10.0, std::round(std::log10(t) - sqr1) - 1.0);
  return std::trunc(t / p1 + 0.55) * p1;
}

// The trigger level of a full re-orthogonalisation pass.  Components removed by such a pass are not recorded in the
// projected matrix, so a Ritz pair's true residual exceeds its estimate by about
// (level at which the pass is triggered) x |H|.  The trigger level therefore follows the
// requested tolerance: tol/10, at most sqrt(eps) (Simon's semi-orthogonality bound), at
// least a few times the rounding floor eps1 of a dot product (below that every step is a
// full pass, which is what full re-orthogonalisation achieves anyway).
double pro_threshold(double eps1, double tol, const char *forced) {
  double t = std::sqrt(2.220446049250313e-16);
  if (tol > 0 && 0.1 * tol < t) t = 0.1 * tol;
  if (t < 4.0 * eps1) t = 4.0 * eps1;
  if (forced) t = atof(forced);
  return t;
}

// ---- the end filter of dnm_eigsolve: where to cut, and the degree --------------------------------------------------
int end_filter_margin(int nev) { return std::max(2, (nev + 1) / 2); }

// The probe's Ritz values are theta_i >= lambda_i (from below at the other end); |H|_inf bounds the far end rigorously.
EndFilterChoice end_filter_choice(const std::vector<double> &wv, double blast, double nrmH, int nev, bool lowest,
                                  const char *degree_knob) {
  EndFilterChoice r{};
  const int kk = (int)wv.size();
  const int margin = end_filter_margin(nev);
  double a_cut, far, near_t, gam;
  if (lowest) {
    far = std::min(nrmH, wv[kk - 1] + blast);
    a_cut = wv[nev + margin - 1];
    near_t = wv[nev - 1];
    gam = (a_cut - near_t) / (far - a_cut);
    r.p.ref = wv[0];
  } else {
    far = std::max(-nrmH, wv[0] - blast);
    a_cut = wv[kk - nev - margin];
    near_t = wv[kk - nev];
    gam = (near_t - a_cut) / (a_cut - far);
    r.p.ref = wv[kk - 1];
  }
  r.a_cut = a_cut; r.far = far; r.near_t = near_t; r.gam = gam;
  r.usable = !(!(gam > 1e-9) || !(std::fabs(far - a_cut) > 0));
  if (!r.usable) return r;
  // Degree: the filter cannot separate the wanted values from EACH OTHER (their images stay as close,
  // relatively, as d times their distance in acosh), so that work stays with the outer Lanczos process at d
  // multiplies per vector: a strong filter needs fewer vectors but more multiplies in all.  With a step costing
  // d multiplies plus two orthogonalisation passes over the basis (about 7 multiply-times at m = 20) the
  // measured optimum is an amplification of the nev-th value of about cosh(3.3) = 14 over the damped interval
  // -- degree 9 for the chains at L = 26...30: L=28, nev=5, tol 1e-10: d = 5 / 9 / 13 / 17 / 21 take
  // 6.2 / 5.6 / 5.9 / 6.1 / 7.3 s (plain restarted scheme: 12.1 s; profiles/r03_exp5_eigs_degree.txt)
  int d = (int)std::ceil(3.3 / (2.0 * std::sqrt(gam)));
  d = std::max(5, std::min(d, 49));
  if (degree_knob) d = std::max(1, atoi(degree_knob));
  d |= 1;
  r.p.d = d;
  r.p.c = 0.5 * (a_cut + far);
  r.p.h = 0.5 * std::fabs(far - a_cut);
  return r;
}

// ---- the window of dnm_eigsolve_interior ---------------------------------------------------------------------------
// The extreme Ritz values lie inside the spectrum, each within its residual of an eigenvalue.
InteriorWindow interior_window(const std::vector<double> &wv, const std::vector<double> &Sv, double blast, double nrmH,
                               int64_t Nglob, int nev, double target, double factor) {
  const int kk = (int)wv.size();
  std::vector<int> ord(kk);
  for (int i = 0; i < kk; ++i) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](int x, int y) { return wv[x] < wv[y]; });
  const int ilo = ord[0], ihi = ord[kk - 1];
  const double width = std::max(wv[ihi] - wv[ilo], 1e-3 * nrmH);
  // outward by the residual of the extreme Ritz pair and one per cent of the width: a bound that is too tight makes
  // p blow up (the solver checks it on a probe vector), one that is too wide costs degree in proportion
  InteriorWindow r;
  r.emin = std::max(-nrmH, wv[ilo] - blast * std::fabs(Sv[(size_t)ilo * kk + kk - 1]) - 0.01 * width);
  r.emax = std::min(nrmH, wv[ihi] + blast * std::fabs(Sv[(size_t)ihi * kk + kk - 1]) + 0.01 * width);
  // cumulative weight at the Ritz values (midpoint rule), linear in between
  std::vector<double> ws(kk), cum(kk);
  double acc = 0.0;
  for (int i = 0; i < kk; ++i) {
    const double wt = Sv[(size_t)ord[i] * kk] * Sv[(size_t)ord[i] * kk];
    ws[i] = wv[ord[i]];
    cum[i] = acc + 0.5 * wt;
    acc += wt;
  }
  auto cdf = [&](double E) {
    if (E <= ws[0]) return 0.0;
    if (E >= ws[kk - 1]) return 1.0;
    const int i = (int)(std::upper_bound(ws.begin(), ws.end(), E) - ws.begin());     // ws[i-1] <= E < ws[i]
    const double t = (E - ws[i - 1]) / std::max(ws[i] - ws[i - 1], 1e-300);
    return cum[i - 1] + t * (cum[i] - cum[i - 1]);
  };
  r.nwant = nev + std::max(4, nev / 2);
  const double hfull = std::max(target - r.emin, r.emax - target);
  double lo = 0.0, hi = hfull;
  for (int it = 0; it < 60; ++it) {
    const double mid = 0.5 * (lo + hi);
    if ((double)Nglob * (cdf(target + mid) - cdf(target - mid)) < r.nwant) lo = mid; else hi = mid;
  }
  double a = std::min(hi, 0.5 * hfull);
  // the estimate times the knob's factor -- f < 1 starts from a window with too few levels, which the solver's
  // widening has to repair (tests); a factor of 1 leaves `a` as it is (a <= hfull / 2 already)
  a = std::min(a * std::max(factor, 1e-3), 0.5 * hfull);
  r.a = std::max(a, 1e-6 * hfull);
  return r;
}

}  // namespace dnm
