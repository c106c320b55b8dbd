// Krylov drivers on top of the matrix-free multiply and the fused vector
// kernels.  They replace the two SLEPc solvers dynamite calls
// (src/dynamite/computations.py:89-112 MFN "expokit", :208-257 EPS
// Krylov-Schur on a Hermitian problem).  SLEPc is a third-party dependency
// that is not part of the reference tree (slepc4py == 3.20.2,
// pyproject.toml:24): the algorithms below restate the published methods
// (Sidje, "Expokit", ACM TOMS 24 (1998) -- the scheme SLEPc's MFNEXPOKIT
// implements; Wu & Simon thick-restart Lanczos = Krylov-Schur for Hermitian
// matrices, Stewart 2001).  Step counts / step sizes are not pinned by any
// reference test; results are (tests/integration/test_evolve.py,
// test_eigsolve.py tolerances).
//
// The host only handles (m+2)^2 dense matrices; every O(dim) operation is a
// HIP kernel.  The host arithmetic that needs neither is in krylov_host.cpp.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <vector>

#include "krylov_host.h"
#include "vec_api.h"

namespace dnm {

// seeded start vector in the layout of A's vectors (padding of an internal SpinConserve layout stays zero)
static int random_start(dnm_mat *A, void *x, int64_t n_local, uint64_t seed, int64_t offset, hipStream_t st) {
  if (A->use_sc3 && A->real_packed)
    return sc3_random_real(*A->sc3->ly, (double *)x, seed, st, A->sc3->T0, A->sc3->T1, &A->sc3->perm);
  if (A->use_sc3) return sc3_random(*A->sc3->ly, x, seed, st, A->sc3->T0, A->sc3->T1, &A->sc3->perm);
  return vk_random(x, n_local, seed, offset, st, A->right.host.swz);
}

// Chebyshev filter p(A) = T_d((A - c) / h) / T_d((ref - c) / h): on the interval [c - h, c + h] |p| <= 1 / |T_d(ref)|,
// outside it p grows exponentially with the distance -- Lanczos on p(A) sees the few eigenvalues beyond one end of
// the interval as huge, well separated ones.  Evaluated by the three-term recurrence on unnormalised vectors
// s_j = h^j T_j: s_{j+1} = 2 (A - c) s_j - h^2 s_{j-1} (s_1 = (A - c) s_0), every term ONE fused multiply
// y = A x - b z + c2 z2 (dnm_mat_mult_sub2); the scale that brings s_d back to O(1) is known on the host
// (ChebPoly, krylov_host.h).
struct ChebFilter : ChebPoly {
  void *ta = nullptr, *tb = nullptr;       // two work vectors
  bool on = false;
};

// Folded-spectrum filter for interior eigenpairs: with G = (A - sigma)^2 the eigenvalues within `a` of sigma are the
// lowest of G, in [0, a^2), the rest lies in [a^2, h^2], h = max(sigma - emin, emax - sigma).  The filter is
//   p(A) = T_d((G - c) / e) / T_d(-c / e),   c = (h^2 + a^2) / 2,  e = (h^2 - a^2) / 2:
// |p| <= 1 / T_d(c / e) on the unwanted part, p(sigma) = 1, monotone in |lambda - sigma| inside the window.
// G - c = (A - (sigma + sqrt c)) (A - (sigma - sqrt c)), so a term of the recurrence is two fused multiplies
// (Ops::apply_fold); the numbers come from dnm_interior_filter_plan.
struct FoldFilter : FoldPoly {
  void *ta = nullptr, *tb = nullptr, *tc = nullptr;     // three work vectors
  bool on = false;
};

struct Ops {
  dnm_mat *A;
  const dnm_hooks *hooks;
  hipStream_t st;
  int64_t n;
  int matvecs = 0;
  ChebFilter *flt = nullptr;
  FoldFilter *fold = nullptr;
  // real-packed operator (DNM_MAT_REAL_PACKED): the vectors are real, two amplitudes to a complex128 element; the
  // real part of the complex inner product of two such vectors IS their real inner product, its imaginary part
  // means nothing and is dropped wherever an inner product comes back
  bool real = false;

  // y = A x - b z + c2 z2, a term of a filter's recurrence (z, z2 may be null: no such term): one fused multiply, or
  // the multiply through the hook and one sweep per term that is there
  int step(const void *x, void *y, const void *z, double b, const void *z2, double c2) {
    ++matvecs;
    if (hooks && hooks->mult) {
      DNM_CHECK(hooks->mult(hooks->ctx, x, y) == 0, "mult hook failed");
      if (z) DNM_TRY(vk_axpby(y, z, n, -b, 0.0, 1.0, 0.0, st));
      if (z2) DNM_TRY(vk_axpby(y, z2, n, c2, 0.0, 1.0, 0.0, st));
      return 0;
    }
    return dnm_mat_mult_sub2(A, x, y, z ? z : x, b, z2, c2, 0.0, (void *)st);
  }
  // y = p(A) x; y must differ from x and from the two work vectors
  // scale_out != null: y is left unscaled and the factor handed back (the caller's next sweep applies it)
  int apply_filter(const void *x, void *y, double *scale_out = nullptr) {
    const ChebFilter &F = *flt;
    // rotate through {ta, tb, y} so that the last term lands in y
    void *buf[3] = {F.ta, F.tb, y};
    const int first = (3 - (F.d % 3)) % 3;              // index of the buffer that takes u_1
    // u_j goes to buf[(first + j - 1) % 3]: u_d -> (first + d - 1) % 3 == 2
    const void *um = nullptr, *uc = x;
    for (int j = 1; j <= F.d; ++j) {
      void *out = buf[(first + j - 1) % 3];
      DNM_TRY(step(uc, out, um, F.step_b(j), uc, -F.c));        // (u_1 has no u_{-1} term: um is null)
      um = uc;
      uc = out;
    }
    if (scale_out) {
      *scale_out = std::exp(F.log_scale());
      return 0;
    }
    return vk_scale(y, n, std::exp(F.log_scale()), 0, st);
  }

  // y = p(A) x for the folded filter; y must differ from x and from the three work vectors.  Unnormalised terms
  // u_j = e^j T_j / 2^(j-1) as in apply_filter (u_1 = (G - c) u_0, u_2 = (G - c) u_1 - (e^2 / 2) u_0,
  // u_{j+1} = (G - c) u_j - (e / 2)^2 u_{j-1}), each (G - c) u = (A - b2)(A - b1) u through the work vector tc; the
  // growth by e / 2 per term is taken out of the two live vectors whenever it passes 1e100 (the degree runs to
  // thousands).  scale_out as in apply_filter.
  int apply_fold(const void *x, void *y, double *scale_out = nullptr) {
    const FoldFilter &F = *fold;
    const double rc = std::sqrt(F.c), b1 = F.sigma - rc, b2 = F.sigma + rc;
    void *buf[3] = {F.ta, F.tb, y};
    const int first = (3 - (F.d % 3)) % 3;
    const void *um = nullptr, *uc = x;
    const double lstep = std::log(0.5 * F.e);
    // (a rescaling touches the two live vectors: after the first term one of them is still the caller's x)
    DNM_CHECK(std::fabs(lstep) < 100.0, "interior filter: spectral interval out of range (e = %g)", F.e);
    double lgrow = 0.0, ltaken = 0.0;         // log of the growth since the last rescaling / of what was taken out
    for (int j = 1; j <= F.d; ++j) {
      void *out = buf[(first + j - 1) % 3];
      const double b = F.step_b(j);
      DNM_TRY(step(uc, F.tc, uc, b1, nullptr, 0.0));
      DNM_TRY(step(F.tc, out, F.tc, b2, j == 1 ? nullptr : um, -b));
      um = uc;
      uc = out;
      lgrow += lstep;
      if (std::fabs(lgrow) > 230.0 && j < F.d) {
        // (j >= 3 here, since |lstep| < 100: um and uc are work vectors, never x)
        const double f = std::exp(-lgrow);
        DNM_TRY(vk_scale(buf[(first + j - 1) % 3], n, f, 0, st));
        DNM_TRY(vk_scale(buf[(first + j - 2) % 3], n, f, 0, st));
        ltaken += lgrow;
        lgrow = 0.0;
      }
    }
    const double sc = F.scale(ltaken);
    if (scale_out) {
      *scale_out = sc;
      return 0;
    }
    return vk_scale(y, n, sc, 0, st);
  }

  int mult(const void *x, void *y) {
    if (fold && fold->on) return apply_fold(x, y);
    if (flt && flt->on) return apply_filter(x, y);
    ++matvecs;
    if (hooks && hooks->mult) {
      DNM_CHECK(hooks->mult(hooks->ctx, x, y) == 0, "mult hook failed");
      return 0;
    }
    return dnm_mat_mult(A, x, y, (void *)st);
  }
  // y = A x - b z (z may be null), d = <x, y> and, if asked for, nn = |y|^2: the multiply of one three-term
  // Lanczos step
  int mult_dot(const void *x, void *y, zc *d, const void *z = nullptr, double b = 0.0, double *nn = nullptr) {
    double buf[3];
    if (flt && flt->on) {
      // the filter's normalisation rides on the sweep that subtracts b z and takes the sums
      double ys = 1.0;
      DNM_TRY(apply_filter(x, y, &ys));
      DNM_TRY(vec_lanczos_dot_host(y, z, x, n, b, buf, st, ys));
      DNM_TRY(sum(buf, 3));
    } else if (hooks && hooks->mult) {
      DNM_TRY(mult(x, y));
      DNM_TRY(vec_lanczos_dot_host(y, z, x, n, b, buf, st));
      DNM_TRY(sum(buf, 3));
    } else {
      ++matvecs;
      DNM_TRY(dnm_mat_mult_lanczos(A, x, y, z, b, buf, (void *)st));
    }
    *d = zc(buf[0], real ? 0.0 : buf[1]);
    if (nn) *nn = buf[2];
    return 0;
  }
  // y = A x - b z (no inner products)
  int mult_sub(const void *x, void *y, const void *z, double b) {
    if (hooks && hooks->mult) {
      DNM_TRY(mult(x, y));
      return vk_axpby(y, z, n, -b, 0.0, 1.0, 0.0, st);
    }
    ++matvecs;
    return dnm_mat_mult_sub(A, x, y, z, b, (void *)st);
  }
  // y = A x - b z + c z2 (single rank: fused where the kernel allows)
  int mult_sub2(const void *x, void *y, const void *z, double b, const void *z2, zc c) {
    ++matvecs;
    return dnm_mat_mult_sub2(A, x, y, z, b, z2, c.real(), c.imag(), (void *)st);
  }
  int sum(double *buf, int cnt) {
    if (hooks && hooks->allreduce_sum)
      DNM_CHECK(hooks->allreduce_sum(hooks->ctx, buf, cnt) == 0, "allreduce_sum hook failed");
    return 0;
  }
  int maxr(double *buf, int cnt) {
    if (hooks && hooks->allreduce_max)
      DNM_CHECK(hooks->allreduce_max(hooks->ctx, buf, cnt) == 0, "allreduce_max hook failed");
    return 0;
  }
  // h = V[:, 0:nv)^H w (global)
  int mdot(const void *V, int nv, const void *w, std::vector<zc> &h) {
    std::vector<double> buf((size_t)2 * nv);
    DNM_TRY(vec_mdot_host(V, n, nv, w, n, buf.data(), st));
    DNM_TRY(sum(buf.data(), 2 * nv));
    h.resize(nv);
    for (int j = 0; j < nv; ++j) h[j] = zc(buf[2 * j], real ? 0.0 : buf[2 * j + 1]);
    return 0;
  }
  int norm(const void *w, double *out) {
    double buf[2];
    DNM_TRY(vec_mdot_host(w, n, 1, w, n, buf, st));
    DNM_TRY(sum(buf, 1));
    *out = std::sqrt(buf[0] > 0 ? buf[0] : 0.0);
    return 0;
  }
  // w += V[:, 0:nv) c
  int maxpy(void *w, const void *V, int nv, const std::vector<zc> &c) {
    std::vector<double> buf((size_t)2 * nv);
    for (int j = 0; j < nv; ++j) { buf[2 * j] = c[j].real(); buf[2 * j + 1] = c[j].imag(); }
    const double *cd = nullptr;
    DNM_TRY(vec_upload_coefs(buf.data(), buf.size(), st, &cd));
    return vk_maxpy(w, V, n, nv, n, cd, st);
  }
  // orthogonalise p against V[:, 0:nv): classical Gram-Schmidt with one
  // refinement pass when needed (the DGKS test SLEPc's BV uses by default,
  // eta = 1/sqrt(2)); coefficients accumulate in h; returns ||p|| afterwards
  int orthogonalize(void *p, const void *V, int nv, std::vector<zc> &h, double *nrm, int min_passes = 1) {
    std::vector<zc> h1, neg;
    h.assign(nv, zc(0));
    if (nv > 4) {
      // H is Hermitian: p = A v_j is dominated by its components along the last
      // two basis vectors.  Removing those first (two vectors, cheap) leaves a
      // full pass that rarely needs refinement.
      const int lo = nv - 2;
      const void *Vl = (const char *)V + (size_t)lo * (size_t)n * 16;
      DNM_TRY(mdot(Vl, 2, p, h1));
      neg.assign(2, zc(0));
      for (int j = 0; j < 2; ++j) { neg[j] = -h1[j]; h[lo + j] += h1[j]; }
      DNM_TRY(maxpy(p, Vl, 2, neg));
    }
    return measured_passes(p, V, nv, h, nrm, min_passes, 3);
  }
  // classical Gram-Schmidt passes with measured coefficients, added to h: at least min_passes, then until a pass
  // takes out no more than the DGKS test allows, at most max_passes
  int measured_passes(void *p, const void *V, int nv, std::vector<zc> &h, double *nrm, int min_passes, int max_passes) {
    std::vector<zc> h1, neg(nv);
    for (int pass = 0; pass < max_passes; ++pass) {
      DNM_TRY(mdot(V, nv, p, h1));
      double hn2 = 0.0;
      for (int j = 0; j < nv; ++j) { neg[j] = -h1[j]; h[j] += h1[j]; hn2 += std::norm(h1[j]); }
      DNM_TRY(maxpy(p, V, nv, neg));
      DNM_TRY(norm(p, nrm));
      const double before = std::sqrt((*nrm) * (*nrm) + hn2);   // ||p|| before this pass
      if (pass + 1 >= min_passes && *nrm >= 0.7071067811865476 * before) break;   // no cancellation: done
    }
    return 0;
  }
  // First vector of a thick-restart cycle, p = A q_l against [u_0..u_{l-1}, q_l]: the components along the kept
  // Ritz vectors are the spikes s_i of the projected matrix (A u_i = theta_i u_i + s_i q_l), so the first
  // Gram-Schmidt pass needs no inner products except <q_l, p>; a measured pass follows (the Ritz vectors of a
  // semi-orthogonal basis are orthonormal to sqrt(eps) only) and its coefficients correct h.
  int orthogonalize_known(void *p, const void *V, int nv, const std::vector<double> &spike, std::vector<zc> &h,
                          double *nrm) {
    std::vector<zc> h1, neg(nv);
    h.assign(nv, zc(0));
    const void *ql = (const char *)V + (size_t)(nv - 1) * (size_t)n * 16;
    DNM_TRY(mdot(ql, 1, p, h1));
    for (int i = 0; i + 1 < nv; ++i) h[i] = zc(spike[(size_t)i], 0.0);
    h[nv - 1] = h1[0];
    for (int i = 0; i < nv; ++i) neg[i] = -h[i];
    DNM_TRY(maxpy(p, V, nv, neg));
    return measured_passes(p, V, nv, h, nrm, 1, 2);
  }
};

// Krylov basis workspace, kept between solves (hipMalloc/hipFree of tens of GiB per
// call costs more than a solve); dnm_release_workspace() returns it.
static DevBuf g_basis;
static int basis_workspace(size_t bytes, void **p) {
  if (g_basis.bytes < bytes) {
    g_basis.release();
    DNM_TRY(g_basis.alloc(bytes));
  }
  *p = g_basis.p;
  return 0;
}

static char *vecptr(void *base, int64_t n, int j) { return (char *)base + (size_t)j * (size_t)n * 16; }

}  // namespace dnm

using namespace dnm;

extern "C" {

int dnm_workspace_bytes(size_t *bytes) {
  DNM_CHECK(bytes, "null argument");
  *bytes = g_basis.bytes;
  return 0;
}

int dnm_workspace_reserve(size_t bytes, void *stream) {
  if (g_basis.bytes >= bytes) return 0;
  void *p = nullptr;
  DNM_TRY(basis_workspace(bytes, &p));
  DNM_HIP(hipMemsetAsync(p, 0, bytes, (hipStream_t)stream));
  DNM_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int dnm_release_workspace(void) {
  g_basis.release();
  rdm_release_scratch();
  return 0;
}

}  // extern "C"

#define BESSEL_MSG "internal: Bessel coefficients have not decayed (z = %g)"
// multiplies the expansion needs for |r t| = ztot at tolerance tol
static int cheb_cost(double ztot, double tol, int64_t *terms) {
  int nsteps;
  double z;
  cheb_steps(ztot, &nsteps, &z);
  std::vector<double> J;
  DNM_CHECK(cheb_coeffs(z, tol / (100.0 * nsteps), J, nullptr) == 0, BESSEL_MSG, z);
  *terms = (int64_t)nsteps * (int64_t)(J.size() - 1);
  return 0;
}

// y <- exp(-i t A) y by the Chebyshev expansion; r >= spectral radius; W: four work vectors
static int cheb_core(Ops &ops, void *y, int64_t n_local, double t, double tol, double r, void *W, int *steps_out,
                     double *err_out) {
  hipStream_t st = ops.st;
  int nsteps;
  double z;
  cheb_steps(std::fabs(r * t), &nsteps, &z);
  std::vector<double> J;
  double tail = 0;
  DNM_CHECK(cheb_coeffs(z, tol / (100.0 * nsteps), J, &tail) == 0, BESSEL_MSG, z);
  const int K = (int)J.size() - 1;
  // a_k = (2 - delta_k0) (-i sgn t)^k J_k(z)
  const zc mi(0.0, t > 0 ? -1.0 : 1.0);
  auto coef = [&](int k) {
    const zc pw = (k & 3) == 0 ? zc(1, 0) : (k & 3) == 1 ? mi : (k & 3) == 2 ? zc(-1, 0) : -mi;
    return (k == 0 ? 1.0 : 2.0) * J[(size_t)k] * pw;
  };
  if (steps_out) *steps_out = nsteps;
  if (err_out) *err_out = tail * nsteps;

  const char *cenv = knob("DNM_CHEB_FORM");
  const bool clenshaw = !(ops.hooks && ops.hooks->mult) && dnm_mat_fuses_init(ops.A) && !(cenv && cenv[0] == 'f');
  if (clenshaw) {
    // Clenshaw's backward recurrence, b_k = a_k x + (2/r) A b_{k+1} - b_{k+2}, result a_0 x + A b_1 / r - b_2:
    // every term is ONE fused multiply (the a_k x term and the b_{k+2} term start the accumulators), three
    // work vectors, x is the state itself.  Unnormalised: B_k = b_k / gamma_k, gamma_K = 1, gamma_k = (2/r) gamma_{k+1}:
    //   B_k = A B_{k+1} - (r/2)^2 B_{k+2} + (a_k / gamma_k) x
    const double beta2 = 0.25 * r * r;
    auto sl = [&](int k) { return (void *)vecptr(W, n_local, k % 3); };
    for (int step = 0; step < nsteps; ++step) {
      double g[3];
      const zc aK = coef(K);
      DNM_TRY(vk_axpby(sl(K), y, n_local, aK.real(), aK.imag(), 0.0, 0.0, st));       // B_K = a_K x
      g[K % 3] = 1.0;
      for (int k = K - 1; k >= 1; --k) {
        const double gk = g[(k + 1) % 3] * (2.0 / r);
        const zc c = coef(k) / gk;
        if (k == K - 1) DNM_TRY(ops.mult_sub2(sl(k + 1), sl(k), y, 0.0, y, c));          // b_{K+1} = 0
        else DNM_TRY(ops.mult_sub2(sl(k + 1), sl(k), sl(k + 2), beta2, y, c));
        g[k % 3] = gk;
        if (gk < 1e-200 || gk > 1e200) {      // (tiny or huge norm bound r) bring the two live vectors back to O(1) by the same factor
          DNM_TRY(vk_scale(sl(k), n_local, gk, 0.0, st));
          DNM_TRY(vk_scale(sl(k + 1), n_local, gk, 0.0, st));
          g[(k + 1) % 3] /= gk;
          g[k % 3] = 1.0;
        }
      }
      // result = a_0 x + (gamma_1 / r) [A B_1 - (r^2/2) B_2]  (gamma_2 / gamma_1 = r / 2)
      const double g1 = g[1 % 3];
      const zc c0 = coef(0) * (r / g1);
      if (K >= 2) DNM_TRY(ops.mult_sub2(sl(1), sl(0), sl(2), 0.5 * r * r, y, c0));
      else DNM_TRY(ops.mult_sub2(sl(1), sl(0), y, 0.0, y, c0));
      DNM_TRY(vk_axpby(y, sl(0), n_local, g1 / r, 0.0, 0.0, 0.0, st));
    }
    return 0;
  }
  // ring of four vectors U_k = T_k(A/r) x / gamma_k in slot k & 3, gamma_0 = 1, gamma_{k+1} = (2/r) gamma_k:
  //   T_{k+1} = (2/r) A T_k - T_{k-1}   <=>   U_{k+1} = A U_k - (r/2)^2 U_{k-1}
  const double beta = 0.25 * r * r;
  auto slot = [&](int k) { return (void *)vecptr(W, n_local, k & 3); };
  for (int step = 0; step < nsteps; ++step) {
    double gam[4];
    // U_0 = the state, U_1 = A U_0 / 2 (T_1 = A x / r = (2/r) U_1)
    DNM_TRY(vk_copy(slot(0), y, n_local, st));
    DNM_TRY(ops.mult(slot(0), slot(1)));
    DNM_TRY(vk_scale(slot(1), n_local, 0.5, 0.0, st));
    gam[0] = 1.0;
    gam[1] = 2.0 / r;
    {   // y holds U_0 already: y += (a_0 - 1) U_0 + a_1 gamma_1 U_1
      std::vector<zc> c = {coef(0) - 1.0, coef(1) * gam[1]};
      DNM_TRY(ops.maxpy(y, slot(0), 2, c));
    }
    for (int k = 1; k < K; ++k) {
      DNM_TRY(ops.mult_sub(slot(k), slot(k + 1), slot(k - 1), beta));
      gam[(k + 1) & 3] = gam[k & 3] * (2.0 / r);
      if (gam[(k + 1) & 3] < 1e-200 || gam[(k + 1) & 3] > 1e200) {
        // bring the two live vectors back to O(1) by the same factor: the recurrence is unchanged
        const double f = gam[(k + 1) & 3];
        DNM_TRY(vk_scale(slot(k + 1), n_local, f, 0.0, st));
        DNM_TRY(vk_scale(slot(k), n_local, f, 0.0, st));
        gam[(k + 1) & 3] /= f;
        gam[k & 3] /= f;
      }
      // terms k (even) and k + 1 sit side by side in the ring: one sweep adds both; an even K leaves its last
      // term alone
      if ((k + 1) & 1) {
        std::vector<zc> c = {coef(k) * gam[k & 3], coef(k + 1) * gam[(k + 1) & 3]};
        DNM_TRY(ops.maxpy(y, slot(k), 2, c));
      } else if (k + 1 == K) {
        std::vector<zc> c = {coef(K) * gam[K & 3]};
        DNM_TRY(ops.maxpy(y, slot(K), 1, c));
      }
    }
  }
  return 0;
}

// ---- what every driver does at its ends: the report, the norm, the basis size, the start vector ----------------------
static void set_stats(dnm_solver_stats *s, const Ops &ops, int reason, int its, int nconv, double err_est) {
  *s = dnm_solver_stats{reason, its, ops.matvecs, nconv, err_est};
}
// the results are in place when the caller reads the report
static int finish(Ops &ops, dnm_solver_stats *s, int reason, int its, int nconv, double err_est) {
  DNM_HIP(hipStreamSynchronize(ops.st));
  set_stats(s, ops, reason, its, nconv, err_est);
  return 0;
}
// |H|_inf, the largest over the ranks; `remember`: a partitioned handle keeps the agreed value
static int operator_norm(Ops &ops, double *nrm, bool remember) {
  DNM_TRY(dnm_mat_norm_inf(ops.A, nrm, (void *)ops.st));
  DNM_TRY(ops.maxr(nrm, 1));
  if (remember && ops.hooks && ops.hooks->allreduce_max) dnm_mat_set_norm(ops.A, *nrm);
  return 0;
}
// every rank sizes its basis from its own free memory and cached workspace: they must run the same m (the
// all-reduce lengths and the multiply counts depend on it), so take the smallest
static int agree_min(Ops &ops, int *m) {
  double neg = -(double)*m;
  DNM_TRY(ops.maxr(&neg, 1));
  *m = (int)(-neg);
  return 0;
}
// Basis size of a restarted eigensolver: ncv vectors, by default max(2 nev, nev + 15); ncv < 0: the default, but at
// most -ncv vectors in all (what fits in device memory: the caller's limit, *cap) -- the m Lanczos vectors, the
// residual and `extra` work vectors; at most max_m; the same on every rank.
static int restarted_basis_size(Ops &ops, int nev, int *ncv, int extra, int64_t max_m, int *m, int *cap) {
  *cap = 0;
  if (*ncv < 0) { *cap = -*ncv; *ncv = 0; }
  *m = *ncv > 0 ? *ncv : std::max(2 * nev, nev + 15);
  if (*cap > 0 && *m + 1 + extra > *cap) *m = *cap - 1 - extra;
  if ((int64_t)*m > max_m) *m = (int)max_m;
  return agree_min(ops, m);
}
// unit start vector: counter-based normal deviates keyed by the global index (`offset` the rank's first row: blocks
// may be uneven, PetscSplitOwnership), written in the vectors' layout
static int unit_random_start(Ops &ops, void *x, uint64_t seed, int64_t offset, double *nrm_out = nullptr) {
  DNM_TRY(random_start(ops.A, x, ops.n, seed, offset, ops.st));
  double nrm = 0;
  DNM_TRY(ops.norm(x, &nrm));
  DNM_CHECK(nrm > 0, "zero start vector");
  DNM_TRY(vk_scale(x, ops.n, 1.0 / nrm, 0, ops.st));
  if (nrm_out) *nrm_out = nrm;
  return 0;
}
// Plain Lanczos, at most k steps of the three-term recurrence on three rotating vectors, the first three of W; slot 0
// holds the unit start vector.  al, be: the tridiagonal matrix.  `stop` ends the run at an invariant subspace: be is
// then as long as al if the rule records the last beta, one shorter if not.  (The multiply's |p|^2 is not asked for:
// that only skips a copy on the host, the kernel is the same.)
static int plain_lanczos(Ops &ops, void *W, int64_t n, int k, const StopRule &stop, std::vector<double> &al,
                         std::vector<double> &be) {
  auto slot = [&](int j) { return (void *)vecptr(W, n, j % 3); };
  al.clear();
  be.clear();
  for (int j = 0; j < k; ++j) {
    void *q = slot(j), *p = slot(j + 1), *qm = slot(j + 2);     // (j + 2) % 3 == (j - 1) % 3
    zc d(0);
    DNM_TRY(ops.mult_dot(q, p, &d, j > 0 ? qm : nullptr, j > 0 ? be[j - 1] : 0.0));
    al.push_back(d.real());
    double n2 = 0;
    DNM_TRY(vec_lanczos_update_host(p, q, nullptr, n, d.real(), d.imag(), 0.0, &n2, ops.st, 1.0));
    DNM_TRY(ops.sum(&n2, 1));
    const double bn = std::sqrt(n2 > 0 ? n2 : 0.0);
    const bool ends = bn <= stop.threshold(al, be);
    if (!ends || stop.record_last) be.push_back(bn);
    if (ends) break;
    DNM_TRY(vk_scale(p, n, 1.0 / bn, 0, ops.st));
  }
  return 0;
}
// What the contract is about, measured on H itself: *rq = <u, H u> and *res = |H u - rq u| (one multiply and one
// sweep; `scratch` takes H u).  No filter may be on.
static int measure_pair(Ops &ops, const void *u, void *scratch, double *rq, double *res) {
  zc d(0);
  DNM_TRY(ops.mult_dot(u, scratch, &d));
  double n2 = 0;
  DNM_TRY(vec_lanczos_update_host(scratch, u, nullptr, ops.n, d.real(), d.imag(), 0.0, &n2, ops.st));
  DNM_TRY(ops.sum(&n2, 1));
  *rq = d.real();
  *res = std::sqrt(n2 > 0 ? n2 : 0.0);
  return 0;
}
static double relative_to(double res, double value) { return res / std::max(std::fabs(value), 1e-300); }

// ---------------------------------------------------------------------------
// Basis-free Lanczos for ONE extremal eigenpair (memory-bound sizes)
// ---------------------------------------------------------------------------
// Lanczos without a stored basis: three work vectors, the three-term recurrence only, the tridiagonal matrix on
// the host.  The extremal Ritz value converges regardless of the loss of orthogonality (Paige); copies of it that
// appear later do not matter because the iteration stops at convergence.  The Ritz vector, if wanted, is built
// in a second run of the same recurrence with the recorded coefficients.  At 16 GiB per vector a step is the
// multiply plus one sweep -- no restarts, no re-orthogonalisation passes over a 240 GiB basis.
//
// nev > 1 (problems whose vectors leave no room for a restarted basis: the 36-site kagome torus, 34 GiB per real
// vector): one pair after the other, each by the same recurrence on the operator deflated by the pairs found --
// every new Lanczos vector is projected against them (one fused inner-product sweep + one update sweep per step).
// A found vector is an eigenvector to the residual tol, so the deflated operator's extremal pair is the next pair
// of H to second order in tol; unlike one Krylov space, deflation also returns every copy of a degenerate level.
// Memory: 4 work vectors + the nev vectors (in `evecs` when the caller wants them, else nev - 1 in the workspace).
static int eigsolve_basis_free(Ops &ops, dnm_mat *A, int64_t n_local, int nev, int which, double tol, int max_steps,
                               uint64_t seed, const dnm_hooks *hooks, double *evals, void *evecs,
                               dnm_solver_stats *stats, hipStream_t st) {
  void *W = nullptr;
  DNM_TRY(basis_workspace((size_t)(4 + (evecs ? 0 : nev - 1)) * (size_t)n_local * 16, &W));
  const int64_t offset = hooks ? A->row0 : 0;
  void *F = evecs ? evecs : (void *)vecptr(W, n_local, 4);        // the pairs found so far, contiguous
  const char *venv = knob("DNM_EIGS_VERIFY");
  const bool verify = venv && venv[0] == '1';
  int nconv = 0, total_steps = 0;
  double worst = 0;
  for (int e = 0; e < nev; ++e) {
    // where this pair's vector goes (the last one is not needed unless the caller wants it)
    void *dst = evecs ? (void *)vecptr(evecs, n_local, e) : (e + 1 < nev ? (void *)vecptr(W, n_local, 4 + e) : nullptr);
    std::vector<double> al, be, svec;
    struct Step { double are, aim, s1, s2; };      // what the update of a step did, so that the second run repeats it
    std::vector<Step> rec;
    std::vector<zc> proj;                          // [step][found]: the projections taken out, for the second run
    double theta = 0, res = 0, err = 0;
    bool converged = false;
    int steps = 0, rounds = 0;
    auto slot = [&](int k) { return (void *)vecptr(W, n_local, k % 3); };
    // p <- p - F F^H p (first run: coefficients measured and recorded; second run: the recorded ones), |p|^2 after.
    // At EVERY step: projecting only every fourth one (a quarter of the sweeps) lets the recurrence alternate between H
    // and the deflated operator, and once the first Ritz value has converged the tridiagonal matrix is that of no
    // symmetric operator any more -- Ritz values far below the spectrum (measured: docs/lab/r05.md section 10).
    auto deflate = [&](void *p, int j, bool replay, double *n2) -> int {
      std::vector<zc> h;
      const size_t at = (size_t)j * e;
      if (replay) h.assign(proj.begin() + at, proj.begin() + at + e);
      else {
        DNM_TRY(ops.mdot(F, e, p, h));
        proj.insert(proj.end(), h.begin(), h.end());
      }
      if (e > 1) {
        std::vector<zc> neg(e - 1);
        for (int i = 0; i + 1 < e; ++i) neg[i] = -h[i];
        DNM_TRY(ops.maxpy(p, F, e - 1, neg));
      }
      DNM_TRY(vec_lanczos_update_host(p, vecptr(F, n_local, e - 1), nullptr, n_local, h[e - 1].real(), h[e - 1].imag(),
                                      0.0, n2, st, 1.0));
      return ops.sum(n2, 1);
    };
    // start vector: seeded normal deviates, or (later rounds) the Ritz vector of the round before, kept in `dst`;
    // without its components along the pairs found
    auto start = [&](bool from_prev) -> int {
      if (from_prev) DNM_TRY(vk_axpby(slot(0), dst, n_local, 1.0, 0.0, 0.0, 0.0, st));
      else DNM_TRY(random_start(A, slot(0), n_local, seed + 7919u * (uint64_t)e, offset, st));
      for (int pass = 0; pass < (e > 0 ? 2 : 0); ++pass) {
        std::vector<zc> h, neg(e);
        DNM_TRY(ops.mdot(F, e, slot(0), h));
        for (int i = 0; i < e; ++i) neg[i] = -h[i];
        DNM_TRY(ops.maxpy(slot(0), F, e, neg));
      }
      double n0 = 0;
      DNM_TRY(ops.norm(slot(0), &n0));
      DNM_CHECK(n0 > 0, "zero start vector");
      return vk_scale(slot(0), n_local, 1.0 / n0, 0, st);
    };
    auto pick = [&](int n, std::vector<double> &z) {
      if (which == DNM_WHICH_LOWEST) return tridiag_eigpair(al, be, n, 0, z);
      if (which == DNM_WHICH_HIGHEST) return tridiag_eigpair(al, be, n, n - 1, z);
      std::vector<double> z2;
      const double lo = tridiag_eigpair(al, be, n, 0, z), hi = tridiag_eigpair(al, be, n, n - 1, z2);
      if (std::fabs(hi) > std::fabs(lo)) { z = z2; return hi; }
      return lo;
    };
    bool measured = false;
    while (true) {
      al.clear(); be.clear(); rec.clear(); proj.clear();
      converged = false;
      steps = 0;
      DNM_TRY(start(rounds > 0));
      for (int j = 0; j < max_steps; ++j) {
        void *q = slot(j), *p = slot(j + 1), *qm = slot(j + 2);     // (j + 2) % 3 == (j - 1) % 3
        zc d(0);
        double pn2 = 0;
        DNM_TRY(ops.mult_dot(q, p, &d, j > 0 ? qm : nullptr, j > 0 ? be[j - 1] : 0.0, &pn2));
        al.push_back(d.real());
        const double b2 = pn2 - std::norm(d);
        const bool fused = b2 > 1e-4 * pn2 && pn2 > 0;
        double n2 = 0, bn;
        Step sr{d.real(), d.imag(), fused ? 1.0 / std::sqrt(b2) : 1.0, 0.0};
        DNM_TRY(vec_lanczos_update_host(p, q, nullptr, n_local, sr.are, sr.aim, 0.0, &n2, st, sr.s1));
        DNM_TRY(ops.sum(&n2, 1));
        if (e > 0) DNM_TRY(deflate(p, j, false, &n2));
        if (fused) {
          const double nu = std::sqrt(n2 > 0 ? n2 : 0.0);
          bn = std::sqrt(b2) * nu;
          if (std::fabs(n2 - 1.0) > 1e-12 && nu > 0) sr.s2 = 1.0 / nu;
        } else {
          bn = std::sqrt(n2 > 0 ? n2 : 0.0);
          if (bn > 0) sr.s2 = 1.0 / bn;
        }
        if (sr.s2 != 0.0) DNM_TRY(vk_scale(p, n_local, sr.s2, 0, st));
        rec.push_back(sr);
        be.push_back(bn);
        steps = j + 1;
        double scale = 0;
        for (int i = 0; i < steps; ++i) scale = std::max(scale, std::fabs(al[i]) + be[i]);
        const bool breakdown = bn <= 1e-14 * std::max(1.0, scale);
        if (steps >= 8 || breakdown || steps == max_steps) {
          theta = pick(steps, svec);
          res = std::fabs(bn * svec[steps - 1]);
          if (breakdown || res <= tol * std::max(std::fabs(theta), 1e-300)) { converged = true; break; }
        }
      }
      total_steps += steps;
      evals[e] = theta;
      err = res / std::max(std::fabs(theta), 1e-300);
      if (!(dst || verify) || steps == 0) break;
      // second run: the same vectors from the same start by the same arithmetic (recorded coefficients and scales),
      // v = sum_j s_j q_j accumulated in the fourth slot
      void *v = vecptr(W, n_local, 3);
      DNM_TRY(start(rounds > 0));
      DNM_TRY(vk_axpby(v, slot(0), n_local, svec[0], 0.0, 0.0, 0.0, st));
      for (int j = 0; j + 1 < steps; ++j) {
        void *q = slot(j), *p = slot(j + 1), *qm = slot(j + 2);
        if (j > 0) DNM_TRY(ops.mult_sub(q, p, qm, be[j - 1]));
        else DNM_TRY(ops.mult(q, p));
        double n2 = 0;
        DNM_TRY(vec_lanczos_update_host(p, q, nullptr, n_local, rec[j].are, rec[j].aim, 0.0, &n2, st, rec[j].s1));
        if (e > 0) DNM_TRY(deflate(p, j, true, &n2));
        if (rec[j].s2 != 0.0) DNM_TRY(vk_scale(p, n_local, rec[j].s2, 0, st));
        DNM_TRY(vk_axpby(v, p, n_local, svec[j + 1], 0.0, 1.0, 0.0, st));
      }
      double vn = 0;
      DNM_TRY(ops.norm(v, &vn));
      DNM_CHECK(vn > 0, "zero Ritz vector");
      DNM_TRY(vk_scale(v, n_local, 1.0 / vn, 0, st));
      // what was promised, measured on H itself (not the deflated operator): |H v - <v, H v> v| / |theta|
      double res_h = 0;
      DNM_TRY(measure_pair(ops, v, slot(0), &evals[e], &res_h));
      err = relative_to(res_h, evals[e]);
      measured = true;
      if (dst) DNM_TRY(vk_copy(dst, v, n_local, st));
      // the contract is a residual below tol (computations.py:274-275 raises otherwise): the estimate of the first
      // run is not the vector's residual once rounding has crept into a long recurrence.  Polish: Lanczos again from
      // the Ritz vector itself (a handful of steps); a vector that still misses tol is reported as not converged.
      if (!converged || !dst || err <= tol) break;
      if (++rounds >= 3) { converged = false; break; }
    }
    if (knob("DNM_KRYLOV_DEBUG"))
      fprintf(stderr, "dnm_eigsolve (basis-free Lanczos, pair %d of %d): %d steps, %d matvecs in all, theta = %.12g, relative residual %.2e (%s)\n",
              e + 1, nev, steps, ops.matvecs, evals[e], err, measured ? "measured" : "Lanczos estimate");
    worst = std::max(worst, err);
    if (!converged) break;
    ++nconv;
  }
  (void)total_steps;
  return finish(ops, stats, nconv == nev ? DNM_CONVERGED_TOL : DNM_DIVERGED_ITS, nev, nconv, worst);
}

// Spectral extent of A as the vector x sees it: k Lanczos steps from x (three work vectors in W, x untouched), the
// larger magnitude of the extreme Ritz values -- a lower bound of the spectral radius that is close after a few
// steps.  0 if the recurrence breaks down (x lies in a small invariant subspace: a Krylov method is exact there).
static int lanczos_extent(Ops &ops, const void *x, double xnorm, int64_t n_local, void *W, int k, double *rho) {
  std::vector<double> al, be, z;
  DNM_TRY(vk_axpby(W, x, n_local, 1.0 / xnorm, 0.0, 0.0, 0.0, ops.st));
  *rho = 0.0;
  DNM_TRY(plain_lanczos(ops, W, n_local, k, StopRule::running(1e-10), al, be));
  if (be.size() < al.size()) return 0;
  const int n = (int)al.size();
  const double lo = tridiag_eigpair(al, be, n, 0, z), hi = tridiag_eigpair(al, be, n, n - 1, z);
  *rho = std::max(std::fabs(lo), std::fabs(hi));
  return 0;
}

// ---- exp(-i t A) x: Expokit's Krylov scheme, the Chebyshev expansion, and the hand-over between them --------------
// Before any Krylov step: skip the Krylov scheme when the expansion -- whose term count is known exactly -- is the
// cheaper one: an earlier solve with this operator ended in it and the Krylov step size seen then still says so for
// this interval; or the whole expansion costs less than ONE outer Krylov step of m multiplies (short time steps:
// no basis, and none of the seconds a 200 GiB workspace takes to acquire).  *done: y holds the result.
static int expm_expansion_first(Ops &ops, void *y, int m, int64_t Nglob, double beta, double anorm, double t_out,
                                zc dir, double tol, dnm_solver_stats *stats, bool *done) {
  dnm_mat *A = ops.A;
  const int64_t n_local = ops.n;
  *done = false;
  int64_t terms = 0;
  DNM_TRY(cheb_cost(anorm * t_out, tol, &terms));
  bool go = false;
  if (A->expm_tstep > 0.0) {
    const double kry = 1.9 * (double)A->expm_m * std::ceil(t_out / A->expm_tstep);
    go = 1.25 * (double)terms < 0.8 * kry;
  }
  if (!go) go = 1.25 * (double)terms <= 1.9 * (double)m;
  void *W = nullptr;
  if (!go) {
    // the Krylov probe would have to acquire a large workspace first (seconds, see basis_workspace) for a basis
    // that memory keeps short -- where the expansion wins unless the norm bound is loose (m = 11 at L = 30: 144
    // Krylov multiplies against 56 terms for t = 1, i.e. the bound may exceed the spectral radius about
    // threefold before the expansion loses).  Ten Lanczos steps from x (the expansion's own four vectors
    // suffice) tell: their extreme Ritz values reach roughly half the radius (random-field Heisenberg chain:
    // 0.3 of the infinity norm; SYK at L = 8, where ten steps see all of it: 0.18), so 0.2 of the bound is the line.
    const double need = (double)(m + 2) * (double)n_local * 16.0;
    double want = (need > (double)g_basis.bytes && need >= 48.0 * 1073741824.0 && m < 30 && Nglob > 64) ? 1.0 : 0.0;
    DNM_TRY(ops.maxr(&want, 1));
    const char *penv = knob("DNM_EXPM_PROBE");
    if (penv) want = penv[0] == '1' && Nglob > 64 ? 1.0 : 0.0;
    if (want > 0.0 && A->expm_bound != 0) {       // probed before with this operator
      go = A->expm_bound > 0;
      want = 0.0;
    }
    if (want > 0.0) {
      DNM_TRY(basis_workspace((size_t)4 * (size_t)n_local * 16, &W));
      double rho = 0;
      DNM_TRY(lanczos_extent(ops, y, beta, n_local, W, 10, &rho));
      go = rho >= 0.2 * anorm;
      A->expm_bound = go ? 1 : -1;
      if (knob("DNM_KRYLOV_DEBUG"))
        fprintf(stderr, "dnm_expm_multiply: spectral extent seen by x %.4g of the bound %.4g -> %s\n", rho, anorm,
                go ? "Chebyshev expansion" : "Krylov");
    }
  }
  if (!go) return 0;
  if (!W) DNM_TRY(basis_workspace((size_t)4 * (size_t)n_local * 16, &W));
  int csteps = 0;
  double cerr = 0;
  DNM_TRY(cheb_core(ops, y, n_local, -dir.imag() * t_out, tol, anorm, W, &csteps, &cerr));
  *done = true;
  return finish(ops, stats, DNM_CONVERGED_TOL, csteps, 0, cerr);
}

// One Krylov basis of an Expokit step, from the state y of norm beta: V = [v_0..v_m, scratch], the projected matrix
// in H (leading dimension m + 2).  k1 = 0: happy breakdown after mb vectors.
struct ExpmBasis {
  int mb, k1;
  double avnorm;                  // || A v_m ||
  std::vector<double> nv;         // PRO path: the norms of the stored vectors
};
static int expm_krylov_basis(Ops &ops, void *V, const void *y, int m, double beta, double anorm, double break_tol,
                             LanczosMonitor *mon, std::vector<zc> &H, ExpmBasis *out) {
  const int64_t n_local = ops.n;
  hipStream_t st = ops.st;
  const bool use_pro = mon != nullptr;
  const int mh = m + 2;
  H.assign((size_t)mh * mh, zc(0));
  out->mb = m;
  out->k1 = 2;
  out->avnorm = 0;
  std::vector<zc> h;
  // PRO path: the basis is stored UNNORMALISED, w_j = nv[j] v_j, so no vector is ever rescaled:
  //   w_{j+1} = H w_j - alpha_j w_j - (beta_j nv[j]/nv[j-1]) w_{j-1},  nv[j+1] = |w_{j+1}| = nv[j] beta_{j+1}
  // (one dot + one fused update per step); the scales enter every coefficient on the host.
  std::vector<double> &nv = out->nv;
  nv.assign(m + 2, 1.0);
  std::vector<double> bet(m + 2, 0.0);
  if (use_pro) {
    DNM_TRY(vk_copy(vecptr(V, n_local, 0), y, n_local, st));
    nv[0] = beta;
  } else {
    // v_0 = w / beta
    DNM_TRY(vk_axpby(vecptr(V, n_local, 0), y, n_local, 1.0 / beta, 0, 0, 0, st));
  }
  for (int j = 0; j < m; ++j) {
    void *p = vecptr(V, n_local, j + 1);
    zc d0(0);
    // the beta term of the recurrence rides on the multiply: p = H w_j - (beta_j nv_j / nv_{j-1}) w_{j-1}
    if (use_pro)
      DNM_TRY(ops.mult_dot(vecptr(V, n_local, j), p, &d0, j > 0 ? vecptr(V, n_local, j - 1) : nullptr,
                           j > 0 ? bet[j] * nv[j] / nv[j - 1] : 0.0));
    else DNM_TRY(ops.mult(vecptr(V, n_local, j), p));
    double hn = 0;
    if (use_pro) {
      const zc alpha = d0 / (nv[j] * nv[j]);
      h.assign(j + 1, zc(0));
      h[j] = alpha;
      if (j > 0) h[j - 1] = bet[j];
      double n2 = 0;
      DNM_TRY(vec_lanczos_update_host(p, vecptr(V, n_local, j), nullptr, n_local, alpha.real(), alpha.imag(), 0.0,
                                      &n2, st));
      DNM_TRY(ops.sum(&n2, 1));
      nv[j + 1] = std::sqrt(n2 > 0 ? n2 : 0.0);
      hn = nv[j + 1] / nv[j];
      if (mon->update(j, alpha.real(), hn)) {
        std::vector<zc> g, c(j + 1);
        DNM_TRY(ops.mdot(V, j + 1, p, g));            // g_i = <w_i, w_{j+1}>
        for (int i = 0; i <= j; ++i) {
          c[i] = -g[i] / (nv[i] * nv[i]);
          h[i] += g[i] / (nv[i] * nv[j]);
        }
        DNM_TRY(ops.maxpy(p, V, j + 1, c));
        double nn = 0;
        DNM_TRY(ops.norm(p, &nn));
        nv[j + 1] = nn;
        hn = nn / nv[j];
        mon->beta[j + 1] = hn;
      }
      bet[j + 1] = hn;
      if (hn > break_tol * anorm && (nv[j + 1] > 1e120 || nv[j + 1] < 1e-120)) {
        DNM_TRY(vk_scale(p, n_local, 1.0 / nv[j + 1], 0, st));     // keep the scales representable
        nv[j + 1] = 1.0;
      }
    } else {
      DNM_TRY(ops.orthogonalize(p, V, j + 1, h, &hn));
    }
    for (int i = 0; i <= j; ++i) H[(size_t)j * mh + i] = h[i];
    if (hn <= break_tol * anorm) {   // happy breakdown
      out->k1 = 0;
      out->mb = j + 1;
      return 0;
    }
    H[(size_t)j * mh + (j + 1)] = hn;
    if (!use_pro) DNM_TRY(vk_scale(p, n_local, 1.0 / hn, 0, st));
  }
  H[(size_t)m * mh + (m + 1)] = 1.0;
  void *tmpv = vecptr(V, n_local, m + 1);
  DNM_TRY(ops.mult(vecptr(V, n_local, m), tmpv));
  DNM_TRY(ops.norm(tmpv, &out->avnorm));
  if (use_pro) out->avnorm /= nv[m];
  return 0;
}

extern "C" {

int dnm_expm_chebyshev(dnm_mat *A, const void *x, void *y, int64_t n_local, double t, double tol,
                       const dnm_hooks *hooks, dnm_solver_stats *stats, void *stream) {
  DNM_CHECK(A && x && y && stats, "null argument");
  DNM_CHECK(!A->real_packed, "exp(-iHt) needs complex vectors: not for a real-packed operator");
  hipStream_t st = (hipStream_t)stream;
  Ops ops{A, hooks, st, n_local};
  *stats = dnm_solver_stats{};
  if (tol <= 0) tol = 1e-8;
  if (x != y) DNM_TRY(vk_copy(y, x, n_local, st));
  if (t == 0.0) { stats->reason = DNM_CONVERGED_TOL; return 0; }
  double r = 0;
  DNM_TRY(operator_norm(ops, &r, true));
  if (r == 0.0) { stats->reason = DNM_CONVERGED_TOL; return 0; }
  void *W = nullptr;
  DNM_TRY(basis_workspace((size_t)4 * (size_t)n_local * 16, &W));
  int nsteps = 0;
  double err = 0;
  DNM_TRY(cheb_core(ops, y, n_local, t, tol, r, W, &nsteps, &err));
  return finish(ops, stats, DNM_CONVERGED_TOL, nsteps, 0, err);
}

int dnm_expm_multiply(dnm_mat *A, const void *x, void *y, int64_t n_local, double scale_re,
                      double scale_im, double tol, int ncv, int max_its, size_t work_limit_bytes,
                      const dnm_hooks *hooks, dnm_solver_stats *stats, void *stream) {
  DNM_CHECK(A && x && y && stats, "null argument");
  DNM_CHECK(!A->real_packed, "exp(-iHt) needs complex vectors: not for a real-packed operator");
  hipStream_t st = (hipStream_t)stream;
  Ops ops{A, hooks, st, n_local};
  *stats = dnm_solver_stats{};
  int64_t Nglob = A->N;
  // defaults everywhere and a real time: the driver may hand the rest of the interval to the Chebyshev expansion
  // (DNM_EXPM_HYBRID=0 keeps it Krylov throughout)
  const char *henv = knob("DNM_EXPM_HYBRID");
  const bool hybrid = ncv <= 0 && max_its <= 0 && scale_re == 0.0 && !(henv && henv[0] == '0');
  if (tol <= 0) tol = 1e-8;
  if (max_its <= 0) max_its = 100;
  int m = ncv > 0 ? ncv : 30;
  if ((int64_t)m > Nglob) m = (int)Nglob;
  if (work_limit_bytes) {
    // the limit is the caller's view of free device memory; the cached workspace is ours to reuse
    int64_t fit = (int64_t)((work_limit_bytes + g_basis.bytes) / ((size_t)n_local * 16)) - 2;
    if (fit < 2) fit = 2;
    if (m > fit) m = (int)fit;
  }
  {
    // a cached workspace of a useful size is reused as it is: growing it by a few vectors means handing back and
    // re-acquiring the whole slab, which the driver clears at ~30 GB/s (seconds at these sizes) -- more than a
    // slightly larger basis saves
    const int64_t have = (int64_t)(g_basis.bytes / ((size_t)n_local * 16));
    if (ncv <= 0 && have >= 12 && (int64_t)m + 2 > have) m = (int)(have - 2);
  }
  if (m < 1) m = 1;
  DNM_TRY(agree_min(ops, &m));

  const zc scale(scale_re, scale_im);
  const double t_out = std::abs(scale);
  DNM_TRY(vk_copy(y, x, n_local, st));
  if (t_out == 0.0) { stats->reason = DNM_CONVERGED_TOL; return 0; }
  const zc dir = scale / t_out;

  double anorm = 0;
  DNM_TRY(operator_norm(ops, &anorm, true));

  double beta = 0;
  DNM_TRY(ops.norm(y, &beta));
  if (beta == 0.0 || anorm == 0.0) { stats->reason = DNM_CONVERGED_TOL; return 0; }

  if (hybrid) {
    bool done = false;
    DNM_TRY(expm_expansion_first(ops, y, m, Nglob, beta, anorm, t_out, dir, tol, stats, &done));
    if (done) return 0;
  }

  void *V = nullptr;   // v_0..v_m plus one scratch vector
  DNM_TRY(basis_workspace((size_t)(m + 2) * (size_t)n_local * 16, &V));

  const double eps = 2.220446049250313e-16;
  const double rndoff = anorm * eps, break_tol = 1e-7, gamma = 0.9, delta = 1.2;
  const int mxrej = 10;
  double xm = 1.0 / m;
  double t_now = 0, s_error = 0;
  const double fact = std::pow((m + 1) / std::exp(1.0), m + 1) * std::sqrt(2.0 * M_PI * (m + 1));
  double t_new = (1.0 / anorm) * std::pow((fact * tol) / (4.0 * beta * anorm), xm);
  t_new = round2(t_new);

  const int mh = m + 2;
  std::vector<zc> H, F, Hs;
  int nstep = 0;
  // DNM_EXPM_ORTHO=full: orthogonalise every Krylov vector against the whole basis (what
  // SLEPc's BV does); default: Lanczos with partial re-orthogonalisation
  const char *oenv = knob("DNM_EXPM_ORTHO");
  const bool use_pro = !(oenv && oenv[0] == 'f');
  LanczosMonitor mon;
  ExpmBasis kb;
  while (t_now < t_out) {
    if (nstep >= max_its) {
      set_stats(stats, ops, DNM_DIVERGED_ITS, nstep, 0, s_error);
      return 0;
    }
    ++nstep;
    double t_step = std::min(t_out - t_now, t_new);
    if (use_pro) mon.reset(m, (double)Nglob, tol, knob("DNM_PRO_THRESH"));
    DNM_TRY(expm_krylov_basis(ops, V, y, m, beta, anorm, break_tol, use_pro ? &mon : nullptr, H, &kb));
    const int mb = kb.mb, k1 = kb.k1;
    if (k1 == 0) t_step = t_out - t_now;
    int ireject = 0;
    double err_loc = 0;
    int mx = mb + k1;
    while (true) {
      mx = mb + k1;
      Hs.assign((size_t)mx * mx, zc(0));
      for (int j = 0; j < mx; ++j)
        for (int i = 0; i < mx; ++i) Hs[(size_t)j * mx + i] = dir * t_step * H[(size_t)j * mh + i];
      DNM_CHECK(zexpm(mx, Hs, F) == 0, "dense expm failed");
      if (k1 == 0) { err_loc = break_tol; break; }
      const double p1 = std::abs(F[m]) * beta;
      const double p2 = std::abs(F[m + 1]) * beta * kb.avnorm;
      if (p1 > 10.0 * p2) { err_loc = p2; xm = 1.0 / m; }
      else if (p1 > p2) { err_loc = (p1 * p2) / (p1 - p2); xm = 1.0 / m; }
      else { err_loc = p1; xm = 1.0 / std::max(1, m - 1); }
      if (err_loc <= delta * t_step * tol) break;
      t_step = gamma * t_step * std::pow(t_step * tol / err_loc, xm);
      t_step = round2(t_step);
      if (++ireject > mxrej) {
        set_stats(stats, ops, DNM_DIVERGED_BREAKDOWN, nstep, 0, s_error);
        return 0;
      }
    }
    // w = V[:, 0:mx') (beta F[0:mx', 0])
    const int mxw = mb + std::max(0, k1 - 1);
    std::vector<zc> c(mxw);
    for (int i = 0; i < mxw; ++i) c[i] = beta * F[i] / (use_pro ? kb.nv[i] : 1.0);
    DNM_TRY(vk_set(y, n_local, 0, 0, st));
    DNM_TRY(ops.maxpy(y, V, mxw, c));
    DNM_TRY(ops.norm(y, &beta));
    t_now += t_step;
    t_new = gamma * t_step * std::pow(t_step * tol / err_loc, xm);
    t_new = round2(t_new);
    err_loc = std::max(err_loc, rndoff);
    s_error += err_loc;
    if (beta == 0.0) break;
    // With the caller's defaults (no ncv / max_its) and a real time, finish by the Chebyshev expansion when the
    // step size the error control has settled on makes that clearly cheaper: it costs ~1.25 multiply-times per
    // term against ~1.9 per Krylov multiply (measured), and its term count is known exactly.
    if (hybrid && m >= 2 && t_now < t_out) {
      const double t_left = t_out - t_now;
      int64_t terms = 0;
      DNM_TRY(cheb_cost(anorm * t_left, tol, &terms));
      const double kry = 1.9 * (double)m * std::ceil(t_left / t_new);
      if (1.25 * (double)terms < 0.8 * kry) {
        int csteps = 0;
        double cerr = 0;
        DNM_TRY(cheb_core(ops, y, n_local, -dir.imag() * t_left, tol, anorm, V, &csteps, &cerr));
        A->expm_tstep = t_new;
        A->expm_m = m;
        nstep += csteps;
        s_error += cerr;
        break;
      }
    }
  }
  return finish(ops, stats, DNM_CONVERGED_TOL, nstep, 0, s_error);
}

}  // extern "C"

// Thick-restart Lanczos (Wu & Simon; Krylov-Schur for a Hermitian matrix), what the two eigensolvers share: the basis
// V = [u_0..u_{l-1}, q_l..q_m] of a cycle and its projected matrix -- kept Ritz pairs (theta_i, u_i) with
// A u_i = theta_i u_i + spike_i q_l, then the Lanczos coefficients alpha_j, betav_j of the steps j = l..m-1.  How a
// step is orthogonalised and when the iteration stops is the solver's business.
struct ThickRestart {
  int m, l = 0;
  std::vector<double> theta, spike;        // kept Ritz values and their coupling to q_l
  std::vector<double> alpha, betav;
  std::vector<double> T, w, Sm;            // the projected matrix (destroyed by the solve), its Ritz values and vectors
  std::vector<int> order;                  // the Ritz pairs, most wanted first
  explicit ThickRestart(int m_) : m(m_), alpha(m_, 0.0), betav(m_, 0.0), order(m_) {}
  // projected matrix: diag(theta) + spike row/col at l, tridiagonal beyond; `before(x, y)`: the Ritz value x is
  // wanted more than y
  template <class Before>
  void project(Before before) {
    T.assign((size_t)m * m, 0.0);
    for (int i = 0; i < l; ++i) {
      T[(size_t)i * m + i] = theta[i];
      T[(size_t)l * m + i] = T[(size_t)i * m + l] = spike[i];
    }
    for (int j = l; j < m; ++j) {
      T[(size_t)j * m + j] = alpha[j];
      if (j + 1 < m) T[(size_t)(j + 1) * m + j] = T[(size_t)j * m + (j + 1)] = betav[j];
    }
    jacobi_eig(m, T, w, Sm);
    for (int i = 0; i < m; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return before(w[a], w[b]); });
  }
  double value(int i) const { return w[order[i]]; }
  // the residual norm of the i-th Ritz pair, |beta_m S[order[i]][m-1]|
  double residual(int i) const { return std::fabs(betav[m - 1] * Sm[(size_t)order[i] * m + (m - 1)]); }
  // how many pairs a restart keeps: the converged ones plus half of the rest, at least `at_least`
  int keep_count(int nconv, int at_least) const {
    const int keep = std::max(at_least, nconv + std::max(1, (m - nconv) / 2));
    return std::min(keep, m - 1);
  }
  // V[:, 0:count) <- V[:, 0:m) S[:, order[0:count)]: the first `count` Ritz vectors
  int rotate(Ops &ops, void *V, int count) const {
    std::vector<double> Ssel((size_t)2 * m * count, 0.0);
    for (int o = 0; o < count; ++o)
      for (int j = 0; j < m; ++j) Ssel[2 * ((size_t)o * m + j)] = Sm[(size_t)order[o] * m + j];
    const double *sd = nullptr;
    DNM_TRY(vec_upload_coefs(Ssel.data(), Ssel.size(), ops.st, &sd));
    return vk_basis_update(V, ops.n, m, count, ops.n, sd, ops.st);
  }
  // the next cycle starts from `keep` Ritz vectors and q_m
  int restart(Ops &ops, void *V, int keep) {
    const double bm = betav[m - 1];
    theta.assign(keep, 0.0);
    spike.assign(keep, 0.0);
    for (int o = 0; o < keep; ++o) {
      theta[o] = w[order[o]];
      spike[o] = bm * Sm[(size_t)order[o] * m + (m - 1)];
    }
    DNM_TRY(rotate(ops, V, keep));
    DNM_TRY(vk_copy(vecptr(V, ops.n, keep), vecptr(V, ops.n, m), ops.n, ops.st));
    l = keep;
    return 0;
  }
  // step j ended in an invariant subspace: q_{j+1} is a fresh seeded direction orthogonal to the basis
  int fresh_direction(Ops &ops, void *V, int j, int its, uint64_t seed, int64_t offset) {
    void *p = vecptr(V, ops.n, j + 1);
    std::vector<zc> h;
    betav[j] = 0.0;
    DNM_TRY(random_start(ops.A, p, ops.n, seed + 7919u * (uint64_t)(its * m + j + 1), offset, ops.st));
    double rn = 0;
    DNM_TRY(ops.orthogonalize(p, V, j + 1, h, &rn, 2));
    DNM_CHECK(rn > 0, "Lanczos breakdown: could not extend the basis");
    return vk_scale(p, ops.n, 1.0 / rn, 0, ops.st);
  }
};

// dnm_eigsolve past the choice of path: the restarted scheme, plain or on the end filter
struct EigsRun {
  Ops &ops;
  void *V;                                 // v_0..v_m, then the filter's two work vectors
  int64_t n;
  int nev, nev_max, which, max_its;
  double tol;
  uint64_t seed;
  int64_t offset;
  ThickRestart tr;
  ChebFilter flt;
  bool filtered = false;
  double tol_p, tol_h;                     // on a filter: its own relative residual / the estimate of H's
  // DNM_EIGS_ORTHO=full: orthogonalise every Lanczos vector against the whole basis (what SLEPc's
  // Krylov-Schur does); default: partial re-orthogonalisation driven by the omega-recurrence
  bool use_pro = true;
  bool known_off = false;                  // DNM_EIGS_KNOWN=0: A/B switch
  // DNM_EIGS_BETA=sweep (1): beta from a norm sweep after the update (never the fused form); =rescale (2): always
  // run the corrective rescaling sweep -- both only to exercise the rarely taken branches in tests
  int beta_mode = 0;
  RestartMonitor mon;
  std::vector<double> row_l;
  std::vector<zc> h;
  double anorm_est = 0;
  int its = 0, nconv = 0, extra_matvecs = 0;
  int nok = 0;                             // filtered: leading Ritz pairs whose MEASURED residual passes
  std::vector<double> rq;                  // ... and their Rayleigh quotients in H
  double worst_true = 0.0;

  EigsRun(Ops &ops_, void *V_, int m, int nev_, int nev_max_, int which_, int max_its_, double tol_, uint64_t seed_,
          int64_t offset_)
      : ops(ops_), V(V_), n(ops_.n), nev(nev_), nev_max(nev_max_), which(which_), max_its(max_its_), tol(tol_),
        seed(seed_), offset(offset_), tr(m), tol_p(tol_), tol_h(0.5 * tol_) {}
  // Several pairs at one end of the spectrum of a large operator: thick-restart Lanczos on a Chebyshev filter p(H).
  // Where to cut: a few steps of plain Lanczos give Ritz values and the last residual norm (end_filter_choice).  The
  // filter stays off when the probe is too short or shows no usable gap: the plain scheme copes.
  int setup_end_filter(int64_t Nglob, double nrm0) {
    const int m = tr.m;
    const int k0 = (int)std::min<int64_t>(Nglob - 1, std::max(40, 10 * nev));
    std::vector<double> al, be;
    DNM_TRY(plain_lanczos(ops, V, n, k0, StopRule::alpha(1e-12), al, be));
    const int kk = (int)al.size();
    if (kk >= nev + end_filter_margin(nev) + 2) {
      std::vector<double> wv, Sv;
      tridiag_ritz(al, be, wv, Sv);
      std::sort(wv.begin(), wv.end());
      double nrmH = 0;
      DNM_TRY(operator_norm(ops, &nrmH, false));
      // (the degree is odd: p < 0 below the interval, so the wanted end of p(H) is the wanted end of H)
      const EndFilterChoice ch = end_filter_choice(wv, be[kk - 1], nrmH, nev, which == DNM_WHICH_LOWEST,
                                                   knob("DNM_EIGS_FILTER_DEGREE"));
      if (ch.usable) {
        static_cast<ChebPoly &>(flt) = ch.p;
        flt.ta = vecptr(V, n, m + 1);
        flt.tb = vecptr(V, n, m + 2);
        flt.on = true;
        ops.flt = &flt;
        filtered = true;
        tol_p = 0.25 * tol;
        if (knob("DNM_KRYLOV_DEBUG"))
          fprintf(stderr, "dnm_eigsolve (filtered): %d probe steps, cut %.6g, far end %.6g (|H|_inf %.6g), nev-th "
                  "estimate %.6g, relative gap %.3g, degree %d\n", kk, ch.a_cut, ch.far, nrmH, ch.near_t, ch.gam, flt.d);
      }
    }
    // the probe used the first three slots: the start vector again
    DNM_TRY(random_start(ops.A, V, n, seed, offset, ops.st));
    return vk_scale(V, n, 1.0 / nrm0, 0, ops.st);
  }
  void choose_orthogonalisation(int64_t Nglob) {
    const char *oenv = knob("DNM_EIGS_ORTHO");
    // (on a filter the basis work is a small share of a step and p(H) has a huge dynamic range: every step in full)
    use_pro = !(oenv && oenv[0] == 'f') && (!filtered || knob("DNM_EIGS_FILTER_PRO") != nullptr);
    known_off = knob("DNM_EIGS_KNOWN") && knob("DNM_EIGS_KNOWN")[0] == '0';
    const char *benv = knob("DNM_EIGS_BETA");
    beta_mode = !benv ? 0 : (benv[0] == 's' ? 1 : (benv[0] == 'r' ? 2 : 0));
    mon.setup(tr.m, (double)Nglob, filtered ? tol_p : tol, knob("DNM_PRO_THRESH"));
  }
  // Step j > l under partial re-orthogonalisation: the three-term recurrence, a full pass when the monitor asks.
  // *normalised: q_{j+1} has unit norm already.
  int three_term_step(int j, double *bn_out, bool *normalised) {
    hipStream_t st = ops.st;
    void *p = vecptr(V, n, j + 1);
    zc d0(0);
    double pn2 = 0, bn = 0;
    DNM_TRY(ops.mult_dot(vecptr(V, n, j), p, &d0, vecptr(V, n, j - 1), tr.betav[j - 1], &pn2));
    tr.alpha[j] = d0.real();
    // |p - alpha q_j|^2 = |p|^2 - |alpha|^2 (q_j has unit norm): beta is known before the update sweep, which
    // then writes q_{j+1} = (p - alpha q_j) / beta directly; its own sum of squares (1 up to the cancellation
    // in the difference) corrects beta and, if it is off, the vector
    const double b2 = pn2 - std::norm(d0);
    const bool fused = b2 > 1e-4 * pn2 && pn2 > 0 && beta_mode != 1;
    const double best = fused ? std::sqrt(b2) : 0.0;
    const bool reorth = fused ? mon.update(j, tr.alpha[j], best) : false;
    double n2 = 0;
    DNM_TRY(vec_lanczos_update_host(p, vecptr(V, n, j), nullptr, n, d0.real(), d0.imag(), 0.0, &n2, st,
                                    (fused && !reorth) ? 1.0 / best : 1.0));
    DNM_TRY(ops.sum(&n2, 1));
    if (fused && !reorth) {
      const double nu = std::sqrt(n2 > 0 ? n2 : 0.0);
      bn = best * nu;
      mon.beta[j + 1] = bn;
      *normalised = true;
      if ((std::fabs(n2 - 1.0) > 1e-12 || beta_mode == 2) && nu > 0) DNM_TRY(vk_scale(p, n, 1.0 / nu, 0, st));
    } else {
      bn = std::sqrt(n2 > 0 ? n2 : 0.0);
      if (fused) mon.beta[j + 1] = bn;
      if (reorth || (!fused && mon.update(j, tr.alpha[j], bn))) {
        std::vector<zc> g, c(j + 1);
        DNM_TRY(ops.mdot(V, j + 1, p, g));
        for (int i = 0; i <= j; ++i) c[i] = -g[i];
        DNM_TRY(ops.maxpy(p, V, j + 1, c));
        DNM_TRY(ops.norm(p, &bn));
        mon.beta[j + 1] = bn;
      }
    }
    *bn_out = bn;
    return 0;
  }
  // one cycle: the Lanczos steps l..m-1
  int cycle() {
    const int l = tr.l, m = tr.m;
    if (use_pro) mon.begin_cycle(l, tr.theta, tr.spike, row_l);
    for (int j = l; j < m; ++j) {
      void *p = vecptr(V, n, j + 1);
      double bn = 0;
      bool normalised = false;
      if (use_pro && j != l) {
        DNM_TRY(three_term_step(j, &bn, &normalised));
      } else {
        DNM_TRY(ops.mult(vecptr(V, n, j), p));
        // the first step of a cycle removes the spike components: whole basis, twice when Ritz vectors are
        // present (they are orthonormal to sqrt(eps) only under partial re-orthogonalisation)
        if (use_pro && l > 0 && j == l && (int)tr.spike.size() == l && !known_off)
          DNM_TRY(ops.orthogonalize_known(p, V, j + 1, tr.spike, h, &bn));
        else
          DNM_TRY(ops.orthogonalize(p, V, j + 1, h, &bn, (use_pro && l > 0) ? 2 : 1));
        tr.alpha[j] = h[j].real();
        if (use_pro) mon.first_step(tr.alpha[j], bn);
      }
      tr.betav[j] = bn;
      anorm_est = std::max(anorm_est, std::fabs(tr.alpha[j]) + bn);
      if (bn <= 1e-14 * std::max(1.0, anorm_est)) {
        // invariant subspace: continue with a fresh direction orthogonal to the basis
        DNM_TRY(tr.fresh_direction(ops, V, j, its, seed, offset));
        if (use_pro) {
          mon.beta[j + 1] = 0.0;
          for (int k = 0; k <= j; ++k) mon.wcur[k] = mon.eps1;
        }
      } else if (!normalised) {
        DNM_TRY(vk_scale(p, n, 1.0 / bn, 0, ops.st));
      }
    }
    return 0;
  }
  // Filtered, after a restart: the kept Ritz vectors sit in the first slots -- measure what the contract is about,
  // |H u - <u,Hu> u| / |<u,Hu>| in H itself (one multiply and one sweep each; the filter's work vectors are free in
  // between)
  int measure_kept(int keep) {
    const int nchk = std::min(std::min(keep, nev_max), std::max(nev, nconv));
    flt.on = false;
    const int mv0 = ops.matvecs;
    rq.assign(nchk, 0.0);
    nok = 0;
    worst_true = 0.0;
    bool chain = true;
    for (int o = 0; o < nchk; ++o) {
      double res = 0;
      DNM_TRY(measure_pair(ops, vecptr(V, n, o), flt.ta, &rq[o], &res));
      const double rel = relative_to(res, rq[o]);
      if (chain && rel <= tol) { ++nok; worst_true = std::max(worst_true, rel); }
      else {
        if (chain && o < nev) worst_true = std::max(worst_true, rel);
        chain = false;
      }
    }
    extra_matvecs += ops.matvecs - mv0;
    ops.matvecs = mv0;
    flt.on = true;
    if (knob("DNM_KRYLOV_DEBUG"))
      fprintf(stderr, "dnm_eigsolve (filtered): restart %d, %d pairs converged on the filter (tol %.1e, estimate for H "
              "%.1e), %d pass in H (worst of the wanted %.2e)\n", its, nconv, tol_p, tol_h, nok, worst_true);
    return 0;
  }
  int iterate() {
    while (true) {
      ++its;
      DNM_TRY(cycle());
      tr.project([&](double x, double y) {
        if (which == DNM_WHICH_LOWEST) return x < y;
        if (which == DNM_WHICH_HIGHEST) return x > y;
        return std::fabs(x) > std::fabs(y);
      });
      nconv = 0;
      for (int i = 0; i < tr.m; ++i) {
        const double res = tr.residual(i);
        // relative to the eigenvalue (SLEPc EPS_CONV_REL); on a filter: the residual as H would see it (the measured
        // residual of the restarted vectors has the last word)
        bool ok = res <= (filtered ? tol_p : tol) * std::max(std::fabs(tr.value(i)), 1e-300);
        if (filtered && !ok) {
          double lam;
          ok = flt.seen_from_a(tr.value(i), res, which == DNM_WHICH_LOWEST, &lam) <= tol_h;
        }
        if (ok) ++nconv; else break;
      }
      const bool stop = nconv >= nev || its >= max_its;
      if (stop && !filtered) break;
      // thick restart: keep the converged pairs plus half of the rest (on a filter the wanted ones at least: they
      // are measured in place)
      const int keep = tr.keep_count(nconv, filtered ? nev : 0);
      DNM_TRY(tr.restart(ops, V, keep));
      if (use_pro) {
        // |q_m^H u_o| <= sum_k |S_ko| |omega_{m,k}|: the new q_l against the rotated basis
        row_l.assign(keep, 0.0);
        for (int o = 0; o < keep; ++o)
          for (int k = 0; k < tr.m; ++k)
            row_l[o] += std::fabs(tr.Sm[(size_t)tr.order[o] * tr.m + k]) * std::fabs(mon.wcur[k]);
      }
      if (filtered && stop) {
        // the filter's estimates say the wanted pairs have converged (or the iteration limit is reached)
        DNM_TRY(measure_kept(keep));
        if (nok >= nev || its >= max_its) break;
        // the estimates were satisfied too early: ask for more, by what the measurement missed
        const double f = std::max(1e-3, std::min(0.3, 0.3 * tol / std::max(worst_true, 1e-300)));
        tol_p *= f;
        tol_h *= f;
      }
    }
    return 0;
  }
  // the Ritz vectors are in place (thick restart) and measured in H: ordered by their Rayleigh quotients
  int finish_filtered(double *evals, void *evecs, dnm_solver_stats *stats) {
    flt.on = false;
    const int nout = std::min(nok, nev_max);
    std::vector<int> ord(nout);
    for (int i = 0; i < nout; ++i) ord[i] = i;
    const bool low = which == DNM_WHICH_LOWEST;
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return low ? rq[a] < rq[b] : rq[a] > rq[b]; });
    for (int i = 0; i < nout; ++i) evals[i] = rq[ord[i]];
    if (evecs)
      for (int i = 0; i < nout; ++i) DNM_TRY(vk_copy(vecptr(evecs, n, i), vecptr(V, n, ord[i]), n, ops.st));
    if (knob("DNM_KRYLOV_DEBUG"))
      fprintf(stderr, "dnm_eigsolve (filtered): %d restarts, %d matvecs (+%d for the checks), degree %d, largest true "
              "relative residual %.2e\n", its, ops.matvecs, extra_matvecs, flt.d, worst_true);
    return finish(ops, stats, (nout >= nev) ? DNM_CONVERGED_TOL : DNM_DIVERGED_ITS, its, nout, worst_true);
  }
  int finish_plain(double *evals, void *evecs, dnm_solver_stats *stats) {
    const int m = tr.m;
    const int nout = std::min(nconv, nev_max);
    double worst = 0.0;
    for (int i = 0; i < nout; ++i) evals[i] = tr.value(i);
    if (nout > 0) {
      DNM_TRY(tr.rotate(ops, V, nout));
      if (use_pro)     // a semi-orthogonal basis leaves the Ritz vectors orthonormal to sqrt(eps) only: Gram-Schmidt
        for (int o = 0; o < nout; ++o) {   // (inside a degenerate level the gap argument does not protect them)
          double nn = 0;
          if (o > 0) DNM_TRY(ops.orthogonalize(vecptr(V, n, o), V, o, h, &nn));
          else DNM_TRY(ops.norm(vecptr(V, n, o), &nn));
          DNM_CHECK(nn > 0, "zero Ritz vector");
          DNM_TRY(vk_scale(vecptr(V, n, o), n, 1.0 / nn, 0, ops.st));
        }
      if (evecs) DNM_TRY(vk_copy(evecs, V, (int64_t)nout * n, ops.st));
      // what was promised, measured: the largest relative residual |H u - <u,Hu> u| / |theta| of the returned
      // pairs (one multiply each; the Lanczos vector in the last slot is no longer needed)
      const int matvecs_solve = ops.matvecs;
      for (int o = 0; o < nout; ++o) {
        if (nout > m) break;
        double rayleigh = 0, res = 0;
        DNM_TRY(measure_pair(ops, vecptr(V, n, o), vecptr(V, n, m), &rayleigh, &res));
        worst = std::max(worst, relative_to(res, evals[o]));
      }
      ops.matvecs = matvecs_solve;      // reported separately from the iteration's multiplies
    }
    if (knob("DNM_KRYLOV_DEBUG"))
      fprintf(stderr, "dnm_eigsolve: %d restarts, %d matvecs, %d three-term steps, %d full re-orthogonalisations, "
              "largest true relative residual %.2e\n", its, ops.matvecs, mon.steps, mon.reorths, worst);
    return finish(ops, stats, (nconv >= nev) ? DNM_CONVERGED_TOL : DNM_DIVERGED_ITS, its, nout, worst);
  }
};

extern "C" {

int dnm_eigsolve(dnm_mat *A, int64_t n_local, int nev, int which, double tol, int ncv, int max_its,
                 uint64_t seed, const dnm_hooks *hooks, int nev_max, double *evals, void *evecs,
                 dnm_solver_stats *stats, void *stream) {
  DNM_CHECK(A && evals && stats && nev >= 1 && nev_max >= nev, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Ops ops{A, hooks, st, n_local};
  ops.real = A->real_packed;
  *stats = dnm_solver_stats{};
  const int64_t Nglob = A->N;
  if (tol <= 0) tol = 1e-8;
  int cap = 0, m = 0;
  DNM_TRY(restarted_basis_size(ops, nev, &ncv, 0, Nglob, &m, &cap));
  // (several pairs whose restarted basis does not fit -- fewer than nev + 2 vectors beside the residual and the
  // filter's two work vectors -- go one after the other through the basis-free recurrence on the deflated
  // operator, see eigsolve_basis_free)
  const bool no_room = cap > 0 && cap < nev + 6;
  DNM_CHECK(m >= nev || no_room, "ncv smaller than nev");
  if (max_its <= 0) max_its = (int)std::min<int64_t>(std::max<int64_t>(100, 2 * Nglob / std::max(m, 1)), 1 << 30);
  bool filtered = false;
  {
    // one extremal pair of a large operator under default parameters: Lanczos without a stored basis (a step is
    // the multiply plus one sweep; the restarted scheme below spends two thirds of its time on basis traffic at
    // these sizes).  DNM_EIGS_BASISFREE=0 / 1 forces the choice; an explicit ncv keeps the restarted scheme.
    const char *bf = knob("DNM_EIGS_BASISFREE");
    double negn = -(double)n_local;       // the smallest block decides, so that every rank takes the same path
    DNM_TRY(ops.maxr(&negn, 1));
    const bool large = -negn >= (double)((int64_t)1 << 22);
    const bool want = bf ? bf[0] == '1' : large;
    const bool forced = bf && bf[0] == '1';
    if (ncv <= 0 && Nglob > 64 && Nglob > 4 * (int64_t)nev && ((want && nev == 1) || forced || no_room)) {
      const int64_t steps64 = std::min<int64_t>((int64_t)max_its * std::max(m, nev + 15), Nglob);
      return eigsolve_basis_free(ops, A, n_local, nev, which, tol, (int)std::min<int64_t>(steps64, 100000), seed,
                                 hooks, evals, evecs, stats, st);
    }
    DNM_CHECK(m >= nev, "not enough memory for a restarted basis");
    // several pairs at one end of the spectrum of a large operator: thick-restart Lanczos on a Chebyshev filter
    // p(H) -- d fused multiplies per Lanczos vector, so the orthogonalisation and restart traffic per multiply
    // drops by d (at 4-16 GiB per vector the plain scheme spends 80 % of its time there).  DNM_EIGS_FILTER=0 / 1
    // forces the choice; an explicit ncv keeps the plain scheme.
    const char *fe = knob("DNM_EIGS_FILTER");
    filtered = (fe ? fe[0] == '1' : (large && nev > 1)) && which != DNM_WHICH_EXTERIOR && ncv <= 0 &&
               Nglob > 8 * (int64_t)m;
    if (filtered && cap > 0 && m + 3 > cap) {        // the filter's two work vectors come out of the same budget
      if (cap - 3 >= nev + 2) m = cap - 3;
      else filtered = false;
    }
  }
  DNM_CHECK((size_t)(m + 1) * 16 <= 160 * 1024, "ncv too large for the basis-rotation kernel");

  void *V = nullptr;
  DNM_TRY(basis_workspace((size_t)(m + 1 + (filtered ? 2 : 0)) * (size_t)n_local * 16, &V));
  EigsRun run(ops, V, m, nev, nev_max, which, max_its, tol, seed, hooks ? A->row0 : 0);
  double nrm0 = 0;
  DNM_TRY(unit_random_start(ops, V, seed, run.offset, &nrm0));
  if (filtered) DNM_TRY(run.setup_end_filter(Nglob, nrm0));
  run.choose_orthogonalisation(Nglob);
  DNM_TRY(run.iterate());
  return run.filtered ? run.finish_filtered(evals, evecs, stats) : run.finish_plain(evals, evecs, stats);
}

}  // extern "C"

// Rayleigh-Ritz in H itself on the first nrr Ritz vectors of p(A), those that have converged -- a nearly invariant
// subspace, so no spurious interior values -- which also separates the pairs sigma - d, sigma + d' that p nearly
// merges; then what the contract is about, |H u - theta u| <= tol |H|_inf, measured pair by pair, nearest first
struct RitzInH {
  int nrr = 0, nok = 0;
  std::vector<double> rth;              // Ritz values in H, nearest the target first
  std::vector<zc> rQ;                   // ... and their vectors in the basis V[:, 0:nrr)
  double worst = 0.0, miss = 0.0;       // largest residual / |H|_inf of the wanted pairs; the first that does not pass
  std::vector<zc> coefs(int i) const { return std::vector<zc>(rQ.begin() + (size_t)i * nrr, rQ.begin() + (size_t)(i + 1) * nrr); }
};
static int rayleigh_ritz_in_h(Ops &ops, void *V, const FoldFilter &F, int nrr, int nev, int nev_max, double target,
                              double tol, double nrmH, RitzInH *r) {
  const int64_t n = ops.n;
  r->nrr = nrr;
  std::vector<zc> Mh((size_t)nrr * nrr), col;
  for (int j = 0; j < nrr; ++j) {
    DNM_TRY(ops.mult(vecptr(V, n, j), F.ta));
    DNM_TRY(ops.mdot(V, nrr, F.ta, col));
    for (int i = 0; i < nrr; ++i) Mh[(size_t)i * nrr + j] = col[i];
  }
  for (int i = 0; i < nrr; ++i) {          // Hermitian part (the basis is orthonormal to rounding)
    Mh[(size_t)i * nrr + i] = Mh[(size_t)i * nrr + i].real();
    for (int j = i + 1; j < nrr; ++j) {
      const zc v = 0.5 * (Mh[(size_t)i * nrr + j] + std::conj(Mh[(size_t)j * nrr + i]));
      Mh[(size_t)i * nrr + j] = v;
      Mh[(size_t)j * nrr + i] = std::conj(v);
    }
  }
  std::vector<double> wh;
  std::vector<zc> Qh;
  hjacobi_eig(nrr, Mh, wh, Qh);
  std::vector<int> oh(nrr);
  for (int i = 0; i < nrr; ++i) oh[i] = i;
  std::sort(oh.begin(), oh.end(), [&](int x, int y) { return std::fabs(wh[x] - target) < std::fabs(wh[y] - target); });
  r->rth.assign(nrr, 0.0);
  r->rQ.assign((size_t)nrr * nrr, zc(0));
  for (int i = 0; i < nrr; ++i) {
    r->rth[i] = wh[oh[i]];
    for (int k = 0; k < nrr; ++k) r->rQ[(size_t)i * nrr + k] = Qh[(size_t)oh[i] * nrr + k];
  }
  r->nok = 0;
  r->worst = r->miss = 0.0;
  for (int i = 0; i < std::min(nrr, nev_max); ++i) {
    DNM_TRY(vk_set(F.ta, n, 0.0, 0.0, ops.st));
    DNM_TRY(ops.maxpy(F.ta, V, nrr, r->coefs(i)));
    DNM_TRY(ops.mult(F.ta, F.tb));
    double n2 = 0;      // (against the Rayleigh-Ritz value, not a fresh inner product: not measure_pair)
    DNM_TRY(vec_lanczos_update_host(F.tb, F.ta, nullptr, n, r->rth[i], 0.0, 0.0, &n2, ops.st, 1.0));
    DNM_TRY(ops.sum(&n2, 1));
    const double res = std::sqrt(n2 > 0 ? n2 : 0.0) / nrmH;
    if (res <= tol) { ++r->nok; r->worst = std::max(r->worst, res); }
    else { r->miss = res; if (i < nev) r->worst = std::max(r->worst, res); break; }
  }
  return 0;
}

extern "C" {

int dnm_interior_filter_plan(double emin, double emax, double target, double a, double damping, int *degree,
                             double *c, double *e) {
  DNM_CHECK(degree && c && e, "null argument");
  DNM_CHECK(emax > emin && a > 0 && damping > 1, "bad argument (emax > emin, a > 0, damping > 1)");
  const double h = std::max(target - emin, emax - target);
  DNM_CHECK(h > a, "the window [target - a, target + a] covers the whole interval");
  *c = 0.5 * (h * h + a * a);
  *e = 0.5 * (h * h - a * a);
  const double d = std::ceil(std::acosh(damping) / std::acosh(*c / *e));
  DNM_CHECK(d < 1e9, "filter degree out of range (window too narrow for the interval)");
  *degree = std::max(1, (int)d);
  return 0;
}

int dnm_eigsolve_interior(dnm_mat *A, int64_t n_local, int nev, double target, double tol, int ncv, int max_its,
                          uint64_t seed, const dnm_hooks *hooks, int nev_max, double *evals, void *evecs,
                          dnm_solver_stats *stats, void *stream) {
  DNM_CHECK(A && evals && stats && nev >= 1 && nev_max >= nev, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Ops ops{A, hooks, st, n_local};
  ops.real = A->real_packed;
  *stats = dnm_solver_stats{};
  // (a real-packed handle counts complex128 elements, two amplitudes each)
  const int64_t Nglob = A->real_packed ? 2 * A->N : A->N;
  if (tol <= 0) tol = 1e-8;
  DNM_CHECK(Nglob >= (int64_t)nev + 3, "operator too small for %d interior pairs (dimension %lld)", nev, (long long)Nglob);
  // basis: ncv as in dnm_eigsolve; beside the m + 1 Lanczos vectors the filter keeps three work vectors
  int cap = 0, m = 0;
  DNM_TRY(restarted_basis_size(ops, nev, &ncv, 3, Nglob - 1, &m, &cap));
  DNM_CHECK(m >= nev + 2, "not enough memory for a restarted basis of %d interior pairs (%d vectors fit beside the "
            "filter's three)", nev, std::max(m, 0));
  DNM_CHECK((size_t)(m + 1) * 16 <= 160 * 1024, "ncv too large for the basis-rotation kernel");
  if (max_its <= 0) max_its = 100;
  if (nev_max > m - 1) nev_max = m - 1;

  void *V = nullptr;
  DNM_TRY(basis_workspace((size_t)(m + 4) * (size_t)n_local * 16, &V));
  FoldFilter F;
  F.sigma = target;
  F.ta = vecptr(V, n_local, m + 1);
  F.tb = vecptr(V, n_local, m + 2);
  F.tc = vecptr(V, n_local, m + 3);
  ops.fold = &F;
  const bool debug = knob("DNM_KRYLOV_DEBUG") != nullptr;
  double nrmH = 0;
  DNM_TRY(operator_norm(ops, &nrmH, false));
  DNM_CHECK(nrmH > 0, "zero operator");

  // ---- the ends of the spectrum and the density of states near the target: one plain Lanczos run (interior_window) -
  const int64_t offset = hooks ? A->row0 : 0;
  double emin = 0, emax = 0, a = 0;
  {
    const int k0 = (int)std::min<int64_t>(Nglob - 1, std::max(60, 4 * nev));
    std::vector<double> al, be, wv, Sv;
    DNM_TRY(unit_random_start(ops, V, seed, offset));
    DNM_TRY(plain_lanczos(ops, V, n_local, k0, StopRule::norm(1e-12, nrmH), al, be));
    tridiag_ritz(al, be, wv, Sv);
    const char *we = knob("DNM_EIGS_INTERIOR_WINDOW");      // (experiments, tests) the estimate times f
    const InteriorWindow win = interior_window(wv, Sv, be[al.size() - 1], nrmH, Nglob, nev, target, we ? atof(we) : 1.0);
    emin = win.emin, emax = win.emax, a = win.a;
    if (debug)
      fprintf(stderr, "dnm_eigsolve_interior: %d probe steps, spectrum in [%.6g, %.6g] (|H|_inf %.6g), half-width %.4g "
              "for about %.0f levels\n", (int)al.size(), emin, emax, nrmH, a, win.nwant);
  }
  const double damping = 100.0;        // |p| <= 1 / damping outside the window: the nev-th wanted value, at about
                                       // two thirds of the half-width, stands cosh(0.745 acosh(100)) = 26 above it
  auto plan = [&]() -> int { return dnm_interior_filter_plan(emin, emax, target, a, damping, &F.d, &F.c, &F.e); };
  DNM_TRY(plan());

  // ---- start vector: p(A) of a random vector, which also shows whether the bounds hold (|p| <= 1 on the spectrum) ---
  F.on = true;
  for (int attempt = 0;; ++attempt) {
    void *x = vecptr(V, n_local, 1), *px = vecptr(V, n_local, 0);
    double npx = 0;
    DNM_TRY(unit_random_start(ops, x, seed + 1, offset));
    DNM_TRY(ops.apply_fold(x, px));
    DNM_TRY(ops.norm(px, &npx));
    if (debug) fprintf(stderr, "dnm_eigsolve_interior: degree %d, |p(A) x| = %.3g on a unit probe vector\n", F.d, npx);
    if (std::isfinite(npx) && npx <= 1.5 && npx > 0) {
      DNM_TRY(vk_scale(px, n_local, 1.0 / npx, 0, st));
      break;
    }
    DNM_CHECK(attempt < 6 && (emin > -nrmH || emax < nrmH), "the interior filter is unbounded on the operator's "
              "spectrum (bounds [%.6g, %.6g])", emin, emax);
    const double wdt = emax - emin;
    emin = std::max(-nrmH, emin - 0.05 * wdt);
    emax = std::min(nrmH, emax + 0.05 * wdt);
    DNM_TRY(plan());
  }

  // ---- thick-restart Lanczos on p(A), every vector against the whole basis -----------------------------------------
  ThickRestart tr(m);
  RitzInH rr;
  std::vector<zc> h;
  int its = 0, widenings = 0, extra_matvecs = 0;
  double tol_p = tol;
  while (true) {
    ++its;
    for (int j = tr.l; j < m; ++j) {
      void *p = vecptr(V, n_local, j + 1);
      DNM_TRY(ops.mult(vecptr(V, n_local, j), p));
      double bn = 0;
      DNM_TRY(ops.orthogonalize(p, V, j + 1, h, &bn, 2));
      tr.alpha[j] = h[j].real();
      tr.betav[j] = bn;
      // (p(A) has norm 1) invariant subspace: a fresh direction orthogonal to the basis
      if (!(bn > 1e-14)) DNM_TRY(tr.fresh_direction(ops, V, j, its, seed, offset));
      else DNM_TRY(vk_scale(p, n_local, 1.0 / bn, 0, st));
    }
    tr.project([](double x, double y) { return x > y; });      // p(sigma) = 1 on top
    int nconv = 0, nin = 0;
    for (int i = 0; i < m; ++i)
      if (tr.residual(i) <= tol_p) ++nconv; else break;
    for (int i = 0; i < m; ++i) if (tr.value(i) > 2.0 * F.bound()) ++nin;
    // thick restart: the converged pairs plus half of the rest, at least nev
    const int keep = tr.keep_count(nconv, nev);
    DNM_TRY(tr.restart(ops, V, keep));
    const bool last = its >= max_its;
    if (debug)
      fprintf(stderr, "dnm_eigsolve_interior: restart %d, %d pairs converged on the filter (tol %.1e), %d Ritz values in "
              "the window, %d multiplies\n", its, nconv, tol_p, nin, ops.matvecs);
    if (nconv >= nev || last) {
      F.on = false;
      const int mv0 = ops.matvecs;
      DNM_TRY(rayleigh_ritz_in_h(ops, V, F, std::min(keep, std::max(nconv, nev)), nev, nev_max, target, tol, nrmH, &rr));
      extra_matvecs += ops.matvecs - mv0;
      ops.matvecs = mv0;
      F.on = true;
      if (debug)
        fprintf(stderr, "dnm_eigsolve_interior: restart %d, Rayleigh-Ritz in H on %d vectors, %d pairs pass "
                "(largest residual / |H|_inf %.2e)\n", its, rr.nrr, rr.nok, rr.worst);
      if (rr.nok >= nev || last) break;
      // the filter's residuals were satisfied too early: ask for more, by what the measurement missed
      tol_p *= std::max(1e-3, std::min(0.3, 0.3 * tol / std::max(rr.miss, 1e-300)));
      continue;
    }
    // Fewer than nev levels in the window, all of them found (after the first cycle the Ritz values inside the window
    // are the well separated ones and converge first): widen it, keep the directions found so far as the new start
    if (its >= 2 && nin < nev && nconv >= nin && widenings < 8) {
      ++widenings;
      const double hfull = std::max(target - emin, emax - target);
      a = std::min(0.5 * hfull, a * std::min(2.0, std::max(1.25, (nev + 4.0) / std::max(nin, 1))));
      DNM_TRY(plan());
      std::vector<zc> ones(keep, zc(1.0 / std::sqrt((double)keep), 0.0));
      DNM_TRY(vk_set(F.ta, n_local, 0.0, 0.0, st));
      DNM_TRY(ops.maxpy(F.ta, V, keep, ones));
      DNM_TRY(vk_copy(vecptr(V, n_local, 0), F.ta, n_local, st));
      tr.l = 0;
      tr.theta.clear();
      tr.spike.clear();
      tol_p = tol;
      if (debug) fprintf(stderr, "dnm_eigsolve_interior: window widened to %.4g, degree %d\n", a, F.d);
    }
  }

  const int nout = std::min(rr.nok, nev_max);
  for (int i = 0; i < nout; ++i) evals[i] = rr.rth[i];
  if (evecs)
    for (int i = 0; i < nout; ++i) {
      void *dst = vecptr(evecs, n_local, i);
      DNM_TRY(vk_set(dst, n_local, 0.0, 0.0, st));
      DNM_TRY(ops.maxpy(dst, V, rr.nrr, rr.coefs(i)));
    }
  if (debug)
    fprintf(stderr, "dnm_eigsolve_interior: %d restarts, %d multiplies (+%d for Rayleigh-Ritz and the checks), degree %d, "
            "half-width %.4g, largest residual / |H|_inf %.2e\n", its, ops.matvecs, extra_matvecs, F.d, a, rr.worst);
  return finish(ops, stats, (nout >= nev) ? DNM_CONVERGED_TOL : DNM_DIVERGED_ITS, its, nout, rr.worst);
}

}  // extern "C"
