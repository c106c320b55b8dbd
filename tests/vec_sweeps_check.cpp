// The vector sweeps that have no C ABI entry, one call at a time on the GPU: dnm::vec_lanczos_update_host,
// dnm::vec_lanczos_dot_host and dnm::vk_reduce_partials, linked from the in-tree libdynamite_amd.so
// (tests/test_gpu_vec.py: test_sweeps_without_abi_entry builds and runs this program).  No kernels in here.
//
// Exact cases: vector entries are non-zero integers with |v| <= 8 from a small LCG, scalars are dyadic, so every
// intermediate value of the kernels is exactly representable in a double whatever the order of summation and
// whatever is contracted into an fma; the references are computed in int64_t and the comparison is bit equality.
// Written vectors carry 64 sentinel elements on either side inside their allocation, read-only ones NaN.
// Rounding cases (n = 100003, normal deviates) are held to gamma_k = k u / (1 - k u), u = 2^-53, k counted from the
// kernels (see rounding_cases).
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "vec_api.h"

namespace {

constexpr int G = 64;                        // guard elements
constexpr double SENT_RE = -1.2345678901234567e+200, SENT_IM = 7.6543210987654321e-200;
int failures = 0;

struct Z { double re, im; };

#define CK(call)                                                                       \
  do {                                                                                 \
    if ((call) != 0) {                                                                 \
      std::printf("FAILED call %s: %s\n", #call, dnm_last_error());                    \
      std::printf("%d failure(s)\n", failures + 1);                                    \
      std::exit(2);                                                                    \
    }                                                                                  \
  } while (0)

void report(bool good, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void report(bool good, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  std::printf("%s %s\n", good ? "ok    " : "FAILED", buf);
  if (!good) ++failures;
}

uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
inline uint32_t lcg() {
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(lcg_state >> 33);
}
// non-zero integer in [-8, 8]
inline int small_int() {
  const uint32_t r = lcg();
  const int m = 1 + (int)(r & 7);
  return (r & 8) ? -m : m;
}

struct IntVec {                              // a vector of Gaussian integers
  std::vector<int8_t> re, im;
  explicit IntVec(int64_t n) : re(n), im(n) {
    for (int64_t i = 0; i < n; ++i) { re[i] = (int8_t)small_int(); im[i] = (int8_t)small_int(); }
  }
};

// device vector of n elements between two guards
struct DevVec {
  void *base = nullptr;
  int64_t n;
  std::vector<Z> guard;
  DevVec(int64_t n_, bool writable) : n(n_), guard(G) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (auto &g : guard) g = writable ? Z{SENT_RE, SENT_IM} : Z{nan, nan};
    CK(dnm_malloc(&base, (size_t)(n + 2 * G) * sizeof(Z)));
    CK(dnm_memcpy_h2d(base, guard.data(), G * sizeof(Z), nullptr));
    CK(dnm_memcpy_h2d((Z *)base + G + n, guard.data(), G * sizeof(Z), nullptr));
  }
  ~DevVec() { dnm_free(base); }
  void *ptr() const { return (Z *)base + G; }
  void put(const std::vector<Z> &h) { CK(dnm_memcpy_h2d(ptr(), h.data(), (size_t)n * sizeof(Z), nullptr)); }
  // the payload; false when a guard has changed
  bool get(std::vector<Z> &h) const {
    std::vector<Z> all(n + 2 * G);
    CK(dnm_memcpy_d2h(all.data(), base, all.size() * sizeof(Z), nullptr));
    h.assign(all.begin() + G, all.begin() + G + n);
    return std::memcmp(all.data(), guard.data(), G * sizeof(Z)) == 0 &&
           std::memcmp(all.data() + G + n, guard.data(), G * sizeof(Z)) == 0;
  }
};

std::vector<Z> as_doubles(const IntVec &v, int64_t n) {
  std::vector<Z> h(n);
  for (int64_t i = 0; i < n; ++i) h[i] = Z{(double)v.re[i], (double)v.im[i]};
  return h;
}

bool same_bits(const std::vector<Z> &a, const std::vector<Z> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Z)) == 0);
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

const int64_t SIZES[] = {1, 255, 256, 257, 100003, (int64_t)1 << 21, ((int64_t)1 << 21) + 1, 3 * ((int64_t)1 << 20) + 77};
constexpr int64_t NMAX = 3 * ((int64_t)1 << 20) + 77;

// ---- p = scale (p - (are + i aim) v - b u), |p|^2 ------------------------------------------------------------------
// are = 3/4, aim = A/4 (A = -5 or 0), b = 1/2: 4 (p - a v - b u) = 4 p - (3 + i A) v - 2 u =: q in integers;
// scale = 1: p' = q / 4, |p'|^2 = sum |q|^2 / 16;  scale = 1/4: p' = q / 16, |p'|^2 = sum |q|^2 / 256
void lanczos_update_cases(const IntVec &P, const IntVec &V, const IntVec &U) {
  for (int64_t n : SIZES) {
    DevVec p(n, true), v(n, false), u(n, false);
    const std::vector<Z> hp = as_doubles(P, n);
    v.put(as_doubles(V, n));
    u.put(as_doubles(U, n));
    for (int with_u = 0; with_u < 2; ++with_u)
      for (int A : {0, -5})
        for (int sdiv : {1, 4}) {
          p.put(hp);
          double norm2 = -1.0;
          CK(dnm::vec_lanczos_update_host(p.ptr(), v.ptr(), with_u ? u.ptr() : nullptr, n, 0.75, A / 4.0, 0.5, &norm2,
                                          nullptr, 1.0 / sdiv));
          std::vector<Z> ref(n), got;
          int64_t sum = 0;
          for (int64_t i = 0; i < n; ++i) {
            int64_t qr = 4 * P.re[i] - (3 * V.re[i] - A * V.im[i]), qi = 4 * P.im[i] - (3 * V.im[i] + A * V.re[i]);
            if (with_u) { qr -= 2 * U.re[i]; qi -= 2 * U.im[i]; }
            ref[i] = Z{(double)qr / (4.0 * sdiv), (double)qi / (4.0 * sdiv)};
            sum += qr * qr + qi * qi;
          }
          const double nref = (double)sum / (16.0 * sdiv * sdiv);
          const bool guards = p.get(got);
          report(guards && same_bits(got, ref) && same_bits(norm2, nref),
                 "lanczos_update n=%lld u=%d aim=%g scale=%g: guards %d, p %d, |p|^2 %.17g (exact %.17g)", (long long)n,
                 with_u, A / 4.0, 1.0 / sdiv, (int)guards, (int)same_bits(got, ref), norm2, nref);
        }
  }
}

// ---- y = ys y - b z, sums conj(x) y and |y|^2 ------------------------------------------------------------------------
// b = 1/4, ys = 1 or 1/2: 4 y' = (4 ys) y - z =: q in integers; conj(x) y' = sum conj(x) q / 4, |y'|^2 = sum |q|^2 / 16
void lanczos_dot_cases(const IntVec &Y, const IntVec &Zv, const IntVec &X) {
  for (int64_t n : SIZES) {
    DevVec y(n, true), z(n, false), x(n, false);
    const std::vector<Z> hy = as_doubles(Y, n);
    z.put(as_doubles(Zv, n));
    x.put(as_doubles(X, n));
    for (int with_z = 0; with_z < 2; ++with_z)
      for (int ys4 : {4, 2}) {
        y.put(hy);
        double out[3] = {-1.0, -1.0, -1.0};
        CK(dnm::vec_lanczos_dot_host(y.ptr(), with_z ? z.ptr() : nullptr, x.ptr(), n, 0.25, out, nullptr, ys4 / 4.0));
        std::vector<Z> ref(n), got;
        int64_t sr = 0, si = 0, sn = 0;
        for (int64_t i = 0; i < n; ++i) {
          int64_t qr = ys4 * Y.re[i], qi = ys4 * Y.im[i];
          if (with_z) { qr -= Zv.re[i]; qi -= Zv.im[i]; }
          ref[i] = Z{(double)qr / 4.0, (double)qi / 4.0};
          sr += X.re[i] * qr + X.im[i] * qi;
          si += X.re[i] * qi - X.im[i] * qr;
          sn += qr * qr + qi * qi;
        }
        const bool guards = y.get(got);
        // (without z and with ys = 1 the reference is y itself: it must come back bit for bit)
        const bool sums = same_bits(out[0], (double)sr / 4.0) && same_bits(out[1], (double)si / 4.0) &&
                          same_bits(out[2], (double)sn / 16.0);
        report(guards && same_bits(got, ref) && sums,
               "lanczos_dot n=%lld z=%d yscale=%g: guards %d, y %d, sums %.17g %.17g %.17g (exact %.17g %.17g %.17g)",
               (long long)n, with_z, ys4 / 4.0, (int)guards, (int)same_bits(got, ref), out[0], out[1], out[2],
               (double)sr / 4.0, (double)si / 4.0, (double)sn / 16.0);
      }
  }
}

// ---- column sums of integer partials -----------------------------------------------------------------------------------
void reduce_cases() {
  const int shapes[][2] = {{1, 1}, {1, 3}, {255, 3}, {256, 3}, {257, 3}, {8192, 3}, {8193, 3}, {20000, 3}, {8193, 7}};
  constexpr int GD = 16;                     // guard doubles round the results
  for (const auto &sh : shapes) {
    const int nblocks = sh[0], ncols = sh[1];
    std::vector<double> part((size_t)nblocks * ncols);
    std::vector<int64_t> ref(ncols, 0);
    for (int b = 0; b < nblocks; ++b)
      for (int c = 0; c < ncols; ++c) {
        const int val = (int)(lcg() % 2001) - 1000;
        part[(size_t)b * ncols + c] = val;
        ref[c] += val;
      }
    void *dpart = nullptr, *dout = nullptr, *dtmp = nullptr;
    CK(dnm_malloc(&dpart, part.size() * sizeof(double)));
    CK(dnm_memcpy_h2d(dpart, part.data(), part.size() * sizeof(double), nullptr));
    CK(dnm_malloc(&dout, (ncols + 2 * GD) * sizeof(double)));
    const size_t ntmp = dnm::vk_reduce_scratch(ncols);
    CK(dnm_malloc(&dtmp, (ntmp + 2 * GD) * sizeof(double)));
    for (int two_level = 0; two_level < (nblocks > 8192 ? 2 : 1); ++two_level) {
      std::vector<double> hout(ncols + 2 * GD, SENT_RE), htmp(ntmp + 2 * GD, SENT_RE);
      CK(dnm_memcpy_h2d(dout, hout.data(), hout.size() * sizeof(double), nullptr));
      CK(dnm_memcpy_h2d(dtmp, htmp.data(), htmp.size() * sizeof(double), nullptr));
      CK(dnm::vk_reduce_partials((const double *)dpart, nblocks, ncols, (double *)dout + GD, nullptr,
                                 two_level ? (double *)dtmp + GD : nullptr));
      CK(dnm_stream_synchronize(nullptr));
      CK(dnm_memcpy_d2h(hout.data(), dout, hout.size() * sizeof(double), nullptr));
      CK(dnm_memcpy_d2h(htmp.data(), dtmp, htmp.size() * sizeof(double), nullptr));
      bool good = true, guards = true;
      for (int c = 0; c < ncols; ++c) good = good && same_bits(hout[GD + c], (double)ref[c]);
      for (int g = 0; g < GD; ++g)
        guards = guards && same_bits(hout[g], SENT_RE) && same_bits(hout[GD + ncols + g], SENT_RE) &&
                 same_bits(htmp[g], SENT_RE) && same_bits(htmp[GD + ntmp + g], SENT_RE);
      report(good && guards, "reduce_partials nblocks=%d ncols=%d tmp=%d: guards %d, column 0 %.17g (exact %lld)", nblocks,
             ncols, two_level, (int)guards, hout[GD], (long long)ref[0]);
    }
    dnm_free(dpart);
    dnm_free(dout);
    dnm_free(dtmp);
  }
}

// ---- rounding ------------------------------------------------------------------------------------------------------------
// n = 100003 runs one element per thread in 391 workgroups, whose partials one workgroup sums (391 <= 8192).
//  * an element of p or y: lanczos_update makes two fma, a third with u, and the multiplication by scale: k = 4;
//    lanczos_dot the multiplication by yscale and one fma: k = 2.  Bound: gamma_k times the sum of the |terms|.
//  * a sum, measured against the long-double sum over the vector THE DEVICE WROTE (so that it bounds the summation
//    alone): 2 fma per thread, 6 shuffle adds, 4 adds over the waves; second stage 2 adds per thread (391 partials
//    on 256 threads), 6 shuffle adds, 4 adds over the waves: k = 2 + 6 + 4 + 2 + 6 + 4 = 24.
long double gamma_k(int k) {
  const long double u = std::ldexp(1.0L, -53);
  return k * u / (1 - k * u);
}

void rounding_cases() {
  const int64_t n = 100003;
  std::mt19937_64 gen(20240607);
  std::normal_distribution<double> nd;
  auto draw = [&](std::vector<Z> &h) { h.resize(n); for (auto &e : h) { e.re = nd(gen); e.im = nd(gen); } };
  std::vector<Z> hp, hv, hu, got;
  draw(hp); draw(hv); draw(hu);
  DevVec p(n, true), v(n, false), u(n, false);
  p.put(hp); v.put(hv); u.put(hu);
  const long double are = 0.3, aim = -0.2, b = 0.7, scale = 1.1;
  {
    double norm2 = -1.0;
    CK(dnm::vec_lanczos_update_host(p.ptr(), v.ptr(), u.ptr(), n, (double)are, (double)aim, (double)b, &norm2, nullptr,
                                    (double)scale));
    const bool guards = p.get(got);
    long double worst = 0, sum = 0;
    bool good = guards;
    for (int64_t i = 0; i < n; ++i) {
      const long double pr = hp[i].re, pi = hp[i].im, vr = hv[i].re, vi = hv[i].im, ur = hu[i].re, ui = hu[i].im;
      const long double rr = scale * (pr - are * vr + aim * vi - b * ur), ri = scale * (pi - are * vi - aim * vr - b * ui);
      const long double mr = std::fabs(scale) * (std::fabs(pr) + std::fabs(are * vr) + std::fabs(aim * vi) + std::fabs(b * ur));
      const long double mi = std::fabs(scale) * (std::fabs(pi) + std::fabs(are * vi) + std::fabs(aim * vr) + std::fabs(b * ui));
      const long double er = std::fabs(got[i].re - rr) / mr, ei = std::fabs(got[i].im - ri) / mi;
      worst = std::fmax(worst, std::fmax(er, ei));
      sum += (long double)got[i].re * got[i].re + (long double)got[i].im * got[i].im;
    }
    good = good && worst <= gamma_k(4);                                                   // k = 4
    const long double es = std::fabs(norm2 - sum) / sum;
    good = good && es <= gamma_k(24);                                                     // k = 24
    report(good, "lanczos_update rounding n=%lld: p within %.2Lf u (gamma_4), |p|^2 within %.2Lf u (gamma_24), guards %d",
           (long long)n, worst / std::ldexp(1.0L, -53), es / std::ldexp(1.0L, -53), (int)guards);
  }
  {
    // y = hp again, z = hu, x = hv
    p.put(hp);
    const long double ys = 0.9, bz = 0.7;
    double out[3] = {-1.0, -1.0, -1.0};
    CK(dnm::vec_lanczos_dot_host(p.ptr(), u.ptr(), v.ptr(), n, (double)bz, out, nullptr, (double)ys));
    const bool guards = p.get(got);
    long double worst = 0, sr = 0, si = 0, sn = 0, mr = 0, mi = 0;
    for (int64_t i = 0; i < n; ++i) {
      const long double yr = hp[i].re, yi = hp[i].im, zr = hu[i].re, zi = hu[i].im;
      const long double er = std::fabs(got[i].re - (ys * yr - bz * zr)) / (std::fabs(ys * yr) + std::fabs(bz * zr));
      const long double ei = std::fabs(got[i].im - (ys * yi - bz * zi)) / (std::fabs(ys * yi) + std::fabs(bz * zi));
      worst = std::fmax(worst, std::fmax(er, ei));
      const long double xr = hv[i].re, xi = hv[i].im, gr = got[i].re, gi = got[i].im;
      sr += xr * gr + xi * gi;
      si += xr * gi - xi * gr;
      sn += gr * gr + gi * gi;
      mr += std::fabs(xr * gr) + std::fabs(xi * gi);
      mi += std::fabs(xr * gi) + std::fabs(xi * gr);
    }
    const long double e0 = std::fabs(out[0] - sr) / mr, e1 = std::fabs(out[1] - si) / mi, e2 = std::fabs(out[2] - sn) / sn;
    const bool good = guards && worst <= gamma_k(2) &&                                    // k = 2
                      e0 <= gamma_k(24) && e1 <= gamma_k(24) && e2 <= gamma_k(24);        // k = 24
    report(good, "lanczos_dot rounding n=%lld: y within %.2Lf u (gamma_2), sums within %.2Lf %.2Lf %.2Lf u (gamma_24), guards %d",
           (long long)n, worst / std::ldexp(1.0L, -53), e0 / std::ldexp(1.0L, -53), e1 / std::ldexp(1.0L, -53),
           e2 / std::ldexp(1.0L, -53), (int)guards);
  }
}

}  // namespace

int main() {
  const auto t0 = std::chrono::steady_clock::now();
  {
    const IntVec A(NMAX), B(NMAX), Cc(NMAX);
    lanczos_update_cases(A, B, Cc);
    lanczos_dot_cases(A, B, Cc);
  }
  reduce_cases();
  rounding_cases();
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("%.2f s\n", secs);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
