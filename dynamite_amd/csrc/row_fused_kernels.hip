// One-thread-per-row multiplies with a fused epilogue, for gfx950 (MI355X).
//
// The row kernels of matvec_kernels.hip (gather_matvec_kernel: any subspace pair through the index maps of
// subspace.h; sc_matvec_kernel: SpinConserve pairs by incremental colex rank) under the contract the tiled and
// SpinConserve block kernels have: a row owns its output element, so the recurrence terms
//   y = A x - b z + c z2
// are added in registers where the row's sum is stored -- one launch and 16 B/row per added vector instead of a
// sweep of 48 B/row each -- and the sums of a Lanczos step, <x, y> and |y|^2, leave the launch as per-workgroup
// partials.  The gathers, the unranking and the kind of store are those of the plain kernels; only single-rank
// launches (no column window, no column-range sweep) exist here.
#include <cstdint>

#include "row_fused.h"

namespace dnm {

typedef double2 c128;
typedef double d2v __attribute__((ext_vector_type(2)));

namespace {

constexpr int ROW_NT = 256;             // = GATHER_NT = SC_NT: gather_num_blocks / sc_num_blocks size the grids
constexpr int NCK_LDS = 2 * 1024;       // int64 entries of a SpinConserve binomial table staged in LDS (16 KB)

struct FuseDev {
  const c128 *z;
  double b;
  const c128 *z2;
  double cre, cim;
  double *dot;
};

__device__ __forceinline__ double flip(double c, uint32_t parity_bit) {
  const int hi = __double2hiint(c) ^ (int)(parity_bit << 31);
  return __hiloint2double(hi, __double2loint(c));
}

// the recurrence terms on a row's sum
__device__ __forceinline__ void add_terms(const FuseDev &f, int64_t pos, double &re, double &im) {
  if (f.z) {
    const c128 zv = f.z[pos];
    re = fma(-f.b, zv.x, re);
    im = fma(-f.b, zv.y, im);
  }
  if (f.z2) {
    const c128 zv = f.z2[pos];
    re = fma(f.cre, zv.x, re);
    im = fma(f.cre, zv.y, im);
    re = fma(-f.cim, zv.y, re);
    im = fma(f.cim, zv.x, im);
  }
}

// workgroup sums of (conj(x) y).re, (conj(x) y).im, |y|^2 -> dot[3 * workgroup + c]; every thread of the
// workgroup calls this (rows past the end with zeros)
__device__ __forceinline__ void block_sums(double *__restrict__ dot, c128 xs, double re, double im) {
  __shared__ double part[ROW_NT / 64][3];
  double s0 = fma(xs.x, re, xs.y * im), s1 = fma(xs.x, im, -xs.y * re), s2 = fma(re, re, im * im);
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, 64);
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = s0;
    part[threadIdx.x >> 6][1] = s1;
    part[threadIdx.x >> 6][2] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int w = 0; w < ROW_NT / 64; ++w) s += part[w][threadIdx.x];
    dot[3 * (int64_t)blockIdx.x + threadIdx.x] = s;
  }
}

template <int T>
__device__ __forceinline__ SubView stage(const SubView &s, int64_t *lds_tab, int &used) {
  SubView r = s;
  if constexpr (T == DNM_SPIN_CONSERVE) {
    const int n = (s.k + 1) * s.ld;
    if (used + n <= NCK_LDS) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) lds_tab[used + i] = s.nchoosek[i];
      r.nchoosek = lds_tab + used;
      used += n;
    }
  }
  return r;
}

// rows [0, M): y[row] = sum_m c_m(row) x[col_m(row)] + the fused terms (gather_matvec_kernel's row loop)
template <int LT, int RT, bool DOT>
__global__ void __launch_bounds__(ROW_NT)
gather_matvec_fused_kernel(const DevMsc msc, const SubView left_g, const SubView right_g, int64_t M,
                           const double *__restrict__ diag, const c128 *__restrict__ x, c128 *__restrict__ y,
                           const FuseDev f) {
  __shared__ int64_t nck[NCK_LDS];
  int used = 0;
  const SubView left = stage<LT>(left_g, nck, used);
  const SubView right = stage<RT>(right_g, nck, used);
  if (used) __syncthreads();

  const int64_t row = (int64_t)blockIdx.x * ROW_NT + threadIdx.x;
  const bool active = row < M;
  if (!DOT && !active) return;
  double accr = 0.0, acci = 0.0;
  c128 xs = make_double2(0.0, 0.0);
  if (active) {
    const int xswz = right.swz;
    const int64_t ket = Sub<LT>::i2s(row, left);
    int m0 = 0;
    if (DOT || diag) xs = x[vec_pos(row, xswz)];
    if (diag) {
      accr = diag[row] * xs.x;
      acci = diag[row] * xs.y;
      m0 = 1;
    }
    for (int m = m0; m < msc.nmasks; ++m) {
      const int64_t mask = msc.masks[m];
      const int64_t bra = ket ^ mask;
      const int64_t col = Sub<RT>::s2i(bra, right);
      if (col < 0) continue;   // projection semantics
      double cre = 0.0, cim = 0.0;
      for (int64_t t = msc.mask_offsets[m]; t < msc.mask_offsets[m + 1]; ++t) {
        const int64_t sg = msc.signs[t];
        const double c = flip(msc.real_coeffs[t], (uint32_t)__popcll((uint64_t)(bra & sg)) & 1u);
        if (__popcll((uint64_t)(mask & sg)) & 1) cim += c; else cre += c;
      }
      const c128 xv = x[vec_pos(col, xswz)];
      accr = fma(cre, xv.x, accr);
      acci = fma(cre, xv.y, acci);
      accr = fma(-cim, xv.y, accr);
      acci = fma(cim, xv.x, acci);
    }
    const int64_t pos = vec_pos(row, left.swz);
    add_terms(f, pos, accr, acci);
    y[pos] = make_double2(accr, acci);
  }
  if (DOT) block_sums(f.dot, xs, accr, acci);
}

// SpinConserve(L,k) on both sides (sc_matvec_kernel's row loop): column = row + a difference of binomials
template <bool IN_LDS, bool DOT>
__global__ void __launch_bounds__(ROW_NT)
sc_matvec_fused_kernel(const DevMsc msc, const ScMask *__restrict__ scm, const ScLow low, const SubView sub_g,
                       int64_t M, const double *__restrict__ diag, const c128 *__restrict__ x,
                       c128 *__restrict__ y, const FuseDev f) {
  __shared__ int64_t nck[NCK_LDS];
  const int ld = sub_g.ld, kk = sub_g.k, Lb = sub_g.L;
  if (IN_LDS) {
    const int ntab = (kk + 1) * ld;
    for (int i = threadIdx.x; i < ntab; i += ROW_NT) nck[i] = sub_g.nchoosek[i];
    __syncthreads();
  }
  // LDS reads when the table fits: a pointer that may be either LDS or global compiles to FLAT loads
#define SC_TAB(i) (IN_LDS ? nck[(i)] : sub_g.nchoosek[(i)])

  const int64_t row = (int64_t)blockIdx.x * ROW_NT + threadIdx.x;
  const bool active = row < M;
  if (!DOT && !active) return;
  double accr = 0.0, acci = 0.0;
  c128 xs = make_double2(0.0, 0.0);
  if (active) {
    // the greedy walk over the positions >= 16, then one lookup for the low 16 bits
    uint64_t ket = 0;
    {
      int64_t idx = row;
      int k = kk;
      for (int n = Lb; n > 16; --n) {
        const int64_t here = (k > n - 1) ? 0 : SC_TAB(k * ld + (n - 1));
        ket <<= 1;
        if (idx >= here) { idx -= here; --k; ket |= 1; }
      }
      const uint64_t lowbits = low.tab[low.off[k] + (int32_t)idx];
      ket = Lb > 16 ? ((ket << 16) | lowbits) : lowbits;
    }
    int m0 = 0;
    if (DOT || diag) xs = x[row];
    if (diag) {
      const double dg = __builtin_nontemporal_load(diag + row);
      accr = dg * xs.x;
      acci = dg * xs.y;
      m0 = 1;
    }
    for (int m = m0; m < msc.nmasks; ++m) {
      if (scm[m].fast) {
        // adjacent bond with local signs: one lookup, two possible coefficients
        const int lo = scm[m].lo;
        const uint32_t pair = (uint32_t)(ket >> lo) & 3u;
        if (pair == 1u || pair == 2u) {
          const bool up = pair == 1u;
          const int ord0 = __popcll(ket & ((1ull << lo) - 1));
          const int64_t d = SC_TAB(ord0 * ld + lo);       // C(lo, ord0)
          const c128 xv = x[up ? row + d : row - d];
          const double cre = up ? scm[m].up_re : scm[m].dn_re;
          const double cim = up ? scm[m].up_im : scm[m].dn_im;
          accr = fma(cre, xv.x, accr);
          acci = fma(cre, xv.y, acci);
          accr = fma(-cim, xv.y, accr);
          acci = fma(cim, xv.x, acci);
        }
        continue;
      }
      const uint64_t mask = (uint64_t)msc.masks[m];
      const uint64_t bra = ket ^ mask;
      int64_t delta = 0;
      if (mask && (mask & (mask + 1)) == 0) {
        // the mask flips every spin below c: among the c-bit patterns with the same number of ones the
        // complement reverses the order -- row = hc + r, col = hc + C(c, n1) - 1 - r
        if (__popcll(bra) != kk) continue;
        const int c = 64 - __clzll((long long)mask);
        const int n1 = __popcll(ket & mask);
        int64_t hc = 0;
        uint64_t hb = ket >> c;
        int o = n1;
        while (hb) {
          const int p = c + __ffsll((long long)hb) - 1;
          ++o;
          hc += SC_TAB(o * ld + p);
          hb &= hb - 1;
        }
        delta = SC_TAB(n1 * ld + c) - 1 - 2 * (row - hc);
      } else if (mask) {
        if (__popcll(bra) != kk) continue;             // leaves the subspace: projection semantics
        const int lo = __ffsll((long long)mask) - 1;
        const int hi = 63 - __clzll((long long)mask);
        const uint64_t span = (hi >= 63 ? ~0ull : ((2ull << hi) - 1)) & ~((1ull << lo) - 1);
        const int ord0 = __popcll(ket & ((1ull << lo) - 1));
        uint64_t bb = bra & span, kb = ket & span;
        int o = ord0;
        while (bb) {
          const int p = __ffsll((long long)bb) - 1;
          ++o;
          if (o <= p) delta += SC_TAB(o * ld + p);
          bb &= bb - 1;
        }
        o = ord0;
        while (kb) {
          const int p = __ffsll((long long)kb) - 1;
          ++o;
          if (o <= p) delta -= SC_TAB(o * ld + p);
          kb &= kb - 1;
        }
      }
      double cre = 0.0, cim = 0.0;
      for (int64_t t = msc.mask_offsets[m]; t < msc.mask_offsets[m + 1]; ++t) {
        const uint64_t sg = (uint64_t)msc.signs[t];
        const double c = flip(msc.real_coeffs[t], (uint32_t)__popcll(bra & sg) & 1u);
        if (__popcll(mask & sg) & 1) cim += c; else cre += c;
      }
      const c128 xv = x[row + delta];
      accr = fma(cre, xv.x, accr);
      acci = fma(cre, xv.y, acci);
      accr = fma(-cim, xv.y, accr);
      acci = fma(cim, xv.x, acci);
    }
    add_terms(f, row, accr, acci);
    const d2v v = {accr, acci};
    __builtin_nontemporal_store(v, reinterpret_cast<d2v *>(y + row));
  }
  if (DOT) block_sums(f.dot, xs, accr, acci);
#undef SC_TAB
}

FuseDev to_dev(const RowFuse &f) {
  return FuseDev{(const c128 *)f.zinit, f.zscale, (const c128 *)f.zinit2, f.z2re, f.z2im, f.dot_out};
}

template <int LT>
int gather_fused_r(const DevMsc &msc, const SubView &l, const SubView &r, int64_t M, const double *diag,
                   const void *x, void *y, const FuseDev &f, hipStream_t st) {
  const dim3 grid((unsigned)gather_num_blocks(M)), blk(ROW_NT);
#define DNM_GF(RT)                                                                                            \
  case RT:                                                                                                    \
    if (f.dot)                                                                                                \
      hipLaunchKernelGGL((gather_matvec_fused_kernel<LT, RT, true>), grid, blk, 0, st, msc, l, r, M, diag,    \
                         (const c128 *)x, (c128 *)y, f);                                                      \
    else                                                                                                      \
      hipLaunchKernelGGL((gather_matvec_fused_kernel<LT, RT, false>), grid, blk, 0, st, msc, l, r, M, diag,   \
                         (const c128 *)x, (c128 *)y, f);                                                      \
    break;
  switch (r.type) {
    DNM_GF(DNM_FULL) DNM_GF(DNM_PARITY) DNM_GF(DNM_SPIN_CONSERVE) DNM_GF(DNM_EXPLICIT)
    default: set_error("bad right subspace type"); return 1;
  }
#undef DNM_GF
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int launch_gather_matvec_fused(const DevMsc &msc, const SubView &left, const SubView &right, int64_t M,
                               const double *diag, const void *x, void *y, const RowFuse &f, hipStream_t st) {
  DNM_CHECK(M > 0 && M + ROW_NT < (int64_t)1 << 32, "row count out of range (one thread per row, fewer than 2^32 per launch)");
  DNM_CHECK(gather_rows_per_block() == ROW_NT, "internal: workgroup size of the row kernels");
  DNM_CHECK(!f.dot_out || (left.type == right.type && left.dim == right.dim && left.swz == right.swz),
            "the fused sums need a square operator on one subspace");
  const FuseDev d = to_dev(f);
  switch (left.type) {
    case DNM_FULL: return gather_fused_r<DNM_FULL>(msc, left, right, M, diag, x, y, d, st);
    case DNM_PARITY: return gather_fused_r<DNM_PARITY>(msc, left, right, M, diag, x, y, d, st);
    case DNM_SPIN_CONSERVE: return gather_fused_r<DNM_SPIN_CONSERVE>(msc, left, right, M, diag, x, y, d, st);
    case DNM_EXPLICIT: return gather_fused_r<DNM_EXPLICIT>(msc, left, right, M, diag, x, y, d, st);
  }
  set_error("bad left subspace type");
  return 1;
}

int launch_sc_matvec_fused(const DevMsc &msc, const ScMask *scm, const ScLow &low, const SubView &sub, int64_t M,
                           const double *diag, const void *x, void *y, const RowFuse &f, hipStream_t st) {
  DNM_CHECK(M > 0 && M + ROW_NT < (int64_t)1 << 32, "row count out of range (one thread per row, fewer than 2^32 per launch)");
  DNM_CHECK(sc_rows_per_block() == ROW_NT, "internal: workgroup size of the row kernels");
  const FuseDev d = to_dev(f);
  const dim3 grid((unsigned)sc_num_blocks(M)), blk(ROW_NT);
  const bool in_lds = (sub.k + 1) * sub.ld <= NCK_LDS;
#define DNM_SF(LDS, DOT)                                                                                     \
  hipLaunchKernelGGL((sc_matvec_fused_kernel<LDS, DOT>), grid, blk, 0, st, msc, scm, low, sub, M, diag,      \
                     (const c128 *)x, (c128 *)y, d)
  if (in_lds) { if (d.dot) DNM_SF(true, true); else DNM_SF(true, false); }
  else { if (d.dot) DNM_SF(false, true); else DNM_SF(false, false); }
#undef DNM_SF
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
