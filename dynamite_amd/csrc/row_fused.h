// Launch interfaces of the one-thread-per-row multiplies with a fused epilogue (row_fused_kernels.hip): the row
// kernels of kernels.h (gather_matvec_kernel, sc_matvec_kernel) under the contract the tiled and block kernels have.
#pragma once

#include "kernels.h"

namespace dnm {

// What rides on the store of a row's sum.  All vectors are local (one element per row, at the position y is stored).
//   zinit  != null: y = A x - zscale * zinit
//   zinit2 != null: ... + (z2re + i z2im) * zinit2
//   dot_out != null: per-workgroup partial sums of conj(x_row) y_row (re, im) and |y_row|^2 -- 3 doubles per
//                    workgroup, [workgroup][3], every entry written by the launch (vk_reduce_partials sums them);
//                    needs a square operator on one subspace: x_row is the amplitude of x at the row's own index
struct RowFuse {
  const void *zinit = nullptr;
  double zscale = 0.0;
  const void *zinit2 = nullptr;
  double z2re = 0.0, z2im = 0.0;
  double *dot_out = nullptr;
};

// rows [0, M) on one rank, x the whole right vector in its own layout; workgroups: gather_num_blocks(M)
int launch_gather_matvec_fused(const DevMsc &msc, const SubView &left, const SubView &right, int64_t M,
                               const double *diag, const void *x, void *y, const RowFuse &f, hipStream_t st);

// SpinConserve(L,k) on both sides, rows [0, M) on one rank; workgroups: sc_num_blocks(M)
int launch_sc_matvec_fused(const DevMsc &msc, const ScMask *scm, const ScLow &low, const SubView &sub, int64_t M,
                           const double *diag, const void *x, void *y, const RowFuse &f, hipStream_t st);

}  // namespace dnm
