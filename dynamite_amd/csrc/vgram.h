// The Gram matrix of nvec <= 64 vectors of n elements (vgram_kernels.hip): G[a][b] = sum_r conj(x_a[r]) x_b[r], column c
// of the operand matrix the vector c as it lies, on the panel scheme of gram_tile.h.
#pragma once
#include "gram_tile.h"

namespace dnm {

// host arithmetic from (nvec, n) alone
int vgram_plan(int nvec, int64_t n, GramPlan *p);
// xs: nvec device pointers (host array; 16-byte aligned, any may repeat); p: vgram_plan(nvec, n), n >= 1; partial:
// p.partial_bytes; out: nvec^2 complex128 (device)
int launch_vec_gram(const void *const *xs, int nvec, const GramPlan &p, void *partial, void *out, hipStream_t st);

}  // namespace dnm
