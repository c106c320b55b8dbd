// The Gram matrix of many vectors in one pass over them: G[a][b] = sum_r conj(x_a[r]) x_b[r] for 1 <= nvec <= 64 device
// vectors of n complex128 elements each -- the overlaps <m|n> of a set of eigenvectors, or with the images O|n> among
// the vectors the matrix elements <m|O|n>.  The operand matrix has vector c as its column c, read as it lies:
//   A[r, c] = x_c[r],   G = A^H A      (nvec x nvec complex128, Hermitian)
// the Hermitian rank-N update of gram_tile.h on v_mfma_f64_16x16x4_f64, NB = ceil(nvec / 16) <= 4 tile rows.  The vectors
// are separate allocations at any 16-byte-aligned addresses and a pointer may repeat; the pointers travel by value in
// the kernel's arguments (64 x 8 bytes), so there is no device table and no upload.
//
// Panel fill: a unit of work is 64 consecutive rows of one column, taken by one wavefront -- consecutive lanes
// consecutive rows, so a wavefront reads a 1 KB run of one vector with 16-byte loads -- and the units of a panel go round
// the four wavefronts.  There are no partner gathers, signs or tables, so the fill is two steps with the matrix cores
// between them: a wavefront fetches its units of the NEXT panel into registers, multiplies the panel in LDS while those
// loads are in flight, and stores the registers into the panel once every wavefront is done with it.  That takes
// 4 NB 2^(B - 6) units of four registers per lane, which is what sets the panel: 2^7 rows up to two tile rows, 2^6 from
// three on (VGRAM_B; at four tile rows the accumulators leave room for no more; measured against the bond-swap sweep's
// rule and two other tables: docs/lab/state_gram.md).  Rows at or beyond n are written as
// zeros; the columns at or beyond nvec and the padding column are zeroed once and never written again.
//
// The workgroups are the bond-swap sweep's: one per 2^9 rows, at most PM_MAX_WG.
//
// No atomics: wavefronts and workgroups are summed in a fixed order (gram_tile.h).  The number of workgroups follows from
// (nvec, n) alone: two calls return the same bits on any device.
#include "vgram.h"

namespace dnm {

// log2 of the panel's rows at 1, 2, 3 and 4 tile rows; overridable for experiments
#ifndef VGRAM_B
#define VGRAM_B 7, 7, 6, 6
#endif
constexpr int VGRAM_B_OF[4] = {VGRAM_B};
constexpr int VGRAM_B_MAX = 9, VGRAM_B_MIN = 6;
constexpr int VGRAM_ROWS_PER_WG_LOG2 = 9;       // workgroups = ceil(n / 2^9), at most PM_MAX_WG

constexpr bool vgram_b_in_range(int nb) {
  return nb == 0 || (VGRAM_B_OF[nb - 1] >= VGRAM_B_MIN && VGRAM_B_OF[nb - 1] <= VGRAM_B_MAX && vgram_b_in_range(nb - 1));
}
static_assert(vgram_b_in_range(4) && VGRAM_B_MAX <= VGRAM_ROWS_PER_WG_LOG2,
              "a panel is at least one wavefront's run, and a workgroup has at least one panel");

int vgram_plan(int nvec, int64_t n, GramPlan *p) {
  GramPlan q{};
  const int64_t nwg = (n + ((int64_t)1 << VGRAM_ROWS_PER_WG_LOG2) - 1) >> VGRAM_ROWS_PER_WG_LOG2;
  const int b = VGRAM_B_OF[(nvec + 15) / 16 - 1];
  if (!gram_plan(nvec, n, 0, VGRAM_B_MAX, VGRAM_B_MAX, VGRAM_B_MIN, b, nwg, &q) || q.B != b) {
    set_error("internal: state Gram panel of %zu bytes", q.lds_bytes);
    return 1;
  }
  *p = q;
  return 0;
}

struct VgramArgs {
  int64_t nrows, npanels, per_wg;
  int32_t nvec;
  const c128 *x[64];
};

template <int NB>
__global__ void __launch_bounds__(PM_NT)
vgram_kernel(const VgramArgs a, double *__restrict__ partial) {
  constexpr int NACC = NB * (NB + 1) / 2 + NB * NB;
  constexpr int LDP = 16 * NB + 1;
  constexpr int B = VGRAM_B_OF[NB - 1], ROWS = 1 << B, RUNS_LOG2 = B - 6;
  constexpr int NWAVES = PM_NT / 64;
  constexpr int UNITS = (16 * NB << RUNS_LOG2) / NWAVES;        // of a wavefront, per panel
  extern __shared__ __align__(16) unsigned char vgram_lds[];
  c128 *panel = reinterpret_cast<c128 *>(vgram_lds);
  const int tid = threadIdx.x;
  // (the padding column and the columns at or beyond nvec stay zero for the whole sweep)
  for (int e = tid; e < LDP * ROWS; e += PM_NT) panel[e] = make_double2(0.0, 0.0);

  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, slot = lane >> 4;
  mfma_acc acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = mfma_acc{0.0, 0.0, 0.0, 0.0};

  // units of 64 rows of one column: unit u = column u >> RUNS_LOG2, run u & (runs - 1) of the panel, and a wavefront
  // takes the units wave, wave + 4, ...; its number is uniform, so the columns' pointers are scalar loads from the
  // arguments, made once: they are the same for every panel
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const c128 *px[UNITS];
#pragma unroll
  for (int i = 0; i < UNITS; ++i) {
    const int col = (wave_u + NWAVES * i) >> RUNS_LOG2;
    px[i] = a.x[col < a.nvec ? col : 0];
  }
  c128 v[UNITS];
  // the wavefront's part of panel g into registers: zeros at and beyond row n (the load then reads row n - 1: in bounds)
  auto fetch = [&](int64_t g) {
    const int64_t base = g << B;
#pragma unroll
    for (int i = 0; i < UNITS; ++i) {
      const int u = wave_u + NWAVES * i;
      const int col = u >> RUNS_LOG2;
      if (col >= a.nvec) break;
      const int64_t p = base + (((u & ((1 << RUNS_LOG2) - 1)) << 6) + lane);
      const bool in = p < a.nrows;
      const c128 w = px[i][in ? p : a.nrows - 1];
      v[i] = in ? w : make_double2(0.0, 0.0);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < UNITS; ++i) {
      const int u = wave_u + NWAVES * i;
      const int col = u >> RUNS_LOG2;
      if (col >= a.nvec) break;
      panel[((((u & ((1 << RUNS_LOG2) - 1)) << 6) + lane)) * LDP + col] = v[i];
    }
  };

  const int64_t g0 = (int64_t)blockIdx.x * a.per_wg;
  int64_t g1 = g0 + a.per_wg;
  if (g1 > a.npanels) g1 = a.npanels;
  if (g0 < g1) fetch(g0);
  __syncthreads();
  for (int64_t g = g0; g < g1; ++g) {
    stage();
    __syncthreads();
    if (g + 1 < g1) fetch(g + 1);
    pm_tile_multiply<NB>(panel, ROWS, wave, slot, r, acc);
    __syncthreads();
  }
  pm_tile_reduce_store<NACC>(reinterpret_cast<double *>(vgram_lds), wave, slot, r, acc,
                             partial + (int64_t)blockIdx.x * (NACC * 256));
}

__global__ void __launch_bounds__(PM_NT)
vgram_finalize_kernel(const double *__restrict__ partial, int nwg, int nb, int D, c128 *__restrict__ out) {
  pm_tile_finalize(partial, nwg, nb, D, out);
}

int launch_vec_gram(const void *const *xs, int nvec, const GramPlan &p, void *partial, void *out, hipStream_t st) {
  if (nvec < 1 || nvec > 64 || p.nb != (nvec + 15) / 16 || p.B != VGRAM_B_OF[p.nb - 1] || p.nrows < 1) {
    set_error("internal: state Gram matrix of %d vectors of %lld rows on %d tile rows, panels of 2^%d rows", nvec,
              (long long)p.nrows, p.nb, p.B);
    return 1;
  }
  VgramArgs a{};
  a.nrows = p.nrows;
  a.npanels = p.npanels;
  a.per_wg = p.per_wg;
  a.nvec = nvec;
  for (int c = 0; c < nvec; ++c) a.x[c] = (const c128 *)xs[c];
  double *pp = (double *)partial;
  // (the fill knows no subspace: one instance per number of tile rows)
  DNM_TRY(gram_dispatch<false>(DNM_FULL, p.nb, "the state Gram matrix", "internal: state Gram matrix type %d",
                               [&](auto, auto NB) {
    auto k = vgram_kernel<decltype(NB)::value>;
    DNM_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.nwg), dim3(PM_NT), p.lds_bytes, st, a, pp);
    DNM_HIP(hipGetLastError());
    return 0;
  }));
  hipLaunchKernelGGL(vgram_finalize_kernel, dim3((unsigned)(p.nb * (p.nb + 1) / 2)), dim3(PM_NT), 0, st,
                     (const double *)pp, p.nwg, p.nb, nvec, (c128 *)out);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
