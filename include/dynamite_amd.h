/*
 * dynamite_amd.h -- C ABI of the MI355X-native matrix-free spin-operator engine.
 *
 * This is the drop-in boundary for dynamite's `_backend` shell-matrix path:
 * the entry points below are what dynamite's Cython layer (bpetsc.pyx /
 * bsubspace.pyx) would bind instead of PETSc MatShell + SLEPc MFN/EPS.  Each
 * declaration cites the reference interface it replaces (paths relative to
 * the reference repository root).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure;
 *     dnm_last_error() returns a thread-local message (the reference returns
 *     PetscErrorCode and raises petsc4py.Error, bpetsc.pyx:135-136);
 *   - all integers describing states / masks / indices are int64_t (the
 *     reference's PetscInt under --with-64-bit-indices, bbuild.pyx:28-33);
 *   - state vectors are device pointers to interleaved complex128
 *     (re, im doubles), length = subspace dimension (local part when
 *     partitioned);
 *   - host arrays passed in are BORROWED for the duration of the call; the
 *     handle keeps its own copies (BuildContext deep-copies,
 *     src/dynamite/_backend/bpetsc_template_2.c:275-297);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Kernels are enqueued asynchronously; functions that return host scalars
 *     synchronise that stream.
 */
#ifndef DYNAMITE_AMD_H
#define DYNAMITE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* errors / device                                                    */
/* ------------------------------------------------------------------ */
const char *dnm_last_error(void);
int dnm_version(void);
int dnm_device_count(int *count);
int dnm_set_device(int device);
/* thin device-memory helpers so a non-torch host (Cython/C) can own vectors;
 * replaces PETSc VecCreate/VecDestroy for VECCUDA
 * (src/dynamite/_backend/bcuda_template_2.cu:110-139 MatCreateVecs_GPU). */
int dnm_malloc(void **dptr, size_t bytes);
int dnm_free(void *dptr);
int dnm_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int dnm_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int dnm_stream_synchronize(void *stream);

/* ------------------------------------------------------------------ */
/* subspaces -- src/dynamite/_backend/bsubspace_impl.h                */
/* ------------------------------------------------------------------ */
/* subspace_type, bsubspace_impl.h:17-23 */
enum { DNM_FULL = 0, DNM_PARITY = 1, DNM_EXPLICIT = 2, DNM_SPIN_CONSERVE = 3 };

/* data_Full / data_Parity / data_SpinConserve / data_Explicit
 * (bsubspace_impl.h:41-44, 95-99, 161-167, 265-272) folded into one POD.
 * Python holders: bsubspace.pyx:68-114 (CFull, CParity, CSpinConserve,
 * CExplicit). */
typedef struct dnm_subspace {
  int32_t type;
  int64_t L;
  int64_t space;               /* Parity: 0 even, 1 odd */
  int64_t k;                   /* SpinConserve */
  int64_t ld_nchoosek;         /* SpinConserve: L+1 */
  const int64_t *nchoosek;     /* SpinConserve: (k+1)*(L+1), [kk*ld+LL] = C(LL,kk) */
  int64_t dim;                 /* Explicit */
  const int64_t *state_map;    /* Explicit: idx -> state */
  const int64_t *rmap_indices; /* Explicit: NULL when state_map is sorted */
  const int64_t *rmap_states;  /* Explicit: sorted states */
  /* Layout of state vectors on this subspace in device memory (no counterpart in the reference: a PETSc Vec is
   * opaque too).  0: element i of a rank's block is at position i.  S >= 5, Full / Parity only: XOR-swizzled,
   * element i is at position  i ^ (((i >> S) & (2^(S-4) - 1)) << 4)  -- index bits [S, 2S-4) folded onto bits
   * [4, S), an involution that keeps 256-byte runs together.  The far-apart runs of the tiled multiply's window
   * passes then spread over the L2 sets.  Every dnm_* call that takes a vector of this
   * subspace expects this layout; dnm_vec_swizzle_copy converts to and from index order.
   * SpinConserve: 0 or a | w << 8 (a low bits, w window bits): the three-field internal layout of
   * dynamite_amd/csrc/sc3.h -- the blocks of equal top bits T = state >> (a + w) stay where the reference order has
   * them, inside a block the rows (T, W) are grouped by popcount(W), ordered by the rank of W, and padded to 128-byte
   * lines (padding holds zeros): a vector then has dnm_vec_layout_size() elements instead of C(L, k).  The two-pass
   * SpinConserve multiply works in this layout; dnm_vec_layout_copy / _positions convert.  Partitions hand whole
   * T blocks to a rank (dnm_vec_layout_partition). */
  int32_t vec_swizzle;
  /* SpinConserve in the internal layout, one rank: NULL, or L entries -- spin i of the reference's labelling is bit
   * site_perm[i] of the states the layout orders (a relabelling of the spins: the subspace is invariant under it).
   * dnm_mat_create rewrites the operator into that labelling, so that the pair hops of an operator on a bond graph
   * (the kagome Heisenberg model of examples/scripts/kagome/run_kagome.py) fall inside the layout's fields wherever
   * the graph allows; vectors pass through it wherever they meet the reference order (dnm_vec_layout_copy,
   * _positions, _set_random).  Everything index-wise at this boundary -- rows of dnm_mat_get_diagonal, indices of
   * dnm_vec_layout_positions, files -- stays in the reference's order.  dnm_sc_choose_site_perm picks one. */
  const int8_t *site_perm;
} dnm_subspace;

/* get_dimension_* (bsubspace.pyx:144-162) -> Dim_* */
int dnm_subspace_dim(const dnm_subspace *s, int64_t *dim);
/* idx_to_state_* (bsubspace.pyx:164-184) -> I2S_*_array; out-of-range idx is an error */
int dnm_idx_to_state(const dnm_subspace *s, int64_t n, const int64_t *idxs, int64_t *states);
/* state_to_idx_* (bsubspace.pyx:186-206) -> S2I_*_array; -1 when not in the subspace */
int dnm_state_to_idx(const dnm_subspace *s, int64_t n, const int64_t *states, int64_t *idxs);

/* Site relabelling (dnm_subspace.site_perm) for an operator with the distinct masks `masks` on SpinConserve(L, .)
 * vectors in the (a, w) internal layout: the assignment of spins to the layout's three fields that leaves the fewest
 * pair hops between fields (host search, deterministic; the identity is kept on ties, so chains stay as they are).
 * fix_top != 0: spin L-1 keeps bit L-1 (what an XParity subspace on top needs).  counts (6 ints, may be NULL): hops
 * of the result inside Lo, inside W, inside T, between Lo-W, Lo-T, W-T.  No counterpart in the reference, whose
 * kernels gather every column (bpetsc_template_2.c:371-412). */
int dnm_sc_choose_site_perm(int L, int a, int w, int64_t nmasks, const int64_t *masks, int fix_top, int8_t *site_perm,
                            int32_t *counts);

/* ------------------------------------------------------------------ */
/* shell matrix -- bpetsc.pyx:78-147, bpetsc_impl.h:42-63             */
/* ------------------------------------------------------------------ */
typedef struct dnm_mat dnm_mat;   /* replaces PETSc Mat(MATSHELL) + shell_context (shell_context.h:12-27) */

/* flags for dnm_mat_create */
enum {
  DNM_MAT_DEFAULT      = 0,
  DNM_MAT_FORCE_GATHER = 1,   /* use only the generic row-gather kernel */
  DNM_MAT_USE_GLDS     = 2,   /* stage LDS tiles with global_load_lds DMA instead of through registers
                                 (measured slower on MI355X for this access pattern; kept for A/B runs) */
  DNM_MAT_AMIN_SHIFT   = 8,   /* flags bits 8..15: log2 of the contiguous run of a window tile (0: the planner's default);
                                 the transposed exchange asks for tiles [0, a) + [f, n) so that sub-pieces are contiguous */
  DNM_MAT_HOST_ONLY    = 4,   /* build the plan and its tables on the host only (no device needed;
                                 diagnostics and CPU tests) -- such a handle cannot multiply */
  DNM_MAT_REAL_PACKED  = 16   /* Real arithmetic for a real-symmetric operator (every matrix element real in the
                                 product basis: Heisenberg, XXZ, Ising, random-field chains ...) on a Full / Parity pair
                                 (one rank or 2^p ranks: the exchange is that of an operator on one index bit less; XParity on top allowed): the handle multiplies REAL vectors of the same dimension, stored two
                                 amplitudes to a complex128 element -- element j holds the amplitudes of indices 2j
                                 (real part) and 2j + 1 (imaginary part), so a vector is dim / 2 elements, 8 bytes per
                                 amplitude, and dnm_mat_sizes reports the halved sizes.  Solver-internal (eigsolve of a
                                 real-symmetric operator needs no complex arithmetic; the reference's PETSc build is
                                 complex throughout).  Also for a SpinConserve pair in the internal layout (chain
                                 operators and operators on bond graphs, XParity on one rank): one double per position, i.e.
                                 dnm_vec_layout_size / 2 complex128 elements (dnm_vec_layout_unpack_real).
                                 dnm_eigsolve on such a handle keeps every inner product real, and
                                 dnm_vec_unpack_real turns a packed vector into the complex128 vector the caller sees.
                                 dnm_mat_create fails (and the caller keeps the complex handle) when the operator has
                                 an imaginary matrix element. */
};

/* Row-block partition of the state vector over `nranks` devices, as PetscSplitOwnership splits it
 * (BuildGPUShell, bcuda_template_2.cu:24-27): dim / nranks rows each, the first dim % nranks ranks one more.
 * Two exchange schemes, chosen by dnm_mat_create (dnm_mat_exchange_plan reports no transfers for the second):
 *   - Full/Full or Parity/Parity on 2^p ranks with blocks of at least one tile: XOR-partner sub-blocks
 *     (dnm_mat_exchange_plan + dnm_mat_mult_local + dnm_mat_mult_remote), MatMult_CPU_Fast's scheme
 *     (bpetsc_template_2.c:787-879);
 *   - every other case -- SpinConserve, Explicit / Auto, projections between different subspaces, Full / Parity
 *     on any other rank count: rows in index order, each rank reads its columns through a window
 *     (dnm_mat_column_window + dnm_mat_mult_window), in place of the scatter-add of MatMult_CPU_General's MPI
 *     branch (bpetsc_template_2.c:413-504). */
typedef struct dnm_partition {
  int32_t rank;
  int32_t nranks;
} dnm_partition;

/* BuildMat(msc, subspaces, GPU_SHELL, xparity, &A)  (bpetsc_impl.h:42,
 * bpetsc.pyx:78-138): masks[nmasks] sorted unique, mask_offsets[nmasks+1],
 * signs[nterms], coeffs[nterms] complex128 interleaved.  part may be NULL
 * (single device).  The operator must be Hermitian in the reference's sense
 * (msc_tools.py:94-118): each term purely real or purely imaginary as
 * TERM_REAL(mask, sign) dictates (bpetsc_impl.h:34). */
int dnm_mat_create(int64_t nmasks, const int64_t *masks, const int64_t *mask_offsets,
                   const int64_t *signs, const double *coeffs,
                   const dnm_subspace *left, const dnm_subspace *right,
                   int xparity, int flags, const dnm_partition *part,
                   dnm_mat **out);
/* CheckConserves(msc, subspaces, xparity, &result)  (bpetsc.pyx:150-193,
 * bpetsc_template_2.c:990-1056): *result = 1 iff every column of the right
 * subspace is mapped into the left subspace (or onto a zero matrix element). */
int dnm_check_conserves(int64_t nmasks, const int64_t *masks, const int64_t *mask_offsets,
                        const int64_t *signs, const double *coeffs,
                        const dnm_subspace *left, const dnm_subspace *right,
                        int xparity, int *result, void *stream);
/* ReducedDensityMatrix(vec, sub_type, sub_data, keep_size, keep, triang, rtn_dim, rtn)
 * (bpetsc_impl.h:52-63, bpetsc_template_1.c:87-165, bpetsc.pyx:245-276): the density
 * matrix of the spins keep[0] < keep[1] < ... of the state x (device pointer, the
 * whole vector), all other spins traced out.  rho: device buffer of 4^keep_size
 * complex128, row-major, bit i of a row/column index = spin keep[i].
 * The kernel walks the 2^(L - keep_size) traced configurations of every kept one, whatever the dimension of the
 * subspace: a subspace of more than 40 spins is refused (before anything touches the device). */
int dnm_reduced_density_matrix(const void *x, const dnm_subspace *sub, int keep_size,
                               const int64_t *keep, void *rho, void *stream);
/* The same matrix block by block, for a state of fixed magnetisation: sub is SpinConserve(L, k) and x either the
 * whole state (xparity_sector = 0) or its XParity half of sector +-1 (the dim / 2 representatives; L = 2 k), in
 * reference order.  Block n couples the kept configurations with n set bits, max(0, k - (L - keep_size)) <= n <=
 * min(k, keep_size), in ascending order: it is rho[idx][:, idx] of the dense matrix, idx = the row indices of
 * popcount n.  keep_size <= 40 and every block below 2^31 rows.
 * dnm_rdm_sector_plan (host only, no device needed): the feasible blocks -- their n, rows and numbers of traced
 * configurations (arrays of min(k, keep_size) + 1 entries suffice; any may be null) -- and the scratch in bytes that
 * a call computing all of them at once takes.
 * dnm_rdm_sector_blocks: the blocks sel_n[0..nsel) in one launch sequence, block i into out_ptrs[i] (device,
 * rows x rows complex128, row-major).  Blocks are Hermitian to the last bit, with real diagonals. */
int dnm_rdm_sector_plan(const dnm_subspace *sub, int keep_size, const int64_t *keep, int xparity_sector,
                        int *nblocks, int32_t *n_of_block, int64_t *dim_of_block, int64_t *traced_of_block,
                        size_t *scratch_bytes_max);
int dnm_rdm_sector_blocks(const void *x, const dnm_subspace *sub, int keep_size, const int64_t *keep,
                          int xparity_sector, int nsel, const int32_t *sel_n, void *const *out_ptrs, void *stream);
/* Every <sigmaz_i> and <sigmaz_i sigmaz_j> of a state in one pass over it (no counterpart in the reference, whose users
 * call Operator.expectation once per site and per pair: one multiply and one temporary vector each).  With s_i(c) = +1
 * where bit i of the configuration c is clear and -1 where it is set, and s~(c) = (1, s_0, ..., s_{L-1}),
 *   M = sum_c |x_c|^2 s~(c) s~(c)^T      ((L + 1) x (L + 1) doubles, row-major, real symmetric):
 * M[0][0] = <x|x>, M[0][1+i] = <sigmaz_i>, M[1+i][1+j] = <sigmaz_i sigmaz_j>.  Sums are raw (nothing is normalised);
 * M is symmetric to the last bit, every diagonal entry equals M[0][0], and two calls return the same bits on any device.
 * x (device) holds the nrows amplitudes of the rows [row0, row0 + nrows) of sub, so that blocks of a partitioned state
 * and the XParity half of a state (the parent's descriptor, nrows = dim / 2: sigmaz_i sigmaz_j commutes with the global
 * flip, the sum over the representatives is <sigmaz_i sigmaz_j>) are summed by the caller.  Layout of x: vec_swizzle 0
 * is index order; the XOR swizzle of Full / Parity is read as it lies and acts on the block's own positions (nrows <=
 * 2^S or a multiple of 2^S, as for dnm_vec_swizzle_copy); the SpinConserve internal layout and a non-null site_perm are
 * refused -- the caller converts (dnm_vec_layout_copy).  L <= 63.  out: HOST, (L + 1)^2 doubles; the call synchronises
 * the stream like dnm_vec_dot.
 * dnm_zz_moments_plan (host only, no device needed): tile_rows = ceil((L + 1) / 16) rows of 16 x 16 tiles, the
 * workgroups of the sweep -- a function of nrows alone, never of the device -- and the bytes of their partial tiles,
 * nworkgroups * tile_rows (tile_rows + 1) / 2 * 256 * 8; any output may be null. */
int dnm_zz_moments_plan(const dnm_subspace *sub, int64_t nrows, int *tile_rows, int *nworkgroups,
                        size_t *scratch_bytes);
int dnm_zz_moments(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, double *out, void *stream);
/* Measurement in the computational basis: rows drawn from w_i = |x_i|^2 / <x|x> without the vector leaving the device
 * (no counterpart in the reference, whose users take State.to_numpy() and numpy.random.choice on the host).  x (device)
 * holds the nrows amplitudes of the rows [row0, row0 + nrows) of sub, as for dnm_zz_moments: vec_swizzle 0 is index
 * order, the XOR swizzle of Full / Parity is read as it lies and acts on the block's own positions, the SpinConserve
 * internal layout and a non-null site_perm are refused.  Rows are counted in index order and returned as indices,
 * never positions; the descriptor serves the checks alone, so an XParity half goes in under its parent's descriptor
 * with nrows = dim / 2.
 * The rows are cut into blocks of block_rows rows (a power of two; the last block may be ragged).  One pass gives the
 * block sums B_b of the weights; their inclusive prefix S_b, started from `before` (the weight of all rows in front of
 * this block: earlier ranks, earlier pieces), is a serial sum and therefore non-decreasing.  A target t >= 0 goes to
 * the smallest b with S_b > t and in it to the smallest row whose in-block prefix (serial chunks of 16 rows on serially
 * summed offsets: non-decreasing too, and flat across rows of weight zero) exceeds t - S_{b-1}; where rounding leaves
 * no such row, to the block's last row of non-zero weight.  A row of weight exactly zero is never returned.  All sums
 * have fixed shapes and use no atomics: two calls return the same bits, on any device.  Cost: one pass over the rows
 * and one block of rows per shot; scratch: the block sums, and 16 bytes per shot.
 * dnm_born_plan (host only, no device needed): block_rows, nblocks = ceil(nrows / block_rows) and the bytes of the
 * block sums -- functions of nrows alone; any output may be null.
 * dnm_born_scan (host only): the scan as the calls below make it, scan[b] = before + sums[0] + ... + sums[b] (in place
 * allowed).  dnm_born_uniforms (host only): u and the flip bit of the shots shot0 .. shot0 + nshots - 1 of
 * dnm_born_sample (flip_host may be null).
 * dnm_born_block_sums: the block sums and their scan from `before` to the HOST (nblocks doubles each, either may be
 * null): a caller of a partitioned state learns each block's weight from it.
 * dnm_born_search: rows_host[s] (HOST) = row0 + the local row of targets_host[s] (HOST) for the targets in [before,
 * before + the weight of these rows), -1 for every other target -- they belong to other blocks.  final_block != 0 says
 * that no rows follow these: targets at or beyond the total (u W can round up to W) then go to the last row of non-zero
 * weight (-1 when these rows carry no weight at all).
 * dnm_born_sample: the whole state in one block (before = 0, final).  Shot s draws Philox-4x32-10 with the counter
 * words (lo32(shot0 + s), hi32(shot0 + s), 0x13198A2E, 0x03707344) under the key seed -- the constant words differ from
 * those of dnm_vec_set_random, whose bits set |x_i| -- and output words c0..c3: u = (((c0 << 32) | c1) >> 11) 2^-53,
 * target t = u W in one rounding with W the last scan value, flip_host[s] (may be null) = c2 & 1, the coin an XParity
 * state's caller uses between a representative and its global flip.  Chunks of shots (shot0) return what one call
 * returns.  Every row is -1 when the state has no weight.
 * These calls synchronise the stream like dnm_vec_dot; scratch comes from the library's workspace
 * (dnm_release_workspace). */
int dnm_born_plan(const dnm_subspace *sub, int64_t nrows, int64_t *block_rows, int64_t *nblocks, size_t *scratch_bytes);
int dnm_born_scan(const double *sums_host, int64_t n, double before, double *scan_host);
int dnm_born_uniforms(uint64_t seed, int64_t shot0, int64_t nshots, double *u_host, uint8_t *flip_host);
int dnm_born_block_sums(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, double before,
                        double *sums_host, double *scan_host, void *stream);
int dnm_born_search(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, double before, int final_block,
                    int64_t nshots, const double *targets_host, int64_t *rows_host, void *stream);
int dnm_born_sample(const void *x, const dnm_subspace *sub, int64_t row0, int64_t nrows, uint64_t seed, int64_t shot0,
                    int64_t nshots, int64_t *rows_host, uint8_t *flip_host, void *stream);
/* The sums behind the participation (basis Renyi) entropies of a vector of n elements in one pass, w_i = |x_i|^2:
 * out (HOST, nq + 4 doubles) = P_0 .. P_{nq-1}, W, H, wmax, nnz with P_k = sum w^q_k for the nq <= 8 exponents q_host
 * (finite, > 0), W = sum w, H = sum of w ln w over the w > 0, wmax = max w and nnz = the number of w > 0.  Exponents 2,
 * 3 and 4 are computed by multiplication (exact on integer weights), every other one by pow.  The order of the elements
 * does not matter: any layout whose padding is zeros goes in as it lies, the SpinConserve internal layout included
 * (n = dnm_vec_layout_size).  Fixed reduction shapes, no atomics; the workgroups are a function of n alone.
 * Synchronises the stream. */
int dnm_vec_power_sums(const void *x, int64_t n, int nq, const double *q_host, double *out_host, void *stream);
/* Every <sigma+_i sigma-_j> of a state in one pass over it -- the transverse part <sigmax_i sigmax_j + sigmay_i sigmay_j>
 * of the spin correlations, where the call above gives the sigmaz part (no counterpart in the reference, whose users
 * call Operator.expectation once per pair).  sigma_minus(j) = sigmax_j - i sigmay_j sets bit j of a configuration with
 * matrix element 2, sigma_plus is its adjoint.  With A[r][j] = x(r ^ e_j) on the configurations r whose bit j is set
 * and 0 elsewhere,
 *   P[i][j] = sum_r conj(A[r][i]) A[r][j]      (L x L complex128, row-major, Hermitian),
 * so that <x|sigma_plus(i) sigma_minus(j)|x> = 4 P[i][j] -- an exact scaling -- and P[i][i] = the weight of the
 * configurations whose bit i is clear, (M[0][0] + M[0][1+i]) / 2 of dnm_zz_moments.  Sums are raw (nothing is
 * normalised).  P equals its conjugate transpose to the last bit, its diagonal is real, and two calls return the same
 * bits on any device (no atomics; the number of workgroups follows from the subspace alone).
 * x (device) is the WHOLE state on one device.  Layouts: Full / Parity in index order (vec_swizzle 0) or XOR-swizzled,
 * read as it lies; SpinConserve(L, k) in reference order -- the rows r are then the configurations with k + 1 set bits,
 * and k = L gives P = 0 without a launch.  Refused, each before any device call: Explicit subspaces, the SpinConserve
 * internal layout and a non-null site_perm (the caller converts: dnm_vec_layout_copy), L > 64, null pointers.
 * out: HOST, L * L * 2 doubles (re, im); the call synchronises the stream like dnm_vec_dot.  Scratch comes from the
 * library's workspace (dnm_release_workspace).
 * dnm_pm_moments_plan (host only, no device needed): tile_rows = ceil(L / 16) rows of 16 x 16 tiles (NB), the panel
 * of 2^panel_rows_log2 rows of A a workgroup stages in LDS, the workgroups of the sweep, the bytes of LDS of a launch
 * (at least the panel, 2^panel_rows_log2 * 16 NB * 16, at most 160 KB) and the bytes of the partial tiles,
 * nworkgroups * (NB (NB + 1) / 2 + NB^2) * 256 * 8; any output may be null.
 * dnm_pm_partner_indices (host only, SpinConserve only): for each of the n rows -- indices in the sector with k + 1 set
 * bits -- out[row * L + j] = the index in sector k of the row's configuration with bit j cleared, or -1 where bit j
 * is clear.  The arithmetic is the kernel's (csrc/pm_rank.h). */
int dnm_pm_moments_plan(const dnm_subspace *sub, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                        size_t *lds_bytes, size_t *scratch_bytes);
int dnm_pm_moments(const void *x, const dnm_subspace *sub, double *out, void *stream);
int dnm_pm_partner_indices(const dnm_subspace *sub, int64_t n, const int64_t *rows, int64_t *out);
/* Every bond-swap (dimer-dimer) correlator of a state in one pass over it (no counterpart in the reference, whose users
 * call Operator.expectation once per pair of bonds).  sigma_a . sigma_b = 2 P_ab - 1 with P_ab the exchange of the spins
 * a and b.  For nbonds bonds (a_m, b_m) = (bonds[2 m], bonds[2 m + 1]), a_m != b_m -- a bond may repeat, bonds may
 * share sites -- and the operand matrix over the rows r of the subspace
 *   A[r][0] = x(r),   A[r][1 + m] = x(r with bits a_m and b_m exchanged),
 *   G = A^H A      ((nbonds + 1) x (nbonds + 1) complex128, row-major, Hermitian):
 * G[0][0] = <x|x>, G[0][1 + m] = <P_m>, G[1 + m][1 + m'] = <P_m P_m'>.  Sums are raw (nothing is normalised).  G equals
 * its conjugate transpose to the last bit, its diagonal is real, and two calls return the same bits on any device (no
 * atomics; the number of workgroups follows from the number of rows alone).
 * x (device) is the WHOLE state on one device.  Layouts: Full / Parity in index order or XOR-swizzled, read as it lies;
 * SpinConserve in reference order.  xparity_sector = +-1: x holds the dim / 2 amplitudes of the representatives of that
 * XParity sector and sub is the parent's descriptor (the convention of dnm_rdm_sector_blocks); a swap commutes with the
 * global flip, so the sum over the representatives -- with the partner of a row taken as the sector's sign times the
 * amplitude of its complement where the swap sets bit L - 1 -- is the expectation value in the sector.
 * Refused, each before any device call: null pointers, Explicit subspaces, an unknown subspace type, L outside [1, 64],
 * nbonds outside [1, 63], a site outside [0, L) or a_m == b_m, a non-null site_perm, the SpinConserve internal layout
 * (the caller converts: dnm_vec_layout_copy), a Full / Parity swizzle shift outside {0} and [5, 24], xparity_sector
 * other than 0, +1, -1, and an XParity parent that cannot carry the flip (Parity with odd L, SpinConserve with L != 2 k).
 * out: HOST, (nbonds + 1)^2 * 2 doubles (re, im); the call synchronises the stream like dnm_vec_dot.  Scratch comes
 * from the library's workspace (dnm_release_workspace).
 * dnm_swap_moments_plan (host only, no device needed): tile_rows = ceil((nbonds + 1) / 16) rows of 16 x 16 tiles (NB),
 * the panel of 2^panel_rows_log2 rows of A a workgroup stages in LDS, the workgroups of the sweep -- ceil(rows / 512),
 * at most 1024 -- the bytes of LDS of a launch (at most 152 KB) and the bytes of the partial tiles, nworkgroups *
 * (NB (NB + 1) / 2 + NB^2) * 256 * 8; any output may be null.
 * dnm_swap_partner_indices (host only): for each of the n rows (indices into x) and each bond, idx[row * nbonds + m] =
 * the reference-order index into x of the amplitude A[row][1 + m] is taken from and sign[row * nbonds + m] its factor:
 * +1, or the sector where the complement's amplitude was taken.  The arithmetic is the kernel's (csrc/swap_rank.h). */
int dnm_swap_moments_plan(const dnm_subspace *sub, int nbonds, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                          size_t *lds_bytes, size_t *scratch_bytes);
int dnm_swap_moments(const void *x, const dnm_subspace *sub, int xparity_sector, int nbonds, const int32_t *bonds,
                     double *out, void *stream);
int dnm_swap_partner_indices(const dnm_subspace *sub, int xparity_sector, int nbonds, const int32_t *bonds, int64_t n,
                             const int64_t *rows, int64_t *idx, int8_t *sign);
/* Every scalar-chirality correlator of a list of triangles in one pass over the state (no counterpart in the reference,
 * whose users call Operator.expectation once per pair of triangles).  For spin 1/2, sigma_a . (sigma_b x sigma_c) =
 * 2i (C - C^H) with C = P_ab P_bc (P_bc acts first) the rotation of the three spins.  For ncycles oriented triples
 * (a_m, b_m, c_m) = (cycles[3 m], cycles[3 m + 1], cycles[3 m + 2]) of pairwise distinct sites -- a triple may repeat,
 * triples may share sites -- and the operand matrix over the rows r of the subspace
 *   A[r][0] = x(r),   A[r][1 + m] = x(r'),  bit a of r' = bit b of r, bit b of r' = bit c of r, bit c of r' = bit a of r,
 *   G = A^H A      ((ncycles + 1) x (ncycles + 1) complex128, row-major, Hermitian):
 * column 1 + m is C_m x, G[0][0] = <x|x>, G[0][1 + m] = <C_m>, G[1 + m][1 + m'] = <C_m^H C_m'>.  The opposite rotation of
 * (a, b, c) is the rotation of (a, c, b): one triple is one column and the caller lists both senses.  Sums are raw
 * (nothing is normalised).  G equals its conjugate transpose to the last bit, its diagonal is real, and two calls return
 * the same bits on any device (no atomics; the number of workgroups follows from the number of rows alone).
 * x (device) is the WHOLE state on one device.  Layouts: Full / Parity in index order or XOR-swizzled, read as it lies;
 * SpinConserve in reference order.  xparity_sector = +-1: x holds the dim / 2 amplitudes of the representatives of that
 * XParity sector and sub is the parent's descriptor (the convention of dnm_swap_moments); a permutation of sites
 * commutes with the global flip, so the sum over the representatives -- with the partner of a row taken as the sector's
 * sign times the amplitude of its complement where the rotation sets bit L - 1 -- is the expectation value in the sector.
 * Refused, each before any device call: null pointers, Explicit subspaces, an unknown subspace type, L outside [1, 64],
 * ncycles outside [1, 63], a site outside [0, L) or two equal sites in a triple, a non-null site_perm, the SpinConserve
 * internal layout (the caller converts: dnm_vec_layout_copy), a Full / Parity swizzle shift outside {0} and [5, 24],
 * xparity_sector other than 0, +1, -1, and an XParity parent that cannot carry the flip (Parity with odd L, SpinConserve
 * with L != 2 k).
 * out: HOST, (ncycles + 1)^2 * 2 doubles (re, im); the call synchronises the stream like dnm_vec_dot.  Scratch comes
 * from the library's workspace (dnm_release_workspace).
 * dnm_cyc_moments_plan (host only, no device needed): the plan of dnm_swap_moments_plan for the same number of columns
 * -- tile_rows = ceil((ncycles + 1) / 16) rows of 16 x 16 tiles (NB), the panel of 2^panel_rows_log2 rows of A a
 * workgroup stages in LDS, the workgroups of the sweep -- ceil(rows / 512), at most 1024 -- the bytes of LDS of a launch
 * (at most 152 KB) and the bytes of the partial tiles, nworkgroups * (NB (NB + 1) / 2 + NB^2) * 256 * 8; any output may
 * be null.
 * dnm_cyc_partner_indices (host only): for each of the n rows (indices into x) and each triple, idx[row * ncycles + m] =
 * the reference-order index into x of the amplitude A[row][1 + m] is taken from and sign[row * ncycles + m] its factor:
 * +1, or the sector where the complement's amplitude was taken.  The arithmetic is the kernel's (csrc/cyc_rank.h,
 * csrc/swap_rank.h). */
int dnm_cyc_moments_plan(const dnm_subspace *sub, int ncycles, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                         size_t *lds_bytes, size_t *scratch_bytes);
int dnm_cyc_moments(const void *x, const dnm_subspace *sub, int xparity_sector, int ncycles, const int32_t *cycles,
                    double *out, void *stream);
int dnm_cyc_partner_indices(const dnm_subspace *sub, int xparity_sector, int ncycles, const int32_t *cycles, int64_t n,
                            const int64_t *rows, int64_t *idx, int8_t *sign);
/* Every two-spin Pauli correlator of a state without a U(1) symmetry in one pass over it (no counterpart in the
 * reference, whose users call Operator.expectation once per pair).  A single-site Pauli applied to x is one partner
 * amplitude times a sign: with s_j(r) = (-1)^(bit j of r), (sigmax_j x)(r) = x(r ^ e_j), (sigmaz_j x)(r) = s_j(r) x(r) and
 * (sigmay_j x)(r) = -i s_j(r) x(r ^ e_j).  For ncols columns (site j_c, kind_c) = (cols[2 c], cols[2 c + 1]) -- kind 1:
 * flip (sigma-x), 2: flip and sign (sigma-y up to the phase -i, which the caller applies), 3: sign (sigma-z); a column
 * may repeat, columns may share a site -- and the operand matrix over the rows q of the vector
 *   A[q][0] = x[q],   A[q][1 + c] = (-1)^(g_c * bit j_c of r_c(q)) x[q ^ m_c]     (f_c: kind 1 or 2, g_c: kind 2 or 3)
 *   G = A^H A      ((ncols + 1) x (ncols + 1) complex128, row-major, Hermitian):
 * G[0][0] = <x|x> and, up to the phases, G[0][1 + c] = <sigma_c> and G[1 + c][1 + c'] = <sigma_c sigma_c'>.  Full: r_c(q) =
 * q and m_c = f_c << j_c.  Parity(space): the index is the configuration without site 0, m_c = (f_c << j_c) >> 1 (a flip
 * of site 0 pairs a row with the amplitude at its own index); a column that does not flip, column 0 among them, reads
 * the signs of the row's own configuration (q << 1) | (par(q) ^ space), a flipping column those of the opposite sector's,
 * (q << 1) | (par(q) ^ space ^ 1); the entries of G between a flipping and a non-flipping column vanish by symmetry and
 * are exact zeros.  Sums are raw (nothing is normalised).  G equals its conjugate transpose to the last bit, its
 * diagonal is real, and two calls return the same bits on any device (no atomics; the number of workgroups follows
 * from the number of rows alone).
 * x (device) is the WHOLE state on one device, in index order or XOR-swizzled, read as it lies.
 * Refused, each before any device call: null pointers, Explicit subspaces, SpinConserve subspaces (a flip leaves the
 * sector: dnm_zz_moments and dnm_pm_moments serve them), an unknown subspace type, L outside [1, 64] or more than 62
 * index bits, a non-null site_perm, a swizzle shift outside {0} and [5, 24], a Parity space other than 0 or 1, ncols
 * outside [1, 63], a site outside [0, L), a kind outside {1, 2, 3}.
 * out: HOST, (ncols + 1)^2 * 2 doubles (re, im); the call synchronises the stream like dnm_vec_dot.  Scratch comes from
 * the library's workspace (dnm_release_workspace).
 * dnm_pauli_moments_plan (host only, no device needed): the plan of dnm_swap_moments_plan for the same number of columns
 * (a rule inherited from that pass, not measured for this one) -- tile_rows = ceil((ncols + 1) / 16) rows of 16 x 16
 * tiles (NB), the panel of 2^panel_rows_log2 rows of A a workgroup stages in LDS, the workgroups of the sweep --
 * ceil(rows / 512), at most 1024 -- the bytes of LDS of a launch (at most 152 KB) and the bytes of the partial tiles,
 * nworkgroups * (NB (NB + 1) / 2 + NB^2) * 256 * 8; any output may be null.
 * dnm_pauli_partner_indices (host only): for each of the n rows (reference-order indices into x; one out of range is
 * refused) and each column, idx[row * ncols + c] = the reference-order index into x of the amplitude A[row][1 + c] is
 * taken from and sign[row * ncols + c] its factor, +1 or -1.  The arithmetic is the kernel's (csrc/pauli_cols.h). */
int dnm_pauli_moments_plan(const dnm_subspace *sub, int ncols, int *tile_rows, int *panel_rows_log2, int *nworkgroups,
                           size_t *lds_bytes, size_t *scratch_bytes);
int dnm_pauli_moments(const void *x, const dnm_subspace *sub, int ncols, const int32_t *cols, double *out,
                      void *stream);
int dnm_pauli_partner_indices(const dnm_subspace *sub, int ncols, const int32_t *cols, int64_t n, const int64_t *rows,
                              int64_t *idx, int8_t *sign);
/* Site permutations of a state -- lattice translations, rotations, mirrors -- in one pass over it (no counterpart in the
 * reference, whose users take the state to the host, gather with numpy and copy it back).  A site permutation is an
 * int32 array pi of length L, a bijection of [0, L).  P_pi moves the spin at site i to site pi(i): P_pi |c> = |c'> with
 * c'_{pi(i)} = c_i, so (P_pi x)(c') = x(c) where the source configuration c has bit i equal to bit pi(i) of c'; hence
 * P_pi sigma^a_i P_pi^H = sigma^a_{pi(i)}.  The rotation of dnm_cyc_moments for the triple (a, b, c) is pi(a) = b, pi(b)
 * = c, pi(c) = a, all else fixed.  perms holds nperm such arrays, row g at perms + g * L.  With p_g(r) the index into the
 * vector of the source of row r under permutation g and s_g(r) its factor:
 *   dnm_perm_apply   y[r] = (accumulate ? y[r] : 0) + sum_g (coef[2 g] + i coef[2 g + 1]) s_g(r) x[p_g(r)]
 *   dnm_perm_dots    out[g] = sum_r conj(phi[r]) s_g(r) psi[p_g(r)] = <phi|P_g|psi>
 * nperm = 1 with coef = (1, 0) is the plain permutation, and then y holds the bits of x; with characters for
 * coefficients the sum is a projector onto an irreducible representation.  Sums are raw (nothing is normalised).
 * dnm_perm_dots uses no atomics and the number of workgroups follows from the number of rows alone: two calls return the
 * same bits on any device.
 * x, y, phi, psi (device) are WHOLE states on one device, all in one layout.  Layouts: Full / Parity in index order or
 * XOR-swizzled, read and written as they lie; SpinConserve in reference order.  A permutation keeps the number of set
 * bits and the parity and commutes with the global flip.  xparity_sector = +-1: the vectors hold the dim / 2 amplitudes
 * of the representatives (bit L - 1 clear) of that XParity sector and sub is the parent's descriptor (the convention of
 * dnm_swap_moments); a source configuration whose bit L - 1 is set is the sector's sign times the amplitude of its
 * complement, sums run over the representatives with no factor 2, and P_pi x lies in the same sector.
 * Refused, each before any device call: null pointers, nperm outside [1, 64], a row of perms that is not a bijection of
 * [0, L), Explicit subspaces, an unknown subspace type, L outside [1, 64] or more than 62 index bits on Full / Parity, a
 * non-null site_perm, the SpinConserve internal layout (the caller converts: dnm_vec_layout_copy), a Full / Parity
 * swizzle shift outside {0} and [5, 24], xparity_sector other than 0, +1, -1, an XParity parent that cannot carry the
 * flip (Parity with odd L, SpinConserve with L != 2 k), and x == y: the pass gathers.
 * coef: HOST, 2 nperm doubles.  out: HOST, 2 nperm doubles (re, im).  Both calls synchronise the stream like
 * dnm_vec_dot.  Scratch comes from the library's workspace (dnm_release_workspace).
 * dnm_perm_plan (host only, no device needed): the workgroups of a launch -- ceil(rows / 1024), at most 4096, at least
 * one, rows those of sub itself -- the bytes of LDS of a launch (the binomials of a SpinConserve subspace and 68 bytes
 * per permutation) and the bytes of scratch of dnm_perm_dots; any output may be null.
 * dnm_perm_partner_indices (host only): for each of the n rows -- positions in the vector as it lies, which are the
 * reference-order indices unless a Full / Parity descriptor carries a swizzle -- and each permutation, idx[row * nperm +
 * g] = the position p_g(row) of the source amplitude and sign[row * nperm + g] = s_g(row): +1, or the sector where the
 * complement's amplitude is taken.  The arithmetic is the kernels' (csrc/perm_rank.h). */
int dnm_perm_plan(const dnm_subspace *sub, int nperm, int *nworkgroups, size_t *lds_bytes, size_t *scratch_bytes);
int dnm_perm_partner_indices(const dnm_subspace *sub, int xparity_sector, int nperm, const int32_t *perms, int64_t n,
                             const int64_t *rows, int64_t *idx, int8_t *sign);
int dnm_perm_apply(const void *x, void *y, const dnm_subspace *sub, int xparity_sector, int nperm, const int32_t *perms,
                   const double *coef, int accumulate, void *stream);
int dnm_perm_dots(const void *phi, const void *psi, const dnm_subspace *sub, int xparity_sector, int nperm,
                  const int32_t *perms, double *out, void *stream);
/* A state moved from one subspace to another of the same L spins on the device -- embed, restrict, into and out of an
 * XParity sector -- and its weight per sector (no counterpart in the reference, whose users take the state to the host;
 * its XParity.convert_state does so too and knows only a sector and its parent).  The result of the map is the
 * orthogonal projection, onto the span of the target subspace, of the source state seen as a vector of the whole 2^L
 * space: an embedding when the source's configurations lie in the target's, a restriction the other way round.  Nothing
 * is normalised: the squared norm of the result is the weight of the state inside the target.  With psi(c) the amplitude
 * of configuration c in the source -- x[i_src(c)], or 0 when c is not in the source; for a source on the XParity sector
 * s over a parent, kappa x[i(c)] for c in the parent with bit L - 1 clear and kappa s x[i(cbar)] with it set, cbar = c
 * with all L spins flipped, kappa the double 0.70710678118654752440 -- and c the configuration of the target row r (the
 * representative, bit L - 1 clear, when the target is an XParity sector t):
 *   plain     -> plain       y[r] = x[i_src(c)] or 0                       the bits of x are copied
 *   XParity s -> plain       y[r] = x[.] * kappa, the sign s on the flipped half, or 0     one multiply per component
 *   plain     -> XParity t   y[r] = (psi(c) + t psi(cbar)) * kappa         one add, then one multiply per component
 *   XParity s -> XParity t   y[r] = x[i(c)] if s == t and c lies in the source's parent, else 0     the bits are copied
 * src_sector / dst_sector = +-1: that side's vector holds the dim / 2 amplitudes of the representatives of that XParity
 * sector and the descriptor is the parent's (the convention of dnm_swap_moments); 0: the subspace itself.  Full, Parity,
 * SpinConserve and Explicit on either side; an Explicit side is searched in its sorted or re-mapped table.
 * x, y (device) are WHOLE states on one device, distinct (the pass gathers).  Layouts: Full / Parity in index order or
 * XOR-swizzled, read and written as they lie, each side by its own descriptor's shift; SpinConserve in reference order
 * (the caller converts: dnm_vec_layout_copy); Explicit in list order.  One target-driven kernel, no atomics; rows whose
 * configuration is not in the source are written as zeros by the same store.  dnm_subspace_map_apply synchronises the
 * stream.
 * Refused, each before any device call: null pointers, x == y, different L on the two sides, L outside [1, 63] or more
 * than 62 index bits, an unknown subspace type, a sector other than 0, +1, -1, an XParity parent that cannot carry the
 * flip (Parity with odd L, SpinConserve with L != 2 k, Explicit with odd dimension or whose rows dim / 2 - 1 and dim / 2
 * do not have bit L - 1 clear and set respectively), a non-null site_perm, the SpinConserve internal layout, a swizzle
 * shift outside {0} and [5, 24].
 * dnm_subspace_map_plan (host only, no device needed): the elements of the two vectors, the adjacent target rows a
 * thread owns (4 for a SpinConserve target, which it unranks once and steps through; 1 otherwise), the workgroups of
 * the launch -- ceil(target rows / 1024), at most 4096, at least one -- and the bytes of LDS of a launch (the binomials
 * of the SpinConserve sides); any output may be null.
 * dnm_subspace_map_indices (host only): for each of the n target positions rows[i] (in the vector as it lies), the
 * positions idx[2 i], idx[2 i + 1] in the source vector (as it lies) of the at most two amplitudes that enter, -1 for a
 * missing one, their signs sign[2 i], sign[2 i + 1] (0 for a missing one) and the one scale of the call, 1.0 or kappa:
 * y[r] = scale * sum sign * x[idx].  The arithmetic is the kernel's (csrc/submap_rank.h).
 * dnm_sector_weights: popcount_out[k] (HOST, L + 1 doubles) = sum of |psi(c)|^2 over the configurations with k set bits
 * -- the counting statistics of the magnetisation, and the squared norm a map to SpinConserve(L, k) keeps; on an XParity
 * state a representative row adds |x|^2 / 2 to bin k and as much to bin L - k.  flip_out (HOST, 2 doubles, may be null) =
 * (F+, F-), F+- = sum over the pairs {c, cbar} of |psi(c) +- psi(cbar)|^2 / 2, the squared norm each XParity sector
 * keeps: the pairs are the rows i and dim - 1 - i of Full, of Parity with even L and of SpinConserve(L, L / 2); on an
 * XParity state the sector's entry is the squared norm and the other 0; a non-null flip_out is refused on Explicit and
 * on subspaces that cannot carry the flip.  One streaming pass, no floating-point atomics, and the number of workgroups
 * follows from the rows alone: two calls return the same bits.  Layouts and refusals as for the map; the call
 * synchronises the stream like dnm_vec_dot, scratch comes from the library's workspace (dnm_release_workspace).
 * dnm_sector_weights_plan (host only): the workgroups -- ceil(rows / 1024), rows counted in pairs where the flip sums
 * come with the bins, at most 2048 -- and the bytes of scratch; any output may be null. */
int dnm_subspace_map_plan(const dnm_subspace *src, int src_sector, const dnm_subspace *dst, int dst_sector,
                          int64_t *src_rows, int64_t *dst_rows, int *run, int *nworkgroups, size_t *lds_bytes);
int dnm_subspace_map_indices(const dnm_subspace *src, int src_sector, const dnm_subspace *dst, int dst_sector,
                             int64_t n, const int64_t *rows, int64_t *idx, int8_t *sign, double *scale);
int dnm_subspace_map_apply(const void *x, const dnm_subspace *src, int src_sector, void *y, const dnm_subspace *dst,
                           int dst_sector, void *stream);
int dnm_sector_weights_plan(const dnm_subspace *sub, int xparity_sector, int *nworkgroups, size_t *scratch_bytes);
int dnm_sector_weights(const void *x, const dnm_subspace *sub, int xparity_sector, double *popcount_out,
                       double *flip_out, void *stream);
/* A product of single-site operators on a state, U = (x)_j M_j with M_j any 2 x 2 complex matrix on spin j -- global and
 * per-site rotations, pulses, a change of the measurement basis (no counterpart in the reference, whose users evolve
 * under a field or take the state to the host).  With spin j = index bit j,
 *   y(c') = sum_c prod_j M_j[c'_j][c_j] x(c).
 * mats_host: HOST, L matrices of 8 doubles, row-major, M[0][0], M[0][1], M[1][0], M[1][1] as (re, im) each; nothing
 * requires them to be unitary.  x, y (device) are WHOLE Full-space states on one device, in index order or XOR-swizzled,
 * read and written as they lie (the swizzle leaves the 4 low index bits alone, so 256-byte runs survive).  x == y is
 * allowed: a tile is read whole before it is written.
 * Sites are classed by bitwise comparison: the identity is skipped (site_pass -1); a diagonal matrix (M[0][1] = M[1][0] =
 * 0) is a factor per row in the first pass and needs no tile bit (-2); every other site is general and belongs to one
 * pass (site_pass = its index).  A pass stages tiles of tile_bits index bits in LDS -- the 4 low bits and tile_bits - 4
 * others, chosen freely -- applies the butterflies of its sites and writes the tile back: every amplitude is read once and
 * written once per pass.  General sites below bit 4 go into pass 0, the n_hi others fill the passes in ascending order:
 * npasses = max(1, ceil(n_hi / (tile_bits - 4))); with L < tile_bits the tile is the whole vector.  All-identity input
 * copies x to y, or returns at once when x == y.  No atomics, the grid follows from L and the plan alone, every index
 * is 64-bit: two calls return the same bits.  The calls are asynchronous on the stream.
 * Refused, each before any device call: null pointers, a subspace other than Full, a non-null site_perm, L outside
 * [1, 62], a swizzle shift outside {0} and [5, 24], a matrix entry that is not finite.
 * Cost: one read and one write of the vector per pass.
 * dnm_site_ops_plan (host only, no device needed): tile_bits, the passes, site_pass (L entries), the workgroups of a
 * pass -- min(2^(L - tile_bits), 2^16), at least one -- and the bytes of LDS of a launch, 16 << min(tile_bits, L); any
 * output may be null. */
int dnm_site_ops_plan(const dnm_subspace *sub, const double *mats_host, int *tile_bits, int *npasses, int8_t *site_pass,
                      int *nworkgroups, size_t *lds_bytes);
int dnm_site_ops_apply(const void *x, void *y, const dnm_subspace *sub, const double *mats_host, void *stream);
/* The Gram matrix of many vectors in one pass over them (no counterpart in the reference, whose users take the overlaps
 * of a set of eigenvectors one State.dot at a time): for 1 <= nvec <= 64 device vectors of n complex128 elements each
 *   G[a][b] = sum_r conj(x_a[r]) x_b[r]      (nvec x nvec complex128, row-major, Hermitian),
 * conjugate-linear in the first index, nothing normalised.  With the images O x_n among the vectors the off-diagonal
 * block of G holds the matrix elements <m|O|n>.  The vectors are separate allocations at any 16-byte-aligned addresses;
 * a pointer may appear more than once.  The sum is elementwise, so any layout serves as long as all vectors share it
 * and its padding is zero.  G equals its conjugate transpose to the last bit, its diagonal is real, and two calls return
 * the same bits on any device (no atomics; the number of workgroups follows from (nvec, n) alone).
 * xs: HOST array of nvec device pointers.  Refused, each before any device call: nvec outside [1, 64], n < 0, null xs
 * or out, a null element of xs when n > 0, an address that is not 16-byte aligned.  n == 0 returns a zero matrix
 * without a launch.
 * out: HOST, nvec^2 * 2 doubles (re, im); the call synchronises the stream like dnm_vec_dot.  Scratch comes from the
 * library's workspace (dnm_release_workspace).
 * dnm_vec_gram_plan (host only, no device needed): tile_rows = ceil(nvec / 16) rows of 16 x 16 tiles (NB), the panel of
 * 2^panel_rows_log2 rows a workgroup stages in LDS (this sweep's own rule: 2^7 at one and two tile rows, 2^6 at three
 * and four, so that a wavefront holds its part of the next panel in registers while it multiplies), the workgroups of
 * the sweep -- ceil(n / 512), at most 1024, at least one -- the bytes of LDS of a launch, (16 NB + 1) * 16 <<
 * panel_rows_log2, and the bytes of the partial tiles, nworkgroups * (NB (NB + 1) / 2 + NB^2) * 256 * 8; any output may
 * be null. */
int dnm_vec_gram_plan(int nvec, int64_t n, int *tile_rows, int *panel_rows_log2, int *nworkgroups, size_t *lds_bytes,
                      size_t *scratch_bytes);
int dnm_vec_gram(const void *const *xs, int nvec, int64_t n, double *out, void *stream);
/* MATOP_DESTROY -> MatDestroyCtx_GPU (bcuda_template_2.cu:110-139) */
int dnm_mat_destroy(dnm_mat *A);
/* MatGetSize / MatGetLocalSize */
int dnm_mat_sizes(const dnm_mat *A, int64_t *M, int64_t *N, int64_t *m_local, int64_t *n_local);
/* PrecomputeDiagonal(A) (bpetsc.pyx:141-147, bcuda_template_1.cu:4-66).  The
 * tiled Full/Parity kernels evaluate the diagonal on the fly and ignore the
 * cache; the generic kernel uses it exactly as the reference does.  An error on a
 * handle whose left and right descriptors name different subspaces, equal dimensions or
 * not (SpinConserve(L, k) / SpinConserve(L, L - k), two Explicit lists of one length). */
int dnm_mat_precompute_diagonal(dnm_mat *A, void *stream);
/* copies the cached diagonal (double[m_local]) to the host; error if absent */
int dnm_mat_get_diagonal(dnm_mat *A, double *diag_host, void *stream);
/* The exponential of a diagonal operator on a state, exact in one streaming pass (no counterpart in the reference, whose
 * users call evolve):
 *   y[p] = exp((s_re + i s_im) d_r) x[p],
 * d_r the handle's diagonal at row r and p the position of r in the layout the handle multiplies in: a swizzled Full /
 * Parity vector is indexed by position and the cached diagonal by row, in the SpinConserve internal layout the cache
 * lies as the vectors do; Explicit and XParity handles work as far as dnm_mat_precompute_diagonal does, which the call
 * runs itself when the handle has no cache.  exp and sincos in fp64.  Where x[p] is exactly 0, y[p] is 0, whatever exp
 * gives for that row (padding, an overflowing exp(s_re d)); s = 0 copies x bit for bit.  x == y is allowed.
 * Refused: null pointers, a host-only handle, a factor that is not finite, a handle with a non-zero mask ("operator is
 * not diagonal"), a real-packed handle, more than one rank, different subspaces on the two sides.
 * Cost: one read of x, 8 bytes per row of the cache and one write.  Asynchronous on the stream. */
int dnm_mat_expm_diagonal(dnm_mat *A, const void *x, void *y, double s_re, double s_im, void *stream);
/* MATOP_MULT -> MatMult_GPU (bcuda_template_2.cu:141-198): y = A x, y overwritten.
 * Single device (or a partition whose operator has no off-rank masks). */
int dnm_mat_mult(dnm_mat *A, const void *x, void *y, void *stream);
/* MATOP_NORM, NORM_INFINITY only (bcuda_template_2.cu:275-329); cached in the
 * handle like ctx->nrm.  With a partition this is the LOCAL max; the caller
 * max-reduces over ranks (MPIU_Allreduce(MAX), bpetsc_template_2.c:975) and
 * stores it back with dnm_mat_set_norm. */
int dnm_mat_norm_inf(dnm_mat *A, double *nrm, void *stream);
/* The vector layouts the matrix works in (dnm_subspace.vec_swizzle codes): what the descriptors asked for when the
 * matrix supports it, 0 (reference order) otherwise -- e.g. a SpinConserve descriptor with the internal layout paired
 * with another subspace or under XParity.  The caller converts (dnm_vec_layout_copy) when a
 * vector's layout differs.  With an internal layout dnm_mat_sizes reports the local lengths incl. padding. */
int dnm_mat_layouts(const dnm_mat *A, int *left, int *right);
/* 1 if the handle was built with DNM_MAT_REAL_PACKED and multiplies real vectors (sizes then count complex128 elements) */
int dnm_mat_is_real_packed(const dnm_mat *A, int *packed);
int dnm_mat_set_norm(dnm_mat *A, double nrm);
/* human-readable description of the execution plan (passes, tiles) */
int dnm_mat_plan_describe(const dnm_mat *A, char *buf, size_t buflen);
/* number of kernel launches one dnm_mat_mult issues */
int dnm_mat_plan_launches(const dnm_mat *A, int *n);
/* plan introspection (diagnostics, CPU tests of the planner): pass counts, and
 * a copy of one pass's tables (layouts: dynamite_amd/csrc/plan.h DevPass /
 * DevQuad; pointers inside the copied DevPass are meaningless). */
int dnm_mat_plan_counts(const dnm_mat *A, int *n_local_passes, int *n_remote_passes, int *tiled,
                        int *B, int *logR, int *n_loc);
/* the pass's tabulated in-tile diagonal (2^tile_bits doubles; an error when the pass has none) */
int dnm_mat_export_dtile(const dnm_mat *A, int remote, int idx, double *out, int64_t n);
int dnm_mat_export_pass(const dnm_mat *A, int remote, int idx, void *desc_out, size_t desc_bytes,
                        void *quads_out, size_t quad_bytes, int max_quads, int *nquads);
/* the pass's table records (plan.h: DevTab -- masks of many terms, one table look-up per row instead of one sign per term)
 * and their tables ((re, im) pairs); null buffers: the counts alone */
int dnm_mat_export_tabs(const dnm_mat *A, int remote, int idx, void *tabs_out, size_t tab_bytes, int max_tabs, int *ntabs,
                        double *vals_out, int64_t max_vals, int64_t *nvals);
/* flip-flop records (plan.h: DevFlip -- two-bit masks whose coefficient is one number where the two bits differ and
 * nothing where they agree): the records of a pass with their class ranges (FL_COUNT + 1 entries) and the constant of its
 * diagonal, *nflips = -1 for a pass that runs on its generic records; and what the kernel reads beside them -- the
 * remaining generic records and the reduced diagonal, in the layouts of dnm_mat_export_pass / _dtile */
int dnm_mat_export_flip(const dnm_mat *A, int remote, int idx, void *flips_out, size_t flip_bytes, int max_flips,
                        int *nflips, uint32_t *loops_out, double *dconst);
int dnm_mat_export_flip_pass(const dnm_mat *A, int remote, int idx, void *desc_out, size_t desc_bytes, void *quads_out,
                             size_t quad_bytes, int max_quads, int *nquads, double *dtile_out, int64_t max_dtile,
                             int64_t *ndtile);
/* the diagonal of a pass as tables, of the form of the pass that the kernel runs on (plan.h: DevPass::dblock): one double
 * per workgroup (the terms outside the tile, the constant of a flip-flop form included), 2^nmasks sections of 2^tile_bits
 * doubles (section s: the terms that see the tile, those that also see outside bits with the sign their outside part takes
 * when parity(row & masks[i]) = bit i of s) and the up to three masks; *ndblock = 0 for a pass that evaluates its
 * diagonal from the records; null buffers: the counts alone */
int dnm_mat_export_diag_tables(const dnm_mat *A, int remote, int idx, double *dblock_out, int64_t max_dblock,
                               int64_t *ndblock, double *dtile_out, int64_t max_dtile, int64_t *ndtile,
                               uint64_t *masks_out, int *nmasks);

/* One host table of the SpinConserve passes of a handle whose vectors are in the internal layout (an error on any other
 * handle; host-only handles have them too), by name: rowsel needT hops wnb ptab pcoef permA permB bond dlo dt_sign
 * dt_coef dt_group -- the bytes the device gets (hops: 64-byte records mT mW mLo half dfield dbit pad pad as int32, then
 * up_re up_im dn_re dn_im).  "op": uint64 present, bondsA, bondsB, then int32 ndt, ngroups, glo[4], nldsA, ngatA, nldsB,
 * ngatB, nhp, ptab_row[18], tiled, graph, sym, real, diag_mode (160 bytes).  *nbytes: the table's size; null out: the
 * size alone */
int dnm_mat_export_sc3(const dnm_mat *A, const char *name, void *out, size_t max_bytes, size_t *nbytes);

/* What the block form of a SpinConserve pair in reference order launches (read-only; diagnostics and tests).  fields[6]:
 * the low bits per block (10 or 13; 0 on every handle that does not run the block form -- the other fields are 0 then),
 * the first and the last high part state >> lb of the handle's rows (the first rounded down to a multiple of 512 under
 * the swizzle), swizzle (1: workgroup b owns high part ((b >> 9) << 9) | ((b & 7) << 6) | ((b >> 3) & 63) counted from
 * the first; the grid is the span rounded up to a multiple of 512), the number of entries of the block order (0: none), and the workgroups of one launch.  perm_out (HOST, may be null; at
 * least fields[4] entries): the block order, workgroup -> high part counted from the first, 0xffffffff for a workgroup
 * without a block. */
int dnm_mat_export_sc_block(const dnm_mat *A, int64_t *fields, uint32_t *perm_out, int64_t max_perm);

/* --- partitioned multiply: replaces the VecScatterCreateToAll all-gather of
 * bcuda_template_2.cu:161-171 with an XOR-partner exchange. ---------------- */
/* One block transfer of the exchange: `count` amplitudes starting at `offset`
 * of the SENDER's local vector.  sends[]: what this rank must send (pass_id = -1);
 * recvs[]: what it receives, recvs[i] feeding dnm_mat_mult_remote(A, i, ...).
 * A mask that flips rank bits couples this rank to rank ^ (mask >> log2(n_local));
 * blocks on which its matrix elements vanish identically (e.g. the half of the
 * rows a flip-flop term XX+YY annihilates) are neither sent nor swept, and the
 * rank's block is split in halves so that only the needed half travels.  Between
 * one pair of ranks the sends of one side are listed in the order of the
 * receives of the other, so in-order point-to-point matching is sufficient. */
typedef struct {
  int32_t partner;   /* peer rank */
  int32_t pass_id;   /* recvs: index for dnm_mat_mult_remote; sends: -1 */
  int64_t offset;    /* first amplitude, in the sender's local vector */
  int64_t count;     /* amplitudes (complex128) */
} dnm_xfer;
int dnm_mat_exchange_plan(const dnm_mat *A, int *nsend, dnm_xfer *sends /* may be NULL */,
                          int *nrecv, dnm_xfer *recvs /* may be NULL */);
/* y = A x and dot[0] + i dot[1] = sum_i conj(x_i) y_i in the same sweep (the Lanczos
 * alpha = <v, H v>; what SLEPc does with MatMult + VecDot).  Single rank only. */
int dnm_mat_mult_dot(dnm_mat *A, const void *x, void *y, double *dot /* [2], host */, void *stream);
/* One Lanczos step's multiply: y = A x - b z (z may be NULL), dot[0] + i dot[1] = <x, y> and
 * dot[2] = |y|^2 (beta^2 = |y|^2 - |alpha|^2 without another sweep); the beta term starts the
 * accumulators of the first pass, the sums close the last.  The sums pair x_i with y_i:
 * an error (here and in dnm_mat_mult_dot) on a handle between two different subspaces. */
int dnm_mat_mult_lanczos(dnm_mat *A, const void *x, void *y, const void *z, double b,
                         double *dot /* [3], host */, void *stream);
/* y = A x - b z (three-term recurrences without inner products, e.g. Chebyshev).  Single rank only. */
int dnm_mat_mult_sub(dnm_mat *A, const void *x, void *y, const void *z, double b, void *stream);
/* 1 if dnm_mat_mult_sub / _sub2 cost no extra vector sweep for this operator (tiled and SpinConserve block kernels) */
int dnm_mat_fuses_init(const dnm_mat *A);
/* y = A x - b z + (c_re + i c_im) z2 (Clenshaw's recurrence; z2 may be NULL).  Single rank only. */
int dnm_mat_mult_sub2(dnm_mat *A, const void *x, void *y, const void *z, double b, const void *z2,
                      double c_re, double c_im, void *stream);
/* y = (masks that stay on this rank) x_local; y overwritten */
int dnm_mat_mult_local(dnm_mat *A, const void *x_local, void *y, void *stream);
/* y += (masks served by receive `recv_index`) x_recv, where x_recv holds the
 * recvs[recv_index].count amplitudes received from that partner; y is the
 * rank's whole local vector (the pass offsets into it itself) */
int dnm_mat_mult_remote(dnm_mat *A, int32_t recv_index, const void *x_recv,
                        void *y, void *stream);

/* --- partitioned multiply through a column window -------------------------------------------------
 * Basis indices are split as PetscSplitOwnership does (M / P rows each, the first M % P ranks one more; any P).
 * The columns a rank's rows read lie in a window (SpinConserve: col = row +- binomials, a few blocks wide, see
 * DESIGN.md; Explicit / projections: whatever the masks reach, found by one device sweep); the host assembles
 * that window IN INDEX ORDER from the owners' blocks (send/recv) and multiplies.  y_local is the rank's block of
 * the left vector in that subspace's own layout. */
int dnm_mat_ownership(const dnm_mat *A, int64_t *row0, int64_t *m_local);
/* Where dnm_mat_window_split says so (SpinConserve pairs in the internal layout, two tiled passes), the window multiply
 * comes in two parts so that compute overlaps the exchange (bpetsc_template_2.c:866-873 overlaps assembly and compute
 * block by block): _local needs the rank's own vector only (bonds inside a block of equal top bits, the diagonal) and
 * WRITES y; _remote reads the assembled window and ADDS the bonds that reach other blocks.  y = _local, then _remote. */
int dnm_mat_window_split(const dnm_mat *A, int *supported);
/* Tiled Full / Parity operators: the rank-local passes over one of `nparts` (a power of two) equal ranges of their
 * workgroups.  dnm_mat_local_part_bits tells what a range is: *top_free_bit = the highest index bit outside every tile
 * (range `part` covers the amplitudes whose log2(nparts) index bits ending there equal `part`), *gathers = records
 * that read outside the tile (0: a range reads and writes its own amplitudes only).  That description of a range holds
 * where the log2(nparts) index bits ending at *top_free_bit lie outside every pass's tile; dnm_mat_mult_local_part
 * refuses a plan of several passes whose ranges are not the same amplitudes in every pass (a later pass adds to what the
 * earlier ones wrote in the same call).  The transposed exchange runs its layout-B pass sub-piece by sub-piece this way. */
int dnm_mat_mult_local_part(dnm_mat *A, const void *x, void *y, int part, int nparts, void *stream);
int dnm_mat_local_part_bits(const dnm_mat *A, int *top_free_bit, int *gathers);
/* *agree = 1 if range `part` of nparts is the same amplitudes in every rank-local pass (always so on a plan of one pass),
 * 0 if dnm_mat_mult_local_part would refuse: for callers that decide beforehand whether to run by ranges */
int dnm_mat_local_part_agree(const dnm_mat *A, int nparts, int *agree);
int dnm_mat_mult_window_local(dnm_mat *A, const void *x_local, void *y_local, void *stream);
int dnm_mat_mult_window_remote(dnm_mat *A, const void *x_window, int64_t win_start, int64_t win_len, void *y_local,
                               void *stream);
/* Every other window partition (SpinConserve in reference order, Explicit, projection pairs, odd rank counts) overlaps
 * by ROWS: dnm_mat_window_local_rows lists up to max_ranges ranges [r0, r1) of the rank's local rows whose columns all
 * lie in [col_lo, col_hi) -- the rank's own block of x, which sits in the window buffer before anything arrives; none
 * shorter than min_blocks workgroups of 256 rows -- and
 * dnm_mat_mult_window_rows multiplies one range of rows; the caller runs the listed ranges under the exchange and the
 * rest after it (bpetsc_template_2.c:866-873). */
int dnm_mat_window_local_rows(dnm_mat *A, int64_t col_lo, int64_t col_hi, int max_ranges, int min_blocks,
                              int64_t *ranges, int *nranges, void *stream);
int dnm_mat_mult_window_rows(dnm_mat *A, const void *x_window, int64_t win_start, int64_t win_len, void *y_local,
                             int64_t r0, int64_t r1, void *stream);
/* SpinConserve pairs in the internal layout (dnm_mat_layouts) partition differently: a rank owns whole blocks of equal
 * top bits T -- a contiguous range of the internal layout (dnm_vec_layout_partition; balanced to within one block)
 * that is also a contiguous range of the reference order -- and ownership, windows and chunks are expressed in
 * positions of the internal layout: ranks exchange ranges of their vectors as they lie. */
/* inclusive column range this rank's rows read; one device sweep, then cached */
int dnm_mat_column_window(dnm_mat *A, int64_t *cmin, int64_t *cmax, void *stream);
/* which chunks of 2^chunk_shift columns inside that window the rank's rows really read:
 * map[(col >> chunk_shift) - (cmin >> chunk_shift)] = 1, nchunks = (cmax >> chunk_shift) - (cmin >> chunk_shift) + 1
 * bytes on the host.  The window is mostly holes for the far hops of a SpinConserve chain (L=24, k=12 on 8
 * ranks: 1.5 blocks needed of a 4.2-block window): only marked chunks have to be received, the multiply never
 * reads the others (the reference scatters exactly the entries it needs, bpetsc_template_2.c:413-504) */
int dnm_mat_column_chunks(dnm_mat *A, int chunk_shift, uint8_t *map, int64_t nchunks, void *stream);
/* The same exactly, where the library knows it without a sweep (SpinConserve pairs in the internal layout: whole blocks of
 * equal top bits): the positions the rank's rows read as maximal runs [lo, hi), ascending -- ranges[2 i], ranges[2 i + 1];
 * *nranges = their number (call with max_ranges = 0 to size the array; 0 for every other partition: use the chunk map).
 * In the block order that keeps the reference's ranges (dnm_subspace.vec_swizzle bits 16-19 = 0) the chunk map is as
 * good; in the order made for partitions (1) the needed blocks interleave with others and only this list is tight. */
int dnm_mat_column_ranges(dnm_mat *A, int64_t max_ranges, int64_t *ranges, int64_t *nranges);
/* y_local = A[own rows, :] x, x_window holding columns [win_start, win_start + win_len) */
int dnm_mat_mult_window(dnm_mat *A, const void *x_window, int64_t win_start, int64_t win_len,
                        void *y_local, void *stream);

/* ------------------------------------------------------------------ */
/* vector kernels (what PETSc Vec / SLEPc BV supply to the Krylov     */
/* loops; states.py:703-797 on the Python side)                       */
/* ------------------------------------------------------------------ */
int dnm_vec_set(void *x, int64_t n, double re, double im, void *stream);          /* VecSet */
int dnm_vec_copy(const void *x, void *y, int64_t n, void *stream);                /* VecCopy */
int dnm_vec_scale(void *x, int64_t n, double re, double im, void *stream);        /* VecScale */
/* y = alpha x + beta y  (VecAXPBY, states.py:779-797) */
int dnm_vec_axpby(void *y, const void *x, int64_t n, double are, double aim,
                  double bre, double bim, void *stream);
/* out[0..1] = sum_i x_i * conj(y_i)  (VecDot(x,y) = y^H x, states.py:703-719) */
int dnm_vec_dot(const void *x, const void *y, int64_t n, double *out, void *stream);
int dnm_vec_norm2(const void *x, int64_t n, double *out, void *stream);           /* VecNorm */
/* Fills x with N(0,1)+iN(0,1) from a counter-based generator keyed by
 * (seed, global index = offset + i): distribution of State.set_random
 * (states.py:292-316), not its MT19937 stream. */
int dnm_vec_set_random(void *x, int64_t n, uint64_t seed, int64_t offset, void *stream);
/* Size condition of the three calls below that take a swizzle shift S != 0: the swizzle maps [0, n) onto itself only
 * when n <= 2^S (no folded bit is ever set: the layout is index order) or n is a multiple of 2^S.  Any other n is
 * refused before anything is launched (n = 2^S + 16 would send element 2^S to position n).  dnm_vec_unpack_real
 * holds n_packed to it under swizzle_packed and 2 * n_packed under swizzle_out. */
/* the same stream of numbers for a vector in the swizzled layout (element i gets what index order would give it) */
int dnm_vec_set_random_swz(void *x, int64_t n, uint64_t seed, int64_t offset, int swizzle, void *stream);
/* dst[i] = src[i ^ sw(i)]: swizzled <-> index order (the map is an involution); dst != src */
int dnm_vec_swizzle_copy(void *dst, const void *src, int64_t n, int swizzle, void *stream);
/* The complex128 vector a real-packed one stands for (DNM_MAT_REAL_PACKED; no counterpart in the reference, whose PETSc
 * build is complex throughout -- what its EPS hands to computations.py:273-284 is what dst holds): src has n_packed
 * elements, element j = the real amplitudes of indices 2j and 2j + 1, in the layout swizzle_packed; dst gets
 * 2 * n_packed elements with zero imaginary parts in the layout swizzle_out; dst != src */
int dnm_vec_unpack_real(void *dst, const void *src, int64_t n_packed, int swizzle_packed, int swizzle_out, void *stream);
/* The same for a SpinConserve subspace in the internal layout: src holds one double per position of the rank's part of
 * the layout (what a DNM_MAT_REAL_PACKED operator of that subspace multiplies; part may be NULL on one rank), dst gets
 * the complex128 vector of the layout with zero imaginary parts; dst != src */
int dnm_vec_layout_unpack_real(const dnm_subspace *s, const dnm_partition *part, void *dst, const void *src, void *stream);
/* Vectors of a SpinConserve subspace in the internal layout (dnm_subspace.vec_swizzle = a | w << 8).  No counterpart
 * in the reference: what a petsc4py Vec of that subspace holds, element by element, is reached through these.
 * size: elements of a vector (rows + padding); copy: to_internal != 0: dst (internal) <- src (reference order, C(L,k)
 * elements), else dst (reference order) <- src (internal), dst != src; zero_padding: after an operation that wrote
 * the padding (VecSet, VecShift); positions: pos[i] = where reference index idx[i] lives (device arrays of n int64);
 * set_random: the numbers dnm_vec_set_random gives reference order, padding zero. */
int dnm_vec_layout_size(const dnm_subspace *s, int64_t *n);
/* the part of such a vector rank `rank` of `nranks` owns: [istart, istart + ilen) of the internal layout =
 * [nstart, nstart + nlen) of the reference order */
int dnm_vec_layout_partition(const dnm_subspace *s, int nranks, int rank, int64_t *istart, int64_t *ilen,
                             int64_t *nstart, int64_t *nlen);
/* the layout's T blocks in the order they lie in memory (the unit a partition shares out, and what moves whole between
 * two layouts that differ in block order only -- vec_swizzle bits 16-19): T[j] = the block's value of the T field,
 * ibase[j] = its first position; ibase[*count] = the layout's size.  max < *count (e.g. 0 with null arrays): the count
 * alone.  T: max entries, ibase: max + 1.  Host tables only. */
int dnm_vec_layout_blocks(const dnm_subspace *s, int64_t max, int64_t *T, int64_t *ibase, int64_t *count);
/* `part` (null: one rank) selects the rank whose part of the vector the pointers hold; indices and positions are
 * then local to that part */
int dnm_vec_layout_copy(const dnm_subspace *s, const dnm_partition *part, void *dst, const void *src, int to_internal,
                        void *stream);
int dnm_vec_layout_copy_f64(const dnm_subspace *s, const dnm_partition *part, double *dst, const double *src,
                            int to_internal, void *stream);
int dnm_vec_layout_zero_padding(const dnm_subspace *s, const dnm_partition *part, void *x, void *stream);
int dnm_vec_layout_positions(const dnm_subspace *s, const dnm_partition *part, int64_t n, const int64_t *idx,
                             int64_t *pos, void *stream);
int dnm_vec_layout_positions_host(const dnm_subspace *s, const dnm_partition *part, int64_t n, const int64_t *idx,
                                  int64_t *pos);  /* host arrays */
int dnm_vec_layout_set_random(const dnm_subspace *s, const dnm_partition *part, void *x, uint64_t seed, void *stream);
/* h[j] = V_j^H w for j < nv (BVDotVec); V = nv vectors of length n, stride ldv elements.
 * h_host: 2*nv doubles. */
int dnm_vec_mdot(const void *V, int64_t ldv, int nv, const void *w, int64_t n,
                 double *h_host, void *stream);
/* w += sum_j c[j] V_j (BVMultVec); c_host: 2*nv doubles */
int dnm_vec_maxpy(void *w, const void *V, int64_t ldv, int nv, int64_t n,
                  const double *c_host, void *stream);
/* V[:, 0:nout) = V[:, 0:nin) * S  (in place, S is nin x nout complex column-major,
 * host): the thick-restart basis update (BVMultInPlace). */
int dnm_vec_basis_update(void *V, int64_t ldv, int nin, int nout, int64_t n,
                         const double *S_host, void *stream);

/* ------------------------------------------------------------------ */
/* Krylov solvers -- computations.py:10-126 (SLEPc MFN expokit) and   */
/* computations.py:128-292 (SLEPc EPS Krylov-Schur, HEP)              */
/* ------------------------------------------------------------------ */
/* Distributed hooks: when non-NULL the solver calls them after every local
 * reduction (sum over ranks of `n` doubles, in place / max) and uses `mult`
 * instead of dnm_mat_mult.  A single-device run passes NULL. */
typedef struct dnm_hooks {
  void *ctx;
  int (*mult)(void *ctx, const void *x, void *y);
  int (*allreduce_sum)(void *ctx, double *buf, int n);
  int (*allreduce_max)(void *ctx, double *buf, int n);
} dnm_hooks;

/* converged reasons (SLEPc MFNConvergedReason / EPSConvergedReason as mapped
 * by computations.py:114-122 and :261-275) */
enum {
  DNM_CONVERGED_TOL = 1,
  DNM_CONVERGED_ITS = 2,        /* MFN_CONVERGED_ITS */
  DNM_DIVERGED_ITS = -1,        /* -> MaxIterationsError */
  DNM_DIVERGED_BREAKDOWN = -2,  /* -> ConvergenceError */
  DNM_DIVERGED_SYMMETRY_LOST = -3
};

typedef struct dnm_solver_stats {
  int32_t reason;
  int32_t its;          /* outer steps (MFN) / restarts (EPS) */
  int32_t matvecs;
  int32_t nconv;        /* EPS only */
  double  err_est;      /* MFN: accumulated local error estimate; EPS: largest measured
                         * |H u - theta u| / |theta| of the returned pairs */
} dnm_solver_stats;

/* y = exp(scale * A) x, scale = (scale_re + i scale_im); evolve() passes
 * scale = -i t (computations.py:89-96).  Sidje-Expokit adaptive Krylov
 * (SLEPc MFNEXPOKIT); because A is Hermitian the basis is built by Lanczos
 * with partial re-orthogonalisation (DNM_EXPM_ORTHO=full: against the whole
 * basis every step, as SLEPc's BV).  tol<=0 -> 1e-8; ncv<=0 -> min(30, N);
 * max_its<=0 -> 100 (SLEPc defaults).  work_limit_bytes bounds the basis
 * allocation (0 = no limit): ncv is reduced to fit.  With ncv <= 0, max_its <= 0
 * and scale_re == 0 (a real time) the driver compares, after every accepted step,
 * what the rest of the interval costs at the step size the error control has
 * settled on with what dnm_expm_chebyshev needs for it (known exactly) and hands
 * the rest over when that is clearly cheaper; the expansion is taken from the
 * start when all of it costs less than one outer step of ncv multiplies, when
 * an earlier hand-over on this operator still applies, or when the basis
 * workspace would have to be acquired for a memory-limited basis and ten Lanczos
 * steps from x show that the norm bound is not loose (DNM_EXPM_HYBRID=0: never). */
int dnm_expm_multiply(dnm_mat *A, const void *x, void *y, int64_t n_local,
                      double scale_re, double scale_im, double tol, int ncv,
                      int max_its, size_t work_limit_bytes, const dnm_hooks *hooks,
                      dnm_solver_stats *stats, void *stream);

/* y = exp(-i t A) x for REAL t by the Chebyshev expansion
 *   exp(-i t A) = sum_k (2 - delta_k0) (-i)^k J_k(r t) T_k(A / r),   r = ||A||_inf >= spectral radius,
 * evaluated with the three-term recurrence on the fused multiply y = A x - b z: one multiply and
 * two thirds of a vector sweep per term, four work vectors, no inner products and no basis --
 * an alternative to dnm_expm_multiply when the Krylov basis is what limits the size or the speed
 * (Operator.evolve(algo='chebyshev')).  The series is cut where the remaining Bessel coefficients sum to
 * less than tol/100 (tol <= 0 -> 1e-8); long times are split into steps of r*t <= 64.  Costs about
 * r*t + 6 (r*t)^(1/3) + 10 multiplies; loose norm bounds (r much larger than the spectral radius)
 * cost proportionally more.  stats->its = number of steps, stats->matvecs = multiplies. */
int dnm_expm_chebyshev(dnm_mat *A, const void *x, void *y, int64_t n_local, double t, double tol,
                       const dnm_hooks *hooks, dnm_solver_stats *stats, void *stream);

/* The solvers keep their Krylov-basis allocation between calls and the reduced
 * density matrix its tile scratch; this frees them.  (The library keeps such
 * per-process buffers and small reduction scratch: calls are not re-entrant --
 * one host thread per process, as the reference's one thread per MPI rank.) */
int dnm_release_workspace(void);
/* bytes of Krylov basis currently cached (reusable by the next solve) */
int dnm_workspace_bytes(size_t *bytes);
/* Acquire (and touch: every page is written once) at least `bytes` of that workspace now, so that the next solve finds
 * it in place -- what a caller that times solves does once, untimed (bench.py: a first solve at L=30 otherwise pays
 * 1-2 s for 64 GiB of fresh device memory).  No-op when the cached workspace is already that large. */
int dnm_workspace_reserve(size_t bytes, void *stream);

/* ------------------------------------------------------------------ */
/* ranks -- the partitioned multiply as one native call                */
/* ------------------------------------------------------------------ */
/* The reference handles its ranks inside C: MatMult_CPU_Fast / _General post their scatters themselves
 * (bpetsc_template_2.c:413-504, 787-879), the CUDA shell all-gathers x (bcuda_template_2.cu:161-171), PETSc's
 * communicator comes with the Mat.  Here a dnm_comm is an RCCL communicator (one rank per GPU, xGMI) plus the
 * library's own exchange stream; RCCL is bound at run time (the library loads without it).
 *   dnm_comm_unique_id: ncclGetUniqueId -- one rank makes the 128 bytes, the host program hands them to the others
 *     (MPI_Bcast, a file, torch.distributed's store);
 *   dnm_comm_create: ncclCommInitRank -- collective;
 *   dnm_mat_mult_partitioned: y = A x on this rank's blocks, A built with the same (rank, nranks) partition: the
 *     exchange -- XOR-partner sub-blocks of a Full / Parity pair on 2^p ranks, the needed ranges of the column window
 *     of every other partition -- is posted on the exchange stream as one group of ncclSend / ncclRecv, the part of
 *     the multiply that reads nothing from other ranks runs under it on `stream`, the rest follows its event.
 *     Collective.
 *   dnm_mat_set_exchange: the scheme of a tiled Full / Parity operator on 2^p ranks.  DNM_EXCHANGE_TRANSPOSE (AUTO: from
 *     four ranks on, where an all-to-all puts less on the busiest xGMI link than the partner blocks): the operator is
 *     split inside the handle into the terms that flip no rank bit and the others rewritten for the layout in which the
 *     rank bits are local (the p index bits [f, f + p), f = n_local_bits - 1 - p, swapped with them); both parts are
 *     rank-local.  dnm_mat_mult_partitioned then sends the state through ONE all-to-all, runs the first part under it,
 *     the second on the redistributed state -- sub-piece by sub-piece as the pieces land, where the plan allows -- and
 *     adds what the returning all-to-all brings (bpetsc_template_2.c:866-873 overlaps assembly and compute block by
 *     block).  *chosen = the scheme in force: an operator that does not split (a term flips a rank bit and the field it
 *     would move to; too few local bits; no tiled plan) keeps DNM_EXCHANGE_PARTNER.  Call it before the first
 *     dnm_mat_mult_partitioned of A (or dnm_comm_forget(c, A) first: a communicator caches buffers per scheme), on every
 *     rank alike.  dnm_mat_exchange_parts hands out the two parts (owned by A; NULL under the partner scheme) and f, for
 *     hosts that run the schedule themselves.
 *   dnm_comm_allreduce: n doubles summed (op 0) / maximised (op 1) over the ranks, in place, host memory;
 *   dnm_comm_hooks: the dnm_hooks of dnm_expm_multiply / dnm_eigsolve filled with the two above (valid until the
 *     communicator is destroyed);
 *   dnm_comm_prepare: allocate now what the first dnm_mat_mult_partitioned of A would (receive buffers, the column
 *     window -- collective --, the two vectors of the transposed exchange), so that a solver sizing its Krylov basis
 *     to the free device memory sees what is really left;
 *   dnm_comm_forget: drop what the communicator caches for A (receive buffers, windows) before A is destroyed;
 *   dnm_comm_loopback (tests): a communicator of ONE rank stands for rank vrank of vranks; peer q's block of x is the
 *     device pointer peer_x[q] (peer_mat[q]: its handle, needed by window partitions and by the transposed exchange,
 *     whose returning pieces are what the PEERS computed -- the loop-back runs their second part too; without handles
 *     the returning pieces carry this rank's own data: right traffic, wrong numbers, for timing; entries for vrank
 *     itself are ignored) and every message becomes an RCCL send of this process to itself -- the schedules and the
 *     transport on a one-GPU box. */
typedef struct dnm_comm dnm_comm;
int dnm_comm_unique_id(void *id128);
int dnm_comm_create(const void *id128, int rank, int nranks, dnm_comm **out);
int dnm_comm_destroy(dnm_comm *c);
int dnm_comm_prepare(dnm_comm *c, dnm_mat *A, void *stream);
int dnm_comm_forget(dnm_comm *c, dnm_mat *A);
int dnm_comm_loopback(dnm_comm *c, int vrank, int vranks, const void *const *peer_x, dnm_mat *const *peer_mat);
int dnm_comm_allreduce(dnm_comm *c, double *vals, int n, int op);
/* Measurement: which half of the schedule the following dnm_mat_mult_partitioned calls run -- the whole multiply
 * (default), its messages alone (what the links sustain: nothing is computed, y is left alone), or its kernels alone (the
 * rank's compute with nothing on the links: results are not those of the multiply).  The three times together say how
 * much of the exchange the schedule hides (bench.py --gpus N).  The reference has no counterpart: its -log_view splits
 * VecScatterBegin/End from MatMult the same way. */
enum { DNM_PHASE_ALL = 0, DNM_PHASE_EXCHANGE = 1, DNM_PHASE_COMPUTE = 2 };
int dnm_comm_set_phase(dnm_comm *c, int phase);
int dnm_mat_mult_partitioned(dnm_mat *A, dnm_comm *c, const void *x, void *y, void *stream);
enum { DNM_EXCHANGE_AUTO = 0, DNM_EXCHANGE_PARTNER = 1, DNM_EXCHANGE_TRANSPOSE = 2 };
int dnm_mat_set_exchange(dnm_mat *A, int scheme, int *chosen);
int dnm_mat_exchange_parts(const dnm_mat *A, dnm_mat **lo, dnm_mat **hi, int *f);
/* The operator a handle holds (its own copies, as BuildContext_* keeps them): counts first (arrays may be NULL), then
 * masks[nmasks], mask_offsets[nmasks + 1], signs[nterms], coeffs[nterms] -- ONE double per term, the real part of the
 * coefficient where that is non-zero, else the imaginary part (ctx->real_coeffs, bpetsc_template_2.c:286-289; which of
 * the two it is follows from mask and sign: TERM_REAL, :398-404). */
int dnm_mat_operator(const dnm_mat *A, int64_t *nmasks, int64_t *nterms, int64_t *masks, int64_t *mask_offsets,
                     int64_t *signs, double *coeffs);
int dnm_comm_hooks(dnm_comm *c, dnm_mat *A, void *stream, dnm_hooks *out);

enum { DNM_WHICH_LOWEST = 0, DNM_WHICH_HIGHEST = 1, DNM_WHICH_EXTERIOR = 2,
       DNM_WHICH_TARGET = 3 /* dnm_eigsolve_interior only: dnm_eigsolve takes the first three */ };

/* Thick-restart Lanczos (SLEPc EPSKRYLOVSCHUR on a HEP).  evals: [nev_max]
 * doubles; evecs (optional, may be NULL): device buffer of nev_max vectors of
 * n_local complex128 each, stride n_local.  nev_max >= nev.  tol<=0 -> 1e-8;
 * ncv<=0 -> max(2*nev, nev+15); max_its<=0 -> max(100, 2N/ncv).  Partial
 * re-orthogonalisation with a tolerance-driven trigger (DNM_EIGS_ORTHO=full:
 * every step against the whole basis, as SLEPc); stats->err_est returns the
 * measured largest relative residual of the returned pairs.
 * Automatic choices under default parameters (ncv <= 0) for large operators: nev = 1 -> Lanczos without a stored basis
 * (four work vectors); nev > 1 -> thick restart on a Chebyshev filter of H; ncv = -c (the caller's memory limit: at most
 * c vectors in all) with c < nev + 6 -> the pairs one after the other by the basis-free recurrence on the operator
 * deflated by the pairs found (four work vectors + the pairs; evals then count multiplicities -- a degenerate level
 * comes back once per copy, where a single Krylov space, SLEPc's included, shows one).  DESIGN.md section 5. */
int dnm_eigsolve(dnm_mat *A, int64_t n_local, int nev, int which, double tol,
                 int ncv, int max_its, uint64_t seed, const dnm_hooks *hooks,
                 int nev_max, double *evals, void *evecs,
                 dnm_solver_stats *stats, void *stream);

/* Eigenpairs of a Hermitian operator NEAREST `target` (SLEPc EPS_TARGET_MAGNITUDE), without a stored matrix and
 * without a linear solve: thick-restart Lanczos on a Chebyshev filter of the folded spectrum,
 *   p(A) = T_d(((A - target)^2 - c) / e) / T_d(-c / e)      (dnm_interior_filter_plan),
 * each term of the recurrence two fused multiplies y = A x - b z + c2 z2 (dnm_mat_mult_sub2; through hooks->mult and
 * one sweep per term when hooks are set), with a Rayleigh-Ritz step in A itself on the converged Ritz vectors.  The
 * ends of the spectrum and the window's half-width (about nev + max(4, nev / 2) levels, from the density of states
 * a Lanczos run estimates) are found by the call; the window is widened if it holds fewer than nev levels.
 * Arguments as dnm_eigsolve (evals [nev_max], evecs optional: nev_max vectors of n_local complex128).  ncv <= 0 ->
 * max(2*nev, nev+15) Lanczos vectors, ncv = -c: at most c vectors in all; the filter keeps three work vectors beside
 * the ncv + 1 of the basis.  tol <= 0 -> 1e-8; max_its <= 0 -> 100 restarts.
 * Convergence: |A u - theta u| <= tol * ||A||_inf, MEASURED for every returned pair (SLEPc EPS_CONV_NORM -- a
 * criterion relative to theta means nothing at theta = 0, where mid-spectrum targets of traceless operators sit).
 * Returns at least nev pairs when converged, ordered by |theta - target| ascending, eigenvectors orthonormal;
 * stats->err_est = the largest measured residual / ||A||_inf, stats->matvecs = multiplies of the iteration (the
 * Rayleigh-Ritz step and the checks are not counted), stats->its = restarts.  DESIGN.md section 5. */
int dnm_eigsolve_interior(dnm_mat *A, int64_t n_local, int nev, double target, double tol,
                          int ncv, int max_its, uint64_t seed, const dnm_hooks *hooks,
                          int nev_max, double *evals, void *evecs,
                          dnm_solver_stats *stats, void *stream);

/* The parameters of that filter as pure arithmetic (host only).  With h = max(target - emin, emax - target):
 * c = (h^2 + a^2) / 2, e = (h^2 - a^2) / 2, and *degree the smallest d >= 1 with T_d(c / e) >= damping, i.e.
 * ceil(acosh(damping) / acosh(c / e)): |p| <= 1 / damping on every eigenvalue farther than a from the target,
 * p(target) = 1.  Needs emax > emin, 0 < a < h, damping > 1. */
int dnm_interior_filter_plan(double emin, double emax, double target, double a, double damping,
                             int *degree, double *c, double *e);

#ifdef __cplusplus
}
#endif
#endif
