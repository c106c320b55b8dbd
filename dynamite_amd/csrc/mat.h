// The shell-matrix handle behind the C ABI (replaces PETSc MatShell +
// shell_context, src/dynamite/_backend/shell_context.h:12-27).
#pragma once

#include <memory>
#include <vector>

#include "dev_buf.h"
#include "kernels.h"
#include "plan.h"
#include "sc3.h"
#include "subspace.h"

namespace dnm {

// A subspace with owned host tables and their device mirrors.
struct SubOwned {
  SubView host{};
  SubView dev{};
  std::vector<int64_t> nck, smap, rind, rstates, bucket;
  DevBuf d_nck, d_smap, d_rind, d_rstates, d_bucket;
  int init(const dnm_subspace *s, bool want_device);
};
// the checked view of a caller's descriptor: its tables stay the caller's (mat.cpp)
int view_from_c(const dnm_subspace *s, SubView *v);
// Do two descriptors name the same subspace -- the same states at the same indices?  (Equal dimensions do not say so:
// SpinConserve(10, 4) and SpinConserve(10, 6), two Explicit lists of one length, the two Parity sectors.)  The vector
// layout is not part of the question.  Explicit: a compare of the two state lists -- dnm_mat_create asks once and keeps
// the answer (dnm_mat::one_subspace); nothing on the path of a multiply calls this.
inline bool same_subspace(const SubOwned &a, const SubOwned &b) {
  const SubView &x = a.host, &y = b.host;
  if (x.type != y.type || x.L != y.L) return false;
  switch (x.type) {
    case DNM_PARITY: return x.space == y.space;
    case DNM_SPIN_CONSERVE: return x.k == y.k;
    case DNM_EXPLICIT: return a.smap == b.smap;
  }
  return true;
}

// What one launch of the tiled kernel reads, as passes.cpp builds it on the host
struct PassRecords {
  DevPass desc{};                 // geometry and record ranges; its device pointers are null until upload()
  std::vector<DevQuad> quads;
  std::vector<double> dtile;      // in-tile diagonal per tile coordinate (DevPass::dtile)
  std::vector<DevTab> tabs;       // table records (plan.h: DevTab) and their tables
  std::vector<double> tabvals;
  bool is_reduced = false;        // the flip-flop form of a pass (plan.h: DevFlip): flips / flip belong to it
  std::vector<DevFlip> flips;
  DevFlipPass flip{};
  // the rest of the diagonal as tables (DevPass::dblock; build_diag_tables), derived from quads / dtile / flip.dconst:
  // dblock empty: the pass has none; dsect: the sectioned in-tile table (empty with dblock set: one section, dtile itself)
  std::vector<double> dblock, dsect;
  const std::vector<double> &dtile_sections() const { return dsect.empty() ? dtile : dsect; }
  DevBuf d_quads, d_dtile, d_tabs, d_tabvals, d_flips, d_dblock;
  int upload();                   // the only place that writes a device pointer into desc / flip
};

struct PassOnDevice {
  PassRecords whole;                      // the pass in the generic vocabulary (dnm_mat_export_pass)
  // passes with flip-flop records: those, the generic records that remain and the diagonal the exchanges leave
  std::unique_ptr<PassRecords> reduced;
  PassRecords &runs() { return reduced ? *reduced : whole; }      // what the kernel is launched on
  const PassRecords &runs() const { return reduced ? *reduced : whole; }
  int partner = -1;
  int n_eff = 0;                  // index bits the pass sweeps
  int64_t y_off = 0, src_off = 0; // partner passes: first local row / first partner amplitude
};

// A mask as a flip-flop record (plan.h: DevFlip; flip_classify / decide_flip_bonds in passes.cpp)
struct FlipBond {
  bool ok = false;        // the mask runs as a flip-flop record
  bool exch = false;      // ... as a tile record, an exchange: the diagonal carries what it leaves
  int b0 = 0, b1 = 0;     // the two index bits, b0 < b1
  double c = 0.0;         // the coefficient on rows whose two bits differ
};

int rdm_release_scratch();   // frees the cached scratch of dnm_reduced_density_matrix

// The kernel family a handle's one-rank multiply runs on.  dnm_mat_create decides it last, after the knobs
// (DNM_SC3_TILED, DNM_SC_BLOCK, DNM_ROW_FUSE, DNM_MAT_FORCE_GATHER) have had their say; nothing changes it afterwards.
enum class Route {
  Tiled,      // Full / Parity pair: the tiled hypercube passes
  Sc3Tiled,   // SpinConserve pair in the internal layout (sc3.h): the two tiled passes
  Sc3Rows,    // ... its row kernel
  ScBlock,    // SpinConserve pair in reference order: one workgroup per block of low bits
  ScRows,     // ... one thread per row
  Gather,     // any other pair: one thread per row with index maps
};
// the last three sweep a range of rows in one launch (mat_mult.cpp: launch_rows) and can run behind a column window
inline bool row_route(Route r) { return r == Route::ScBlock || r == Route::ScRows || r == Route::Gather; }

}  // namespace dnm

struct dnm_mat {
  // operator as given (deep copies, BuildContext semantics)
  std::vector<int64_t> masks, mask_offsets, signs;
  std::vector<double> real_coeffs;
  dnm::SubOwned left, right;
  int64_t M = 0, N = 0, m_local = 0, n_local = 0;
  int64_t row0 = 0;               // first row / column this rank owns
  bool sc_pair = false;           // SpinConserve(L,k) on both sides: incremental-rank kernel
  bool one_subspace = false;      // left and right name the same subspace (same_subspace, asked once by dnm_mat_create)
  // SpinConserve(L,k) on both sides with vectors in the internal layout (sc3.h): m_local / n_local then count the
  // padding too (they are what the vector kernels sweep), rows_local the rows
  bool use_sc3 = false;
  std::unique_ptr<dnm::Sc3Mat> sc3;
  int64_t rows_local = 0;
  int64_t win_min = 0, win_max = -1;   // partitioned SpinConserve: columns this rank reads (cached)
  int rank = 0, nranks = 1;
  int flags = 0;
  bool xparity = false;
  bool host_only = false;         // DNM_MAT_HOST_ONLY: plan and tables only, no device
  dnm::Route route = dnm::Route::Gather;   // a host-only handle has the route its flags imply and refuses to launch

  bool hypercube = false;        // Full/Full or Parity/Parity: index space is a hypercube
  // DNM_MAT_REAL_PACKED: vectors are real, two amplitudes per complex128 element (M, N, m_local, n_local count
  // elements; rows_local / row0 still describe the operator's rows for the norm kernel)
  bool real_packed = false;
  dnm::OpForm op;
  dnm::Plan plan;
  std::vector<std::unique_ptr<dnm::PassOnDevice>> local_passes, remote_passes;
  std::vector<dnm::FlipBond> flip_bonds;   // per op.masks entry; empty: the operator has no flip-flop records

  // generic-kernel tables
  dnm::DevBuf d_masks, d_offsets, d_signs, d_rcoeffs;
  dnm::DevMsc dmsc{};
  dnm::DevBuf d_pmasks, d_poffsets, d_psigns, d_prcoeffs;     // the same in the labelling of a relabelled sc3 layout
  dnm::DevMsc dmsc_sc3{};         // what the sc3 row kernel reads (dmsc unless the layout is relabelled)
  dnm::DevBuf d_sclow;            // SpinConserve kernel: 16-bit unranking table
  dnm::ScLow sclow{};
  dnm::DevBuf d_scblock;          // block kernel: lb-bit patterns grouped by popcount
  dnm::DevBuf d_scperm;           // block kernel: optional block order
  dnm::ScBlock scblock{};         // lb == 0: block kernel not used
  bool row_fuse = true;           // one-thread-per-row kernels with the fused epilogue (DNM_ROW_FUSE=0 at creation: off)
  int sc_nfast = 0;               // masks that are chain bonds with local signs
  // evolve: the Krylov step size at which the driver last handed over to the Chebyshev expansion (0: never) and
  // the basis size it belonged to -- later calls on this operator skip the Krylov probe when the estimate still holds
  double expm_tstep = 0.0;
  int expm_m = 0;
  int expm_bound = 0;             // what the Lanczos probe of the norm bound found: +1 tight, -1 loose, 0 not probed
  dnm::DevBuf d_scmasks;          // SpinConserve kernel: per-mask precomputation (ScMask[nmasks])

  // transposed exchange (dnm_mat_set_exchange): the terms that flip no rank bit in the vectors' own layout, the
  // others with the rank bits swapped against the local field [tr_f, tr_f + p) -- both rank-local; owned by this handle
  dnm_mat *tr_lo = nullptr, *tr_hi = nullptr;
  int tr_f = -1;
  ~dnm_mat();

  dnm::DevBuf diag;              // cached diagonal (double[m_local]) if precomputed
  bool have_diag = false;
  const double *cached_diag() const { return have_diag ? (const double *)diag.p : nullptr; }
  double nrm = -1.0;             // ctx->nrm cache, -1 = unset (bpetsc_template_2.c:926-929)
  dnm::DevBuf scratch;
};

namespace dnm {

// What the route of a handle fuses into y = A x - b z + c z2 (mat_mult.cpp: mult_fused does the rest in sweeps).
//   start: -b z + c z2 joins the kernel's accumulators (dnm_mat_fuses_init: the recurrence costs no extra sweep)
//   sums:  <x, y> and |y|^2 leave the kernel as workgroup partials
struct RouteFuses {
  bool start = false, sums = false;
};
inline RouteFuses route_fuses(const dnm_mat &A) {
  RouteFuses f;
  if (A.host_only || !A.remote_passes.empty()) return f;     // nothing launches; nothing fused beside remote passes
  switch (A.route) {
    case Route::Tiled:        // the first pass starts from the vectors; the last takes the sums if it stages x (need_tile)
      f.start = !A.local_passes.empty();
      f.sums = f.start && A.local_passes.back()->whole.desc.need_tile != 0;
      break;
    case Route::Sc3Tiled: f.start = f.sums = true; break;
    case Route::Sc3Rows: f.start = true; break;                // the row kernel takes the start vectors, not the sums
    case Route::ScBlock: f.start = f.sums = A.nranks == 1; break;       // one rank only
    case Route::ScRows:
    case Route::Gather:       // the fused twins (row_fused.h): one rank only, and not under DNM_ROW_FUSE=0
      f.start = A.nranks == 1 && A.row_fuse;
      f.sums = f.start && A.M == A.N && A.left.host.swz == A.right.host.swz;      // x_row is x at the row's own index
      break;
  }
  return f;
}

}  // namespace dnm
