// The subspace maps (submap_kernels.hip): a state moved from one subspace to another on the device -- embed, restrict,
// into and out of an XParity sector -- and the weight of a state per magnetisation sector and per flip sector.
// Definitions and index arithmetic: submap_rank.h.
#pragma once
#include <type_traits>

#include "kernels.h"
#include "submap_rank.h"

namespace dnm {

constexpr int SUBMAP_NT = 256;                // threads of a workgroup
constexpr int SUBMAP_RUN = 4;                 // SpinConserve targets: adjacent rows a thread unranks once and steps through
constexpr int SUBMAP_ROWS_PER_WG_LOG2 = 10;   // workgroups = ceil(target rows / 2^10), at most SUBMAP_MAX_WG, at least one
constexpr int64_t SUBMAP_MAX_WG = 4096;
constexpr int SW_ROWS_PER_WG = 1024;          // sector weights: adjacent rows (or pairs) a workgroup takes at a time
constexpr int64_t SW_MAX_WG = 2048;

// What a launch of the map is made with: host arithmetic from the two descriptors and sectors alone.
struct SubmapPlan {
  SubmapSide src, dst;             // (tables: whatever the views handed to submap_plan point to)
  int32_t mode, run, nwg;          // SUBMAP_COPY ...; rows of a thread's run; workgroups
  int32_t ntab_src, ntab_dst;      // entries of the binomial tables staged in LDS (SpinConserve sides)
  size_t lds_bytes;
};
int submap_plan(const SubView &src, int src_xsec, const SubView &dst, int dst_xsec, SubmapPlan *p);

// y = the map of x (device, distinct); p.src.v / p.dst.v carry device tables
int launch_submap(const void *x, void *y, const SubmapPlan &p, hipStream_t st);

// What a launch of the sector weights is made with
struct SectorWeightsPlan {
  SubmapSide side;
  int32_t pairs;                   // the rows are taken as pairs (i, dim - 1 - i): the flip sums come with the bins
  int32_t ncols, nwg;              // L + 1 magnetisation bins, F+, F-; workgroups
  int64_t items;                   // rows, or pairs
  size_t lds_bytes, partial_bytes;
};
int sector_weights_plan(const SubView &v, int xsec, SectorWeightsPlan *p);
// out (device, p.ncols doubles) = [popcount bins 0..L | F+ | F-]; partial: p.partial_bytes
int launch_sector_weights(const void *x, const SectorWeightsPlan &p, void *partial, void *out, hipStream_t st);

// f(integral_constant<int, type>) for a subspace type; -1 for an unknown one
template <class F>
static inline int submap_dispatch1(int type, F f) {
  switch (type) {
    case DNM_FULL: return f(std::integral_constant<int, DNM_FULL>{});
    case DNM_PARITY: return f(std::integral_constant<int, DNM_PARITY>{});
    case DNM_EXPLICIT: return f(std::integral_constant<int, DNM_EXPLICIT>{});
    case DNM_SPIN_CONSERVE: return f(std::integral_constant<int, DNM_SPIN_CONSERVE>{});
  }
  return -1;
}
// f(source type, target type)
template <class F>
static inline int submap_dispatch(int stype, int dtype, F f) {
  return submap_dispatch1(stype, [&](auto S) { return submap_dispatch1(dtype, [&](auto D) { return f(S, D); }); });
}

}  // namespace dnm
