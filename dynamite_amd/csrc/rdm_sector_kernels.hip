// Reduced density matrix of a fixed-magnetisation state, block by block.
//
// A state on SpinConserve(L, k) -- or on the XParity half of SpinConserve(L, L/2) -- has a reduced density matrix that
// is a direct sum of blocks rho_n, n = number of set bits among the kept spins:
//   rho_n[i, j] = sum_t psi(a_i, t) conj(psi(a_j, t))
// with a_0 < a_1 < ... the kept configurations of n set bits (ascending = colex order) and t the traced configurations
// of k - n set bits.  Every product state a | t lies inside the subspace: no fetch is masked, none returns zero, and the
// work is sum_n C(kA, n)^2 C(L - kA, k - n) products instead of 4^kA 2^(L - kA) (rdm_kernels.hip).
//
// One kernel serves every block size: the 64 x 64 matrix-core tile of the dense form (rdm_tile.h: rdm_mfma_tile, the
// one piece of code both kernels run) under a gather of its own; rows and columns past a block's dimension are
// zero-filled, so a block of dimension < 64 is one padded tile.  The grid runs over a host-built table of (block, tile row, tile column)
// records, times the slices of the traced index: small blocks ride along with the large ones in one launch.  Slices go
// to the scratch in the format of the dense form ([slice][tile][64 x 64]) and are summed by the same fan-in tree
// (rdm_sum_slices); the finalize kernel takes the lower triangle, mirrors it and makes the diagonal real.
//
// Position of psi(a, t) in x:
//   general `keep`:      Sub<SpinConserve>::rank(deposit(a) | deposit(t)); a is unranked once per workgroup and tile row,
//                        t once per chunk by one lane each
//   keep = [0, kA):      the colex rank separates, rank(a | t << kA) = rank_n(a) + r(t; n), and rank_n(a) is the row
//                        index itself: for a fixed t the rows of the operand are one contiguous run of x -- coalesced
//                        16-byte loads, no per-amplitude ranking, no unranking of kept configurations at all
// XParity(sector s): x holds the representatives (spin L-1 up = bit L-1 clear, the first half of the parent's basis) of
// (|c> + s |~c>) / sqrt 2.  A product state with bit L-1 set is fetched as s * x[rank(~c)], one with the bit clear as
// x[rank(c)]; the factor 1/2 of the two 1/sqrt 2 is applied once, exactly, by the finalize kernel.  On the contiguous
// path the complement reverses the order inside a popcount class: rank(~a) = C(kA, n) - 1 - rank_n(a), the run of x is
// walked downwards.
#include "rdm_tile.h"

namespace dnm {

constexpr int RS_TM = RDM_TM;
constexpr int RS_MST = 1024;             // amplitudes per operand in a staged chunk
constexpr int RS_TK = RS_MST / RS_TM;    // traced configurations per chunk (16: four MFMA steps)

// the idx-th pattern of npos bits with nbits set, in ascending order (Sub<SpinConserve>::i2s on npos positions)
__device__ __forceinline__ uint64_t rs_unrank(int64_t idx, int nbits, int npos, const SubView &s) {
  uint64_t st = 0;
  int j = nbits;
  for (int p = npos; p > 0; --p) {
    const int64_t here = (j > p - 1) ? 0 : s.nchoosek[(int64_t)j * s.ld + (p - 1)];
    st <<= 1;
    if (idx >= here) {
      idx -= here;
      --j;
      st |= 1;
    }
  }
  return st;
}

// r(t; nlow): what the set bits of t, moved up by `shift` positions above nlow lower set bits, add to the colex rank
__device__ __forceinline__ int64_t rs_rank_high(uint64_t t, int shift, int nlow, const SubView &s) {
  int64_t idx = 0;
  int j = nlow;
  while (t) {
    const int p = hd_ctz(t) + shift;
    ++j;
    if (j <= p) idx += s.nchoosek[(int64_t)j * s.ld + p];
    t &= t - 1;
  }
  return idx;
}

template <bool CONTIG, bool XPAR>
__global__ void __launch_bounds__(RDM_NT, DNM_RDM_WAVES)
rdm_sector_mfma_kernel(const c128 *__restrict__ x, const SubView sub, const RdmGeom geo,
                       const RdmSectorBlock *__restrict__ blocks, const RdmSectorTile *__restrict__ tiles, int ntiles,
                       double sector, c128 *__restrict__ partial) {
  constexpr int TM = RS_TM, MST = RS_MST, TK = RS_TK;
  constexpr int EPT = MST / RDM_NT;       // amplitudes per thread and operand in a chunk
  __shared__ c128 As[MST];
  __shared__ c128 Bs[MST];
  __shared__ uint64_t pa[TM], pb[TM];
  // per traced configuration of a chunk: its deposited bits (general) or the start of its run of x (contiguous);
  // pdir: 0 = past the end of the slice, +1, -1 = the run is walked downwards (the complement is stored)
  __shared__ int64_t pts[2][TK];
  __shared__ int pdir[2][TK];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const RdmSectorTile rec = tiles[tile];
  const RdmSectorBlock blk = blocks[rec.blk];
  const bool diag_tile = rec.ti == rec.tj;
  const int64_t D = blk.dim, T = blk.traced;
  const int64_t a0 = (int64_t)rec.ti * TM, b0 = (int64_t)rec.tj * TM;
  const int kA = geo.k, nT = geo.L - geo.k;
  const uint64_t all = geo.L >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << geo.L) - 1);
  if (!CONTIG) {
    if (tid < TM) {
      pa[tid] = a0 + tid < D ? rdm_deposit(rs_unrank(a0 + tid, blk.n, kA, sub), geo.klen, geo.kpos, geo.nseg_keep) : 0;
      pb[tid] = b0 + tid < D ? rdm_deposit(rs_unrank(b0 + tid, blk.n, kA, sub), geo.klen, geo.kpos, geo.nseg_keep) : 0;
    }
    __syncthreads();
  }

  // the slice of this block's traced configurations (a multiple of TK per slice; slices past the end are empty)
  const int64_t tr_begin = (int64_t)blockIdx.y * blk.per_slice;
  int64_t tr_end = tr_begin + blk.per_slice;
  if (tr_end > T) tr_end = T;
  const int64_t c_end = tr_end > tr_begin ? (tr_end - tr_begin + TK - 1) / TK : 0;

  const int rr = tid % TM, t0 = tid / TM;
  const uint64_t par = CONTIG ? 0 : pa[rr], pbr = CONTIG ? 0 : pb[rr];
  const bool arow = a0 + rr < D, brow = !diag_tile && b0 + rr < D;
  auto deposit_chunk = [&](int64_t c) {
    if (tid < TK) {
      const int64_t tr = tr_begin + c * TK + tid;
      int64_t p = 0;
      int d = 0;
      if (tr < tr_end) {
        const uint64_t t = rs_unrank(tr, blk.m, nT, sub);
        d = 1;
        if (CONTIG) {
          if (XPAR && ((t >> (nT - 1)) & 1)) {       // bit L-1 is traced and set: the representative is the complement
            const uint64_t tb = ~t & (((uint64_t)1 << nT) - 1);
            p = rs_rank_high(tb, kA, kA - blk.n, sub) + (D - 1);
            d = -1;
          } else {
            p = rs_rank_high(t, kA, blk.n, sub);
          }
        } else {
          p = (int64_t)rdm_deposit(t, geo.tlen, geo.tpos, geo.nseg_tr);
        }
      }
      pts[c & 1][tid] = p;
      pdir[c & 1][tid] = d;
    }
  };
  auto fetch = [&](uint64_t s) {
    double cf = 1.0;
    if (XPAR && ((s >> (geo.L - 1)) & 1)) {
      s = ~s & all;
      cf = sector;
    }
    const c128 v = x[Sub<DNM_SPIN_CONSERVE>::rank((int64_t)s, sub)];
    return make_double2(v.x * cf, v.y * cf);
  };
  auto gather = [&](int64_t c, c128 (&va)[EPT], c128 (&vb)[EPT]) {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int slot = t0 + i * (RDM_NT / TM);
      const int64_t p = pts[c & 1][slot];
      const int d = pdir[c & 1][slot];
      va[i] = vb[i] = make_double2(0.0, 0.0);
      if (d != 0) {
        if (CONTIG) {
          const double cf = (XPAR && d < 0) ? sector : 1.0;
          if (arow) {
            const c128 v = x[p + d * (a0 + rr)];
            va[i] = make_double2(v.x * cf, v.y * cf);
          }
          if (brow) {
            const c128 v = x[p + d * (b0 + rr)];
            vb[i] = make_double2(v.x * cf, v.y * cf);
          }
        } else {
          if (arow) va[i] = fetch(par | (uint64_t)p);
          if (brow) vb[i] = fetch(pbr | (uint64_t)p);
        }
      }
    }
  };
  rdm_mfma_tile<MST>(As, Bs, diag_tile, c_end, partial + ((int64_t)blockIdx.y * ntiles + tile) * (TM * TM),
                     deposit_chunk, gather);
}

// rho_n = scale * sum over the slices rdm_sum_slices left, mirrored: a tile of the block the table names
__global__ void __launch_bounds__(RDM_NT)
rdm_sector_finalize_kernel(const c128 *__restrict__ partial, const RdmSectorBlock *__restrict__ blocks,
                           const RdmSectorTile *__restrict__ tiles, int ntiles, int nsplit, double scale) {
  const RdmSectorTile rec = tiles[blockIdx.x];
  const RdmSectorBlock blk = blocks[rec.blk];
  rdm_finalize_tile<RS_TM>(partial, ntiles, nsplit, blockIdx.x, rec.ti, rec.tj, blk.dim, scale, (c128 *)blk.out);
}

int rdm_sector_plan(int nblocks, RdmSectorBlock *blocks, int64_t *ntiles, int *nsplit, size_t *table_bytes,
                    size_t *partial_bytes) {
  int64_t nt = 0, maxchunks = 1;
  for (int i = 0; i < nblocks; ++i) {
    const int64_t side = (blocks[i].dim + RS_TM - 1) / RS_TM;
    nt += side * (side + 1) / 2;
    const int64_t ch = (blocks[i].traced + RS_TK - 1) / RS_TK;
    if (ch > maxchunks) maxchunks = ch;
  }
  if (nt < 1 || nt > ((int64_t)1 << 23)) {          // (grid: tiles x 256 threads stays below 2^32)
    set_error("reduced density matrix blocks of %lld tiles in one launch: too many", (long long)nt);
    return 1;
  }
  int64_t ns = (4096 + nt - 1) / nt;          // enough workgroups to fill 256 CUs several times over
  if (ns > maxchunks) ns = maxchunks;
  // DNM_RDM_SECTOR_SLICES: the number of slices of the traced index (slices past a block's end are empty)
  if (const char *e = knob("DNM_RDM_SECTOR_SLICES")) ns = atoll(e);
  if (ns < 1) ns = 1;
  if (ns > 4096) ns = 4096;
  for (int i = 0; i < nblocks; ++i) {
    const int64_t per = (blocks[i].traced + ns - 1) / ns;
    blocks[i].per_slice = (per + RS_TK - 1) / RS_TK * RS_TK;
  }
  *ntiles = nt;
  *nsplit = (int)ns;
  // the two tables at the head of the scratch, then slices + the intermediate levels of the fan-in sum
  size_t tb = (size_t)nblocks * sizeof(RdmSectorBlock) + (size_t)nt * sizeof(RdmSectorTile);
  *table_bytes = (tb + 255) / 256 * 256;
  *partial_bytes = rdm_partial_bytes(ns, nt * (RS_TM * RS_TM));
  return 0;
}

int launch_rdm_sector(const void *x, const SubView &sub, const RdmGeom &geo, bool contig, int xparity_sector,
                      int nblocks, const RdmSectorBlock *blocks, int64_t ntiles, int nsplit, size_t table_bytes,
                      void *scratch, hipStream_t st) {
  std::vector<RdmSectorTile> tiles;
  tiles.reserve((size_t)ntiles);
  for (int i = 0; i < nblocks; ++i) {
    const int32_t side = (int32_t)((blocks[i].dim + RS_TM - 1) / RS_TM);
    for (int32_t ti = 0; ti < side; ++ti)
      for (int32_t tj = 0; tj <= ti; ++tj) tiles.push_back(RdmSectorTile{i, ti, tj, 0});
  }
  if ((int64_t)tiles.size() != ntiles) {
    set_error("internal: sector RDM tile table of %zu records, planned %lld", tiles.size(), (long long)ntiles);
    return 1;
  }
  char *base = (char *)scratch;
  RdmSectorBlock *dblocks = (RdmSectorBlock *)base;
  RdmSectorTile *dtiles = (RdmSectorTile *)(base + (size_t)nblocks * sizeof(RdmSectorBlock));
  c128 *partial = (c128 *)(base + table_bytes);
  DNM_HIP(hipMemcpyAsync(dblocks, blocks, (size_t)nblocks * sizeof(RdmSectorBlock), hipMemcpyHostToDevice, st));
  DNM_HIP(hipMemcpyAsync(dtiles, tiles.data(), tiles.size() * sizeof(RdmSectorTile), hipMemcpyHostToDevice, st));
  DNM_HIP(hipStreamSynchronize(st));          // `tiles` is released on return
  const dim3 grid((unsigned)ntiles, (unsigned)nsplit), wg(RDM_NT);
  const c128 *xp = (const c128 *)x;
  const double sector = (double)xparity_sector;
  const int nt = (int)ntiles;
  if (xparity_sector == 0) {
    if (contig)
      hipLaunchKernelGGL((rdm_sector_mfma_kernel<true, false>), grid, wg, 0, st, xp, sub, geo, dblocks, dtiles, nt, sector, partial);
    else
      hipLaunchKernelGGL((rdm_sector_mfma_kernel<false, false>), grid, wg, 0, st, xp, sub, geo, dblocks, dtiles, nt, sector, partial);
  } else {
    if (contig)
      hipLaunchKernelGGL((rdm_sector_mfma_kernel<true, true>), grid, wg, 0, st, xp, sub, geo, dblocks, dtiles, nt, sector, partial);
    else
      hipLaunchKernelGGL((rdm_sector_mfma_kernel<false, true>), grid, wg, 0, st, xp, sub, geo, dblocks, dtiles, nt, sector, partial);
  }
  void *level = nullptr;
  DNM_TRY(rdm_sum_slices(partial, ntiles * (int64_t)(RS_TM * RS_TM), &nsplit, &level, st));
  hipLaunchKernelGGL(rdm_sector_finalize_kernel, dim3((unsigned)ntiles), wg, 0, st, (const c128 *)level, dblocks,
                     dtiles, nt, nsplit, xparity_sector ? 0.5 : 1.0);
  DNM_HIP(hipGetLastError());
  return 0;
}

}  // namespace dnm
