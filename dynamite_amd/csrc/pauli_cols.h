// Column arithmetic of the two-spin Pauli pass (pauli_kernels.hip, dnm_pauli_partner_indices), for host and device alike
// -- tests/pauli_cols_check.cpp runs these very functions under the sanitizers.
//
// A column is a pair (site j, kind): 1 flips the spin (sigma-x), 2 flips it and takes the sign (sigma-y up to -i),
// 3 takes the sign (sigma-z).  With s_j(r) = (-1)^(bit j of r):
//   (sigma-x_j psi)(r) = psi(r ^ e_j),   (sigma-z_j psi)(r) = s_j(r) psi(r),   (sigma-y_j psi)(r) = -i s_j(r) psi(r ^ e_j)
// so column c of the operand matrix is A[q, 1 + c] = (-1)^(g_c bit j_c of r_c(q)) x[q ^ m_c] with f = flips, g = signs.
//
// Full: the index is the configuration, r_c(q) = q and m_c = f_c << j_c.
// Parity(space): the index is the configuration without site 0, m_c = (f_c << j_c) >> 1 -- a flip of site 0 pairs a row
// with the amplitude at its own index.  A flip leaves the sector: the rows of a flipping column are the configurations
// of the opposite sector, (q << 1) | (par(q) ^ space ^ 1), those of a column that does not flip the sector's own,
// (q << 1) | (par(q) ^ space).  (Products of a flipping and a non-flipping column pair rows of two different sectors;
// their expectation values vanish by symmetry and the caller writes those entries of G as zeros.)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define DNM_PAULI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DNM_PAULI_HD inline
#endif

namespace dnm {

constexpr int PAULI_X = 1, PAULI_Y = 2, PAULI_Z = 3;

DNM_PAULI_HD bool pauli_flips(int kind) { return kind == PAULI_X || kind == PAULI_Y; }
DNM_PAULI_HD bool pauli_signs(int kind) { return kind == PAULI_Y || kind == PAULI_Z; }

// the XOR mask in index space that takes a row to the row of its partner amplitude
DNM_PAULI_HD uint64_t pauli_index_mask(bool parity, int site, int kind) {
  if (!pauli_flips(kind)) return 0;
  const uint64_t m = (uint64_t)1 << site;
  return parity ? m >> 1 : m;
}

// the configuration whose bits a column reads for its sign at index idx: par = popcount(idx) & 1 (Parity)
DNM_PAULI_HD uint64_t pauli_row_config(bool parity, int space, uint64_t idx, int par, bool flips) {
  if (!parity) return idx;
  return (idx << 1) | (uint64_t)((par ^ space ^ (flips ? 1 : 0)) & 1);
}

// the factor of the column is -1
DNM_PAULI_HD bool pauli_negative(uint64_t cfg, int site, int kind) {
  return pauli_signs(kind) && ((cfg >> site) & 1);
}

}  // namespace dnm
