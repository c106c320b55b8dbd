// Host-side builder of the tiled kernel's records (passes.cpp): the operator in index-space form, then per pass of the
// plan a PassOnDevice (mat.h) -- generic form first, flip-flop form once the operator's bonds are decided.
#pragma once

#include "mat.h"

namespace dnm {

int build_opform(const dnm_mat &A, OpForm *op);
int pack_opform(OpForm *op);
int build_pass(const dnm_mat &A, const PassSpec &ps, PassOnDevice *out);
void decide_flip_bonds(dnm_mat *A);      // after every build_pass of the handle
int build_flip_pass(const dnm_mat &A, const PassSpec &ps, PassOnDevice *out);
int build_diag_tables(const dnm_mat &A, PassOnDevice *out);      // last: on the form of the pass that the kernel runs on

}  // namespace dnm
