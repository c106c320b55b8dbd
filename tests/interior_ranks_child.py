"""
Child of tests/test_gpu_interior_ranks.py: ONE RANK of a partitioned interior solve, binding the C ABI with ctypes alone
(no torch, no dynamite_amd/backend.py -- the style of tests/native_ranks_child.py).  The 128-byte communicator id comes
through a file; the transport is whatever DNM_RCCL_LIB names (on a one-GPU box: tests/fake_rccl).

    python interior_ranks_child.py CASE.npz RANK WORLD IDFILE OUT.json

The rank builds its handle of the row-block partition (SpinConserve in reference order: column windows), takes the
solver hooks from dnm_comm_hooks and calls dnm_eigsolve_interior ACROSS the rank processes: start vectors keyed by the
global row, the basis size agreed by a max-reduction, every inner product and residual norm summed over the ranks.  It
writes the values, the solver's statistics and -- measured here, with dnm_mat_mult_partitioned and a sum over the ranks --
the residual and the norm of every returned vector.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from dynamite_amd import _lib as B            # signatures and structs only
    assert "torch" not in sys.modules and "dynamite_amd.backend" not in sys.modules
    fn_case, rank, world, idfile, fn_out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    L = C.CDLL(os.path.join(ROOT, "dynamite_amd", "libdynamite_amd.so"))
    for name, (res, args) in B.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    L.dnm_last_error.restype = C.c_char_p

    def ck(rc):
        if rc != 0:
            raise RuntimeError(L.dnm_last_error().decode())
    ck(L.dnm_set_device(0))
    vp = C.c_void_p
    ident = (C.c_char * 128)()
    if rank == 0:
        ck(L.dnm_comm_unique_id(ident))
        with open(idfile + ".tmp", "wb") as f:
            f.write(bytes(ident.raw))
        os.rename(idfile + ".tmp", idfile)
    else:
        t0 = time.time()
        while not os.path.exists(idfile):
            assert time.time() - t0 < 120, "no communicator id"
            time.sleep(0.01)
        ident = (C.c_char * 128).from_buffer_copy(open(idfile, "rb").read())
    comm = vp()
    ck(L.dnm_comm_create(ident, rank, world, C.byref(comm)))

    g = np.load(fn_case, allow_pickle=False)
    Lsp, k, nev, nev_max = int(g["L"]), int(g["k"]), int(g["nev"]), int(g["nev_max"])
    sigma, tol = float(g["sigma"]), float(g["tol"])
    nck = np.ascontiguousarray(g["nck"], dtype=np.int64)
    sub = B.Subspace()
    sub.type, sub.L, sub.k, sub.space = 3, Lsp, k, 0          # SpinConserve, reference order
    sub.ld_nchoosek = Lsp + 1
    sub.nchoosek = nck.ctypes.data_as(B.i64p)
    sub.vec_swizzle = 0
    masks, offs = np.ascontiguousarray(g["masks"]), np.ascontiguousarray(g["mask_offsets"])
    signs, coeffs = np.ascontiguousarray(g["signs"]), np.ascontiguousarray(g["coeffs"])
    dim = int(g["dim"])
    qn, rem = divmod(dim, world)
    nloc = qn + (1 if rank < rem else 0)
    part = B.Partition(rank, world)
    h = vp()
    ck(L.dnm_mat_create(masks.size, B.p64(masks), B.p64(offs), B.p64(signs), coeffs.view(np.float64).ctypes.data_as(B.f64p),
                        C.byref(sub), C.byref(sub), 0, 0, C.byref(part), C.byref(h)))
    if masks.size and masks[0] == 0:
        ck(L.dnm_mat_precompute_diagonal(h, None))
    hooks = B.Hooks()
    ck(L.dnm_comm_hooks(comm, h, None, C.byref(hooks)))

    evecs = vp()
    ck(L.dnm_malloc(C.byref(evecs), 16 * nloc * nev_max))
    work = vp()
    ck(L.dnm_malloc(C.byref(work), 16 * nloc))
    evals = np.zeros(nev_max)
    stats = B.SolverStats()
    ck(L.dnm_eigsolve_interior(h, nloc, nev, sigma, tol, 0, 0, 0, C.byref(hooks), nev_max, B.pf64(evals), evecs,
                               C.byref(stats), None))
    nconv = int(stats.nconv)
    # what was promised, measured by this host: |H v - theta v| and |v| over the ranks
    res, nrm = [], []
    for i in range(nconv):
        v = vp(evecs.value + 16 * nloc * i)
        ck(L.dnm_mat_mult_partitioned(h, comm, v, work, None))
        ck(L.dnm_vec_axpby(work, v, nloc, -float(evals[i]), 0.0, 1.0, 0.0, None))
        two = (C.c_double * 2)()
        d = C.c_double()
        ck(L.dnm_vec_norm2(work, nloc, C.byref(d), None))
        two[0] = d.value ** 2
        ck(L.dnm_vec_norm2(v, nloc, C.byref(d), None))
        two[1] = d.value ** 2
        ck(L.dnm_comm_allreduce(comm, two, 2, 0))
        res.append(float(np.sqrt(two[0])))
        nrm.append(float(np.sqrt(two[1])))
    json.dump({"rank": rank, "nloc": nloc, "reason": int(stats.reason), "nconv": nconv, "its": int(stats.its),
               "matvecs": int(stats.matvecs), "err_est": float(stats.err_est), "evals": [float(e) for e in evals[:nconv]],
               "residuals": res, "norms": nrm}, open(fn_out, "w"))
    ck(L.dnm_comm_forget(comm, h))
    ck(L.dnm_mat_destroy(h))
    ck(L.dnm_comm_destroy(comm))
    return 0


if __name__ == "__main__":
    sys.exit(main())
