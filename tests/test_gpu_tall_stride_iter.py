"""The fused Chebyshev step (k_cheb_step_csr, rails_amd/csrc/csr_row_gather.inc: k_spmm_narrow's 24-bit row numbers and unsigned 32-bit byte
offsets) on work panels whose byte extent lies between 2^31 and the guard's 0xffffff00 (cheb_coef.h: rails_cheb_fused_eligible).  The
iterative object's work panels are 32 columns wide whatever the solve's width, so rows alone reach the line: the 1-D Laplacian
tridiag(-1, 2, -1) on 9,000,000 rows has work panels of 9e6 x 32 x 8 = 2.304e9 bytes, and rows from 8,388,608 on are gathered at byte
offsets of 2^31 and more.  A signed intermediate in that arithmetic would go wrong there while the guard still says yes.

`precondition` with poly_degree 2 on two columns, fused and unfused (stats()["fused_launches"] says which ran), against
tests/cheb_reference.py evaluated in longdouble.  The bound is the one tests/test_gpu_iter_poly.py::test_precondition_against_longdouble
derives, computed here for this operator: per column 4 times the float64 restatement's error against longdouble, at least
64 eps ||z||_inf.

Measured on an MI355X machine: 5.1 s for the test, of which 3.9 s are the host's (the matrix, the longdouble and the float64 restatement on
9e6 x 2) and 1.1 s the device part; largest error / allowed error 0.059 (bound 4.57e-14), fused and unfused alike.  That is not under
5 s, so the second case the shapes allow -- 2^24 - 2 rows, 256 bytes below the guard -- is not run; the host test pins that shape against
the header."""
import time

import numpy as np
import pytest

import cheb_reference as C
import iter_reference as R
import tall_stride_cases as T
import tall_stride_device as D

pytestmark = pytest.mark.gpu

RATIO, DEGREE = 30.0, 2
EPS = np.finfo(float).eps


def test_precondition_on_work_panels_past_2_gib():
    import scipy.sparse as sp

    import rails_amd

    m, nc = T.ITER_M, 2
    assert T.TWO31 < T.panel_bytes(m, T.ITER_LD) < T.LEAN_LIMIT and T.cheb_fused_allowed(m)
    t0 = time.time()
    A = sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")
    g = C.g_of(A, True)
    hi = C.gershgorin(A, g)
    Xm = R.rhs(m, nc, seed=9)
    Zl = C.polynomial(A, Xm, DEGREE, hi, RATIO, g, dtype=np.longdouble)
    Z64 = C.polynomial(A, Xm, DEGREE, hi, RATIO, g)
    bound = np.maximum(4 * np.abs(Z64 - Zl).max(0), 64 * EPS * np.abs(Zl).max(0)).astype(float)
    t_host = time.time() - t0
    with D.context(seed=3) as ctx:
        t0 = time.time()
        inv = rails_amd.IterativeInverse(ctx, A, method="cg", poly_degree=DEGREE, poly_ratio=RATIO)
        try:
            X = D.MV(ctx, data=Xm)
            got = {}
            for fused in (1, 0):
                inv.set("poly_fused", fused)
                Z = inv.precondition(X).to_host()
                st = inv.stats()
                assert st["poly_applications"] == 1 and st["products"] == DEGREE
                assert st["fused_launches"] == (DEGREE if fused else 0), (fused, st)
                assert abs(st["eig_hi"] - hi) <= 4 * EPS * hi
                err = np.abs(Z - Zl).astype(float)
                ratio = err.max(0) / bound
                rows = np.argmax(err, axis=0)
                print("fused %d: largest error / allowed error %.3f (bound %.3e), at rows %s; rows from %d on lie past 2^31 bytes" % (
                    fused, ratio.max(), bound.max(), rows, T.TWO31 // (T.ITER_LD * 8)))
                assert np.all(err <= bound[None, :]), (fused, ratio)
                got[fused] = Z
            assert np.all(np.abs(got[1] - got[0]) <= bound[None, :])
            assert np.array_equal(X.to_host(), Xm)
        finally:
            inv.close()
        print("host reference %.1f s, device part %.1f s" % (t_host, time.time() - t0))
