"""matlab/test/test_MOC.m:38-63 (test_MOC_inv): the bordered MOC ocean model on its Schur complement, solved with the extended
Krylov projection ("Projection method" 2.2) and Ainv = Sinv (RAILSschur.m:60-64; here SchurOperator.inverse(), a device sparse LU of the
full bordered matrix restricted to the Schur rows), with the reference's two Frobenius residual checks -- and fewer trips than
method 1 from the same seed."""
import numpy as np
import pytest

from moc_problem import add_border, load, schur_dense

pytestmark = pytest.mark.gpu

PARAMS = {"Maximum iterations": 1000, "Tolerance": 1e-3, "Expand size": 3, "Lanczos iterations": 10}


@pytest.mark.parametrize("subspace", [1, 0])
def test_moc_inverse_projection(subspace):
    import rails_amd
    from rails_amd.schur import SchurOperator

    A, mdiag, B = load()
    n = A.shape[0]
    A2, m2, B2 = add_border(A, mdiag, B)
    Sd, ms, BSd, i1, i2 = schur_dense(A2, m2, B2)
    trips = {}
    for method in (1.0, 2.2):
        ctx = rails_amd.Context(device=0, seed=1)
        S = SchurOperator(ctx, (A2.indptr.astype(np.int64), A2.indices.astype(np.int32), A2.data.astype(np.float64)), m2, tol=1e-12)
        BS = S.restrict(B2)
        Mop = rails_amd.HipOperatorWrapper(ctx, np.arange(S.m2 + 1, dtype=np.int64), np.arange(S.m2, dtype=np.int32), S.mass22)
        s = rails_amd.Solver(ctx, S.op, BS, M=Mop)
        Sinv = S.inverse()
        s.set_inverse(Sinv)
        assert s.set_parameters({**PARAMS, "Projection method": method}) == 0
        s.set_option("verbose", 0)
        s.set_option("mass", 1)
        s.set_option("subspace", subspace)
        code, V, T = s.solve()
        assert code == 0
        trips[method] = s.trips()
        X = V @ T @ V.T
        R = Sd @ X * ms[None, :] + (ms[:, None] * X) @ Sd.T + BSd @ BSd.T  # test_MOC.m:54-55
        assert np.linalg.norm(R) < 1e-3, (method, np.linalg.norm(R))
        Vf = S.prolongate(V)[:n]  # test_MOC.m:57-61
        Xf = Vf @ T @ Vf.T
        Ad = A.toarray()
        Rf = Ad @ Xf * mdiag[None, :] + (mdiag[:, None] * Xf) @ Ad.T + B @ B.T
        assert np.linalg.norm(Rf) < 1e-3, (method, np.linalg.norm(Rf))
        s.close()
        Sinv.close()
        ctx.close()
    print("MOC trips (%s back end): method 1: %d, method 2.2: %d" % ("coordinate-space" if subspace else "direct", trips[1.0], trips[2.2]))
    assert trips[2.2] < trips[1.0], trips
