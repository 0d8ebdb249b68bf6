"""The extended Krylov projection ("Projection method" 2.2) with the iterative A^-1 operator preconditioned by its multigrid V-cycle
(IterativeInverse(amg=True)): the acceptance problem of tests/test_gpu_iter_projection.py -- the MATLAB tests' Laplace 256 with a diagonal
M under the reference's own four bounds (test_Laplace.m:39-42) -- holds the same bounds as with Jacobi alone, and the inverse takes a
fraction of the inner iterations."""
import pytest

import generalized_problems as G

pytestmark = pytest.mark.gpu


def run(amg):
    import rails_amd

    A, Md, B, params, bound, seed = G.build("Laplace_256")
    ctx = rails_amd.Context(device=0, seed=seed)
    op = rails_amd.HipOperatorWrapper(ctx, *G.csr(A))
    mop = rails_amd.HipOperatorWrapper(ctx, *G.diag_csr(Md))
    s = rails_amd.Solver(ctx, op, B, M=mop)
    s.set_option("verbose", 0)
    s.set_option("mass", 1)
    inv = rails_amd.IterativeInverse(ctx, G.csr(A), method="cg", tol=1e-10, amg=amg, amg_coarse=32)  # 256 rows: 32 leaves a level
    s.set_inverse(inv)
    assert s.set_parameters({**params, "Projection method": 2.2}) == 0
    code, V, T = s.solve()
    assert code == 0
    G.check_acceptance(A, Md, B, V, T, abs(s.history()[-1]), s.trips(), bound)  # true residual below 1e-4, trips below n - 10
    trips, st, info = s.trips(), inv.stats(), inv.amg_info()
    s.close()
    inv.close()
    ctx.close()
    return trips, st, info


def test_acceptance_laplace_256_with_the_multigrid_cycle():
    trips0, st0, info0 = run(False)
    trips1, st1, info1 = run(True)
    print("method 2.2, cg: Jacobi: %d trips, %d inner iterations, %d products; multigrid (rows %s): %d trips, %d inner iterations, %d products" % (
        trips0, st0["total_iterations"], st0["total_products"], info1["rows"], trips1, st1["total_iterations"], st1["total_products"]))
    assert st0["total_flagged_columns"] == 0 and st1["total_flagged_columns"] == 0
    assert info0["levels"] == 0 and info1["levels"] >= 2 and info1["cycles"] > 0
    # both inverses are A^-1 to 1e-10: the outer iteration cannot tell them apart by more than a trip
    assert abs(trips1 - trips0) <= 1
    assert st1["total_iterations"] < 0.5 * st0["total_iterations"]
