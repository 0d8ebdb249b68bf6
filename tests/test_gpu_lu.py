"""The device sparse LU solve (include/rails_hip.h: rails_lu_*, rails_amd/csrc/splu.hip; rails_amd.SparseLU) against scipy's
splu(...).solve on the host: random nonsymmetric matrices, the MATLAB tests' laplacian2, the bordered MOC matrix; both transposes,
several widths; the restriction to a subsystem (a Schur complement's inverse) and the operator handle."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import generalized_problems as G
from moc_problem import add_border, load

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 16, 17, 32, 40)


def random_dd(n, seed):
    """nonsymmetric, diagonally dominant, about 5 nonzeros per row off the diagonal"""
    g = np.random.default_rng(seed)
    R = sp.random(n, n, density=min(1.0, 5.0 / n), random_state=seed, format="csr")
    R.data = g.uniform(-1.0, 1.0, R.data.size)
    d = np.asarray(abs(R).sum(axis=1)).ravel() + 1.0
    return (R + sp.diags(d * np.where(g.random(n) < 0.5, -1.0, 1.0))).tocsr()


def moc_matrix():
    A, mdiag, B = load()
    A2, _, _ = add_border(A, mdiag, B)
    return sp.csr_matrix(A2)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


def check_solves(ctx, A, tol, seed=0):
    import rails_amd

    lu = rails_amd.SparseLU(ctx, A)
    n = A.shape[0]
    g = np.random.default_rng(seed)
    for trans in (False, True):
        for nc in WIDTHS:
            X = g.uniform(-1.0, 1.0, (n, nc))
            Xd = rails_amd.HipMultiVectorWrapper(ctx, data=X)
            Y = lu.solve(Xd, trans=trans).to_host()
            ref = lu.lu.solve(np.asfortranarray(X), trans="T" if trans else "N")
            err = np.linalg.norm(Y - ref) / np.linalg.norm(ref)
            assert err <= tol, (n, trans, nc, err)
            np.testing.assert_array_equal(Xd.to_host(), X)  # the input panel is unchanged
    st = lu.stats()
    assert st["n"] == n and st["launches"] >= 2 and min(st[k] for k in ("levels_L", "levels_U", "levels_Ut", "levels_Lt")) >= 1
    lu.close()


@pytest.mark.parametrize("n", [1, 2, 7, 100, 1000, 5000])
def test_random_matrices(ctx, n):
    check_solves(ctx, random_dd(n, seed=n), 1e-12, seed=n)


def test_laplacian2_64x64(ctx):
    check_solves(ctx, G.laplacian2(64 * 64), 1e-12)


def test_bordered_moc_matrix(ctx):
    # the MOC Jacobian is ill-conditioned (cond ~1e8 by the 1-norm estimate): the device and host triangular solves, which sum in
    # different orders, agree to ~cond * eps relative, so 1e-10 here
    check_solves(ctx, moc_matrix(), 1e-10)


def test_columns_are_independent_bitwise(ctx):
    """column j of a 32-column solve is bitwise the one-column solve of column j (each column is computed by the same operations)"""
    import rails_amd

    A = G.laplacian2(64 * 64)
    lu = rails_amd.SparseLU(ctx, A)
    X = np.random.default_rng(5).uniform(-1.0, 1.0, (A.shape[0], 32))
    for trans in (False, True):
        Y = lu.solve(rails_amd.HipMultiVectorWrapper(ctx, data=X), trans=trans).to_host()
        for j in (0, 1, 17, 31):
            y = lu.solve(rails_amd.HipMultiVectorWrapper(ctx, data=X[:, j:j + 1]), trans=trans).to_host()
            assert np.array_equal(Y[:, j:j + 1], y), (trans, j)
    lu.close()


def test_operator_handle(ctx):
    """the LU as an operator: rails_spmm on the handle (both transposes) and HipOperatorWrapper.apply give the solve"""
    import rails_amd

    A = random_dd(700, seed=3)
    lu = rails_amd.SparseLU(ctx, A)
    X = np.random.default_rng(1).uniform(-1.0, 1.0, (700, 5))
    Xd = rails_amd.HipMultiVectorWrapper(ctx, data=X)
    for trans in (0, 1):
        Y = rails_amd.HipMultiVectorWrapper(ctx, 700, 5)
        assert ctx.lib.rails_spmm(ctx.h, lu.op.h.h, trans, Xd.panel.h, 0, 5, Y.panel.h, 0) == 0
        ref = lu.lu.solve(np.asfortranarray(X), trans="T" if trans else "N")
        assert np.linalg.norm(Y.to_host() - ref) <= 1e-12 * np.linalg.norm(ref)
    Y = lu.op.apply(Xd).to_host()
    assert np.linalg.norm(Y - lu.lu.solve(np.asfortranarray(X))) <= 1e-12 * np.linalg.norm(Y)
    assert ctx.lib.rails_csr_rows(lu.op.h.h) == 700
    assert ctx.lib.rails_csr_set_halo(lu.op.h.h, 0, None, 0, rails_amd._lib.HALO_FN(0), None) != 0  # single GPU only
    lu.close()


def test_restriction_and_schur_inverse(ctx):
    """rows = idx2 gives x -> (A^-1 E x)[idx2]; on MOC, SchurOperator.inverse() times S.dense() is the identity"""
    import rails_amd
    from rails_amd.schur import SchurOperator

    A, mdiag, B = load()
    A2, m2, B2 = add_border(A, mdiag, B)
    A2 = sp.csr_matrix(A2)
    S = SchurOperator(ctx, (A2.indptr.astype(np.int64), A2.indices.astype(np.int32), A2.data.astype(np.float64)), m2, tol=1e-12)
    Sinv = S.inverse()
    assert Sinv.m == S.m2
    Sd = S.dense()
    # cond(S) is 1.9e7 here: scipy's own splu(A).solve on the host leaves 1.4e-10 in Sinv S - I and 4.4e-9 in Sinv' S' - I (measured);
    # the device solve 1.3e-10 and 1.8e-9
    P = Sinv.solve_host(Sd)
    assert np.abs(P - np.eye(S.m2)).max() < 3e-10, np.abs(P - np.eye(S.m2)).max()
    Pt = Sinv.solve_host(Sd.T, trans=True)
    assert np.abs(Pt - np.eye(S.m2)).max() < 1e-8, np.abs(Pt - np.eye(S.m2)).max()
    # the same restriction on a random matrix, against the dense definition
    Ar = random_dd(300, seed=9)
    rows = np.sort(np.random.default_rng(2).choice(300, 120, replace=False))
    lu = rails_amd.SparseLU(ctx, Ar, rows=rows)
    X = np.random.default_rng(3).uniform(-1.0, 1.0, (120, 4))
    E = np.zeros((300, 4))
    E[rows] = X
    for trans in (False, True):
        ref = (np.linalg.solve(Ar.toarray().T if trans else Ar.toarray(), E))[rows]
        assert np.linalg.norm(lu.solve_host(X, trans=trans) - ref) <= 1e-12 * np.linalg.norm(ref)
    lu.close()
    Sinv.close()
