"""rails_orthogonalize_range and rails_panel_colnorms2 (include/rails_hip.h, rails_amd/csrc/orth.hip, dense_gram.hip): the rank-revealing
orthonormal range basis of a start space against a longdouble in-order Gram-Schmidt with two passes that drops a column of which less
than 1e-8 survives -- the reference's Morth, matlab/RAILSsolver.m:567-580.

Inputs: m = 1037 rows (no multiple of 16 or 64), Gaussian columns scaled by exp(U(-3, 3)), [N, V_old] from a QR factorisation, and
dependent columns planted by construction: column 1 = 3 x column 0, column 4 = 0, column 20 inside span(N), column 21 inside
span(V_old), column 130 = column 2 - 2 column 100 + a vector of span([N V_old]) (across the 128-column block boundary), column 260 =
column 129 + column 7, the last column = -1e-3 x its predecessor.  On these inputs the reference drops exactly the planted columns;
every dropped column keeps at most 1e-16 of its length and every kept one at least 0.14, so no case sits near the threshold.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(1037, 1, 0, 0), (1037, 5, 0, 0), (1037, 33, 7, 0), (1037, 129, 0, 3), (1037, 300, 7, 3), (1037, 300, 0, 0), (523, 512, 0, 3)]


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1234)
    yield c
    c.close()


def MV(ctx, data=None, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=data, **kw)


def build(m, w, k_old, q, seed):
    r = np.random.default_rng(seed)
    P = np.linalg.qr(r.standard_normal((m, q + k_old)))[0]
    W = r.standard_normal((m, w)) * np.exp(r.uniform(-3, 3, w))  # column scales over e^6
    dep = []

    def setdep(j, vec):
        if j < w:
            W[:, j] = vec
            dep.append(j)

    if w > 1:
        setdep(1, 3.0 * W[:, 0])  # scaled copy of its neighbour
    if w > 4:
        setdep(4, np.zeros(m))  # zero column
    if w > 20 and q:
        setdep(20, P[:, :q] @ r.standard_normal(q))  # inside the nullspace
    if w > 21 and k_old:
        setdep(21, P[:, q:] @ r.standard_normal(k_old))  # inside the old columns
    if w > 130:
        setdep(130, W[:, 2] - 2 * W[:, 100] + (P @ r.standard_normal(q + k_old) if q + k_old else 0))  # across a 128 block
    if w > 260:
        setdep(260, W[:, 129] + W[:, 7])
    if w > 299:
        setdep(w - 1, W[:, w - 2] * -1e-3)
    return P, W, sorted(set(dep))


def mgs_ref(P, W, tol=1e-8):
    """in-order Gram-Schmidt in longdouble: unit length, two passes against [P, kept], drop below tol"""
    Q = P.astype(np.longdouble).copy()
    kept, res = [], []
    for j in range(W.shape[1]):
        v = W[:, j].astype(np.longdouble)
        n0 = np.sqrt(v @ v)
        if n0 == 0:
            res.append(0.0)
            continue
        v = v / n0
        for _ in range(2):
            v = v - Q @ (Q.T @ v)
        n1 = float(np.sqrt(v @ v))
        res.append(n1)
        if n1 < tol:
            continue
        Q = np.hstack([Q, (v / n1)[:, None]])
        kept.append(j)
    return kept, np.array(res)


_REFERENCE = {}


def reference(case):
    """(P, W, planted, kept, surviving fractions) of a case, computed once and handed out read-only"""
    if case not in _REFERENCE:
        m, w, k_old, q = case
        P, W, dep = build(m, w, k_old, q, 5)
        kept, res = mgs_ref(P, W)
        for a in (P, W, res):
            a.setflags(write=False)
        _REFERENCE[case] = (P, W, dep, kept, res)
    return _REFERENCE[case]


def run_range(ctx, P, W, k_old, q, tol=0.0):
    """V = [V_old, W] with the watermark at k_old, N = the first q columns of P in a panel of its own (at an offset, to exercise nc0)"""
    w = W.shape[1]
    Vold = P[:, q:]
    X = MV(ctx, np.hstack([Vold, W]), capacity=k_old + w + 5)
    X.orthogonalized = k_old
    N = None
    if q:
        Nfull = MV(ctx, np.hstack([np.full((P.shape[0], 2), 7.0), P[:, :q]]))
        N = Nfull.view(2, 2 + q - 1) if q > 1 else Nfull.view(2)
    kept, idx = X.orthogonalize_range(N, tol)
    assert X.n == k_old + kept and X.orthogonalized == X.n
    full = X._alias(0, k_old + w, True).to_host()  # the whole window, tail included
    Nh = Nfull.to_host() if q else None
    return kept, idx, full, Nh


def check_basis(P, W, k_old, q, kept_ref, kept, idx, full, Nh):
    w = W.shape[1]
    assert list(idx) == kept_ref and kept == len(kept_ref)
    Q = full[:, k_old:k_old + kept]
    eye = np.eye(kept)
    print("orthonormality %.2e" % np.abs(Q.T @ Q - eye).max())
    assert np.abs(Q.T @ Q - eye).max() < 1e-13
    if q + k_old:
        print("against [N V_old] %.2e" % np.abs(P.T @ Q).max())
        assert np.abs(P.T @ Q).max() < 1e-13
    Wp = W - P @ (P.T @ W)
    print("span %.2e of %.2e" % (np.abs(Wp - Q @ (Q.T @ Wp)).max(), np.abs(W).max()))
    assert np.abs(Wp - Q @ (Q.T @ Wp)).max() <= 1e-10 * np.abs(W).max()
    # in-order semantics: Q' Wp restricted to the kept columns is upper triangular with a positive diagonal
    R = Q.T @ Wp[:, kept_ref]
    norms = np.linalg.norm(Wp[:, kept_ref], axis=0)
    assert np.all(np.diag(R) > 0)
    print("below the diagonal %.2e" % (np.abs(np.tril(R, -1)) / norms).max())
    assert (np.abs(np.tril(R, -1)) / norms).max() <= 1e-10
    # the tail is exactly zero; the old columns and N are bitwise unchanged
    assert np.all(full[:, k_old + kept:k_old + w] == 0.0)
    assert np.array_equal(full[:, :k_old], P[:, q:])
    if q:
        assert np.array_equal(Nh[:, 2:], P[:, :q]) and np.all(Nh[:, :2] == 7.0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "m%d-w%d-k%d-q%d" % c)
def test_range_basis_matches_longdouble_gram_schmidt(ctx, case):
    m, w, k_old, q = case
    P, W, dep, kept_ref, res = reference(case)
    # the reference itself: exactly the planted columns go, and nothing sits near the threshold
    dropped = [j for j in range(w) if j not in kept_ref]
    assert dropped == dep
    assert all(res[j] <= 1e-16 for j in dropped) and all(res[j] >= 0.14 for j in kept_ref)
    kept, idx, full, Nh = run_range(ctx, P, W, k_old, q)
    check_basis(P, W, k_old, q, kept_ref, kept, idx, full, Nh)


def test_nearly_dependent_columns_are_kept(ctx):
    """column j = column j-1 + 1e-6 |column j-1| u, u a random unit vector: about 1e-6 survives, two decades above the threshold and one
    below what the Gram matrix can decide (1e-5) -- the second stage of the rank decision keeps it"""
    g = np.random.default_rng(11)
    m, w = 1037, 140
    W = g.standard_normal((m, w)) * np.exp(g.uniform(-3, 3, w))
    for j in (5, 17, 129):
        u = g.standard_normal(m)
        u /= np.linalg.norm(u)
        W[:, j] = W[:, j - 1] + 1e-6 * np.linalg.norm(W[:, j - 1]) * u
    P = np.zeros((m, 0))
    kept_ref, res = mgs_ref(P, W)
    assert kept_ref == list(range(w))
    assert all(3e-7 < res[j] < 3e-6 for j in (5, 17, 129))
    kept, idx, full, _ = run_range(ctx, P, W, 0, 0)
    assert kept == w and list(idx) == kept_ref
    Q = full[:, :w]
    print("orthonormality %.2e" % np.abs(Q.T @ Q - np.eye(w)).max())
    assert np.abs(Q.T @ Q - np.eye(w)).max() < 1e-13
    assert np.abs(W - Q @ (Q.T @ W)).max() <= 1e-10 * np.abs(W).max()


@pytest.fixture(scope="module")
def norms_input():
    g = np.random.default_rng(3)
    X = g.standard_normal((1037, 520)) * np.exp(g.uniform(-3, 3, 520))
    X.setflags(write=False)
    return X, np.sum(X.astype(np.longdouble) ** 2, 0)


@pytest.mark.parametrize("c0", [0, 3])
@pytest.mark.parametrize("nc", [1, 17, 512])
def test_colnorms2(ctx, norms_input, c0, nc):
    X, ref = norms_input
    a = MV(ctx, X)
    v = a.view(c0, c0 + nc - 1) if nc > 1 else a.view(c0)
    n1 = v.colnorms2()
    n2 = v.colnorms2()
    assert n1.shape == (nc,)
    assert np.array_equal(n1, n2)  # every order of summation is fixed
    np.testing.assert_allclose(n1, ref[c0:c0 + nc].astype(np.float64), rtol=1e-14, atol=0)
    assert np.array_equal(a.to_host(), X)


def test_argument_errors(ctx):
    import rails_amd

    lib = ctx.lib
    g = np.random.default_rng(4)
    X = g.standard_normal((100, 6))
    a, short = MV(ctx, X, capacity=8), MV(ctx, g.standard_normal((99, 2)))
    kept = C.c_int(-5)
    out = np.zeros(16)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    calls = {
        "window outside the capacity": lambda: lib.rails_orthogonalize_range(ctx.h, a.panel.h, 4, 5, None, 0, 0, 0.0, C.byref(kept), None),
        "N == V": lambda: lib.rails_orthogonalize_range(ctx.h, a.panel.h, 2, 4, a.panel.h, 0, 2, 0.0, C.byref(kept), None),
        "row mismatch": lambda: lib.rails_orthogonalize_range(ctx.h, a.panel.h, 0, 6, short.panel.h, 0, 2, 0.0, C.byref(kept), None),
        "nullspace window": lambda: lib.rails_orthogonalize_range(ctx.h, a.panel.h, 0, 6, short.panel.h, 1, 2, 0.0, C.byref(kept), None),
        "norms outside the capacity": lambda: lib.rails_panel_colnorms2(ctx.h, a.panel.h, 5, 4, dp),
    }
    for what, call in calls.items():
        assert call() == -1, what  # RAILS_EINVAL
        assert lib.rails_last_error(), what
        assert np.array_equal(a.to_host(), X), what
    with pytest.raises(rails_amd.RailsError):
        b = MV(ctx, X, capacity=8)
        b.orthogonalize_range(short)
