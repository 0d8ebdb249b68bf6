"""rails_orthogonalize_deflated (orth.hip): the block orthogonalisation with a nullspace N projected out in every round, against numpy.

Bounds: a full-rank block equals numpy's QR of (I - [N V][N V]') W (signs fixed by a positive diagonal of R) to 1e-12; every path --
block, repair round, column-wise -- leaves ||[N V_old]' W|| and ||W'W - I|| (largest entry) below 1e-13 at m = 1000.  At m = 1M the
same quantities carry the rounding of sums over a million rows, in the kernels and in numpy's check alike: 5e-15 sqrt(m), the scaling
tests/test_gpu_kernels.py uses for rails_orthogonalize."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=4321)
    yield c
    c.close()


def MV(ctx, data, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=data, **kw)


def orth_bound(m):
    return max(1e-13, 5e-15 * np.sqrt(m))


def basis(g, m, k):
    return np.linalg.qr(g.uniform(-1, 1, (m, k)))[0] if k else np.zeros((m, 0))


def run(ctx, Vold, W, N, method=0):
    k_old, w = Vold.shape[1], W.shape[1]
    X = MV(ctx, np.hstack([Vold, W]), capacity=k_old + w)
    X.orthogonalized = k_old
    Nm = MV(ctx, N) if N is not None and N.shape[1] else None
    used = X.orthogonalize_deflated(Nm, method)
    return X.to_host()[:, k_old:], used


def reference(Vold, W, N):
    L = np.hstack([N, Vold])
    Q, R = np.linalg.qr(W - L @ (L.T @ W))
    return Q * np.sign(np.diag(R))[None, :]


def check(Q, Vold, N, m):
    L = np.hstack([N, Vold])
    assert np.all(np.isfinite(Q))
    assert np.abs(L.T @ Q).max() <= orth_bound(m)
    assert np.abs(Q.T @ Q - np.eye(Q.shape[1])).max() <= orth_bound(m)


@pytest.mark.parametrize("k_old", [0, 1, 64, 300])
@pytest.mark.parametrize("q", [1, 4, 16, 32, 40])
@pytest.mark.parametrize("w", [1, 3, 16, 17, 33])
def test_full_rank_blocks_match_numpy(ctx, k_old, q, w):
    m = 1000
    g = np.random.default_rng(1000 * k_old + 10 * q + w)
    NV = basis(g, m, q + k_old)
    N, Vold = NV[:, :q], NV[:, q:]
    W = g.uniform(-1, 1, (m, w))
    Q, used = run(ctx, Vold, W, N)
    assert used in (1, 2, 3)
    np.testing.assert_allclose(Q, reference(Vold, W, N), rtol=0, atol=1e-12)
    check(Q, Vold, N, m)


@pytest.mark.parametrize("k_old,q,w", [(0, 4, 17), (64, 1, 16), (300, 16, 17), (64, 40, 33)])
def test_full_rank_blocks_at_a_million_rows(ctx, k_old, q, w):
    m = 1000037
    g = np.random.default_rng(7 + k_old + q + w)
    NV = basis(g, m, q + k_old)
    N, Vold = NV[:, :q], NV[:, q:]
    W = g.uniform(-1, 1, (m, w))
    Q, used = run(ctx, Vold, W, N)
    np.testing.assert_allclose(Q, reference(Vold, W, N), rtol=0, atol=1e-12)
    check(Q, Vold, N, m)


@pytest.mark.parametrize("m", [1000, 1000037])
@pytest.mark.parametrize("q", [4, 40])
def test_adversarial_blocks(ctx, m, q):
    """a column in span(N), a column in span([N V_old]), two equal columns: the repair round or a column-wise path, bounds met"""
    g = np.random.default_rng(q + (m % 97))
    k_old = 20
    NV = basis(g, m, q + k_old)
    N, Vold = NV[:, :q], NV[:, q:]
    w = 6
    W = g.uniform(-1, 1, (m, w))
    W[:, 1] = N @ g.uniform(-1, 1, q)
    W[:, 3] = N @ g.uniform(-1, 1, q) + Vold @ g.uniform(-1, 1, k_old)
    W[:, 5] = W[:, 4]
    Q, used = run(ctx, Vold, W, N)
    assert used in (1, 3)
    check(Q, Vold, N, m)
    # the independent columns span what numpy's projection of them spans
    keep = [0, 2, 4]
    P = reference(Vold, W[:, keep], N)
    assert np.abs(P - Q[:, :] @ (Q.T @ P)).max() <= 1e-10


def test_columnwise_method(ctx):
    m, k_old, q, w = 1000, 30, 5, 7
    g = np.random.default_rng(11)
    NV = basis(g, m, q + k_old)
    N, Vold = NV[:, :q], NV[:, q:]
    W = g.uniform(-1, 1, (m, w))
    Q, used = run(ctx, Vold, W, N, method=1)
    assert used == 1
    np.testing.assert_allclose(Q, reference(Vold, W, N), rtol=0, atol=1e-12)
    check(Q, Vold, N, m)


@pytest.mark.parametrize("k_old,w", [(0, 5), (37, 17), (300, 33)])
def test_without_a_nullspace_is_bitwise_rails_orthogonalize(ctx, k_old, w):
    m = 5003
    g = np.random.default_rng(k_old + w)
    Vold = basis(g, m, k_old)
    W = g.uniform(-1, 1, (m, w))
    W[:, -1] = W[:, 0]  # a dependent column: the repair round too
    X1 = MV(ctx, np.hstack([Vold, W]), capacity=k_old + w)
    X2 = MV(ctx, np.hstack([Vold, W]), capacity=k_old + w)
    X1.orthogonalized = X2.orthogonalized = k_old
    u1 = X1.orthogonalize(0)
    u2 = X2.orthogonalize_deflated(None, 0)
    assert u1 == u2
    assert np.array_equal(X1.to_host(), X2.to_host())


@pytest.mark.parametrize("q,k_old,w", [(3, 0, 5), (1, 127, 16), (5, 37, 17), (4, 300, 17), (32, 128, 32)])
def test_deflating_is_bitwise_orthogonalize_on_one_panel(ctx, q, k_old, w):
    """[N | V_old] in two panels (the two-segment kernels) against the same columns in one panel (the one-segment kernels): one kernel
    body for both operand forms and the same summation order, so the new columns agree bit for bit"""
    m = 5003
    g = np.random.default_rng(100 * q + k_old + w)
    NV = basis(g, m, q + k_old)
    N, Vold = NV[:, :q], NV[:, q:]
    W = g.uniform(-1, 1, (m, w))
    X1 = MV(ctx, np.hstack([Vold, W]), capacity=k_old + w)
    X1.orthogonalized = k_old
    u1 = X1.orthogonalize_deflated(MV(ctx, N), 0)
    X2 = MV(ctx, np.hstack([N, Vold, W]), capacity=q + k_old + w)
    X2.orthogonalized = q + k_old
    u2 = X2.orthogonalize(0)
    assert u1 == u2
    assert np.array_equal(X1.to_host()[:, k_old:], X2.to_host()[:, q + k_old:])
