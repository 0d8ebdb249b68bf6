"""Test matrices, case list and a plain-numpy emulation for the sparse right-hand side (rails_sprhs, rails_resid_lanczos_sparse).  numpy
and scipy only, no project imports: the host tests and the device tests share everything in here.

The bounds are those of tests/lanczos_reference.py with parts["B"] = B.toarray(): they were derived for the dense sum over p columns, and
the sparse sum of a row (or of a transposed row) has fewer terms, in any order, so every bound still holds.

emulate() restates the step order of the sparse form in fp64: the pass makes r = [AV MV] g + B g_B - alpha q_i - beta q_{i-1} with B's
part of a row summed entry by entry (rows of at most SHORT entries) or in 64 strands (longer rows); [c'_AV | c'_MV | rr] go wave -> block
-> 16 strands as in lanczos_reference.emulate; c'_B = B'r is summed per transposed row: entry by entry for at most SHORT entries,
otherwise in items of CHUNK entries (64 strands each) whose sums are added in 64 strands again."""
import numpy as np
import scipy.sparse as sp

import lanczos_reference as R

SHORT, CHUNK = 32, 512  # RAILS_SPRHS_SHORT, RAILS_SPRHS_CHUNK of rails_amd/csrc/rails_internal.h


# ------------------------------------------------------------------------------------------------------------ the matrices
def make_B(form, m, p, lanczos=False):
    """the test matrices, m x p CSR, rng = default_rng(3).  lanczos: the extra structure of "mixed" for the Lanczos cases"""
    rng = np.random.default_rng(3)
    if p == 0:
        return sp.csr_matrix((m, 0))
    j = np.arange(p)
    if form == "selection":
        rows = j * (m // p) + 1
        assert rows.max() < m
        B = sp.csr_matrix((rng.uniform(0.5, 1.5, p), (rows, j)), shape=(m, p))
    elif form == "mixed":
        rows = (j[:, None] * (m // p) + np.arange(3)[None, :]) % m
        D = sp.lil_matrix((m, p))
        vals = rng.uniform(-1, 1, (p, 3))
        for t in range(3):
            D[rows[:, t], j] = vals[:, t]
        D[:, 0] = (rng.uniform(-1, 1, m) / np.sqrt(m)).reshape(m, 1)
        if lanczos:
            D[m // 2, :] = rng.uniform(-1, 1, p).reshape(1, p)  # one dense row: p entries, more than a wave's 64 for p = 300
            D[0:70, :] = 0.0  # a whole 64-row group (and a bit) without entries
            if p >= 2:
                D[:, p - 2] = 0.0
        B = sp.csr_matrix(D)
        B.eliminate_zeros()
    elif form == "random3":
        B = sp.random(m, p, density=min(1.0, 3.0 / p), format="csr", random_state=rng)
    elif form == "dense":
        B = sp.csr_matrix(rng.uniform(-1, 1, (m, p)))
    else:
        raise ValueError(form)
    B.sort_indices()
    return B


def csr_arrays(B):
    return (np.ascontiguousarray(B.indptr, dtype=np.int64), np.ascontiguousarray(B.indices, dtype=np.int32),
            np.ascontiguousarray(B.data, dtype=np.float64))


# --------------------------------------------------------------------------------------------------------------- the cases
# (m, k, p, form, L) and where AV / MV sit: some in windows of wider NaN-filled panels (even first columns)
_LIST = [
    (741, 6, 5, "random3", 4, None),
    (741, 129, 300, "mixed", 4, None),
    (741, 37, 129, "random3", 5, dict(av=("x", 2), mv=("x", 40), panels={"x": 80})),
    (330, 37, 200, "selection", 5, dict(av=("a48", 4), mv=("m64", 10), panels={"a48": 48, "m64": 64})),
    (65, 2, 1, "dense", 2, None),
    (64, 2, 3, "mixed", 2, None),
    (63, 2, 130, "random3", 2, dict(av=("x", 6), mv=("x", 12), panels={"x": 16})),
    (1, 2, 1, "dense", 2, None),
    (200, 0, 260, "random3", 3, None),
    (200, 4, 0, "none", 3, None),
    (500, 2, 1, "dense", 10, None),
    (741, 385, 16, "mixed", 4, None),
]


def _cases():
    out = []
    for i, (m, k, p, form, L, win) in enumerate(_LIST):
        c = R._case("sparse", "m%d_k%d_p%d_%s_L%d" % (m, k, p, form, L), m, k, 0, L, **(win or {}))
        c.update(p=p, form=form, seed=2000 + i, stream=i)
        out.append(c)
    return out


CASES = _cases()
GRID_STRIDE = dict(R._case("sparse", "grid_stride", 2 * 262144 + 229, 6, 0, 3), p=1000, form="selection", seed=2100, stream=3)


def case_id(c):
    return c["name"]


def make_case(c):
    """AV, MV, T and the NaN-filled panels of lanczos_reference.make_case; B: the CSR matrix, parts["B"] its dense form for check_run"""
    parts = R.make_case(dict(c, p=0))
    Bs = make_B(c["form"], c["m"], c["p"], lanczos=True)
    parts["Bs"] = Bs
    parts["B"] = Bs.toarray()
    return parts


# ----------------------------------------------------------------------------------------------------------- the emulation
BUGS = ("no_B_in_r", "stale_cB", "own_pattern", "row_cut_64", "last_row_dropped")


def _tree(x):
    """sum of 64 values in a fixed pairwise order (wave_sum)"""
    x = np.asarray(x, dtype=np.float64)
    while x.size > 1:
        x = x[0::2] + x[1::2]
    return float(x[0])


def _strands(x):
    """64 strands (entry e to strand e mod 64, each in order), then the tree"""
    n = (x.size + 63) // 64 * 64
    y = np.zeros(n)
    y[:x.size] = x
    return _tree(y.reshape(-1, 64).sum(axis=0))


def _seq(x):
    s = 0.0
    for v in x:
        s += v
    return s


def _row_sums(ptr, idx, val, x, cut=None):
    """per row: sum val * x[idx], entry by entry up to SHORT entries, in strands beyond"""
    out = np.zeros(ptr.size - 1)
    for i in range(ptr.size - 1):
        a, b = ptr[i], ptr[i + 1]
        if cut is not None:
            b = min(b, a + cut)
        prod = val[a:b] * x[idx[a:b]]
        out[i] = _seq(prod) if b - a <= SHORT else _strands(prod)
    return out


def _bt_sums(tptr, tidx, tval, r):
    out = np.zeros(tptr.size - 1)
    for j in range(tptr.size - 1):
        a, b = tptr[j], tptr[j + 1]
        prod = tval[a:b] * r[tidx[a:b]]
        if b - a <= SHORT:
            out[j] = _seq(prod)
        else:
            out[j] = _strands(np.array([_strands(prod[s:s + CHUNK]) for s in range(0, b - a, CHUNK)]))
    return out


def emulate(AV, MV, Bs, T, q0, L, nblocks_cap=1024, bug=None):
    """the sparse form's one-pass algorithm in fp64 numpy (q0: the raw start vector); returns dict(H, steps, Q)"""
    assert bug is None or bug in BUGS
    m, k = AV.shape
    p = Bs.shape[1]
    Bs = sp.csr_matrix(Bs)
    Bt = sp.csr_matrix(Bs.T)
    Bt.sort_indices()
    bp, bi, bv = Bs.indptr, Bs.indices, Bs.data
    tp, ti, tv = Bt.indptr, Bt.indices, Bt.data
    P = np.hstack([AV, MV])
    n = 2 * k
    mpad = max((m + 63) // 64 * 64, 64)
    ngroups = mpad // 64
    nblocks = max(1, min((ngroups + 3) // 4, nblocks_cap))

    def sums(r):
        X = np.zeros((mpad, n + 1))
        X[:m, :n] = P * r[:, None]
        X[:m, n] = r * r
        grp = X.reshape(ngroups, 64, n + 1).sum(axis=1)
        slots = 4 * nblocks
        trips = (ngroups + slots - 1) // slots
        G = np.zeros((trips * slots, n + 1))
        G[:ngroups] = grp
        wave = np.zeros((nblocks, 4, n + 1))
        for t in range(trips):
            wave += G[t * slots:(t + 1) * slots].reshape(nblocks, 4, n + 1)
        blk = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
        strands = np.zeros((16, n + 1))
        for t in range(nblocks):
            strands[t % 16] += blk[t]
        s = np.zeros(n + 1)
        for gi in range(16):
            s += strands[gi]
        if bug == "own_pattern":  # B's own arrays read as if they were the transposed ones
            cB = np.zeros(p)
            for j in range(min(p, m)):
                cB[j] = _seq(bv[bp[j]:bp[j + 1]] * r[bi[bp[j]:bp[j + 1]] % m])
        else:
            cB = _bt_sums(tp, ti, tv, r)
        if bug == "last_row_dropped" and p:
            cB[p - 1] = 0.0
        return np.concatenate([s[:n], cB, s[n:]])

    prev_cB = [np.zeros(p)]

    def small(s, beta):
        inv = 1.0 / beta
        c = s[:n + p] * inv
        gB = c[n:]
        if bug == "stale_cB":
            gB, prev_cB[0] = prev_cB[0], c[n:].copy()
        g = np.concatenate([T @ c[k:2 * k], T @ c[:k], gB])
        return inv, g, float(c[:n] @ g[:n] + c[n:] @ c[n:])

    Qc = np.zeros((m, L + 2))
    Qc[:, 0] = q0
    H = np.zeros((L + 1, L + 1))
    s = sums(Qc[:, 0])
    inv, g, alpha = small(s, np.sqrt(s[n + p]))
    alphas, betap, steps = [alpha], 0.0, L
    for i in range(L):
        Qc[:, i] = Qc[:, i] * inv
        r = P @ g[:n]
        if bug != "no_B_in_r":
            r = r + _row_sums(bp, bi, bv, g[n:], cut=64 if bug == "row_cut_64" else None)
        r = r - alpha * Qc[:, i]
        if i > 0:
            r = r - betap * Qc[:, i - 1]
        Qc[:, i + 1] = r
        s = sums(r)
        beta = np.sqrt(s[n + p])
        H[i, i] = alphas[i]
        if beta < R.BREAKDOWN:
            steps = i + 1
            break
        H[i + 1, i] = H[i, i + 1] = beta
        inv, g, alpha = small(s, beta)
        alphas.append(alpha)
        betap = beta
    return dict(H=H, steps=steps, Q=Qc[:, :steps].copy())


# ------------------------------------------------------------------- the step-local reference without the dense form of B
def _coo(Bs):
    C = sp.coo_matrix(Bs)
    return C.row, C.col, C.data.astype(R.LD)


def step_local_sparse(AV, MV, Bs, T, Q, alphas, betas):
    """lanczos_reference.step_local, the same formulas and bounds, with the products with B and |B| taken from its entries in
    np.longdouble: for cases whose m x p dense form does not fit (the grid-stride case).  tests/test_sparse_rhs_host.py checks that
    the two agree where both can run."""
    LD = R.LD
    k, p = AV.shape[1], Bs.shape[1]
    m = AV.shape[0]
    n = 2 * k + p
    P2 = np.hstack([AV, MV]).astype(LD)
    P2abs = np.abs(P2)
    bi, bj, bv = _coo(Bs)
    bva = np.abs(bv)
    T = np.asarray(T, dtype=LD).reshape(k, k)
    Tabs = np.abs(T)

    def Bt(vals, x):  # B'x
        out = np.zeros(p, dtype=LD)
        np.add.at(out, bj, vals * x[bi])
        return out

    def Bx(vals, y):  # B y
        out = np.zeros(m, dtype=LD)
        np.add.at(out, bi, vals * y[bj])
        return out

    def G(Tm, c):  # [[0 T 0], [T 0 0], [0 0 I]] c
        return np.concatenate([Tm @ c[k:2 * k], Tm @ c[:k], c[2 * k:]])

    gN = LD(R.gamma(4 * (m + 2 * n + 16)))
    Q = np.asarray(Q, dtype=LD)
    out = []
    for i in range(Q.shape[1]):
        q = Q[:, i]
        qp = Q[:, i - 1] if i > 0 else np.zeros(m, dtype=LD)
        bp = LD(betas[i - 1]) if i > 0 else LD(0)
        al = LD(alphas[i])
        c = np.concatenate([P2.T @ q, Bt(bv, q)])
        g = G(T, c)
        alpha_ref = c @ g
        a = np.concatenate([P2abs.T @ np.abs(q), Bt(bva, np.abs(q))])
        Ga = G(Tabs, a)
        ea = 2 * gN * (a @ Ga)
        r_ref = P2 @ g[:2 * k] + Bx(bv, g[2 * k:]) - al * q - bp * qp
        er = gN * (P2abs @ Ga[:2 * k] + Bx(bva, Ga[2 * k:]) + abs(al) * np.abs(q) + abs(bp) * np.abs(qp)) + np.abs(q) * ea + 4 * LD(R.EPS) * np.abs(r_ref)
        beta_ref = np.sqrt(r_ref @ r_ref)
        eb = np.sqrt(er @ er) + LD(R.gamma(m + 4)) * beta_ref
        out.append(dict(alpha_ref=alpha_ref, ea=ea, r_ref=r_ref, er=er, beta_ref=beta_ref, eb=eb))
    return out


def check_run_sparse(parts, L, H, steps, Q):
    """lanczos_reference.check_run over step_local_sparse (parts["Bs"], no parts["B"] needed)"""
    LD = R.LD
    AV, MV, Bs, T = parts["AV"], parts["MV"], parts["Bs"], parts["T"]
    m = AV.shape[0]
    H = np.asarray(H)
    assert 1 <= steps <= L and Q.shape == (m, steps) and H.shape[0] >= L + 1
    broke = steps < L
    alphas = np.array([H[i, i] for i in range(steps)])
    nb = steps - 1 if broke else steps
    betas = np.array([H[i + 1, i] for i in range(nb)])
    assert all(H[i, i + 1] == H[i + 1, i] for i in range(nb))
    ref = step_local_sparse(AV, MV, Bs, T, Q, alphas, betas)
    worst = dict(alpha=0.0, beta=0.0, r=0.0, norm=0.0)
    Ql = np.asarray(Q, dtype=LD)
    for i in range(steps):
        s = ref[i]
        worst["alpha"] = max(worst["alpha"], R._ratio(abs(LD(alphas[i]) - s["alpha_ref"]), s["ea"]))
        if i < nb:
            worst["beta"] = max(worst["beta"], R._ratio(abs(LD(betas[i]) - s["beta_ref"]), s["eb"]))
        else:
            worst["beta"] = max(worst["beta"], R._ratio(max(s["beta_ref"] - LD(R.BREAKDOWN), LD(0)), s["eb"]))
        if i + 1 < steps:
            worst["r"] = max(worst["r"], R._ratio(np.abs(LD(betas[i]) * Ql[:, i + 1] - s["r_ref"]), s["er"]))
        worst["norm"] = max(worst["norm"], R._ratio(abs(Ql[:, i] @ Ql[:, i] - 1), R.gamma(m + 8)))
    return worst
