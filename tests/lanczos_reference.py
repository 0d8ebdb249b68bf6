"""Step-local reference, derived bounds, a plain-numpy emulation and the case list for the fused residual Lanczos
(rails_amd/csrc/lanczos.hip).  numpy only, no project imports: a host test and a device test can share everything in here.

The operator.  P = [AV MV B] (m x n, n = 2k + p) and R = AV T MV' + MV T AV' + B B' = P G P' with the block matrix
G = [[0 T 0], [T 0 0], [0 0 I]], so with c = P'q = [c_AV; c_MV; c_B] the kernel's coefficients are g = G c = [T c_MV; T c_AV; c_B].

Why step-local.  A Lanczos recurrence run freely amplifies rounding differences, so a whole run can only be compared loosely.  One step
taken from the vectors the device itself stored is an ordinary finite computation with a componentwise error bound.  step_local() takes
the stored q_i, q_{i-1}, alpha_i, beta_{i-1} and computes in np.longdouble

    c = P'q_i,  g = G c,  alpha_ref = c.g,  r_ref = P g - alpha_dev q_i - beta_dev_{i-1} q_{i-1},  beta_ref = ||r_ref||.

What the kernel computes for the same step (eps = 2^-52, gamma(N) = N eps / (1 - N eps), a = |P|'|q_i|, Gabs = |G|):

  c      The pass before summed c' = P'r over the m rows of the raw r (any order: waves, blocks, 16 strands) and k_lz_small scaled it by
         inv = fl(1 / beta); the stored q_i is fl(r inv).  Both are sums of the same m products up to one rounding per factor, so
         |c_dev - c| <= gamma(m + 3) a.
  g      k (or 1) further products per entry, one more rounding for the scaling: |g_dev - g| <= gamma(m + n + 4) Gabs a, and |g| <= Gabs a.
  alpha  an n-term inner product of c_dev and g_dev:  |alpha_dev - alpha_ref| <= (gamma(m+3) + gamma(m+n+4) + gamma(n+1)) a'Gabs a
         <= gamma(2m + 2n + 8) a'Gabs a.
  r      row j:  t = P_j . g_dev (n fused multiply-adds and a 64-lane sum), then two subtractions of products:
         |r_dev - r_ref|_j <= gamma(m + 2n + 8) (|P| Gabs a)_j + gamma(3) (|alpha||q_i| + |beta_{i-1}||q_{i-1}|)_j.
  beta   rr sums m squares (relative error gamma(m + 1) whatever the order), beta = fl(sqrt(rr)):
         |beta_dev - ||r_dev|| | <= gamma(m/2 + 2) ||r_dev||, and | ||r_dev|| - ||r_ref|| | <= ||r_dev - r_ref||_2.
  q_i+1  is stored as fl(r_dev inv) with inv = fl(1 / beta_dev): beta_dev q_{i+1} = r_dev (1 + d), |d| <= 3 eps to first order.
  norm   ||q||^2 = ||r||^2 inv^2 (1 + 2 eps)-ish per element against rr (1 + gamma(m+1)), beta and inv one rounding each (squared):
         | ||q||^2 - 1 | <= gamma(m + 7).

The asserted bounds use one generous N = 4 (m + 2n + 16) for all of the above -- the factor 4 is the slack tests/test_gpu_solution.py
leaves for the order of summation and the reference value's own error:

    ea = 2 gamma(N) a'Gabs a                                             >= |alpha_dev - alpha_ref|
    er = gamma(N) (|P| Gabs a + |alpha||q_i| + |beta_{i-1}||q_{i-1}|) + |q_i| ea + 4 eps |r_ref|
                                                                         >= |beta_dev q_{i+1,dev} - r_ref|   (rowwise; no division)
    eb = ||er||_2 + gamma(m + 4) beta_ref                                >= |beta_dev - beta_ref|
    gamma(m + 8)                                                         >= | ||q_i||^2 - 1 |  for every stored vector

(|q_i| ea is slack for a kernel that would fold alpha's own error into r; this one does not.)  The rows of r of the last step cannot be
checked: the raw q_L is not retrievable; its alpha and beta are.  When a run stopped early the last step's beta is not reported either
(H omits it); it was below 1e-14 on the device, so beta_ref <= 1e-14 + eb is asserted instead.

tests/test_lanczos_reference_host.py shows on this list of cases that a correct fp64 implementation (emulate) stays within a quarter of
every bound and that seeded mistakes exceed one of them by far more than 10x."""
import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
BREAKDOWN = 1e-14  # src/LyapunovSolver.hpp:419-426


def gamma(N):
    return N * EPS / (1.0 - N * EPS)


def pad16(c):
    return (max(int(c), 1) + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------- the cases
# A case is plain data.  "av" / "mv" / "b" = (panel name, first column); "panels" = name -> capacity (a multiple of 16, so the
# capacity is the leading dimension and every column is writable).  Every column outside the three windows holds NaN.
def _case(group, name, m, k, p, L, av=None, mv=None, b=None, panels=None):
    panels = dict(panels or {})
    if av is None:
        av = ("av", 0)
        panels["av"] = pad16(k)
    if mv is None:
        mv = ("mv", 0)
        panels["mv"] = pad16(k)
    if b is None:
        b = ("b", 0)
        panels["b"] = pad16(p)
    for (pn, c0), w in ((av, k), (mv, k), (b, p)):
        assert panels[pn] % 16 == 0 and c0 % 2 == 0 and c0 + w <= panels[pn]
    return dict(group=group, name=name, m=m, k=k, p=p, L=L, av=av, mv=mv, b=b, panels=panels)


def _cases():
    out = []
    # both ends of every range of NCH = ceil(k / 128); 741 rows = 11 full groups of 64 + 37 (odd, 37 mod 4 = 1)
    for k in (6, 128, 129, 255, 257, 384, 385, 512):
        out.append(_case("instantiations", "k%d" % k, 741, k, 5, 4))
    out.append(_case("windows", "one_panel", 330, 37, 3, 5, av=("x", 2), mv=("x", 40), b=("b", 6), panels={"x": 80, "b": 16}))
    out.append(_case("windows", "ld48_ld64", 330, 37, 3, 5, av=("a48", 4), mv=("m64", 10), panels={"a48": 48, "m64": 64}))
    out.append(_case("windows", "last_column", 330, 46, 3, 5, av=("a48", 2), mv=("m64", 18), b=("b", 12), panels={"a48": 48, "m64": 64, "b": 16}))
    for m in (1, 63, 64, 65):
        out.append(_case("tiny", "m%d" % m, m, 2, 1, 2))
    out.append(_case("empty", "k0", 200, 0, 3, 3))
    out.append(_case("empty", "p0", 200, 4, 0, 3))
    out.append(_case("grid_stride", "wraps", 2 * 262144 + 229, 6, 3, 3))
    out.append(_case("past_rank", "L10", 500, 2, 1, 10))
    for i, c in enumerate(out):
        c["seed"], c["stream"] = 1000 + i, i
    return out


CASES = _cases()


def case_id(c):
    return "%s-%s" % (c["group"], c["name"])


def cases(group=None):
    return [c for c in CASES if group is None or c["group"] == group]


def problem(m, k, p, rng):
    """AV, MV, B uniform(-1, 1), scaled like _lanczos_case of tests/test_gpu_kernels.py: MV's columns of about unit norm (an orthonormal V
    there), AV twice that (A V = -2 V + ... there), B unscaled, T = 0.05 (U + U')."""
    s = np.sqrt(3.0 / m)
    MV = s * rng.uniform(-1, 1, (m, k))
    AV = 2.0 * s * rng.uniform(-1, 1, (m, k))
    B = rng.uniform(-1, 1, (m, p))
    T = rng.uniform(-1, 1, (k, k))
    T = 0.05 * (T + T.T)
    return AV, MV, B, T


def make_case(c):
    """Host data of a case: the clean parts and the NaN-filled panels with the parts in their windows."""
    rng = np.random.default_rng(c["seed"])
    AV, MV, B, T = problem(c["m"], c["k"], c["p"], rng)
    panels = {pn: np.full((c["m"], cap), np.nan) for pn, cap in c["panels"].items()}
    for (pn, c0), X in ((c["av"], AV), (c["mv"], MV), (c["b"], B)):
        panels[pn][:, c0:c0 + X.shape[1]] = X
    return dict(AV=AV, MV=MV, B=B, T=T, panels=panels)


# ------------------------------------------------------------------------------------------------- the step-local reference
def _blocks(T, k, p):
    n = 2 * k + p
    G = np.zeros((n, n), dtype=LD)
    G[:k, k:2 * k] = T
    G[k:2 * k, :k] = T
    G[2 * k:, 2 * k:] = np.eye(p)
    return G


def step_local(AV, MV, B, T, Q, alphas, betas):
    """One dict per step i < Q.shape[1] from the stored vectors and coefficients: alpha_ref, ea, r_ref, er, beta_ref, eb (np.longdouble).
    betas may be shorter than alphas (a run that stopped early reports no last beta)."""
    k, p = AV.shape[1], B.shape[1]
    P = np.hstack([AV, MV, B]).astype(LD)
    m, n = P.shape
    Pabs = np.abs(P)
    G = _blocks(np.asarray(T, dtype=LD).reshape(k, k), k, p)
    Gabs = np.abs(G)
    gN = LD(gamma(4 * (m + 2 * n + 16)))
    Q = np.asarray(Q, dtype=LD)
    out = []
    for i in range(Q.shape[1]):
        q = Q[:, i]
        qp = Q[:, i - 1] if i > 0 else np.zeros(m, dtype=LD)
        bp = LD(betas[i - 1]) if i > 0 else LD(0)
        al = LD(alphas[i])
        c = P.T @ q
        g = G @ c
        alpha_ref = c @ g
        a = Pabs.T @ np.abs(q)
        Ga = Gabs @ a
        ea = 2 * gN * (a @ Ga)
        r_ref = P @ g - al * q - bp * qp
        er = gN * (Pabs @ Ga + abs(al) * np.abs(q) + abs(bp) * np.abs(qp)) + np.abs(q) * ea + 4 * LD(EPS) * np.abs(r_ref)
        beta_ref = np.sqrt(r_ref @ r_ref)
        eb = np.sqrt(er @ er) + LD(gamma(m + 4)) * beta_ref
        out.append(dict(alpha_ref=alpha_ref, ea=ea, r_ref=r_ref, er=er, beta_ref=beta_ref, eb=eb))
    return out


def _ratio(err, bound):
    """max err / bound; a zero bound admits only a zero error"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bound, dtype=LD))
    r = np.zeros(err.shape, dtype=LD)
    nz = bound > 0
    r[nz] = err[nz] / bound[nz]
    r[~nz & (err > 0)] = np.inf
    r[np.isnan(err)] = np.inf
    return float(r.max()) if r.size else 0.0


def check_run(parts, L, H, steps, Q):
    """error / bound of a run (H (L+1) x (L+1), steps, Q m x steps: the stored, normalised vectors) against every bound of the module
    docstring.  Returns the largest ratios: dict(alpha=, beta=, r=, norm=)."""
    AV, MV, B, T = parts["AV"], parts["MV"], parts["B"], parts["T"]
    m = AV.shape[0]
    H = np.asarray(H)
    assert 1 <= steps <= L and Q.shape == (m, steps) and H.shape[0] >= L + 1
    broke = steps < L
    alphas = np.array([H[i, i] for i in range(steps)])
    nb = steps - 1 if broke else steps
    betas = np.array([H[i + 1, i] for i in range(nb)])
    assert all(H[i, i + 1] == H[i + 1, i] for i in range(nb))
    ref = step_local(AV, MV, B, T, Q, alphas, betas)
    worst = dict(alpha=0.0, beta=0.0, r=0.0, norm=0.0)
    Ql = np.asarray(Q, dtype=LD)
    for i in range(steps):
        s = ref[i]
        worst["alpha"] = max(worst["alpha"], _ratio(abs(LD(alphas[i]) - s["alpha_ref"]), s["ea"]))
        if i < nb:
            worst["beta"] = max(worst["beta"], _ratio(abs(LD(betas[i]) - s["beta_ref"]), s["eb"]))
        else:  # the step that stopped the run: its beta was below the threshold on the device
            worst["beta"] = max(worst["beta"], _ratio(max(s["beta_ref"] - LD(BREAKDOWN), LD(0)), s["eb"]))
        if i + 1 < steps:
            worst["r"] = max(worst["r"], _ratio(np.abs(LD(betas[i]) * Ql[:, i + 1] - s["r_ref"]), s["er"]))
        worst["norm"] = max(worst["norm"], _ratio(abs(Ql[:, i] @ Ql[:, i] - 1), gamma(m + 8)))
    return worst


def assert_within(worst, fraction=1.0, what=""):
    bad = {key: v for key, v in worst.items() if not v <= fraction}
    assert not bad, "%s: error / bound above %g: %r (all: %r)" % (what, fraction, bad, worst)


# --------------------------------------------------------------------------------------------------------- the emulation
BUGS = ("drop_beta_term", "uncrossed", "wave_partial", "strand", "odd_k_last_col", "stale_alpha", "inv_twice")


def emulate(AV, MV, B, T, q0, L, nblocks_cap=1024, bug=None):
    """The kernel's one-pass algorithm in fp64 numpy (q0: the raw start vector).  Each pass makes r from the coefficients of the pass
    before and, in the same sweep, c' = P'r and rr = r.r from the unnormalised r; sums go wave (a row group of 64 at a time, grid
    stride) -> block (wave 0 + 1 + 2 + 3) -> 16 interleaved strands of blocks -> strands 0..15; then inv = 1 / beta, the next q is
    r * inv, alpha comes from the scaled coefficients, and a step with beta < 1e-14 ends the run.  Returns dict(H, steps, Q).
    bug: one of BUGS, a seeded mistake for the sensitivity test."""
    assert bug is None or bug in BUGS
    m, k = AV.shape
    p = B.shape[1]
    n = 2 * k + p
    P = np.hstack([AV, MV, B])
    Pp = P  # the panels as the pass reads them
    if bug == "odd_k_last_col" and k % 2 == 1 and k > 1:
        Pp = P.copy()
        Pp[:, k - 1] = P[:, k - 2]
        Pp[:, 2 * k - 1] = P[:, 2 * k - 2]
    mpad = max((m + 63) // 64 * 64, 64)
    ngroups = mpad // 64
    nblocks = max(1, min((ngroups + 3) // 4, nblocks_cap))

    def sums(r):
        X = np.zeros((mpad, n + 1))
        X[:m, :n] = Pp * r[:, None]
        X[:m, n] = r * r
        grp = X.reshape(ngroups, 64, n + 1).sum(axis=1)
        slots = 4 * nblocks
        trips = (ngroups + slots - 1) // slots
        G = np.zeros((trips * slots, n + 1))
        G[:ngroups] = grp
        wave = np.zeros((nblocks, 4, n + 1))
        for t in range(trips):  # a wave adds its row groups in the order it walks them
            wave += G[t * slots:(t + 1) * slots].reshape(nblocks, 4, n + 1)
        blk = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
        if bug == "wave_partial":
            blk[:, :n] = (wave[:, 0, :n] + wave[:, 2, :n]) + wave[:, 3, :n]
        strands = np.zeros((16, n + 1))
        for t in range(nblocks):
            strands[t % 16] += blk[t]
        s = np.zeros(n + 1)
        for gi in range(16):
            if bug == "strand" and gi == 1:
                continue
            s += strands[gi]
        return s

    def small(s, beta):
        inv = 1.0 / beta
        c = s[:n] * inv
        if bug == "uncrossed":
            g = np.concatenate([T @ c[:k], T @ c[k:2 * k], c[2 * k:]])
        else:
            g = np.concatenate([T @ c[k:2 * k], T @ c[:k], c[2 * k:]])
        return inv, g, float(c @ g)

    Qc = np.zeros((m, L + 2))
    Qc[:, 0] = q0
    H = np.zeros((L + 1, L + 1))
    s = sums(Qc[:, 0])  # init pass: r := raw q_0
    inv, g, alpha = small(s, np.sqrt(s[n]))
    alphas, betap, steps, stale = [alpha], 0.0, L, 0.0
    for i in range(L):
        Qc[:, i] = Qc[:, i] * inv
        if bug == "inv_twice":
            Qc[:, i] = Qc[:, i] * inv
        a_used = stale if bug == "stale_alpha" else alpha
        r = Pp @ g - a_used * Qc[:, i]
        if i > 0 and bug != "drop_beta_term":
            r = r - betap * Qc[:, i - 1]
        Qc[:, i + 1] = r
        s = sums(r)
        beta = np.sqrt(s[n])
        H[i, i] = alphas[i]
        if beta < BREAKDOWN:
            steps = i + 1
            break
        H[i + 1, i] = H[i, i + 1] = beta
        stale = alpha
        inv, g, alpha = small(s, beta)
        alphas.append(alpha)
        betap = beta
    return dict(H=H, steps=steps, Q=Qc[:, :steps].copy())


# ------------------------------------------------------------------------------------------------- determined breakdowns
BREAKDOWN_M, BREAKDOWN_ROW = 64, 17


def breakdown_parts(which):
    """k = 0, p = 1, 64 rows, R = B B' of rank at most one: "zero" (B = 0), "tiny" (one nonzero row of value 2^-30: beta_0 <= 2^-60)
    and "second" (B = 2^-18 ones: ||B||^2 = 2^-30, beta_0 about 1e-10 passes, beta_1 is rounding of it and stops the run)."""
    m = BREAKDOWN_M
    B = np.zeros((m, 1))
    if which == "tiny":
        B[BREAKDOWN_ROW, 0] = 2.0 ** -30
    elif which == "second":
        B[:, 0] = 2.0 ** -18
    else:
        assert which == "zero"
    seed = {"zero": 31, "tiny": 32, "second": 33}[which]
    return dict(AV=np.zeros((m, 0)), MV=np.zeros((m, 0)), B=B, T=np.zeros((0, 0)), seed=seed, stream=2)
