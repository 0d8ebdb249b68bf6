"""Bits, launches and counters of the fused residual Lanczos (rails_amd/csrc/lanczos.hip) over a fixed list of cases, to compare two
builds of the library: a refactoring of the host code must leave every result, every launch and every counter as they were.

    python scripts/lanczos_identity.py --tree PATH --out ONE.json     # imports rails_amd from PATH in fresh child processes, runs the cases
    python scripts/lanczos_identity.py --compare PARENT.json NEW.json --out profiles/lanczos_refactor_identity.json

The cases are run by the helpers of THIS tree (tests/lanczos_reference.py, tests/lanczos_steps_device.py, tests/sparse_rhs_reference.py)
on the library of the tree given: every case of tests/lanczos_reference.py (the "instantiations" group once per RAILS_LZ_UNROLL in 1, 2, 4,
which is read once per process: one child each, one after another, nothing started after one that fails), every case of
tests/sparse_rhs_reference.py with its GRID_STRIDE, the three determined breakdowns, rails_lanczos_start, rails_lanczos_vectors at
w in (1, 16, 17, 33) and oc0 in (0, 3, 16), and the three runs on one context (and the first again) of
test_state_reuse_and_determinism_on_one_context.  Per case: the SHA-256 of H, of the stored vectors and of the written output window
with what lies around it, the steps, what rails_lanczos_last_launch says, and how far the context's lanczos, lanczos_start and
device-allocation counters and the RNG's next stream moved over the call."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*arrays):
    import numpy as np

    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class Probe:
    """counters and the RNG's next stream before a call; moved(): how far each went"""

    def __init__(self, ctx):
        self.ctx, self.before = ctx, self.read(ctx)

    @staticmethod
    def read(ctx):
        s = ctx.stats()
        seed, nxt = C.c_uint64(0), C.c_uint64(0)
        ctx.lib.rails_ctx_rng_state(ctx.h, C.byref(seed), C.byref(nxt))
        return {"lanczos": s["lanczos"], "lanczos_start": s["lanczos_start"], "dev_alloc": s["device_allocations"], "next_stream": nxt.value}

    def moved(self):
        now = self.read(self.ctx)
        return {key: now[key] - self.before[key] for key in now}


def record(D, ctx, m, H, steps, moved):
    Q = D.stored_vectors(ctx, m, steps)
    return {"H": sha(H), "Q": sha(Q), "steps": steps, "launch": list(D.last_launch(ctx)), "moved": moved}


def dense_case(D, ctx, windows, T, L, seed, stream):
    ctx.set_seed(seed, stream)
    probe = Probe(ctx)
    rc, H, steps = D.call(ctx, windows[0], windows[1], windows[2], T, L)
    moved = probe.moved()
    assert rc == 0, ctx.lib.rails_last_error()
    return record(D, ctx, windows[0].M(), H, steps, moved)


def sparse_case(np, rails_amd, D, ctx, c, parts):
    MV = rails_amd.HipMultiVectorWrapper
    dev = {pn: MV(ctx, data=host, capacity=host.shape[1]) for pn, host in parts["panels"].items()}
    AV, MVw = (dev[pn]._alias(c0, c["k"], True) for pn, c0 in (c["av"], c["mv"]))
    B = rails_amd.SparseRHS.from_scipy(ctx, parts["Bs"])
    k, L = c["k"], c["L"]
    T = np.asfortranarray(np.asarray(parts["T"], dtype=np.float64).reshape(k, k))
    H = np.full((L + 1, L + 1), np.nan, order="F")
    steps = C.c_int(-1)
    ctx.set_seed(c["seed"], c["stream"])
    probe = Probe(ctx)
    rc = ctx.lib.rails_resid_lanczos_sparse(ctx.h, AV.panel.h, AV.c0, MVw.panel.h, MVw.c0, k, D._ptr(T), max(1, k), B.h, L, D._ptr(H), L + 1, C.byref(steps))
    moved = probe.moved()
    assert rc == 0, ctx.lib.rails_last_error()
    out = record(D, ctx, c["m"], H, steps.value, moved)
    B.close()
    return out


def run_cases(group):
    """group "instantiations": that group of tests/lanczos_reference.py alone (under the caller's RAILS_LZ_UNROLL); "rest": everything else"""
    import numpy as np
    import rails_amd

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lanczos_reference as R
    import lanczos_steps_device as D
    import sparse_rhs_reference as S

    MV = rails_amd.HipMultiVectorWrapper
    out = {}
    ctx = rails_amd.Context(device=0, seed=1234)
    if group == "instantiations":
        for c in R.cases("instantiations"):
            parts = R.make_case(c)
            out["U%s %s" % (os.environ["RAILS_LZ_UNROLL"], R.case_id(c))] = dense_case(D, ctx, D.upload(ctx, c, parts), parts["T"], c["L"], c["seed"], c["stream"])
        ctx.close()
        return out
    for c in R.CASES:
        if c["group"] != "instantiations":
            parts = R.make_case(c)
            out["dense " + R.case_id(c)] = dense_case(D, ctx, D.upload(ctx, c, parts), parts["T"], c["L"], c["seed"], c["stream"])
    for c in S.CASES:
        out["sparse " + S.case_id(c)] = sparse_case(np, rails_amd, D, ctx, c, S.make_case(c))
    c = S.GRID_STRIDE
    parts = R.make_case(dict(c, p=0))
    parts["Bs"] = S.make_B(c["form"], c["m"], c["p"])
    out["sparse " + S.case_id(c)] = sparse_case(np, rails_amd, D, ctx, c, parts)
    # the determined breakdowns: k = 0, p = 1, 64 rows
    for which in ("zero", "tiny", "second"):
        bp = R.breakdown_parts(which)
        m = R.BREAKDOWN_M
        Bpanel = np.full((m, 16), np.nan)
        Bpanel[:, 0] = bp["B"][:, 0]
        nan = lambda: MV(ctx, data=np.full((m, 16), np.nan), capacity=16)  # noqa: E731
        windows = (nan()._alias(0, 0, True), nan()._alias(0, 0, True), MV(ctx, data=Bpanel, capacity=16)._alias(0, 1, True))
        out["breakdown " + which] = dense_case(D, ctx, windows, bp["T"], 4, bp["seed"], bp["stream"])
    # rails_lanczos_start: AV at [2, 39), MV at [40, 77) of one 80-column panel, B at [6, 9) of 16, 741 rows
    c = dict(R.cases("windows")[0], m=741)
    c["seed"], c["stream"] = 77, 5
    parts = R.make_case(c)
    AV, MVw, B = D.upload(ctx, c, parts)
    ctx.set_seed(c["seed"], c["stream"])
    sums = np.full(2 * c["k"] + c["p"] + 1, np.nan)
    probe = Probe(ctx)
    rc = ctx.lib.rails_lanczos_start(ctx.h, AV.panel.h, AV.c0, MVw.panel.h, MVw.c0, c["k"], B.panel.h, B.c0, c["p"], D._ptr(sums))
    moved = probe.moved()
    assert rc == 0, ctx.lib.rails_last_error()
    out["lanczos_start"] = {"sums": sha(sums), "Q": sha(D.stored_vectors(ctx, c["m"], 1)), "launch": list(D.last_launch(ctx)), "moved": moved}
    # rails_lanczos_vectors: 1000 rows, 7 stored vectors, S with leading dimension 10, a 64-column output full of a sentinel
    m, k, p, steps = 1000, 6, 3, 7
    rng = np.random.default_rng(11)
    AVh, MVh, Bh, T = R.problem(m, k, p, rng)
    out["vectors run"] = dense_case(D, ctx, (MV(ctx, data=AVh, capacity=16), MV(ctx, data=MVh, capacity=16), MV(ctx, data=Bh, capacity=16)), T, steps, 5, 9)
    assert out["vectors run"]["steps"] == steps
    for w in (1, 16, 17, 33):
        Sm = np.asfortranarray(np.full((steps + 3, w), np.nan))
        Sm[:steps] = rng.uniform(-1, 1, (steps, w))
        for oc0 in (0, 3, 16):
            O = MV(ctx, data=np.full((m, 64), -7.25), capacity=64)
            probe = Probe(ctx)
            rc = ctx.lib.rails_lanczos_vectors(ctx.h, D._ptr(Sm), steps + 3, w, O.panel.h, oc0)
            assert rc == 0, ctx.lib.rails_last_error()
            out["vectors w%d oc%d" % (w, oc0)] = {"out": sha(O.to_host()), "moved": probe.moved()}
    ctx.close()
    # one context: a run, a shorter one in the same buffers, a longer one that regrows them, the first again
    ctx = rails_amd.Context(device=0, seed=1)
    k, p = 12, 4
    runs = []
    for i, (m, L) in enumerate(((5000, 12), (100, 3), (5000, 20))):
        AVh, MVh, Bh, T = R.problem(m, k, p, np.random.default_rng(50 + i))
        runs.append(((MV(ctx, data=AVh, capacity=16), MV(ctx, data=MVh, capacity=16), MV(ctx, data=Bh, capacity=16)), T, L))
        out["reuse run %d" % i] = dense_case(D, ctx, runs[-1][0], T, L, 900 + i, 3)
    out["reuse run 0 again"] = dense_case(D, ctx, runs[0][0], runs[0][1], runs[0][2], 900, 3)
    assert out["reuse run 0 again"]["H"] == out["reuse run 0"]["H"] and out["reuse run 0 again"]["Q"] == out["reuse run 0"]["Q"]
    ctx.close()
    return out


def child(tree, group, path):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import rails_amd  # before this tree's helpers are imported: they put their own tree first on the path

    assert os.path.dirname(os.path.abspath(rails_amd.__file__)) == os.path.join(tree, "rails_amd"), rails_amd.__file__
    out = run_cases(group)
    with open(path, "w") as fh:
        json.dump({"cases": out}, fh)
    print("%s: %d cases" % (group, len(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="the tree to import rails_amd from (built)")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT.json", "NEW.json"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds each child process may take")
    a = ap.parse_args()
    if a.compare:
        sides = [json.load(open(p)) for p in a.compare]
        keys = sorted(set(sides[0]["cases"]) | set(sides[1]["cases"]))
        differ = [k for k in keys if sides[0]["cases"].get(k) != sides[1]["cases"].get(k)]
        equal = not differ and len(keys) > 0
        with open(a.out, "w") as fh:  # one line per case; both sides where they differ
            fh.write('{"equal": %s, "cases": %d, "differ": %s, "sides": {\n' % (json.dumps(equal), len(keys), json.dumps(differ)))
            fh.write(",\n".join(' %s: %s' % (json.dumps(k), json.dumps(sides[0]["cases"].get(k) if k not in differ else
                                                                     {"parent": sides[0]["cases"].get(k), "new": sides[1]["cases"].get(k)})) for k in keys))
            fh.write("\n}}\n")
        print("equal: %s (%d cases, %d differ)" % (equal, len(keys), len(differ)))
        for k in differ[:20]:
            print(k, sides[0]["cases"].get(k), sides[1]["cases"].get(k))
        sys.exit(0 if equal else 1)
    if a.child:
        child(a.tree, a.child, a.out)
        return
    cases = {}
    for group, unroll in (("rest", None), ("instantiations", "1"), ("instantiations", "2"), ("instantiations", "4")):
        env = dict(os.environ)
        env.pop("RAILS_LZ_UNROLL", None)
        if unroll:
            env["RAILS_LZ_UNROLL"] = unroll
        part = a.out + ".part"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", group, "--tree", a.tree, "--out", part], env=env, timeout=a.timeout)
        if p.returncode != 0:  # nothing is started after a child that failed
            sys.exit(p.returncode if p.returncode > 0 else 1)
        cases.update(json.load(open(part))["cases"])
        os.remove(part)
    with open(a.out, "w") as fh:
        json.dump({"cases": cases}, fh)
    print("%d cases" % len(cases))


if __name__ == "__main__":
    main()
