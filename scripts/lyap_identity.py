#!/usr/bin/env python3
"""Bits and counters of the host dense numerics (rails_sb03md with its four routes, the LAPACK pass-throughs) over a fixed sequence of
calls, to compare two builds after a change that must leave results alone.

  lyap_identity.py LIB                               one process: after every call a line with the SHA-256 of X, of A as left behind,
                                                     scale, info and the four route counters
  lyap_identity.py --compare PARENT_LIB NEW_LIB --label NAME --out FILE.json
                                                     both libraries in fresh child processes, once with the defaults and once per
                                                     RAILS_SB03MD_* switch set to 0 (they are read once per process); appends a record to FILE

LIB is any shared object that exports the host ABI of include/rails_hip.h (librails_hip.so, or the host objects linked with a stub
rails_set_error).  Run it with the default single LAPACK thread: with more the bits change from run to run."""
import argparse
import ctypes as C
import hashlib
import json
import os
import platform
import subprocess
import sys

import numpy as np

SWITCHES = ["RAILS_SB03MD_SYMMETRIC", "RAILS_SB03MD_SMITH", "RAILS_SB03MD_BLOCKED", "RAILS_SB03MD_ADI_INHERIT", "RAILS_SB03MD_ADI_INVERSE"]
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)


def sha(a):
    return hashlib.sha256(np.asfortranarray(a).tobytes(order="F")).hexdigest()[:20]


def padded(a, ld):
    """a in a column-major array of ld rows; the padding rows hold a value a stray write would change"""
    out = np.full((ld, a.shape[1]), 7.25, order="F")
    out[: a.shape[0], :] = a
    return out


class Sequence:
    def __init__(self, path):
        lib = self.lib = C.CDLL(path)
        lib.rails_sb03md.argtypes = [C.c_char, C.c_char, C.c_char, C.c_char, C.c_int, dp, C.c_int, dp, C.c_int, dp, ip]
        lib.rails_sb03md_counts.argtypes = [C.POINTER(C.c_long)] * 2
        lib.rails_sb03md_adi_counts.argtypes = [C.POINTER(C.c_long)] * 2
        lib.rails_sb03md_set_pause.argtypes = [C.c_int]
        lib.rails_dsyev.argtypes = [C.c_char, C.c_char, C.c_int, dp, C.c_int, dp, ip]
        lib.rails_dsteqr.argtypes = [C.c_char, C.c_int, dp, dp, dp, C.c_int, dp, ip]
        lib.rails_dtrsm.argtypes = [C.c_char] * 4 + [C.c_int, C.c_int, C.c_double, dp, C.c_int, dp, C.c_int]
        lib.rails_dpstrf.argtypes = [C.c_char, C.c_int, dp, C.c_int, ip, ip, C.c_double, ip]
        lib.rails_range_basis.argtypes = [C.c_int, C.c_int, dp, C.c_int, C.c_double, dp, C.c_int, ip, ip]
        for f in (lib.rails_sb03md, lib.rails_sb03md_counts, lib.rails_sb03md_adi_counts, lib.rails_sb03md_set_pause, lib.rails_dsyev, lib.rails_dsteqr, lib.rails_dtrsm,
                  lib.rails_dpstrf, lib.rails_range_basis):
            f.restype = None
        self.calls = 0

    def counts(self):
        v = [C.c_long(0) for _ in range(4)]
        self.lib.rails_sb03md_counts(C.byref(v[0]), C.byref(v[1]))
        self.lib.rails_sb03md_adi_counts(C.byref(v[2]), C.byref(v[3]))
        return "iter %d schur %d ext %d fresh %d" % tuple(x.value for x in v)

    def pause(self, calls):
        self.lib.rails_sb03md_set_pause(calls)
        print("set_pause(%d)" % calls)

    def solve(self, tag, A, Cm, trans=b"T", lda=None, ldx=None, dico=b"C"):
        n = A.shape[0]
        Ab, Xb = padded(A, lda or n), padded(Cm, ldx or n)
        scale, info = C.c_double(-1.0), C.c_int(-77)
        self.lib.rails_sb03md(dico, b"X", b"N", trans, n, Ab.ctypes.data_as(dp), Ab.shape[0], Xb.ctypes.data_as(dp), Xb.shape[0], C.byref(scale), C.byref(info))
        self.calls += 1
        print("%4d %-31s n %3d %s X %s A %s scale %s info %d | %s" % (self.calls, tag, n, trans.decode(), sha(Xb), sha(Ab), float(scale.value).hex(), info.value, self.counts()), flush=True)

    def lowrank(self, tag, A, Bm, **kw):
        self.solve(tag, A, -(Bm @ Bm.T), **kw)


def stable(g, n, shift=3.0, spread=0.8):
    return -shift * np.eye(n) + spread * g.standard_normal((n, n)) / np.sqrt(n)


def sb03md_sequence(s):
    g = np.random.default_rng(11)
    # small and symmetric
    s.solve("n=1", np.array([[-2.0]]), np.array([[-1.0]]))
    s.solve("n=2", np.array([[-2.0, 0.5], [-0.25, -1.0]]), np.array([[-1.0, 0.5], [0.5, -3.0]]), trans=b"N")
    for n in (8, 13, 31):
        for trans in (b"T", b"N"):
            s.lowrank("nonsymmetric small", stable(g, n), g.standard_normal((n, 3)), trans=trans)
    for n in (8, 100, 256):
        S = g.standard_normal((n, n))
        s.lowrank("symmetric", -(S @ S.T) / n - np.eye(n), g.standard_normal((n, 16)))
    for n in (8, 40):  # eigenvalues +-1: lambda_i + lambda_j = 0 ends the symmetric route, and Bartels-Stewart reports info = n + 1
        s.pause(0)
        s.lowrank("symmetric, eigenvalues +-1", np.diag([1.0, -1.0] * (n // 2)), g.standard_normal((n, 2)))
    # the bordered sequence of tests/test_abi.py
    g = np.random.default_rng(3)
    N = 208
    Afull, Bfull = stable(g, N), g.standard_normal((N, 16))
    Aw = np.zeros((N + 16, N + 16))  # a border that widens the spectrum by two orders of magnitude
    Aw[:N, :N] = Afull
    Aw[N:, N:] = -0.03 * np.eye(16)
    Aw[:N, N:] = 0.01 * g.standard_normal((N, 16))
    Aw[N:, :N] = 0.01 * g.standard_normal((16, N))
    A2 = stable(g, N + 32, 2.0, 0.5)
    for trans in (b"T", b"N"):
        s.pause(0)
        for n in range(48, N + 1, 16):
            s.lowrank("bordered", Afull[:n, :n], Bfull[:n], trans=trans)
        s.lowrank("the same matrix again", Afull, g.standard_normal((N, 16)), trans=trans)
        s.lowrank("widening border", Aw, g.standard_normal((N + 16, 16)), trans=trans)
        s.lowrank("unrelated", A2, g.standard_normal((N + 32, 16)), trans=trans)
        s.lowrank("smaller", A2[:100, :100], g.standard_normal((100, 16)), trans=trans)
    for n in (40, 52, 63, 64, 100, 164, 100, 165):  # LU factors extended; LU form -> explicit operators; borders of 64 (extended) and 65 rows (fresh)
        s.lowrank("40->52->63->64, borders 64 / 65", Afull[:n, :n], Bfull[:n])
    # rank and spectrum
    g = np.random.default_rng(7)
    s.pause(0)
    s.lowrank("rank above n/3", stable(g, 60), g.standard_normal((60, 25)))
    n = 96
    spread = -np.diag(np.logspace(-1, 2, n)) + 0.02 * g.standard_normal((n, n))
    s.lowrank("three-decade spectrum", spread, g.standard_normal((n, 3)))
    wide = -np.diag(np.logspace(-3, 3, n)) + 1e-4 * g.standard_normal((n, n))
    s.lowrank("b/a > 1e5", wide, g.standard_normal((n, 3)))
    Cfull = g.standard_normal((n, n))
    s.pause(0)
    s.solve("indefinite full-rank C", wide, Cfull + Cfull.T)
    # the rests: an unstable matrix in a row, stable probes between
    unstable = spread.copy()
    unstable[0, 0] = 3.0
    Bu, probe, Bp = g.standard_normal((n, 3)), stable(g, 80, 14.0, 0.6), g.standard_normal((80, 5))
    s.pause(0)
    for i in range(31):
        s.lowrank("unstable", unstable, Bu)
    for i in range(35):  # Smith answers while the ADI rest counts down, then ADI
        s.lowrank("stable probe", probe, Bp)
    for i in range(130):
        s.lowrank("unstable", unstable, Bu)
        if i % 31 == 30 or i == 64:
            s.lowrank("stable probe", probe, Bp)
    s.pause(5)
    for i in range(12):
        s.lowrank("stable probe after pause 5", probe, Bp)
    s.lowrank("unstable", unstable, Bu)
    s.pause(0)
    s.lowrank("stable probe after pause 0", probe, Bp)
    # leading dimensions and bad input
    s.lowrank("lda 57, ldx 61", stable(g, 50), g.standard_normal((50, 4)), lda=57, ldx=61)
    s.lowrank("lda 70, ldx 66, N", stable(g, 64), g.standard_normal((64, 4)), lda=70, ldx=66, trans=b"N")
    S = g.standard_normal((20, 20))
    s.lowrank("symmetric, lda 23, ldx 29", -(S @ S.T) / 20 - np.eye(20), g.standard_normal((20, 4)), lda=23, ldx=29)
    s.lowrank("small, lda 12, ldx 15", stable(g, 10), g.standard_normal((10, 2)), lda=12, ldx=15)
    s.pause(30)
    s.lowrank("resting, lda 90, ldx 81", stable(g, 80), g.standard_normal((80, 4)), lda=90, ldx=81)
    s.pause(0)
    bad = stable(g, 40)
    bad[3, 5] = np.nan
    s.lowrank("NaN in A", bad, g.standard_normal((40, 2)))
    s.lowrank("unsupported dico", stable(g, 40), g.standard_normal((40, 2)), dico=b"D")


def shim_sequence(s):
    lib, g = s.lib, np.random.default_rng(5)
    for n, jobz in ((20, b"V"), (100, b"V"), (100, b"N")):
        S = g.standard_normal((n, n))
        T, w, info = padded(S + S.T, n + 3), np.zeros(n), C.c_int(-77)
        lib.rails_dsyev(jobz, b"U", n, T.ctypes.data_as(dp), n + 3, w.ctypes.data_as(dp), C.byref(info))
        print("dsyev %s n %d: a %s w %s info %d" % (jobz.decode(), n, sha(T), sha(w), info.value))
    n = 30
    d, e, z, work, info = g.standard_normal(n), g.standard_normal(n - 1), np.zeros((n, n), order="F"), np.zeros(2 * n), C.c_int(-77)
    lib.rails_dsteqr(b"I", n, d.ctypes.data_as(dp), e.ctypes.data_as(dp), z.ctypes.data_as(dp), n, work.ctypes.data_as(dp), C.byref(info))
    print("dsteqr n %d: d %s z %s info %d" % (n, sha(d), sha(z), info.value))
    for loops in ("0", "1"):  # the library's form and the loops
        os.environ["RAILS_DTRSM_LOOPS"] = loops
        for side, uplo, ta, diag in ((b"L", b"U", b"N", b"N"), (b"R", b"L", b"T", b"U"), (b"L", b"L", b"T", b"N"), (b"R", b"U", b"N", b"N")):
            m, k = 9, 6
            na = m if side == b"L" else k
            Am, Bm = padded(g.standard_normal((na, na)) + 4.0 * np.eye(na), na + 2), padded(g.standard_normal((m, k)), m + 1)
            lib.rails_dtrsm(side, uplo, ta, diag, m, k, 0.75, Am.ctypes.data_as(dp), na + 2, Bm.ctypes.data_as(dp), m + 1)
            print("dtrsm loops %s %s%s%s%s: %s" % (loops, side.decode(), uplo.decode(), ta.decode(), diag.decode(), sha(Bm)))
    del os.environ["RAILS_DTRSM_LOOPS"]
    n = 40
    Bm = g.standard_normal((n, 7))
    Am, piv, rank, info = padded(Bm @ Bm.T, n + 1), np.zeros(n, dtype=np.int32), C.c_int(-77), C.c_int(-77)
    lib.rails_dpstrf(b"U", n, Am.ctypes.data_as(dp), n + 1, piv.ctypes.data_as(ip), C.byref(rank), 1e-12 * np.abs(Am[:n]).max(), C.byref(info))
    print("dpstrf n %d: a %s piv %s rank %d info %d" % (n, sha(Am), sha(piv), rank.value, info.value))
    for m, k, r in ((60, 40, 25), (90, 30, 30)):
        Am, Q = padded(g.standard_normal((m, r)) @ g.standard_normal((r, k)), m + 2), np.zeros((m + 1, min(m, k)), order="F")
        rank, info = C.c_int(-77), C.c_int(-77)
        lib.rails_range_basis(m, k, Am.ctypes.data_as(dp), m + 2, 1e-12, Q.ctypes.data_as(dp), m + 1, C.byref(rank), C.byref(info))
        print("range_basis %d x %d: a %s q %s rank %d info %d" % (m, k, sha(Am), sha(Q), rank.value, info.value))


def compare(parent, new, label, out):
    def run(lib, env):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), lib], env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
        assert p.returncode == 0, (lib, p.returncode)
        return p.stdout.splitlines()

    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), platform.processor())
    record = {"label": label, "cpu": cpu, "settings": {}}
    for setting in ["defaults"] + [v + "=0" for v in SWITCHES]:
        env = {k: v for k, v in os.environ.items() if not k.startswith("RAILS_SB03MD_")}
        if "=" in setting:
            env[setting.split("=")[0]] = "0"
        a, b = run(parent, env), run(new, env)
        diff = [i for i in range(max(len(a), len(b))) if i >= len(a) or i >= len(b) or a[i] != b[i]]
        record["settings"][setting] = {"lines": len(a), "sha256_parent": hashlib.sha256("\n".join(a).encode()).hexdigest(), "sha256_new": hashlib.sha256("\n".join(b).encode()).hexdigest(),
                                       "equal": not diff, "last_line": a[-1] if a else None, "first_difference": None if not diff else [a[diff[0]] if diff[0] < len(a) else None, b[diff[0]] if diff[0] < len(b) else None]}
        print("%-28s %4d lines, %s" % (setting, len(a), "equal" if not diff else "DIFFERENT from line %d" % (diff[0] + 1)), flush=True)
    record["equal"] = all(v["equal"] for v in record["settings"].values())
    doc = json.load(open(out)) if os.path.exists(out) else {"what": "scripts/lyap_identity.py --compare: the parent commit's library against this one's, fixed call sequence, fresh process per setting", "runs": []}
    doc["runs"].append(record)
    doc["equal"] = all(r["equal"] for r in doc["runs"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if record["equal"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_LIB", "NEW_LIB"))
    ap.add_argument("--label", default=platform.node())
    ap.add_argument("--out", default="lyap_identity.json")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.label, args.out))
    seq = Sequence(args.lib)
    sb03md_sequence(seq)
    shim_sequence(seq)
    print("final | %s" % seq.counts())
