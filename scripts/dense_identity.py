"""Bits and launch read-backs of the dense kernels (rails_amd/csrc/dense_*.hip) over a fixed list of cases, to compare two builds of the
library: a refactoring of the host code must leave every result, every kernel choice and every counter as they were.

    python scripts/dense_identity.py --tree PATH --out ONE.json      # imports rails_amd from PATH in a fresh child process, runs the cases
    python scripts/dense_identity.py --compare PARENT.json NEW.json --out profiles/dense_refactor_identity.json

The cases are run by tests/dense_choice_cases.py of THIS tree on the library of the tree given: the rows of this tree's
rails_amd/lib/dense_choice_host --table (one shape per instantiation), the shapes of tests/test_gpu_tile_fit.py with the tile fit on and
off, and one call per entry point with everything at its default (the library GEMM included: not asked for).  Per case: the SHA-256 of
the bytes the call wrote with what lies around the written window, what rails_dense_last_tiles and rails_dense_last_update_gram_form
say afterwards, and how far the context's update_gram_fused counter moved."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dense_choice_cases as cases

    out = cases.table()
    # tests/test_gpu_tile_fit.py: the fused pass around the edges of five blocks per wave, the wide-X Gram around five tiles per wave, the
    # rotation at 13, 15, 17 output tiles and their even neighbours with the last chunk's second half past k and not
    for fit in (1, 0):
        sw = {"tile_fit": fit}
        for k in (257, 268, 319, 320, 321, 384):
            for r, r2 in ((17, 16), (16, 16)):
                out.append({"primitive": "update_gram", "m": 4099, "k": k, "r": r, "r2": r2, "switches": sw})
        for a in (273, 285, 288, 289, 304, 320, 321, 336):
            for b in (16, 17):
                out.append({"primitive": "gram", "m": 4099, "a": a, "b": b, "switches": sw})
        for r in (200, 232, 241, 257, 268, 272, 273, 288):
            for k in (324, 336, 337, 352, 353, 357, 368):
                out.append({"primitive": "gemm_wide", "m": 1003, "k": k, "r": r, "switches": sw})
        out.append({"primitive": "gemm_wide", "m": 1003, "k": 357, "r": 268, "alpha": -0.5, "beta": 1.0, "switches": sw})
    # one call per entry point, nothing set: a Gram product, a panel GEMM, a rotation in two slices, the fused pass and its two-kernel
    # form (too few rows), the deflated orthogonalisation
    out += [{"primitive": "gram", "m": 20011, "a": 369, "b": 17}, {"primitive": "panel_gemm", "m": 20011, "k": 352, "r": 16},
            {"primitive": "gemm_wide", "m": 20011, "k": 324, "r": 300}, {"primitive": "gemm_wide", "m": 1003, "k": 20, "r": 300},
            {"primitive": "update_gram", "m": 20011, "k": 352, "r": 17, "r2": 16}, {"primitive": "update_gram", "m": 1003, "k": 352, "r": 17, "r2": 16},
            {"primitive": "gram2", "m": 20011, "a": 304, "b": 17}]
    return cases, out


def child(tree, path):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import numpy as np
    import rails_amd

    assert os.path.dirname(os.path.abspath(rails_amd.__file__)) == os.path.join(tree, "rails_amd"), rails_amd.__file__
    cases, todo = rows()
    out = {}
    ctx = rails_amd.Context(device=0, seed=5)
    for n, row in enumerate(todo):
        assert not cases.env_of(row), row
        arrays, launched, _, _ = cases.run_row(rails_amd, ctx, row)
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        out["%03d %s" % (n, cases.row_id(row))] = {"sha256": h.hexdigest(), "launched": launched}
    ctx.close()
    with open(path, "w") as fh:
        json.dump({"cases": out}, fh)
    print("%d cases" % len(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="the tree to import rails_amd from (built)")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT.json", "NEW.json"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds the child process may take")
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
        child(a.tree, a.out)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", a.tree, "--out", a.out], timeout=a.timeout)
    sys.exit(p.returncode)


if __name__ == "__main__":
    main()
