"""The rule of the iterative A^-1 operator's preconditioners (rails_amd/csrc/iter_precond.h), restated: whether a request to turn a
preconditioner on is granted on an object of given facts, with the refusal's text, and what is in effect for a call.  The texts are the
strings the library's sources held before the rule was gathered into the header (rails_iter_set, amg_check, bamg_check,
rails_iter_block_jacobi and rails_iter_amg_setup of itsolve.hip), copied from there, and the reasons are tried in the order they were tried
there.  tests/test_iter_precond_host.py compares the header with this over the whole product of `product()`, line by line of
`iter_precond_host --table`; tests/test_gpu_iter_precond.py compares the library's messages with the same lines."""
import itertools

OPS = ("stored", "stored_nohost", "bsr", "bsr_nohost", "callback", "lu", "iter")
BLOCK = 3
ROWS = (3000, 3001, 16777218, 16777217)
POLY = 5
W = {n: i for i, n in enumerate(("X", "R", "P", "Q", "Z", "RH", "T", "SH", "D", "Z2"))}
# (request, the function that reports, the values it is made with)
REQUESTS = (("poly_degree", "rails_iter_set", (0, POLY)), ("amg", "rails_iter_set", (1,)), ("block_amg", "rails_iter_set", (1,)), ("block_jacobi", "rails_iter_set", (1,)),
            ("install_blocks", "rails_iter_block_jacobi", (BLOCK,)), ("amg_setup", "rails_iter_amg_setup", (1,)), ("block_amg_setup", "rails_iter_block_amg_setup", (1,)))
WHO = {r: who for r, who, _ in REQUESTS}
FIELDS = ("cg", "op", "reduces", "exchanges", "m", "diag", "blocks", "defsign", "jacobi", "poly_degree", "amg", "block_amg", "block_jacobi")


def facts(cg=1, op="stored", reduces=0, exchanges=0, m=3000, diag=1, blocks=0, defsign=1, jacobi=1, poly_degree=0, amg=0, block_amg=0, block_jacobi=0):
    """cg: conjugate gradients (0: BiCGStab); op: one of OPS (a block-CSR operator has block size BLOCK); blocks: the size of the installed
    diagonal blocks (0: none); diag: the inverse diagonal exists; the five settings"""
    assert op in OPS
    return dict(zip(FIELDS, (int(cg), op, int(reduces), int(exchanges), int(m), int(diag), int(blocks), int(defsign), int(jacobi), int(poly_degree), int(amg), int(block_amg),
                             int(block_jacobi))))


def key(f):
    return " ".join("%s=%s" % (n, f[n]) for n in FIELDS)


def bamg_rows_ok(m, b):
    return 2 <= b <= 8 and m >= b and m % b == 0 and m < 2 ** 24


def _amg(f, who, setup):
    if not f["cg"]:
        return '%s: "amg" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)' % who
    if f["poly_degree"]:
        return '%s: "amg" together with poly_degree %d: one preconditioner at a time' % (who, f["poly_degree"])
    if f["block_jacobi"]:
        return '%s: "amg" together with "block_jacobi": one preconditioner at a time' % who
    if f["block_amg"]:
        return '%s: "amg" together with "block_amg": one preconditioner at a time' % who
    if f["op"] == "callback":
        return '%s: "amg" needs the entries of the matrix: the operator is a callback' % who
    if f["op"] in ("lu", "iter"):
        return '%s: "amg" needs the entries of the matrix: the operator is an LU or an iterative solve' % who
    if f["op"].startswith("bsr"):
        return '%s: "amg" needs the entries of the matrix as scalar CSR arrays: the operator is block-CSR (keep a CSR handle for the preconditioner)' % who
    if f["reduces"] or f["exchanges"]:
        return '%s: "amg" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU' % who
    if f["m"] >= 2 ** 24:
        return '%s: "amg" on %d rows: the multigrid preconditioner takes fewer than 2^24' % (who, f["m"])
    if setup and f["op"] != "stored":
        return "rails_iter_amg_setup: the operator keeps no CSR arrays on the host to build the hierarchy from"
    return None


def _block_amg(f, who):
    if not f["cg"]:
        return '%s: "block_amg" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)' % who
    if f["poly_degree"]:
        return '%s: "block_amg" together with poly_degree %d: one preconditioner at a time' % (who, f["poly_degree"])
    if f["block_jacobi"]:
        return '%s: "block_amg" together with "block_jacobi": one preconditioner at a time' % who
    if f["amg"]:
        return '%s: "block_amg" together with "amg": one preconditioner at a time' % who
    if f["op"] != "bsr":
        return '%s: "block_amg" needs the blocks of the matrix: the operator is not a block-CSR handle with a host copy (rails_csr_create_bsr)' % who
    if f["reduces"]:
        return '%s: "block_amg" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU' % who
    if not bamg_rows_ok(f["m"], BLOCK):
        return '%s: "block_amg" on %d rows of block size %d: the multigrid cycle\'s kernels address fewer than 2^24 rows' % (who, f["m"], BLOCK)
    return None


def refusal(f, request, value):
    """None where the request is granted, else the text"""
    who = WHO[request]
    if request == "poly_degree":
        if value == 0:
            return None
        if f["amg"]:
            return 'rails_iter_set: poly_degree %g together with "amg": one preconditioner at a time' % value
        if f["block_jacobi"]:
            return 'rails_iter_set: poly_degree %g together with "block_jacobi": one preconditioner at a time' % value
        if f["block_amg"]:
            return 'rails_iter_set: poly_degree %g together with "block_amg": one preconditioner at a time' % value
        if not f["cg"]:
            return "rails_iter_set: poly_degree %g on a BiCGStab object: the polynomial preconditioner is for conjugate gradients (a real spectrum)" % value
        return None
    if request == "block_jacobi":
        if not f["blocks"]:
            return 'rails_iter_set: "block_jacobi" 1 without blocks: install them first (rails_iter_block_jacobi)'
        if f["poly_degree"]:
            return 'rails_iter_set: "block_jacobi" together with poly_degree %d: one preconditioner at a time' % f["poly_degree"]
        if f["amg"]:
            return 'rails_iter_set: "block_jacobi" together with "amg": one preconditioner at a time'
        if f["block_amg"]:
            return 'rails_iter_set: "block_jacobi" together with "block_amg": one preconditioner at a time'
        return None
    if request == "install_blocks":
        if f["poly_degree"]:
            return "rails_iter_block_jacobi: together with poly_degree %d: one preconditioner at a time" % f["poly_degree"]
        if f["amg"]:
            return 'rails_iter_block_jacobi: together with "amg": one preconditioner at a time'
        if f["block_amg"]:
            return 'rails_iter_block_jacobi: together with "block_amg": one preconditioner at a time'
        return None
    if request in ("amg", "amg_setup"):
        return _amg(f, who, request == "amg_setup")
    if request in ("block_amg", "block_amg_setup"):
        return _block_amg(f, who)
    raise KeyError(request)


def effect(f):
    """{"pass": 0 nothing, 1 the diagonal, 2 the blocks; "b"; "beyond": 0 nothing, 1 the polynomial, 2 the scalar cycle, 3 the block cycle;
    "K"; "sign"; "panels": the bit mask over W}"""
    bj = f["blocks"] if f["block_jacobi"] and f["blocks"] else 0
    jac = bool(bj) or bool(f["jacobi"] and f["diag"])
    K = f["poly_degree"]
    cycle = bool(f["amg"] or f["block_amg"])
    other = K > 0 or cycle
    panels = 0
    g = bool(f["diag"] or f["blocks"])  # what exists, not what is on
    for name, k in W.items():
        if name in ("D", "Z2"):
            uses = other
        elif name == "Z" and other:
            uses = True
        elif f["cg"]:
            uses = name in ("X", "R", "P", "Q") or (name == "Z" and g)
        else:
            uses = name in ("X", "R", "P", "Q", "RH", "T") or (name in ("Z", "SH") and g)
        panels |= int(uses) << k
    return {"pass": 2 if bj else 1 if jac else 0, "b": bj, "beyond": 3 if f["block_amg"] else 2 if f["amg"] else 1 if K > 0 else 0, "K": 0 if cycle else K,
            "sign": 1 if (jac or other) else f["defsign"], "panels": panels}


def product():
    """every combination of facts the host program runs over, in its order"""
    for cg, op, net, m, have, on in itertools.product((0, 1), OPS, range(4), ROWS, range(8), range(32)):
        yield facts(cg, op, net & 1, (net >> 1) & 1, m, have & 1, BLOCK if have & 2 else 0, -1 if have & 4 else 1, on & 1, POLY if on & 2 else 0, (on >> 2) & 1, (on >> 3) & 1,
                    (on >> 4) & 1)


def effect_line(f):
    e = effect(f)
    return "E %s | pass=%d b=%d beyond=%d K=%d sign=%d panels=%d" % (key(f), e["pass"], e["b"], e["beyond"], e["K"], e["sign"], e["panels"])


def request_line(f, request, value):
    return "R %s | %s %d | %s" % (key(f), request, value, refusal(f, request, value) or "granted")


def table():
    """the lines of `iter_precond_host --table`, in its order"""
    for f in product():
        yield effect_line(f)
        if f["defsign"] < 0:
            continue
        for request, _, values in REQUESTS:
            for v in values:
                yield request_line(f, request, v)
