"""Command-line driver: solve A X M' + M X A' + B B' = 0 for X = V T V' with matrices from MatrixMarket files.

    python -m rails_amd.main [params.xml] [--dir DIR] [--A A.mtx] [--B B.mtx] [--M M.mtx] [--V V.mtx] [--T T.mtx]
                               [--eigs K] [--variance FILE] [--pairs FILE [--pairs-out FILE]]
                               [--maps R1,R2,... [--correlation] [--maps-out FILE.mtx]] [--sparse-B] [--warm-start V.mtx | --start-space S.mtx] [--restart-upon-start]
                               [--inverse {lu,cg,bicgstab,iterative}] [--inverse-tol T] [--inverse-poly K] [--inverse-amg] [--block-size b]
                               [--inverse-block-jacobi] [--inverse-block-amg]
    python -m torch.distributed.run --nproc-per-node N -m rails_amd.main ... [--backend {nccl,gloo}] [--one-device]
                                                                                  (one rank per GPU, rows partitioned)

File names, formats and the parameter file follow the reference's driver (src/main.cpp:57-68,111,123-126): `A.mtx`, `B.mtx`
and `M.mtx` in, `V.mtx` and `T.mtx` out, solver parameters from the "Lyapunov Solver" sublist of a Teuchos XML file.  A diagonal
mass matrix with zeros on its diagonal (a descriptor system) is handled as the reference's driver does (src/main.cpp:77-99): the
Lyapunov equation is solved on the Schur complement A22 - A21 A11^-1 A12 of the rows where M is nonzero (rails_amd/schur.py; one
rank), B is restricted to those rows and V has that many rows.  Otherwise M must be absent (identity) or symmetric positive
definite.

`--sparse-B` keeps B sparse, as the reference's driver does (src/main.cpp:67 reads B.mtx as a CrsMatrix, :98 hands the operator to the
solver): B.mtx is read as CSR and goes to the solver as a rails_amd.SparseRHS (one rank, direct back end); after a Schur reduction it
keeps the rows of the Schur complement.

`--inverse` chooses the A^-1 of a "Projection method" above 1 (opts.Ainv, matlab/RAILSsolver.m:19-23): `lu` (the default) a sparse LU
factorised on the host and applied on the device, `cg` / `bicgstab` an iteration on the device to the relative tolerance `--inverse-tol`
(rails_amd.IterativeInverse; the reference allows an approximate inverse), `iterative` conjugate gradients when A equals its transpose and
BiCGStab otherwise.  `--inverse-poly K` preconditions the conjugate gradients with a Chebyshev polynomial of degree K (K products in a
row without an inner product between them; 0, the default, is off); with an inverse that resolves to BiCGStab the driver refuses it.
`--inverse-amg` preconditions them with one V-cycle of smoothed-aggregation multigrid instead (rails_amd.IterativeInverse(amg=True): an
iteration count that does not grow with the grid); the driver refuses it together with `--inverse-poly`, with an inverse that resolves to
BiCGStab, with the sparse LU and on more than one rank.  A
Schur-complement problem keeps the inverse of its Schur operator.  On more than one rank the sparse LU is not available (a factorisation
does not partition by rows): name one of the iterative inverses there.  Each rank then builds its inverse from its own row block, the
inner products of the iteration are all-reduced, and `iterative` decides symmetry on the whole matrix, which every rank has read.  No run
on more than one GPU has been made yet; what an inner iteration costs on a real partition is unmeasured.

`--block-size b` (2 .. 8) keeps A, and M when given, as block-CSR operators of dense b x b blocks (rails_amd.HipOperatorWrapper.from_bsr;
the matrix of a PDE system with b unknowns per cell): the files are read as before and converted on the host, zeros filling the touched
blocks, and the driver prints the blocks, the fill ratio (stored entries over the file's) and the bytes on the device.  The number of rows
must be a multiple of b, and the run has one rank (a block-CSR operator is single GPU).  The inverse of a "Projection method" above 1 is
built from the CSR arrays unless `--inverse-block-jacobi` is given: an iterative inverse (`--inverse cg`, `bicgstab` or `iterative`) then
iterates on the block-CSR operator itself and preconditions with the inverses of its b x b diagonal blocks
(rails_amd.IterativeInverse(block_jacobi=True): for a matrix whose coupling inside a cell is the stiff part, where the scalar diagonal
says little).  The driver prints b, the number of blocks and, after the solve, the iterations the solve's first application of the inverse
took (the solver reaches the inverse through a callback handle that notes them); it refuses the flag without `--block-size`, together
with `--inverse-poly` or `--inverse-amg`, with the sparse LU and on more than one rank, and says so when "Projection method" 1 makes it
moot.

`--inverse-block-amg` (with `--block-size b` and a conjugate-gradients inverse, `--inverse cg` or `iterative` on a symmetric matrix)
iterates on the block-CSR operator as well and preconditions with one V-cycle of block multigrid
(rails_amd.IterativeInverse(block_amg=True): for a diffusion-dominated system on a fine grid, where block Jacobi's iteration count grows
with the grid).  The driver prints b, the rows of the levels, the operator complexity and the set-up time, and after the solve the cycles,
products and launches of the last application; it refuses the flag without `--block-size`, together with `--inverse-poly`,
`--inverse-amg` or `--inverse-block-jacobi`, with the sparse LU or BiCGStab and on more than one rank.

`--backend gloo` runs the collectives through torch.distributed's gloo backend, staged through host memory, and `--one-device` puts every
rank on device 0: a rehearsal of the multi-process path on a machine with one GPU, as bench.py has it.

`--eigs K` and `--variance FILE` are the second half of the reference's driver (src/main.cpp:140-170) on the solution object
(rails_amd.Solution): the K eigenvalues of largest modulus of the covariance X, each next to its share of the trace, written to
`eigenvalues.mtx` / `eigenvectors.mtx`, and the pointwise variance diag(X).  After a Schur reduction both refer to the solution lifted to
all unknowns (SchurOperator.lift), in the original row order.  `--pairs FILE` (lines `i j`, 1-based) writes the covariances X[i, j] and
`--maps R1,R2,...` the covariance (`--correlation`: correlation) of every unknown with the reference unknowns, on the same object.
"""
import argparse
import os
import sys
import time

import numpy as np


def _log(rank, *a):
    if rank == 0:
        print(*a, flush=True)


def _read_indices(text, what, m_all):
    """1-based integers -> 0-based int64 array, every one inside [0, m_all)"""
    try:
        idx = np.array([int(t) for t in text], dtype=np.int64) - 1
    except ValueError:
        raise SystemExit("%s: not an integer in %r" % (what, text[:4]))
    if idx.size and (idx.min() < 0 or idx.max() >= m_all):
        raise SystemExit("%s: indices are 1-based and at most %d, got %d" % (what, m_all, int(idx[(idx < 0) | (idx >= m_all)][0]) + 1))
    return idx


def read_pairs(file, m_all):
    """--pairs FILE: lines `i j`, 1-based (lines starting with % or # are comments) -> two 0-based int64 arrays"""
    lines = [ln.split() for ln in open(file) if ln.strip() and not ln.lstrip().startswith(("%", "#"))]
    if any(len(t) != 2 for t in lines):
        raise SystemExit("--pairs: every line of %s holds two integers" % file)
    return _read_indices([t[0] for t in lines], "--pairs", m_all), _read_indices([t[1] for t in lines], "--pairs", m_all)


def read_refs(text, m_all):
    """--maps R1,R2,...: 1-based reference unknowns -> 0-based int64 array of 1 to 64 entries"""
    ref = _read_indices([t for t in text.split(",") if t.strip()], "--maps", m_all)
    if not 1 <= ref.size <= 64:
        raise SystemExit("--maps: between 1 and 64 reference unknowns, got %d" % ref.size)
    return ref


def _write_pairs(args, pairs, sol, path, rank, world, r0, dist):
    """--pairs: X[i, j] for every pair, through Solution.covariance (one pass on the device)"""
    from rails_amd import mmio

    ia, ib = pairs
    if world == 1:
        cov = sol.covariance(ia.astype(np.int32), ib.astype(np.int32)) if ia.size else np.zeros(0)
    else:  # every rank does the pairs it holds both unknowns of; a pair nobody holds whole is an error
        mine = (ia >= r0) & (ia < r0 + sol.m) & (ib >= r0) & (ib < r0 + sol.m)
        part = np.zeros(ia.size)
        if mine.any():
            part[mine] = sol.covariance((ia[mine] - r0).astype(np.int32), (ib[mine] - r0).astype(np.int32))
        parts = [None] * world
        dist.all_gather_object(parts, (mine, part))
        held = sum(p[0].astype(int) for p in parts)
        if np.any(held != 1):
            raise SystemExit("--pairs: pair %d has its two unknowns on different ranks (not supported)" % (int(np.flatnonzero(held != 1)[0]) + 1))
        cov = sum(p[1] for p in parts)
    if rank == 0:
        mmio.write_array(path(args.pairs_out), cov.reshape(-1, 1), comment="rails_amd: X[i, j] for the pairs of %s, X = V T V'" % args.pairs)
        print("wrote %s (%d x 1)" % (path(args.pairs_out), cov.size), flush=True)


def _write_maps(args, ref, sol, path, rank, world, r0, dist):
    """--maps: the covariance (--correlation: correlation) of every unknown with the reference unknowns, through Solution.maps"""
    from rails_amd import mmio

    local = np.where((ref >= r0) & (ref < r0 + sol.m), ref - r0, -1).astype(np.int32)
    out = sol.maps(local, correlation=args.correlation)
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, out)
        out = np.vstack(parts)
    if rank == 0:
        what = "correlation" if args.correlation else "covariance"
        mmio.write_array(path(args.maps_out), out, comment="rails_amd: the %s of every unknown with unknowns %s of X = V T V'" % (what, args.maps))
        print("wrote %s (%d x %d, %s)" % (path(args.maps_out), out.shape[0], out.shape[1], what), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m rails_amd.main", description=__doc__.split("\n\n")[0])
    ap.add_argument("params", nargs="?", help="Teuchos XML (or JSON) parameter file; the 'Lyapunov Solver' sublist is used")
    ap.add_argument("--dir", default=".", help="directory of the input / output files")
    ap.add_argument("--A", default="A.mtx")
    ap.add_argument("--B", default="B.mtx")
    ap.add_argument("--M", default="M.mtx", help="mass matrix (used when the file exists unless --no-mass)")
    ap.add_argument("--no-mass", action="store_true", help="solve the standard equation (M = I) even if M.mtx exists")
    ap.add_argument("--V", default="V.mtx")
    ap.add_argument("--T", default="T.mtx")
    ap.add_argument("--warm-start", default=None, help="V.mtx of a previous solve (orthonormal columns): sets 'Restart from solution'")
    ap.add_argument("--start-space", default=None, metavar="FILE.mtx", help="a raw start space (opts.space): any columns -- a previous V, [V, B], several "
                                                                            "solutions side by side; orthonormalised on the device, dependent columns dropped")
    ap.add_argument("--restart-upon-start", action="store_true", help="shrink the space right after the first projected solve (opts.restart_upon_start; "
                                                                      "'Restart upon start' in the parameter file)")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="override one solver parameter, e.g. --set 'Tolerance=1e-6'")
    ap.add_argument("--nullspace", default=None, help="N.mtx (dense array): a space projected out of the solution space (opts.nullspace), "
                                                      "with the rows of the equation solved (the Schur rows after a Schur reduction)")
    ap.add_argument("--eigs", type=int, default=0, metavar="K", help="print the K leading eigenvalues of X and their share of the trace "
                                                                   "(src/main.cpp:162-168); writes eigenvalues.mtx and eigenvectors.mtx")
    ap.add_argument("--variance", default=None, metavar="FILE", help="write diag(X), the pointwise variance, to FILE (MatrixMarket array)")
    ap.add_argument("--pairs", default=None, metavar="FILE", help="two integer columns, 1-based as MatrixMarket: the pairs (i, j) of unknowns whose covariance "
                    "X[i, j] is wanted (after a Schur reduction: indices of the original row order); on several ranks both unknowns of a pair must be on one rank")
    ap.add_argument("--pairs-out", default="pairs.mtx", metavar="FILE", help="where the covariances of --pairs go (MatrixMarket array, n x 1)")
    ap.add_argument("--maps", default=None, metavar="R1,R2,...", help="one-point maps: the covariance of every unknown with each of these (1-based, at most 64) "
                    "reference unknowns")
    ap.add_argument("--correlation", action="store_true", help="the maps of --maps as correlations X[i, r] / sqrt(X[i, i] X[r, r])")
    ap.add_argument("--maps-out", default="maps.mtx", metavar="FILE.mtx", help="where the maps go (MatrixMarket array, m x q)")
    ap.add_argument("--direct", action="store_true", help="direct back end (device panels for V, AV) instead of the default coordinate-space back end")
    ap.add_argument("--projected-lanczos", action="store_true", help="direct back end with the coefficient-space residual Lanczos (M = I only)")
    ap.add_argument("--sparse-B", action="store_true", help="keep B sparse (B.mtx in coordinate format): a device CSR operator instead of a dense panel; one rank")
    ap.add_argument("--inverse", choices=("lu", "cg", "bicgstab", "iterative"), default="lu", help="the A^-1 of a 'Projection method' above 1: a sparse LU (default), "
                                                                                                   "or an iteration on the device (iterative: CG for a symmetric A, BiCGStab otherwise)")
    ap.add_argument("--inverse-tol", type=float, default=1e-10, metavar="T", help="relative tolerance of an iterative inverse (per column)")
    ap.add_argument("--inverse-poly", type=int, default=0, metavar="K", help="degree of the Chebyshev polynomial preconditioner of a conjugate-gradients inverse "
                                                                            "(K products per application; 0: off)")
    ap.add_argument("--inverse-amg", action="store_true", help="precondition a conjugate-gradients inverse with a smoothed-aggregation multigrid V-cycle "
                                                             "(one rank; not together with --inverse-poly)")
    ap.add_argument("--inverse-block-jacobi", action="store_true", help="build an iterative inverse on the block-CSR operator of --block-size b and precondition it with "
                                                                      "the inverses of the b x b diagonal blocks (one rank; not together with --inverse-poly or "
                                                                      "--inverse-amg)")
    ap.add_argument("--inverse-block-amg", action="store_true", help="build a conjugate-gradients inverse on the block-CSR operator of --block-size b and precondition "
                                                                   "it with one V-cycle of block multigrid (one rank; not together with --inverse-poly, "
                                                                   "--inverse-amg or --inverse-block-jacobi)")
    ap.add_argument("--block-size", type=int, default=0, metavar="b", help="keep A (and M) as block-CSR operators of b x b blocks, 2 .. 8; the rows must be a multiple of b; "
                                                                          "one rank")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend of a run on several ranks; gloo = rehearsal of the "
                                                                                "multi-process path (collectives staged through host memory)")
    ap.add_argument("--one-device", action="store_true", help="every rank uses device 0 (rehearsal on a machine with one GPU)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    if args.block_size and not 2 <= args.block_size <= 8:
        raise SystemExit("--block-size %d: blocks of 2 .. 8" % args.block_size)
    if args.block_size and int(os.environ.get("WORLD_SIZE", "1")) > 1:  # refused before the ranks meet
        raise SystemExit("--block-size on %s ranks: a block-CSR operator is single GPU" % os.environ["WORLD_SIZE"])
    # The early refusals of the preconditioner flags below (and of --inverse-amg further down) restate, for the command line and in its
    # words, what the library's one rule decides for an object: rails_amd/csrc/iter_precond.h (one preconditioner at a time, single GPU).
    if args.inverse_block_jacobi:  # what the arguments alone decide, before anything is read or built
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--inverse-block-jacobi on %s ranks: the block-Jacobi preconditioner is single GPU" % os.environ["WORLD_SIZE"])
        if not args.block_size:
            raise SystemExit("--inverse-block-jacobi needs --block-size b: the diagonal blocks are those of the block-CSR operator")
        if args.inverse_poly:
            raise SystemExit("--inverse-block-jacobi together with --inverse-poly %d: one preconditioner at a time" % args.inverse_poly)
        if args.inverse_amg:
            raise SystemExit("--inverse-block-jacobi together with --inverse-amg: one preconditioner at a time")
        if args.inverse == "lu":
            raise SystemExit("--inverse-block-jacobi: the block-Jacobi preconditioner is for an iterative inverse (--inverse cg, bicgstab or iterative), and the "
                             "inverse chosen is a sparse LU")
    if args.inverse_block_amg:  # what the arguments alone decide, before anything is read or built
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--inverse-block-amg on %s ranks: the block multigrid preconditioner is single GPU" % os.environ["WORLD_SIZE"])
        if not args.block_size:
            raise SystemExit("--inverse-block-amg needs --block-size b: the hierarchy is built from the block-CSR operator")
        if args.inverse_poly:
            raise SystemExit("--inverse-block-amg together with --inverse-poly %d: one preconditioner at a time" % args.inverse_poly)
        if args.inverse_amg:
            raise SystemExit("--inverse-block-amg together with --inverse-amg: one preconditioner at a time")
        if args.inverse_block_jacobi:
            raise SystemExit("--inverse-block-amg together with --inverse-block-jacobi: one preconditioner at a time")
        if args.inverse == "lu":
            raise SystemExit("--inverse-block-amg: the block multigrid preconditioner is for a conjugate-gradients inverse (--inverse cg or iterative), and the "
                             "inverse chosen is a sparse LU")
        if args.inverse == "bicgstab":
            raise SystemExit("--inverse-block-amg: the block multigrid preconditioner is for conjugate gradients, and the inverse chosen is bicgstab")

    import torch

    import rails_amd
    from rails_amd import mmio, partition

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.one_device else int(os.environ.get("LOCAL_RANK", "0"))
    staged = args.backend != "nccl"  # device buffers travel through host tensors
    dist = None
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo")

    def path(name):
        return name if os.path.isabs(name) else os.path.join(args.dir, name)

    params = mmio.read_parameters(args.params) if args.params else {}
    for kv in args.set:
        k, _, v = kv.partition("=")
        params[k.strip()] = float(v)
    if "restart_upon_start" in params:  # the reference's (MATLAB) spelling
        params["Restart upon start"] = params.pop("restart_upon_start")
    if args.restart_upon_start:
        params["Restart upon start"] = 1
    if args.start_space and args.warm_start:
        raise SystemExit("--start-space and --warm-start: give one of them")

    _log(rank, "Loading matrices")
    t0 = time.time()
    m, n, rowptr, col, val = mmio.read_csr(path(args.A))
    if m != n:
        raise SystemExit("A must be square, got %d x %d" % (m, n))
    if args.sparse_B:
        if world > 1:
            raise SystemExit("--sparse-B: a sparse right-hand side runs on one rank")
        import scipy.sparse as sp

        bm, bp, brp, bcol, bval = mmio.read_csr(path(args.B))
        B = sp.csr_matrix((bval, bcol, brp), shape=(bm, bp))
    else:
        B = mmio.read_dense(path(args.B))
    if B.shape[0] != m:
        raise SystemExit("B has %d rows, A has %d" % (B.shape[0], m))
    # the unknowns --pairs and --maps name are those of A as given (after a Schur reduction: of the lifted solution), checked before the solve
    pairs = read_pairs(path(args.pairs), m) if args.pairs else None
    refs = read_refs(args.maps, m) if args.maps else None
    Mcsr = None
    if not args.no_mass and os.path.exists(path(args.M)):
        mm, mn, mrp, mcol, mval = mmio.read_csr(path(args.M))
        if (mm, mn) != (m, m):
            raise SystemExit("M must be %d x %d" % (m, m))
        Mcsr = (mrp, mcol, mval)
    V0 = mmio.read_dense(path(args.warm_start)) if args.warm_start else None
    S0 = mmio.read_dense(path(args.start_space)) if args.start_space else None
    Nsp = mmio.read_dense(path(args.nullspace)) if args.nullspace else None
    if V0 is not None:
        params["Restart from solution"] = 1
    _log(rank, "  A %d x %d, %d nonzeros; B %d x %d; %s; read in %.2f s" % (m, m, val.size, B.shape[0], B.shape[1],
                                                                          "M given" if Mcsr else "M = I", time.time() - t0))

    # one non-default torch stream for the library and the collectives (see bench.py)
    tstream = torch.cuda.Stream(device=local_rank)
    torch.cuda.set_stream(tstream)
    ctx = rails_amd.Context(device=local_rank, stream=tstream.cuda_stream, seed=args.seed)
    starts = partition.row_ranges(m, world)
    r0, r1 = int(starts[rank]), int(starts[rank + 1])
    ctx.set_partition(rank, world, r0, m)

    def operator(csr, name="A"):
        rp, cg, vv = csr
        if args.block_size:
            b, rows = args.block_size, len(rp) - 1
            if rows % b:
                raise SystemExit("--block-size %d: %s has %d rows, no multiple of %d" % (b, name, rows, b))
            op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *rails_amd.csr_to_bsr(rows, rows, b, rp, cg, vv))
            st = op.bsr_stats()
            _log(rank, "  %s as block-CSR: %d blocks of %d x %d, fill ratio %.3f (%d stored entries for %d), %d bytes on the device" % (
                name, st["nnzb"], b, b, st["nnzb"] * b * b / max(1, len(vv)), st["nnzb"] * b * b, len(vv), st["device_bytes"]))
            return op
        if world == 1:
            return rails_amd.HipOperatorWrapper(ctx, rp, cg.astype(np.int32), vv)
        p0, p1 = rp[r0], rp[r1]
        plan = partition.HaloPlan(starts, rank, cg[p0:p1], partition.all_gather_object_fn())
        op = rails_amd.HipOperatorWrapper(ctx, (rp[r0:r1 + 1] - p0).astype(np.int64), plan.col_local, vv[p0:p1], ncols_ext=plan.m_local + plan.n_ghost)
        op.set_halo(plan, partition.make_halo(plan, on_device=True, host_staged=staged))
        return op

    schur = None
    if Mcsr is not None:
        mrp, mcol, mval = Mcsr
        rows = np.repeat(np.arange(m), np.diff(mrp))
        diagonal = bool(np.all(rows == mcol))
        mdiag = np.zeros(m)
        mdiag[rows[rows == mcol]] = mval[rows == mcol]
        if diagonal and np.any(mdiag == 0.0):
            if world > 1:
                raise SystemExit("a singular mass matrix (Schur complement) runs on one rank, as in the reference (src/SchurOperator.cpp:226)")
            from rails_amd.schur import SchurOperator

            _log(rank, "Computing Schur complement")
            t0 = time.time()
            schur = SchurOperator(ctx, (rowptr, col, val), mdiag)
            _log(rank, "  %d algebraic rows eliminated, %d remain; A11 factorised in %.2f s" % (schur.m1, schur.m2, time.time() - t0))
            if args.sparse_B:  # the rows of the Schur complement; the correction A21 A11^-1 B1 of restrict() would fill B
                B1 = B[schur.idx1]
                if B1.nnz and np.abs(B1.data).max() > np.sqrt(np.finfo(float).eps):
                    raise SystemExit("--sparse-B: B has entries on the eliminated rows; run without --sparse-B")
                B = B[schur.idx2]
            else:
                B = schur.restrict(B)
            if V0 is not None and V0.shape[0] == m:
                V0 = V0[schur.idx2]
            if S0 is not None and S0.shape[0] == m:
                S0 = S0[schur.idx2]
            d2 = schur.mass22
            Mcsr = None if np.all(d2 == 1.0) else (np.arange(schur.m2 + 1, dtype=np.int64), np.arange(schur.m2, dtype=np.int64), d2)
            m = schur.m2
            r0, r1 = 0, m
            ctx.set_partition(0, 1, 0, m)
        elif not diagonal and np.any(mdiag == 0.0):
            raise SystemExit("M has zero diagonal entries but is not diagonal: not supported")

    if Nsp is not None and Nsp.shape[0] != m:
        raise SystemExit("--nullspace: N has %d rows, the equation solved has %d%s" % (Nsp.shape[0], m, " (the rows of the Schur complement)" if schur is not None else ""))
    _log(rank, "Creating solver")
    A = schur.op if schur is not None else operator((rowptr, col, val))
    Mop = operator(Mcsr, "M") if Mcsr else None
    if world > 1:
        ctx.set_allreduce(partition.make_allreduce(on_device=True, host_staged=staged))
    solver = rails_amd.Solver(ctx, A, B if args.sparse_B else B[r0:r1], M=Mop, m_global=m)
    code = solver.set_parameters(params)
    if code != 0:
        raise SystemExit("set_parameters rejected the parameter set (code %d)" % code)
    solver.set_option("verbose", 0 if (args.quiet or rank != 0) else 1)
    if Mop is not None:
        solver.set_option("mass", 1)
    if args.direct or args.projected_lanczos:
        solver.set_option("subspace", 0)
    if args.projected_lanczos and Mop is None:
        solver.set_option("projected_lanczos", 1)
    if Nsp is not None:
        solver.set_nullspace(Nsp[r0:r1])  # each rank its own rows, like B
    # "Projection method" above 1 (opts.projection_method, matlab/RAILSsolver.m:7-24): the driver builds the inverse it needs
    method = next((float(v) for k, v in params.items() if k.lower() == "projection method"), 1.0)
    inverse = None
    if method > 1 and args.inverse_amg:  # refused before anything is built (the rule itself: rails_amd/csrc/iter_precond.h)
        if args.inverse_poly:
            raise SystemExit("--inverse-amg together with --inverse-poly %d: one preconditioner at a time" % args.inverse_poly)
        if world > 1:
            raise SystemExit("--inverse-amg on %d ranks: the multigrid preconditioner is single GPU" % world)
        if args.inverse == "lu" or schur is not None:
            raise SystemExit("--inverse-amg: the multigrid preconditioner is for a conjugate-gradients inverse (--inverse cg or iterative), and the inverse chosen is "
                             "a sparse LU")
    if args.inverse_block_jacobi and method <= 1:
        _log(rank, "--inverse-block-jacobi has no effect: 'Projection method' %g applies no inverse" % method)
    if args.inverse_block_jacobi and schur is not None:  # (the other refusals of the flag need the arguments alone: above)
        raise SystemExit("--inverse-block-jacobi: a Schur-complement problem keeps the sparse LU inverse of its Schur operator")
    if args.inverse_block_amg and method <= 1:
        _log(rank, "--inverse-block-amg has no effect: 'Projection method' %g applies no inverse" % method)
    if args.inverse_block_amg and schur is not None:
        raise SystemExit("--inverse-block-amg: a Schur-complement problem keeps the sparse LU inverse of its Schur operator")
    if method > 1:
        if world > 1 and args.inverse == "lu":
            raise SystemExit("'Projection method' %g on %d ranks: the sparse LU inverse runs on one rank; use --inverse iterative (or cg, bicgstab), "
                             "the inverse that partitions by rows" % (method, world))
        t0 = time.time()
        if schur is not None:
            inverse = schur.inverse()
            what = "Sinv, a sparse LU of the full matrix restricted to the %d Schur rows (matlab/RAILSschur.m:60-64)" % schur.m2
        elif args.inverse == "lu":
            inverse = rails_amd.SparseLU(ctx, (rowptr, col.astype(np.int32), val))
            what = "a sparse LU of A"
        elif world > 1 or args.inverse_block_jacobi or args.inverse_block_amg:
            # the rank's own row block with its halo plan; the all-reduce hook is in place (above).  Symmetry is a property of the whole
            # matrix, which every rank has read: every rank reaches the same method.  With --inverse-block-jacobi (one rank): the
            # block-CSR operator itself, whose diagonal blocks precondition; with --inverse-block-amg the same handle, whose blocks the
            # hierarchy is built from
            how = args.inverse
            if how == "iterative":
                import scipy.sparse as sp

                Afull = sp.csr_matrix((val, col, rowptr), shape=(m, m))
                how = "cg" if (Afull != Afull.T).nnz == 0 else "bicgstab"
            inverse = rails_amd.IterativeInverse(ctx, A, method=how, tol=args.inverse_tol)
        else:
            inverse = rails_amd.IterativeInverse(ctx, (rowptr, col.astype(np.int32), val), method="auto" if args.inverse == "iterative" else args.inverse,
                                                 tol=args.inverse_tol)
        if isinstance(inverse, rails_amd.IterativeInverse) and args.inverse_poly:  # on one rank or on several: the method is the same on every rank
            if inverse.method != "cg":
                raise SystemExit("--inverse-poly %d: the polynomial preconditioner is for conjugate gradients, and the inverse chosen is %s" % (
                    args.inverse_poly, inverse.method))
            inverse.set("poly_degree", args.inverse_poly)
        if isinstance(inverse, rails_amd.IterativeInverse) and args.inverse_amg:
            if inverse.method != "cg":
                raise SystemExit("--inverse-amg: the multigrid preconditioner is for conjugate gradients, and the inverse chosen is %s" % inverse.method)
            inverse.set("amg", 1)
            amg = inverse.amg_setup()
        if isinstance(inverse, rails_amd.IterativeInverse) and args.inverse_block_amg:
            if inverse.method != "cg":
                raise SystemExit("--inverse-block-amg: the block multigrid preconditioner is for conjugate gradients, and the inverse chosen is %s" % inverse.method)
            inverse.set("block_amg", 1)
            bamg = inverse.block_amg_setup()
        if isinstance(inverse, rails_amd.IterativeInverse) and args.inverse_block_jacobi:
            bj = inverse.block_jacobi()
            bj_first = {}

            def counted(trans, X, Y):
                # the solve's own applications, through a callback handle that notes what the first of them took
                inverse.solve(X, Y, trans=trans)
                if not bj_first:
                    bj_first.update(columns=X.n, iterations=inverse.stats()["max_iterations_of_a_column"])
                return 0

            bj_handle = rails_amd.HipOperatorWrapper.from_callback(ctx, m, counted)
            solver.set_inverse(bj_handle)
        else:
            solver.set_inverse(inverse)
        if isinstance(inverse, rails_amd.IterativeInverse):
            _log(rank, "Projection method %g: A^-1 is an iterative solve on the device, method %s, %s, tolerance %g" % (
                method, inverse.method, "block Jacobi" if args.inverse_block_jacobi else "block multigrid" if args.inverse_block_amg else "Jacobi", args.inverse_tol))
            if args.inverse_poly:
                _log(rank, "its preconditioner: a Chebyshev polynomial of degree %d in the Jacobi-scaled matrix" % args.inverse_poly)
            if args.inverse_block_jacobi:
                _log(rank, "its preconditioner: block Jacobi on the block-CSR operator, b = %d, %d blocks" % (bj["b"], bj["blocks"]))
            if args.inverse_block_amg:
                _log(rank, "its preconditioner: a block multigrid V-cycle on the block-CSR operator, b = %d, %d levels of %s rows, operator complexity %.2f, set up in %.3f s" % (
                    args.block_size, bamg["levels"], " / ".join(str(r) for r in bamg["rows"]), bamg["operator_complexity"], bamg["host_seconds"] + bamg["upload_seconds"]))
            if args.inverse_amg:
                _log(rank, "its preconditioner: a smoothed-aggregation multigrid V-cycle, %d levels of %s rows, operator complexity %.2f, set up in %.3f s" % (
                    amg["levels"], " / ".join(str(r) for r in amg["rows"]), amg["operator_complexity"], amg["host_seconds"] + amg["upload_seconds"]))
        else:
            _log(rank, "Projection method %g: A^-1 is %s; nnz(L+U) %d, factorised in %.2f s" % (method, what, inverse.nnz, time.time() - t0))

    if S0 is not None:
        if S0.shape[0] != m:
            raise SystemExit("--start-space: %d rows, the equation solved has %d" % (S0.shape[0], m))
        solver.set_start_space(S0[r0:r1])  # uploaded once; each rank its own rows
    _log(rank, "Performing solve")
    ctx.sync()
    t0 = time.perf_counter()
    code, V, T = solver.solve(V0=V0[r0:r1] if V0 is not None else None)
    ctx.sync()
    dt = time.perf_counter() - t0
    rel = solver.relative_residual()
    if schur is not None:
        _log(rank, "Amount of matrix-vector products after the solve: %d" % schur.applies)
    _log(rank, "solve returned %d after %d iterations in %.3f s: V is %d x %d, relative residual %.3e" % (code, solver.trips(), dt, m, solver.k, rel))
    if isinstance(inverse, rails_amd.IterativeInverse):
        st = inverse.stats()
        _log(rank, "iterative inverse (%s): %d solves of %d columns, %d inner iterations in all, %d flagged columns" % (
            inverse.method, st["total_solves"], st["total_columns"], st["total_iterations"], st["total_flagged_columns"]))
        if args.inverse_block_jacobi and bj_first:
            _log(rank, "its first application (%d columns): %d iterations at most" % (bj_first["columns"], bj_first["iterations"]))
        if args.inverse_poly:  # what the object itself counted in its last solve, not what was asked for
            _log(rank, "its last solve: %d applications of the polynomial, %d products with A, %d of them in fused steps" % (
                st["poly_applications"], st["products"], st["fused_launches"]))
        if args.inverse_block_amg:
            bamg = inverse.block_amg_info()
            _log(rank, "its last solve: %d inner iterations at most, %d block multigrid cycles, %d products and %d launches inside them" % (
                st["max_iterations_of_a_column"], bamg["cycles"], bamg["cycle_products"], bamg["cycle_launches"]))
        if args.inverse_amg:
            amg = inverse.amg_info()
            _log(rank, "its last solve: %d inner iterations at most, %d multigrid cycles, %d products and %d launches inside them" % (
                st["max_iterations_of_a_column"], amg["cycles"], amg["cycle_products"], amg["cycle_launches"]))
    if Nsp is not None:
        _log(rank, "nullspace: %d of %d columns kept" % (solver.nullspace_rank, Nsp.shape[1]))
    if S0 is not None:
        _log(rank, "start space: %d of %d columns kept" % (solver.start_rank, S0.shape[1]))
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, V)
        V = np.vstack(parts)
    if rank == 0:
        note = "rails_amd: X = V T V' solves A X M' + M X A' + B B' = 0; return code %d, relative residual %.3e" % (code, rel)
        mmio.write_array(path(args.V), V, comment=note)
        mmio.write_array(path(args.T), T, comment=note)
        print("wrote %s (%d x %d) and %s (%d x %d)" % (path(args.V), V.shape[0], V.shape[1], path(args.T), T.shape[0], T.shape[1]), flush=True)
    if args.eigs > 0 or args.variance or args.pairs or args.maps:
        sol = solver.solution()
        if schur is not None:
            sol, small = schur.lift(sol), sol
            small.close()
        if args.pairs:
            _write_pairs(args, pairs, sol, path, rank, world, r0, dist)
        if args.maps:
            _write_maps(args, refs, sol, path, rank, world, r0, dist)
        if args.variance:
            var = sol.variance()
            if world > 1:
                parts = [None] * world
                dist.all_gather_object(parts, var)
                var = np.concatenate(parts)
            if rank == 0:
                mmio.write_array(path(args.variance), var.reshape(-1, 1), comment="rails_amd: diag(X), the pointwise variance of X = V T V'")
                print("wrote %s (%d x 1)" % (path(args.variance), var.size), flush=True)
        if args.eigs > 0:
            trace = sol.trace()
            lam, Z = sol.eigs(args.eigs)
            if world > 1:
                parts = [None] * world
                dist.all_gather_object(parts, Z)
                Z = np.vstack(parts)
            if rank == 0:
                for x in lam:
                    print("%20.6g%20.6g" % (x, x / trace), flush=True)
                note = "rails_amd: the %d eigenpairs of largest modulus of X = V T V'; trace %.17g" % (lam.size, trace)
                mmio.write_array(path("eigenvalues.mtx"), lam.reshape(-1, 1), comment=note)
                mmio.write_array(path("eigenvectors.mtx"), Z, comment=note)
                print("wrote %s (%d x 1) and %s (%d x %d)" % (path("eigenvalues.mtx"), lam.size, path("eigenvectors.mtx"), Z.shape[0], Z.shape[1]), flush=True)
        sol.close()
    solver.close()
    if inverse is not None:
        inverse.close()
    ctx.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if code == 0 else 3


if __name__ == "__main__":
    sys.exit(main())
