// iter_precond.h -- the one rule of the iterative A^-1 operator's preconditioners (Jacobi, the Chebyshev polynomial, the multigrid cycle,
// block Jacobi, the block multigrid cycle; DESIGN.md section 14, "One rule for the preconditioners"): whether a request to turn one on
// is granted -- one at a time, and what each refuses of the method, the operator, the context and the row count, with the refusal's text
// -- and what is in effect for a call: what the passes apply in place, what is applied beyond them, the sign of the scalar step, the work
// panels.  The settings (iter_setup.hip), the set-ups and the install of blocks (iter_hierarchy.hip) ask the first question, a call
// (itsolve.hip: begin_call) and the work panels (grow_work) the second; nothing else derives either.  Plain arithmetic on integers and
// booleans, no HIP, no I/O, no environment, no pointers into the object: checked on the host alone by tests/cpp/iter_precond_host.cpp
// against the restatement in tests/iter_precond_reference.py.  The refusals that look at the entries stay where the entries are read:
// rails_bj_plan (block_jacobi_host.h) and the host builders (amg_host.h, block_amg_host.h).
#ifndef RAILS_ITER_PRECOND_H
#define RAILS_ITER_PRECOND_H

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "block_amg_choice.h"

// The work panels.  CG: x r p q [z]; BiCGStab: x r p v(=Q) [p^(=Z)] r^ t [s^]; the polynomial and the cycles: z, its direction d, the
// second z of the fused step's ping-pong
enum { W_X = 0, W_R, W_P, W_Q, W_Z, W_RH, W_T, W_SH, W_D, W_Z2, W_COUNT };

// the operator the object iterates on, as far as a preconditioner depends on it
enum { RAILS_PC_OP_STORED = 0, RAILS_PC_OP_BSR, RAILS_PC_OP_CALLBACK, RAILS_PC_OP_LU, RAILS_PC_OP_ITER };

struct rails_precond_facts {
    bool cg = true;          // the method: conjugate gradients, else BiCGStab
    int op = RAILS_PC_OP_STORED;
    bool host_csr = false;   // a stored operator that keeps its scalar CSR arrays on the host
    int host_b = 0;          // a block-CSR operator that keeps its block arrays on the host: their block size (0: no host copy)
    bool reduces = false;    // the context reduces (more than one rank, an all-reduce hook, a communicator)
    bool exchanges = false;  // the operator has ghost rows or rows to send
    int64_t m = 0;
    bool diag = false;       // the inverse of the diagonal exists
    int blocks_b = 0;        // the size of the installed diagonal blocks (0: none)
    int defsign = 1;         // -1: every diagonal entry is known and negative
    // the five settings as they stand
    bool jacobi = true;
    int poly_degree = 0;
    bool amg = false, block_amg = false, block_jacobi = false;
};

// What may be asked for.  Turning a setting off, and "jacobi" either way, is never refused and is no request.
enum {
    RAILS_PC_POLY = 0,         // "poly_degree" = v (0: off, always granted)
    RAILS_PC_AMG,              // "amg" 1
    RAILS_PC_BLOCK_AMG,        // "block_amg" 1
    RAILS_PC_BLOCK_JACOBI,     // "block_jacobi" 1
    RAILS_PC_INSTALL_BLOCKS,   // rails_iter_block_jacobi with blocks to install (after rails_bj_plan has found their source)
    RAILS_PC_SETUP_AMG,        // rails_iter_amg_setup, whatever "amg" is
    RAILS_PC_SETUP_BLOCK_AMG,  // rails_iter_block_amg_setup, whatever "block_amg" is
    RAILS_PC_REQUESTS
};

// May the request be granted?  True: yes.  False: the refusal in err, the first of the reasons in the order below that applies.  `who` is
// the function the caller reports as (the settings: "rails_iter_set").
inline bool rails_precond_grant(const rails_precond_facts &f, int request, int v, const char *who, char *err, size_t cap)
{
#define RAILS_PC_REFUSE_IF(cond, ...)                                                                                                             \
    do {                                                                                                                                          \
        if (cond) {                                                                                                                               \
            snprintf(err, cap, __VA_ARGS__);                                                                                                      \
            return false;                                                                                                                         \
        }                                                                                                                                         \
    } while (0)
    switch (request) {
    case RAILS_PC_POLY:
        if (v == 0) return true;
        RAILS_PC_REFUSE_IF(f.amg, "%s: poly_degree %d together with \"amg\": one preconditioner at a time", who, v);
        RAILS_PC_REFUSE_IF(f.block_jacobi, "%s: poly_degree %d together with \"block_jacobi\": one preconditioner at a time", who, v);
        RAILS_PC_REFUSE_IF(f.block_amg, "%s: poly_degree %d together with \"block_amg\": one preconditioner at a time", who, v);
        RAILS_PC_REFUSE_IF(!f.cg, "%s: poly_degree %d on a BiCGStab object: the polynomial preconditioner is for conjugate gradients (a real spectrum)", who, v);
        return true;
    case RAILS_PC_BLOCK_JACOBI:
        RAILS_PC_REFUSE_IF(f.blocks_b == 0, "%s: \"block_jacobi\" 1 without blocks: install them first (rails_iter_block_jacobi)", who);
        RAILS_PC_REFUSE_IF(f.poly_degree != 0, "%s: \"block_jacobi\" together with poly_degree %d: one preconditioner at a time", who, f.poly_degree);
        RAILS_PC_REFUSE_IF(f.amg, "%s: \"block_jacobi\" together with \"amg\": one preconditioner at a time", who);
        RAILS_PC_REFUSE_IF(f.block_amg, "%s: \"block_jacobi\" together with \"block_amg\": one preconditioner at a time", who);
        return true;
    case RAILS_PC_INSTALL_BLOCKS:
        RAILS_PC_REFUSE_IF(f.poly_degree != 0, "%s: together with poly_degree %d: one preconditioner at a time", who, f.poly_degree);
        RAILS_PC_REFUSE_IF(f.amg, "%s: together with \"amg\": one preconditioner at a time", who);
        RAILS_PC_REFUSE_IF(f.block_amg, "%s: together with \"block_amg\": one preconditioner at a time", who);
        return true;
    case RAILS_PC_AMG:
    case RAILS_PC_SETUP_AMG:
        // (a sparse right-hand side or a rectangular operator never gets this far: rails_iter_create refuses them)
        RAILS_PC_REFUSE_IF(!f.cg, "%s: \"amg\" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)", who);
        RAILS_PC_REFUSE_IF(f.poly_degree != 0, "%s: \"amg\" together with poly_degree %d: one preconditioner at a time", who, f.poly_degree);
        RAILS_PC_REFUSE_IF(f.block_jacobi, "%s: \"amg\" together with \"block_jacobi\": one preconditioner at a time", who);
        RAILS_PC_REFUSE_IF(f.block_amg, "%s: \"amg\" together with \"block_amg\": one preconditioner at a time", who);
        RAILS_PC_REFUSE_IF(f.op == RAILS_PC_OP_CALLBACK, "%s: \"amg\" needs the entries of the matrix: the operator is a callback", who);
        RAILS_PC_REFUSE_IF(f.op == RAILS_PC_OP_LU || f.op == RAILS_PC_OP_ITER, "%s: \"amg\" needs the entries of the matrix: the operator is an LU or an iterative solve", who);
        RAILS_PC_REFUSE_IF(f.op == RAILS_PC_OP_BSR,
                           "%s: \"amg\" needs the entries of the matrix as scalar CSR arrays: the operator is block-CSR (keep a CSR handle for the preconditioner)", who);
        RAILS_PC_REFUSE_IF(f.reduces || f.exchanges,
                           "%s: \"amg\" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU", who);
        RAILS_PC_REFUSE_IF(f.m >= ((int64_t)1 << 24), "%s: \"amg\" on %lld rows: the multigrid preconditioner takes fewer than 2^24", who, (long long)f.m);
        // the set-up alone: the setting is granted without the arrays and the first solve's set-up refuses.  (The set-up drops the old
        // hierarchy between the reasons above and this one, which nobody can see: a handle without the arrays never had a hierarchy.)
        RAILS_PC_REFUSE_IF(request == RAILS_PC_SETUP_AMG && !f.host_csr, "%s: the operator keeps no CSR arrays on the host to build the hierarchy from", who);
        return true;
    case RAILS_PC_BLOCK_AMG:
    case RAILS_PC_SETUP_BLOCK_AMG:
        RAILS_PC_REFUSE_IF(!f.cg, "%s: \"block_amg\" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)", who);
        RAILS_PC_REFUSE_IF(f.poly_degree != 0, "%s: \"block_amg\" together with poly_degree %d: one preconditioner at a time", who, f.poly_degree);
        RAILS_PC_REFUSE_IF(f.block_jacobi, "%s: \"block_amg\" together with \"block_jacobi\": one preconditioner at a time", who);
        RAILS_PC_REFUSE_IF(f.amg, "%s: \"block_amg\" together with \"amg\": one preconditioner at a time", who);
        RAILS_PC_REFUSE_IF(f.op != RAILS_PC_OP_BSR || f.host_b == 0,
                           "%s: \"block_amg\" needs the blocks of the matrix: the operator is not a block-CSR handle with a host copy (rails_csr_create_bsr)", who);
        RAILS_PC_REFUSE_IF(f.reduces, "%s: \"block_amg\" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU", who);
        RAILS_PC_REFUSE_IF(!rails_bamg_rows_ok(f.m, f.host_b), "%s: \"block_amg\" on %lld rows of block size %d: the multigrid cycle's kernels address fewer than 2^24 rows", who,
                           (long long)f.m, f.host_b);
        return true;
    }
#undef RAILS_PC_REFUSE_IF
    snprintf(err, cap, "%s: no request %d", who, request);
    return false;
}

// What is in effect for a call.
enum { RAILS_PC_PASS_NONE = 0, RAILS_PC_PASS_DIAG, RAILS_PC_PASS_BLOCKS };                       // applied in place by the passes
enum { RAILS_PC_BEYOND_NONE = 0, RAILS_PC_BEYOND_POLY, RAILS_PC_BEYOND_CYCLE, RAILS_PC_BEYOND_BLOCK_CYCLE }; // applied beyond them
struct rails_precond_effect {
    int pass = RAILS_PC_PASS_NONE;
    int b = 0;  // RAILS_PC_PASS_BLOCKS: their size (the passes that apply G take their block form, on the block geometry)
    int beyond = RAILS_PC_BEYOND_NONE;
    int K = 0;  // RAILS_PC_BEYOND_POLY: the degree
    int sign = 1; // handed to the scalar step: with any preconditioner r.z carries the sign of the operator itself
    unsigned panels = 0; // bits 1 << W_...: the work panels the object holds for such calls
    bool cycle() const { return beyond == RAILS_PC_BEYOND_CYCLE || beyond == RAILS_PC_BEYOND_BLOCK_CYCLE; }
};

inline rails_precond_effect rails_precond_effect_of(const rails_precond_facts &f)
{
    rails_precond_effect e;
    if (f.block_jacobi && f.blocks_b > 0) {
        e.pass = RAILS_PC_PASS_BLOCKS;
        e.b = f.blocks_b;
    } else if (f.jacobi && f.diag)
        e.pass = RAILS_PC_PASS_DIAG;
    if (f.block_amg)
        e.beyond = RAILS_PC_BEYOND_BLOCK_CYCLE;
    else if (f.amg)
        e.beyond = RAILS_PC_BEYOND_CYCLE;
    else if (f.poly_degree > 0) {
        e.beyond = RAILS_PC_BEYOND_POLY;
        e.K = f.poly_degree;
    }
    e.sign = (e.pass != RAILS_PC_PASS_NONE || e.beyond != RAILS_PC_BEYOND_NONE) ? 1 : f.defsign;
    // The panels follow what exists -- the diagonal, the blocks -- not "jacobi" or "block_jacobi": a superset of what the call reads, so
    // that turning either on between two calls asks for no new panel.
    const bool g = f.diag || f.blocks_b > 0;
    e.panels = 1u << W_X | 1u << W_R | 1u << W_P | 1u << W_Q;
    if (!f.cg) e.panels |= 1u << W_RH | 1u << W_T;
    if (g) e.panels |= f.cg ? 1u << W_Z : 1u << W_Z | 1u << W_SH;
    if (e.beyond != RAILS_PC_BEYOND_NONE) e.panels |= 1u << W_Z | 1u << W_D | 1u << W_Z2;
    return e;
}

#endif
