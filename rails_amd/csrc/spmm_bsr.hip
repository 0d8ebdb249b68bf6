// spmm_bsr.hip -- block-CSR x tall-skinny panel product Y = op(A) X for gfx950, and the operator object behind rails_csr_create_bsr.
//
// A is a sparse matrix of dense B x B blocks (2 <= B <= 8), block rows in CSR form with row-major blocks.  LPR lanes own a block row; a
// lane owns two adjacent columns of the panel and holds B x 2 accumulators.  Per block it loads its 16 bytes of each of the block's B rows
// of X and makes 2 B^2 multiply-adds, whose B^2 matrix values come as LDS broadcasts from the run of blocks the workgroup staged (as
// k_spmm_narrow stages its (col, val) run).  So a gathered X row serves B scalar rows from registers: c * 8 / B gathered bytes per
// scalar entry where the CSR kernels move c * 8, and 4 / B^2 index bytes where they move 4.  HBM- and gather-bound streaming work: no MFMA
// (whose internal order of summation would also give up the identity below).
//
// The arithmetic is fixed: every Y[i, j] is one accumulator, from +0, updated by one __builtin_fma per stored entry of scalar row i in
// stored order -- blocks in browptr order, columns ascending inside a block, the zeros inside a block included.  That is the order and the
// operation of k_spmm_rowgather (spmm.hip), so the product is bit for bit the row-gather product of the expanded CSR matrix.
//
// How a product is launched (instantiation, block rows per workgroup, grid) is decided in one place, bsr_choice.h.
#include "rails_internal.h"
#include "bsr_choice.h"

#include <algorithm>

// the block-CSR matrix behind a handle of kind BSR (and behind its lazily built transposed copy)
struct rails_bsr {
    int b = 0;
    int64_t mb = 0, nnzb = 0, max_brow = 0;
    int64_t *browptr = nullptr; // device
    int32_t *bcol = nullptr;
    double *bval = nullptr;
    std::vector<int64_t> h_browptr; // host copy, kept for the transposed copy
    std::vector<int32_t> h_bcol;
    std::vector<double> h_bval;
    rails_bsr *T = nullptr; // transposed copy, built at the first transposed product
    BsrChoice last{};       // of the last launch (either direction)
    size_t bytes() const { return (size_t)nnzb * ((size_t)b * b * 8 + 4) + (size_t)(mb + 1) * 8; }
};

namespace {

#include "bsr_row_gather.inc"

// The product itself: the shared block-row body with a storing epilogue.
template <int B, int LPR>
__global__ __launch_bounds__(rails_bsr_threads(B)) void k_spmm_bsr(int64_t mb, const int64_t *__restrict__ browptr, const int32_t *__restrict__ bcol,
                                                                   const double *__restrict__ bval, const double *__restrict__ X, int ldx,
                                                                   double *__restrict__ Y, int ldy, int nc, int rpg, int64_t blocks_per_xcd, int y_vec)
{
    bsr_row_gather<B, LPR>(mb, browptr, bcol, bval, X, ldx, nc, rpg, blocks_per_xcd, [&](int64_t brow, int cb, const bsr_v2 (&acc)[B], bool full, bool one) {
        double *dst = Y + brow * B * (int64_t)ldy + cb;
        if (full) {
#pragma unroll
            for (int r = 0; r < B; ++r) {
                if (y_vec)
                    *reinterpret_cast<bsr_v2 *>(dst + r * (int64_t)ldy) = acc[r];
                else { // Y window on an odd column: two 8-byte stores
                    dst[r * (int64_t)ldy] = acc[r].x;
                    dst[r * (int64_t)ldy + 1] = acc[r].y;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < B; ++r) dst[r * (int64_t)ldy] = one ? acc[r].x : acc[r].y;
        }
    });
}

int launch_bsr(rails_ctx *c, rails_bsr *M, const BsrChoice &ch, const double *X, int ldx, double *Y, int ldy, int nc)
{
    RAILS_REQUIRE(ch.ok, "rails_spmm: no block-CSR kernel for b = %d, %d columns, %lld block rows", M->b, nc, (long long)M->mb);
#define RAILS_BSR_CASE(B, LPR)                                                                                                                    \
    case rails_bsr_inst(B, LPR):                                                                                                                  \
        RAILS_LAUNCH((k_spmm_bsr<B, LPR>), dim3((unsigned)ch.grid), dim3(ch.threads), 0, c->stream, M->mb, M->browptr, M->bcol, M->bval, X, ldx, Y, ldy, nc, \
                     ch.rpg, ch.bpx, ch.y_vec ? 1 : 0);                                                                                           \
        break;
    switch (ch.key()) {
        RAILS_BSR_TABLE(RAILS_BSR_CASE)
    default:
        rails_set_error("rails_spmm: k_spmm_bsr<%d, %d> is not among the instantiations of bsr_choice.h", ch.b, ch.lpr);
        return RAILS_EINVAL;
    }
#undef RAILS_BSR_CASE
    M->last = ch;
    return RAILS_OK;
}

void bsr_release(rails_bsr *M)
{
    if (!M) return;
    bsr_release(M->T);
    if (M->browptr) hipFree(M->browptr);
    if (M->bcol) hipFree(M->bcol);
    if (M->bval) hipFree(M->bval);
    delete M;
}

// uploads a validated block matrix
int bsr_upload(rails_ctx *c, int64_t mb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval, rails_bsr **out)
{
    rails_bsr *M = new rails_bsr;
    M->b = b;
    M->mb = mb;
    M->nnzb = browptr[mb];
    for (int64_t i = 0; i < mb; ++i) M->max_brow = std::max(M->max_brow, browptr[i + 1] - browptr[i]);
    M->h_browptr.assign(browptr, browptr + mb + 1);
    if (M->nnzb) {
        M->h_bcol.assign(bcol, bcol + M->nnzb);
        M->h_bval.assign(bval, bval + M->nnzb * b * b);
    }
    const size_t nb = (size_t)(M->nnzb ? M->nnzb : 1);
    hipError_t e1 = hipMalloc((void **)&M->browptr, (size_t)(mb + 1) * sizeof(int64_t));
    hipError_t e2 = hipMalloc((void **)&M->bcol, nb * sizeof(int32_t));
    hipError_t e3 = hipMalloc((void **)&M->bval, nb * b * b * sizeof(double));
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        rails_set_error("rails_csr_create_bsr: device allocation failed");
        bsr_release(M);
        return RAILS_ENOMEM;
    }
    hipError_t ce = hipMemcpyAsync(M->browptr, browptr, (size_t)(mb + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess && M->nnzb) ce = hipMemcpyAsync(M->bcol, bcol, (size_t)M->nnzb * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess && M->nnzb) ce = hipMemcpyAsync(M->bval, bval, (size_t)M->nnzb * b * b * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess) ce = rails_stream_sync(c);
    if (ce != hipSuccess) { // the half-made matrix is released, not leaked
        rails_set_error("rails_csr_create_bsr: upload failed: %s", hipGetErrorString(ce));
        bsr_release(M);
        return RAILS_EHIP;
    }
    *out = M;
    return RAILS_OK;
}

int build_transpose(rails_ctx *c, rails_bsr *M)
{
    if (M->T) return RAILS_OK;
    std::vector<int64_t> rp((size_t)M->mb + 1);
    std::vector<int32_t> ci((size_t)(M->nnzb ? M->nnzb : 1));
    std::vector<double> va((size_t)(M->nnzb ? M->nnzb : 1) * M->b * M->b);
    RAILS_TRY(rails_bsr_transpose_host(M->mb, M->mb, M->b, M->h_browptr.data(), M->h_bcol.data(), M->h_bval.data(), rp.data(), ci.data(), va.data()));
    return bsr_upload(c, M->mb, M->b, rp.data(), ci.data(), va.data(), &M->T);
}

} // namespace

extern "C" int rails_csr_create_bsr(rails_ctx *c, int64_t mb, int64_t nb_ext, int b, const int64_t *browptr, const int32_t *bcol, const double *bval,
                                    rails_csr **out)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && out && browptr, "rails_csr_create_bsr: null argument");
    RAILS_REQUIRE(b >= 2 && b <= 8, "rails_csr_create_bsr: block size %d outside 2 .. 8", b);
    RAILS_REQUIRE(mb >= 0 && mb * b <= 0x7fffffffLL, "rails_csr_create_bsr: bad shape: %lld block rows of %d", (long long)mb, b);
    RAILS_REQUIRE(nb_ext == mb, "rails_csr_create_bsr: %lld block rows but %lld block columns: a block-CSR operator is square (single GPU, no ghost columns)",
                  (long long)mb, (long long)nb_ext);
    RAILS_REQUIRE(c->nranks <= 1 && !c->allreduce && !c->rccl,
                  "rails_csr_create_bsr: the context has a partition, an all-reduce hook or a communicator: a block-CSR operator is single GPU only");
    RAILS_REQUIRE(browptr[0] == 0, "rails_csr_create_bsr: browptr[0] != 0");
    for (int64_t i = 0; i < mb; ++i)
        RAILS_REQUIRE(browptr[i + 1] >= browptr[i] && browptr[i + 1] - browptr[i] <= 0x7fffffffLL, "rails_csr_create_bsr: browptr not monotone at block row %lld", (long long)i);
    const int64_t nnzb = browptr[mb];
    RAILS_REQUIRE(nnzb == 0 || (bcol && bval), "rails_csr_create_bsr: null arrays with %lld blocks", (long long)nnzb);
    // host-side index validation: an out-of-range block column would fault the kernel
    for (int64_t q = 0; q < nnzb; ++q)
        RAILS_REQUIRE(bcol[q] >= 0 && bcol[q] < mb, "rails_csr_create_bsr: block column %d out of range at block %lld", bcol[q], (long long)q);
    rails_bsr *M = nullptr;
    RAILS_TRY(bsr_upload(c, mb, b, browptr, bcol, bval, &M));
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = mb * b;
    A->ncols_ext = mb * b;
    A->nnz = nnzb * b * b;
    A->kind = rails_csr::BSR;
    A->delegate = M;
    A->last_kernel = "";
    *out = A;
    return RAILS_OK;
}

extern "C" int rails_csr_block_size(const rails_csr *A) { return A && A->bsr() ? A->bsr()->b : 1; }

extern "C" int rails_csr_bsr_stats(const rails_csr *A, int64_t *info, int cap)
{
    RAILS_REQUIRE(A && info && cap >= 0, "rails_csr_bsr_stats: bad argument");
    const rails_bsr *M = A->bsr();
    RAILS_REQUIRE(M, "rails_csr_bsr_stats: not a block-CSR operator");
    const BsrChoice &l = M->last;
    const int64_t v[10] = {M->nnzb, M->b, M->max_brow, (int64_t)(M->bytes() + (M->T ? M->T->bytes() : 0)), l.b, l.lpr, l.threads, l.rpg, l.all_staged ? 1 : 0, l.grid};
    for (int i = 0; i < cap && i < 10; ++i) info[i] = v[i];
    return RAILS_OK;
}

// the block matrix of a BSR handle goes with the handle (rails_csr_destroy)
// the host copy a block-CSR handle keeps (block Jacobi of the iterative A^-1 takes its diagonal blocks from it, iter_hierarchy.hip)
bool rails_bsr_host_arrays(const rails_csr *A, int *b, int64_t *mb, const int64_t **browptr, const int32_t **bcol, const double **bval)
{
    const rails_bsr *M = A->bsr();
    if (!M || (int64_t)M->h_browptr.size() != M->mb + 1) return false;
    *b = M->b;
    *mb = M->mb;
    *browptr = M->h_browptr.data();
    *bcol = M->h_bcol.data();
    *bval = M->h_bval.data();
    return true;
}

// the device arrays of a block-CSR handle and the two facts its launch rule needs (the block multigrid cycle's own kernels on the shared
// block-row body, itsolve.hip)
bool rails_bsr_device_arrays(const rails_csr *A, int64_t *mb, int64_t *max_brow, const int64_t **browptr, const int32_t **bcol, const double **bval)
{
    const rails_bsr *M = A->bsr();
    if (!M) return false;
    *mb = M->mb;
    *max_brow = M->max_brow;
    *browptr = M->browptr;
    *bcol = M->bcol;
    *bval = M->bval;
    return true;
}

void rails_bsr_release(rails_csr *A)
{
    if (A->kind != rails_csr::BSR) return;
    bsr_release(static_cast<rails_bsr *>(A->delegate));
    A->delegate = nullptr;
}

// rails_spmm on a BSR handle: windows checked by the caller, nc >= 1, m >= 1
int rails_bsr_apply(rails_ctx *c, rails_csr *A, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    rails_bsr *M = A->bsr();
    RAILS_REQUIRE(M, "rails_spmm: not a block-CSR operator");
    rails_bsr *P = M;
    if (trans) {
        RAILS_TRY(build_transpose(c, M));
        P = M->T;
    }
    BsrFacts f;
    f.b = P->b; f.nc = nc; f.mb = P->mb; f.max_brow = P->max_brow; f.num_cu = c->num_cu;
    f.ldx = X->ld; f.ldy = Y->ld;
    f.y_vec2 = (yc0 & 1) == 0 && (Y->ld % 2 == 0);
    RAILS_TRY(launch_bsr(c, P, rails_bsr_choice(f), X->d + xc0, X->ld, Y->d + yc0, Y->ld, nc));
    M->last = P->last;
    A->last_kernel = trans ? "k_spmm_bsr (transposed copy)" : "k_spmm_bsr";
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}
