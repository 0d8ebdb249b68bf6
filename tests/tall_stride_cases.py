"""Shapes, operators, operands and the case table of the tall-stride tests: every kernel takes a window of a row-major panel
(base + row * ld + column), and a panel reaches 2^31 and 2^32 bytes through rows x leading dimension, not through many rows.  With
rails_panel_create_ld a panel of 268 rows whose rows are 2,000,000 doubles apart is 4.29 GB of device memory of which a product touches
a few columns.  numpy only, no project imports: the host test (test_tall_stride_cases_host.py) pins what is in here, the device tests
(test_gpu_tall_stride_*.py) run it.

  LD_TALL = 2,000,000   a multiple of 16; LD_TALL * 8 = 16,000,000 < 2^24, so the lean row kernel's stride condition holds.  Row r starts
                        at byte r * 16e6: past 2^31 from row 135, past 2^32 from row 269.
  M_BELOW = 268         268 * 16e6 = 4,288,000,000 < 0xffffff00: the lean kernel qualifies, its largest byte offset is 4.27e9.
  M_ABOVE = 269         269 * 16e6 = 4,304,000,000 >= 0xffffff00: the guard refuses.
  M_FAR   = 300         plain 64-bit arithmetic well above 4 GiB.
  LD_WIDE = 2,097,152   ld * 8 = 2^24: the lean kernel is refused whatever the row count.

Operands are integers (spmm_reference: val in [-8, 8] without 0, panels in [-16, 16]; dense coefficient matrices in [-8, 8]), every
partial sum stays far below 2^53 (assert_exact), so a device result equals the int64 reference bit for bit whatever the order of
summation or the fusing.

The guards are restated here in Python (row_choice, tiled_reg_allowed, planes_allowed, cheb_fused_allowed) from
rails_amd/csrc/row_choice.h, spmm_tiled.hip, spmm_planes.hip and cheb_coef.h; the host test reads the constants back out of those
sources, so a moved guard fails there before a device test goes looking for a kernel that no longer runs."""
import collections

import numpy as np

import spmm_reference as R

LD_TALL = 2_000_000
LD_WIDE = 2_097_152
M_BELOW, M_ABOVE, M_FAR = 268, 269, 300
TWO31, TWO32, LEAN_LIMIT = 1 << 31, 1 << 32, 0xFFFFFF00
ROW_PAST_2G = 135  # the first row of an LD_TALL panel that starts past 2^31 bytes
ROW_PAST_4G = 269  # ... past 2^32
LDS_STAGED = 2048  # entries of a 64-row block that the lean and the chunked kernel stage in LDS
CAP = 144          # capacity of a tall panel: the widest window (130 columns at offset 3) and its two guard columns on either side
GUARD = 2          # columns of NaN on either side of a window

NARROW, CC, PLAIN = "k_spmm_narrow", "k_spmm_rowgather_cc", "k_spmm_rowgather"
TILED_REG, TILED_PIPE, TILED = "k_spmm_tiled_reg", "k_spmm_tiled_pipe", "k_spmm_tiled"


def panel_bytes(rows, ld):
    return int(rows) * int(ld) * 8


def row_start_byte(row, ld):
    return int(row) * int(ld) * 8


# ------------------------------------------------------------------------------------------------------------------ operators
DENSE_BLOCK = (64, 128)  # the block of 64 rows (one workgroup of the lean and the chunked kernel) whose entries exceed LDS_STAGED
SHORT_ROWS = {3: 0, 5: 1, 7: 7, 8: 8, 9: 9}  # row -> number of entries


def tall_operator(n_rows, n_cols=None, seed=1, band=60):
    """Banded-random CSR of n_rows x n_cols (square by default): (rowptr int64, col int32), columns sorted and distinct inside a row.

    A row has 4..37 columns within `band` of its own index and additionally column 0, a column in [135, min(268, n_cols)) and column
    n_cols - 1: at most 40 entries, gathered from both sides of row 135 (2^31 bytes at LD_TALL) and, where n_cols > 269, of row 269
    (2^32).  Rows DENSE_BLOCK have 37 band columns each, so the block holds more than LDS_STAGED entries and its workgroup reads
    (col, val) from global memory.  Rows SHORT_ROWS have 0, 1, 7, 8 and 9 entries (the lean kernel's groups of eight and four): the
    single entry is column n_cols - 1, the others include the three far columns."""
    n_cols = n_rows if n_cols is None else n_cols
    assert n_cols > ROW_PAST_2G + 1 and n_rows > DENSE_BLOCK[1]
    g = np.random.default_rng(seed)
    rowptr, cols = [0], []
    for i in range(n_rows):
        far = np.array([0, int(g.integers(ROW_PAST_2G, min(268, n_cols))), n_cols - 1])
        lo, hi = max(0, min(i, n_cols - 1) - band), min(n_cols - 1, i + band)
        n = 37 if DENSE_BLOCK[0] <= i < DENSE_BLOCK[1] else int(g.integers(4, 38))
        near = g.choice(np.arange(lo, hi + 1), size=min(n, hi - lo + 1), replace=False)
        c = np.unique(np.concatenate([near, far]))
        if i in SHORT_ROWS:
            want = SHORT_ROWS[i]
            if want == 0:
                c = c[:0]
            elif want == 1:
                c = far[2:]
            else:
                rest = np.setdiff1d(np.arange(lo, hi + 1), far)
                c = np.unique(np.concatenate([far, g.choice(rest, size=want - np.unique(far).size, replace=False)]))
                assert c.size == want
        cols.append(c)
        rowptr.append(rowptr[-1] + c.size)
    return np.asarray(rowptr, dtype=np.int64), np.concatenate(cols).astype(np.int32)


Operator = collections.namedtuple("Operator", "n_rows n_cols rowptr col val X ref")
_OPERATORS = {}
WMAX = 130


def operator(n_rows, n_cols=None):
    """the operator of that shape with its integer values, its X panel (n_cols x WMAX) and the exact product (n_rows x WMAX, int64):
    made once, read-only; a narrower case uses the leading columns"""
    key = (n_rows, n_rows if n_cols is None else n_cols)
    if key not in _OPERATORS:
        rowptr, col = tall_operator(*key, seed=key[0] + key[1])
        val = R.int_values(col.size, seed=7)
        X = R.int_panel(key[1], WMAX)
        ref = R.spmm_exact_int(rowptr, col, val, X)
        assert_exact(ref, 40 * 8 * 16)
        for a in (rowptr, col, val, X, ref):
            a.setflags(write=False)
        _OPERATORS[key] = Operator(key[0], key[1], rowptr, col, val, X, ref)
    return _OPERATORS[key]


def assert_exact(ref, partial_bound):
    """every entry of the reference and the bound on every partial sum are integers below 2^53: doubles hold them exactly"""
    assert int(partial_bound) < 2 ** 53, partial_bound
    ref = np.asarray(ref)
    if ref.size:
        assert np.array_equal(ref, np.rint(ref)) and float(np.abs(ref).max()) <= int(partial_bound), (float(np.abs(ref).max()), partial_bound)


# ---------------------------------------------------------------------------------------------------------- dense operands
def dense_panel(rows, nc, shift=0):
    """rows x nc integers in [-16, 16] (spmm_reference.int_panel, moved by `shift` columns so that two panels differ)"""
    return R.int_panel(rows, nc + shift)[:, shift:]


def dense_coef(k, n, seed):
    """k x n integers in [-8, 8]"""
    return np.random.default_rng(seed).integers(-8, 9, (k, n)).astype(np.float64)


def dense_partial_bound(rows, k):
    """rows x 16 x 16 x k: a Gram entry sums `rows` products of two panel entries, a panel update k products of a panel entry and a
    coefficient, the fused update + projection both (|update| <= 16 x 8 x k)"""
    return int(rows) * 16 * 16 * int(k)


# ------------------------------------------------------------------------------------------------------- the guards, restated
def row_choice(variant, nc, xoff, yoff, ldx, ldy, m, ncols_ext, max_row_nnz, rect_tail=False):
    """rails_row_choice (row_choice.h) for a serial product without ghost rows, all switches at their defaults: the kernel's name"""
    x_vec2 = xoff % 2 == 0 and ldx % 2 == 0
    vec2 = (xoff | yoff) % 2 == 0 and ldx % 2 == 0
    lpr, narrow_only = 0, False
    if vec2:
        chunk = 32 * (variant - 3) if variant in (4, 5) else 0
        if chunk and nc > chunk:
            lpr = chunk // 2
    narrow_width = variant != 3 and nc > 8 and max_row_nnz <= 64
    if not lpr and narrow_width and x_vec2 and nc <= 32:
        lpr = 8 if nc <= 16 else 16
    elif not lpr and narrow_width and not x_vec2 and nc <= 16:
        lpr, narrow_only = 8, True
    if lpr:
        if lpr <= 16 and nc <= 2 * lpr:
            flat = ncols_ext == m or rect_tail
            small = ncols_ext < (1 << 24) and ldx * 8 < (1 << 24)
            if small and flat and ncols_ext * ldx * 8 < LEAN_LIMIT:
                return NARROW
        if not narrow_only:
            return CC
    return PLAIN


def tiled_reg_allowed(m, ldx):
    """spmm_tiled.hip: the register kernel's 31-bit element offsets"""
    return m * ldx < 0x7FFFFFFF


def planes_allowed(gx, gy, ldx, ldy, rec=0):
    """spmm_planes.hip: int element offsets inside a plane"""
    return gx * gy * max(ldx, ldy, rec) * 8 < 0x7FFFFFFF


def cheb_fused_allowed(m, ld=32):
    """cheb_coef.h: the fused step's 32-bit byte offsets into the 32-column work panels"""
    return m < (1 << 24) and ld * 8 < (1 << 24) and m * ld * 8 < LEAN_LIMIT


# ------------------------------------------------------------------------------------------------------------- the case table
# rows, cols: the operator (X has `cols` rows); ldx, ldy: leading dimensions, None = a compact panel; claims: what the name says about the
# X panel's byte extent -- "<2^32", ">=2^32", "<lean", ">=lean", ">2^31" -- checked by the host test
Case = collections.namedtuple("Case", "name rows cols ldx ldy nc xoff yoff variant kernel claims")


def _cases():
    out = []

    def add(name, rows, cols, ldx, ldy, nc, xoff, yoff, variant, kernel, claims):
        out.append(Case(name, rows, cols, ldx, ldy, nc, xoff, yoff, variant, kernel, tuple(claims)))

    below = (">2^31", "<lean", "<2^32")
    above = (">2^31", ">=lean", ">=2^32")
    # the lean kernel just below its guard: 8 lanes per row up to 16 columns, 16 beyond, an odd last column; Y compact, then tall
    for nc in (9, 16, 17, 32):
        add("below_nc%d" % nc, M_BELOW, M_BELOW, LD_TALL, None, nc, 2, 0, 1, NARROW, below)
        add("below_nc%d_tall_y" % nc, M_BELOW, M_BELOW, LD_TALL, LD_TALL, nc, 2, 3 if nc == 16 else 2, 1, NARROW, below)
    # X rows only 8-byte aligned
    add("below_nc16_odd_x", M_BELOW, M_BELOW, LD_TALL, None, 16, 3, 0, 1, NARROW, below)
    add("below_nc16_odd_x_tall_y", M_BELOW, M_BELOW, LD_TALL, LD_TALL, 16, 3, 2, 1, NARROW, below)
    # one row more: the guard refuses
    add("above_nc16", M_ABOVE, M_ABOVE, LD_TALL, None, 16, 2, 0, 1, CC, above)
    add("above_nc32_tall_y", M_ABOVE, M_ABOVE, LD_TALL, LD_TALL, 32, 2, 3, 1, CC, above)
    add("above_nc16_odd_x", M_ABOVE, M_ABOVE, LD_TALL, None, 16, 3, 0, 1, PLAIN, above)
    # ld * 8 = 2^24: refused whatever the row count
    add("wide_nc16", M_BELOW, M_BELOW, LD_WIDE, None, 16, 2, 0, 1, CC, (">2^31", ">=2^32"))
    add("wide_nc16_odd_x_tall_y", M_BELOW, M_BELOW, LD_WIDE, LD_WIDE, 16, 3, 2, 1, PLAIN, (">2^31", ">=2^32"))
    # the plain and the chunked kernels well above 4 GiB
    for variant, kernels in ((3, (PLAIN, PLAIN, PLAIN, PLAIN)), (4, (PLAIN, CC, CC, CC)), (5, (PLAIN, PLAIN, CC, CC))):
        for nc, kernel in zip((8, 48, 80, 130), kernels):
            tall_y = nc in (48, 130)
            add("far_v%d_nc%d" % (variant, nc), M_FAR, M_FAR, LD_TALL, LD_TALL if tall_y else None, nc, 2, 2 if tall_y else 0, variant, kernel, above)
    add("far_v3_nc130_odd", M_FAR, M_FAR, LD_TALL, LD_TALL, 130, 3, 3, 3, PLAIN, above)
    # a rectangular operator whose extra rows follow X in the same panel, on both sides of the guard
    add("rect_below_nc16", 200, M_BELOW, LD_TALL, None, 16, 2, 0, 1, NARROW, below)
    add("rect_below_nc32_tall_y", 200, M_BELOW, LD_TALL, LD_TALL, 32, 2, 3, 1, NARROW, below)
    add("rect_above_nc16", 200, M_ABOVE, LD_TALL, None, 16, 2, 0, 1, CC, above)
    add("rect_above_nc16_tall_y", 200, M_FAR, LD_TALL, LD_TALL, 16, 2, 3, 1, CC, above)
    return out


ROW_CASES = _cases()

# dense panels: M_FAR x LD_TALL, windows at offsets 0 and 3
DENSE_ROWS, DENSE_LD, DENSE_OFFSETS = M_FAR, LD_TALL, (0, 3)

# the iterative object's 32-column work panels: rows alone reach the lines
ITER_LD = 32
ITER_M = 9_000_000           # 2.30e9 bytes: above 2^31, below the lean limit
ITER_M_LAST = (1 << 24) - 2  # 4,294,966,784 bytes: 256 below the limit, the last m the guard accepts
