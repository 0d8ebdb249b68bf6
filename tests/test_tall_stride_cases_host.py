"""Pins tests/tall_stride_cases.py on the CPU: every case's byte extent lies on the side of 2^31, 2^32 and 0xffffff00 that its name
claims, the exactness bound holds, the operators gather from both sides of the lines, and the guards restated there agree with the
library's own headers -- asked through a stand-alone program (tests/cpp/tall_stride_guard_host.cpp, built by rails_amd/csrc/Makefile into
rails_amd/lib/tall_stride_guard_host from row_choice.h and cheb_coef.h alone: no HIP, no library).  The guards of the LDS-staged and the
plane-sweep kernel sit inside .hip files; their constants are read back out of the source text."""
import os
import re
import subprocess

import numpy as np
import pytest

import tall_stride_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "tall_stride_guard_host")
CSRC = os.path.join(ROOT, "rails_amd", "csrc")


def ask(lines):
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:]
    out = p.stdout.split()
    assert len(out) == len(lines), p.stdout[-2000:]
    return out


def test_the_shapes_sit_where_the_names_say():
    assert T.LD_TALL % 16 == 0 and T.LD_TALL * 8 == 16_000_000 < (1 << 24) and T.LD_WIDE * 8 == 1 << 24
    # row r of an LD_TALL panel starts past 2^31 from row 135 and past 2^32 from row 269
    assert T.row_start_byte(T.ROW_PAST_2G - 1, T.LD_TALL) < T.TWO31 <= T.row_start_byte(T.ROW_PAST_2G, T.LD_TALL)
    assert T.row_start_byte(T.ROW_PAST_4G - 1, T.LD_TALL) < T.TWO32 <= T.row_start_byte(T.ROW_PAST_4G, T.LD_TALL)
    assert T.TWO31 < T.panel_bytes(T.M_BELOW, T.LD_TALL) < T.LEAN_LIMIT <= T.panel_bytes(T.M_ABOVE, T.LD_TALL)
    # the lean kernel's largest offset, the last row's start plus the widest window, is past 4.27e9 and an unsigned 32-bit number
    assert 4.27e9 < T.row_start_byte(T.M_BELOW - 1, T.LD_TALL) + T.CAP * 8 < T.TWO32
    assert T.panel_bytes(T.M_FAR, T.LD_TALL) > T.TWO32 + (1 << 28) and T.row_start_byte(T.M_FAR - 1, T.LD_TALL) > T.TWO32
    assert T.panel_bytes(T.DENSE_ROWS, T.DENSE_LD) > T.TWO32 and T.DENSE_OFFSETS == (0, 3)
    # a tall panel holds the widest window at the odd offset and its guards; device tests keep at most 24 GiB: four M_FAR panels are 19.2 GB
    assert T.CAP >= 3 + T.WMAX + 2 * T.GUARD and 4 * T.panel_bytes(T.M_FAR, T.LD_WIDE) < 24 << 30
    # the iterative object's work panels
    assert T.TWO31 < T.panel_bytes(T.ITER_M, T.ITER_LD) == 2_304_000_000 < T.LEAN_LIMIT
    assert T.panel_bytes(T.ITER_M_LAST, T.ITER_LD) == 4_294_966_784 == T.LEAN_LIMIT - 256 and T.panel_bytes(T.ITER_M_LAST + 1, T.ITER_LD) == T.LEAN_LIMIT


@pytest.mark.parametrize("case", T.ROW_CASES, ids=[c.name for c in T.ROW_CASES])
def test_a_case_lies_on_the_side_its_name_claims(case):
    extent = T.panel_bytes(case.cols, case.ldx)
    last_row = T.row_start_byte(case.cols - 1, case.ldx)
    sides = {">2^31": last_row > T.TWO31, "<2^32": extent < T.TWO32, ">=2^32": extent >= T.TWO32, "<lean": extent < T.LEAN_LIMIT,
             ">=lean": extent >= T.LEAN_LIMIT}
    assert case.claims and all(sides[c] for c in case.claims), (case, extent)
    for word, claim in (("below", "<lean"), ("above", ">=lean"), ("far", ">=2^32"), ("wide", ">=2^32")):
        if word in case.name.split("_"):
            assert claim in case.claims, case
    if "far" in case.name:
        assert last_row > T.TWO32  # rows that start beyond byte 2^32 are read
    assert ("odd" in case.name) == (case.xoff % 2 == 1) and case.xoff + case.nc + T.GUARD <= T.CAP and case.yoff + case.nc + T.GUARD <= T.CAP
    assert (case.ldy is not None) == ("tall_y" in case.name or case.name.startswith("far") and case.nc in (48, 130))
    if case.ldy is not None:
        assert T.row_start_byte(case.rows - 1, case.ldy) > T.TWO31
    # what the restated rule says is what the table expects
    op = T.operator(case.rows, case.cols)
    max_row_nnz = int(np.diff(op.rowptr).max())
    got = T.row_choice(case.variant, case.nc, case.xoff, case.yoff, case.ldx, case.ldy or 16, case.rows, case.cols, max_row_nnz, rect_tail=case.rows != case.cols)
    assert got == case.kernel, (case, got)


def test_the_table_covers_both_sides_of_every_line():
    by = {c.name: c for c in T.ROW_CASES}
    assert len(by) == len(T.ROW_CASES)
    for nc in (9, 16, 17, 32):
        assert by["below_nc%d" % nc].kernel == T.NARROW and by["below_nc%d_tall_y" % nc].kernel == T.NARROW
    assert by["below_nc16_odd_x"].kernel == T.NARROW
    above = [c for c in T.ROW_CASES if ">=lean" in c.claims or c.ldx == T.LD_WIDE]
    assert above and all(c.kernel != T.NARROW for c in above)
    assert {c.kernel for c in above} == {T.CC, T.PLAIN}
    far = {(c.variant, c.nc) for c in T.ROW_CASES if c.name.startswith("far")}
    assert far >= {(v, nc) for v in (3, 4, 5) for nc in (8, 48, 80, 130)}
    assert {c.kernel for c in T.ROW_CASES if c.rows != c.cols} == {T.NARROW, T.CC}
    assert {c.xoff % 2 for c in T.ROW_CASES} == {0, 1} and {c.yoff % 2 for c in T.ROW_CASES if c.ldy} == {0, 1}


def test_the_restated_row_rule_is_the_header_s():
    names = {"PLAIN": T.PLAIN, "CC": T.CC, "NARROW": T.NARROW}
    facts = []
    for c in T.ROW_CASES:
        facts.append((c.variant, c.nc, c.xoff, c.yoff, c.ldx, c.rows, c.cols, 40, int(c.rows != c.cols)))
    # ... and around the guard itself: every variant and width of the table at the three row counts and both leading dimensions
    for variant in (1, 3, 4, 5):
        for nc in (8, 9, 16, 17, 32, 33, 48, 80, 130):
            for xoff, yoff in ((0, 0), (2, 3), (3, 0), (3, 3)):
                for m in (T.M_BELOW, T.M_ABOVE, T.M_FAR):
                    for ld in (T.LD_TALL, T.LD_WIDE, 144):
                        facts.append((variant, nc, xoff, yoff, ld, m, m, 40, 0))
    facts.append((1, 16, 0, 0, 144, 300, 300, 65, 0))  # a long row
    got = ask(["row %d %d %d %d %d %d %d %d %d" % f for f in facts])
    for f, g in zip(facts, got):
        variant, nc, xoff, yoff, ld, m, cols, nnz, rect = f
        assert names[g] == T.row_choice(variant, nc, xoff, yoff, ld, ld, m, cols, nnz, rect_tail=bool(rect)), (f, g)
    for c, g in zip(T.ROW_CASES, got):
        assert names[g] == c.kernel, (c, g)


def test_the_restated_fused_step_rule_is_the_header_s():
    ms = [1, T.ITER_M, T.ITER_M_LAST - 1, T.ITER_M_LAST, T.ITER_M_LAST + 1, 1 << 24, 20_000_000]
    lds = [T.ITER_LD, 64, T.LD_TALL, T.LD_WIDE]
    q = [(m, ld) for m in ms for ld in lds] + [(T.M_BELOW, T.LD_TALL), (T.M_ABOVE, T.LD_TALL)]
    got = ask(["cheb %d %d" % x for x in q])
    for (m, ld), g in zip(q, got):
        assert bool(int(g)) == T.cheb_fused_allowed(m, ld), (m, ld, g)
    assert T.cheb_fused_allowed(T.ITER_M) and T.cheb_fused_allowed(T.ITER_M_LAST) and not T.cheb_fused_allowed(T.ITER_M_LAST + 1)


def test_the_guards_inside_the_kernel_sources_read_as_restated():
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    assert T.LEAN_LIMIT == 0xFFFFFF00 and len(re.findall(r"< 0xffffff00ull", text("row_choice.h"))) == 3
    assert "(int64_t)A->m * ldx < 0x7fffffffLL" in text("spmm_tiled.hip")
    assert "P->gx * P->gy * std::max(std::max(ldx, ldy), PL_REC) * 8 < 0x7fffffffLL" in text("spmm_planes.hip")
    assert "constexpr int GROUPS = 256 / LPR, ROWS = GROUPS * RPG, CAP = %d;" % T.LDS_STAGED in text("spmm.hip")
    assert "const int lds_cap = %d;" % T.LDS_STAGED in text("spmm.hip")
    # the register kernel of the LDS-staged product: element offsets of 2^29 and more (4 GiB in bytes) below its guard, refused from
    # 0x7fffffff elements on
    assert T.tiled_reg_allowed(1073, T.LD_TALL) and 1072 * T.LD_TALL >= 1 << 29 and not T.tiled_reg_allowed(1100, T.LD_TALL)
    assert 1100 * T.LD_TALL * 8 < 24 << 30


@pytest.mark.parametrize("shape", sorted({(c.rows, c.cols) for c in T.ROW_CASES}))
def test_an_operator_gathers_from_both_sides_of_the_lines(shape):
    op = T.operator(*shape)
    n_rows, n_cols = shape
    cnt = np.diff(op.rowptr)
    assert cnt.max() <= 40 and op.col.min() == 0 and op.col.max() == n_cols - 1
    for i in range(n_rows):
        c = op.col[op.rowptr[i]:op.rowptr[i + 1]]
        assert np.all(np.diff(c) > 0)
        if i in T.SHORT_ROWS:
            assert c.size == T.SHORT_ROWS[i]
            if c.size == 1:
                assert c[0] == n_cols - 1
            continue
        # column 0, a column whose X row starts past 2^31 at LD_TALL, the last column
        assert c[0] == 0 and c[-1] == n_cols - 1 and ((c >= T.ROW_PAST_2G) & (c < 268)).any() and (c >= 256).any(), i
        if n_cols > T.ROW_PAST_4G:
            assert (c >= T.ROW_PAST_4G).any()
    short = sorted(T.SHORT_ROWS.values())
    assert short == [0, 1, 7, 8, 9]
    lo, hi = T.DENSE_BLOCK
    assert lo % 64 == 0 and hi - lo == 64 and op.rowptr[hi] - op.rowptr[lo] > T.LDS_STAGED
    # the other blocks of 64 rows are staged
    for r0 in range(0, n_rows, 64):
        if r0 != lo:
            assert op.rowptr[min(n_rows, r0 + 64)] - op.rowptr[r0] <= T.LDS_STAGED
    # operands and the reference: integers, exact
    assert np.abs(op.val).max() <= 8 and (op.val != 0).all() and np.abs(op.X).max() <= 16 and op.ref.dtype == np.int64
    T.assert_exact(op.ref, 40 * 8 * 16)
    assert op.X.shape == (n_cols, T.WMAX) and op.ref.shape == (n_rows, T.WMAX) and not op.ref.flags.writeable


def test_the_dense_operands_are_exact():
    for k in (1, 16, 64, 256):
        assert T.dense_partial_bound(T.DENSE_ROWS, k) < 2 ** 53
    V = T.dense_panel(T.DENSE_ROWS, 40)
    W = T.dense_panel(T.DENSE_ROWS, 24, shift=5)
    S = T.dense_coef(40, 24, seed=3)
    assert np.abs(V).max() <= 16 and np.abs(W).max() <= 16 and np.abs(S).max() <= 8 and np.array_equal(S, np.rint(S)) and not np.array_equal(V[:, :24], W)
    T.assert_exact(V.T @ W, T.dense_partial_bound(T.DENSE_ROWS, 1))
    T.assert_exact(V @ S, T.dense_partial_bound(1, 40))
    with pytest.raises(AssertionError):
        T.assert_exact(np.array([0.5]), 10)
    with pytest.raises(AssertionError):
        T.assert_exact(np.array([2.0]), 2 ** 53)
