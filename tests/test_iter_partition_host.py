"""The step cases of the row-partitioned iterative A^-1 tests (tests/iter_partition_cases.py) on the CPU: every one of them -- those taken
from tests/iter_steps_reference.py's list and those constructed beside it -- meets the two conditions of that module: no bound above
CAP = 4096 eps, and in the longdouble run every column still has rr_k / bb >= 1e-20 at the last step asked for.  A case that misses one
gets fewer steps; the cap is not raised and no case is dropped."""
import numpy as np
import pytest

import iter_partition_cases as PC
import iter_steps_reference as S


def test_the_case_list_is_the_intended_one():
    ids = [c.id for c, _ in PC.STEP_CASES]
    assert len(set(ids)) == len(ids)
    listed = {c.id for c in S.CASES}
    constructed = sorted(c.id for c in PC.CONSTRUCTED)
    assert constructed == ["cg-poly-fused-m72-w1", "cg-poly-fused-m72-w17", "cg-poly-unfused-m72-w1", "cg-poly-unfused-m72-w17"]
    assert not listed & set(constructed) and set(ids) - listed == set(constructed)
    for c, ranks in PC.STEP_CASES:
        assert ranks == ((2,) if (c.m == 2181 and c.poly) else (2, 3))
        assert not c.trans  # the transposed solve of a row block is refused
        if c.id in listed:  # the steps CASES / LOWERED give it
            assert c.steps == S.LOWERED.get((c.variant, c.m, c.w), S.SHAPES[c.m][1])
    assert len(PC.STEP_PARAMS) == 2 * len(ids) - 2


@pytest.mark.parametrize("case_id", [c.id for c, _ in PC.STEP_CASES])
def test_conditions(case_id):
    c = PC.step_case(case_id)
    e = S.expected(c)
    for k in c.steps:
        assert np.all(e.xmax[k] > 0)
        assert np.all(e.bound_x[k] <= S.CAP * e.xmax[k]), (case_id, k, (e.bound_x[k] / e.xmax[k]).max() / S.EPS)  # condition 1
        assert np.all(e.bound_r[k] <= S.CAP), (case_id, k, e.bound_r[k].max() / S.EPS)
    k = max(c.steps)
    assert np.all(e.decay[k] >= S.RR_FLOOR), (case_id, e.decay[k].min())  # condition 2
    print("%s: largest bound %.1f eps of |x|_inf, %.1f eps in the relative residual; rr_K / bb >= %.1e" % (
        case_id, max((e.bound_x[q] / e.xmax[q]).max() for q in c.steps) / S.EPS, max(e.bound_r[q].max() for q in c.steps) / S.EPS, e.decay[k].min()))
