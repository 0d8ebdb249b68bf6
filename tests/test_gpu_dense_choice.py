"""Every instantiation of the dense kernels on the device, once: the rows that rails_amd/lib/dense_choice_host --table prints (the
smallest shape that reaches each instantiation listed in rails_amd/csrc/dense_choice.h, and the switch setting where it takes one) are
run through the public entry points by tests/dense_choice_cases.py -- rails_gram, rails_panel_gemm, rails_panel_gemm_wide,
rails_update_gram_deferred and, for the two-segment kernels, the deflated orthogonalisation -- at m = 1003 rows (4099 for the fused pass,
which starts at 4096), and held against a float64 numpy product within the bounds the existing tests of those entry points use (cited in
dense_choice_cases.py).  Where rails_dense_last_tiles and rails_dense_last_update_gram_form expose the choice it must be the table's.
The two process-wide switches are set with their setters and put back; a row that needs an environment variable runs in a fresh process."""
import os

import pytest

import dense_choice_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=5)
    before = c.lib.rails_dense_tile_fit(), c.lib.rails_dense_update_gram_pipeline()
    yield c
    c.lib.rails_dense_set_tile_fit(before[0])
    c.lib.rails_dense_set_update_gram_pipeline(before[1])
    c.close()


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(cases.EXE):
        import rails_amd.build

        rails_amd.build.build()
    return cases.table()


def test_table_covers_every_primitive(rows):
    assert {r["primitive"] for r in rows} == {"gram", "gram2", "panel_gemm", "panel_gemm2", "gemm_wide", "update_gram"}
    assert all(r["m"] == (4099 if r["primitive"] == "update_gram" else 1003) for r in rows)


@pytest.mark.parametrize("primitive", ["gram", "gram2", "panel_gemm", "panel_gemm2", "gemm_wide", "update_gram"])
def test_every_instantiation_matches_numpy(ctx, rows, primitive):
    import rails_amd

    mine = [r for r in rows if r["primitive"] == primitive]
    assert mine
    for row in mine:
        print(cases.row_id(row))
        if cases.env_of(row):
            cases.check_row_in_child(row)
        else:
            cases.check_row(rails_amd, ctx, row)
