"""The host-side tile plan of the LDS-staged SpMM (rails_amd/csrc/tile_plan.cpp), checked on the CPU by a stand-alone program
(tests/cpp/tile_plan_host.cpp, built by rails_amd/csrc/Makefile into rails_amd/lib/tile_plan_host, linked against tile_plan.o only:
no HIP, no library).

The program generates its patterns itself -- banded, the 7- and 27-point stencils, a 2-D grid, ragged rows with an empty last tile, a
grid whose tiles do not all fit their halo box -- and checks on each what the kernels of spmm_tiled.hip rely on (its header lists it).
For the banded pattern the longest row, the largest footprint and the reuse are computed here, in numpy, from the same generator
(spmm_reference.tile_stats_host) and handed to the program: the expected values never come from the code under test."""
import os
import subprocess

import numpy as np

import spmm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "tile_plan_host")


def banded(m, n, bw):
    """the generator `banded` of tile_plan_host.cpp: n - 1 entries at i +- (1 .. bw), reflected at the ends, and the diagonal"""
    i = np.arange(m, dtype=np.uint64)[:, None]
    k = np.arange(n - 1, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + k * np.uint64(40503) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    off = 1 + ((h >> np.uint64(8)) % np.uint64(bw)).astype(np.int64)
    ii = i.astype(np.int64)
    j = np.where(((h >> np.uint64(4)) & np.uint64(1)) == 1, ii + off, ii - off)
    j = np.where((j < 0) | (j >= m), 2 * ii - j, j)
    col = np.sort(np.concatenate([j, ii], axis=1), axis=1)
    assert col.min() >= 0 and col.max() < m
    return np.arange(m + 1, dtype=np.int64) * n, col.ravel().astype(np.int32)


def test_tile_plan_on_the_host():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    st = R.tile_stats_host(*banded(3000, 12, 40))
    assert st["max_row_nnz"] == 12 and st["reuse"] >= 1.8, st
    p = subprocess.run([EXE, str(st["max_row_nnz"]), str(st["max_fp"]), repr(st["reuse"])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("PASS ")] == ["banded", "grid7", "grid27", "grid9_2d", "ragged", "box_fail"]
