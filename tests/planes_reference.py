"""The plane-sweep SpMM's launch plan restated in plain Python, grids that drive the kernel into long z segments, and a 7-point stencil
whose coefficients can be told apart.  Not a test module.

plan() restates two pieces of host code of rails_amd/csrc/spmm_planes.hip by hand: planes_dispatch's table (the instantiation
k_spmm_planes<LPR, RW, WX, WY> by the panel's width) and planes_launch's segment rule (the z range of a launch is cut into nseg
segments of seglen planes: the workgroups run in rounds of one per CU, a segment of len planes costs len + 4 steps, the cheapest
rounds * (len + 4) wins, the first of equals).  The GPU tests compare it with what the library reports (rails_csr_planes_stats), so a
case that was meant to run a long segment and did not is a failure.

A segment of len planes runs len + 2 steps of the kernel's loop; the step that stores a plane while the next ones are in flight
(`s >= 3`) needs len >= 2, both X buffers and the three record buffers have been re-used once len >= 5.

find_grid() searches the small grids for the one with the fewest rows whose plan has long segments on a device of num_cu compute
units, with whole and partial patches on both sides (a strip one patch wide would leave most lanes of every wave without a row).
For a given number of patches per plane the smallest grid has one grid column in the last patch of a line and one line in the last
patch row, so the search walks patch counts, not grid sizes."""
import functools

import numpy as np

SHAPES = ((16, (8, 2, 4, 2)), (32, (16, 2, 4, 3)), (64, (32, 2, 4, 4)), (None, (64, 2, 4, 4)))  # widest panel -> LPR, RW, WX, WY
MAX_SEGMENTS = 256
GZ_MAX = 64   # find_grid: most planes of a grid it looks at
NP_MAX = 96   # ... most patches per direction


def shape(nc):
    """k_spmm_planes<LPR, RW, WX, WY> for a panel of nc columns, and the patch PX x PY of grid columns a workgroup owns."""
    for widest, s in SHAPES:
        if widest is None or nc <= widest:
            LPR, RW, WX, WY = s
            return dict(LPR=LPR, RW=RW, WX=WX, WY=WY, PX=RW * WX, PY=WY * (64 // LPR))


@functools.lru_cache(maxsize=None)
def segments(wgs_per_segment, nz, num_cu):
    """(seglen, nseg) for nz output planes when one segment of the whole grid takes wgs_per_segment workgroups (patches x column chunks)."""
    best, best_len = None, nz
    for nseg in range(1, min(nz, MAX_SEGMENTS) + 1):
        length = -(-nz // nseg)
        ns = -(-nz // length)
        rounds = -(-(wgs_per_segment * ns) // num_cu)
        cost = rounds * (length + 4)
        if best is None or cost < best:
            best, best_len = cost, length
    return best_len, -(-nz // best_len)


def plan(grid, nc, num_cu, z_lo=0, z_hi=None):
    gx, gy, gz = grid
    z_hi = gz if z_hi is None else z_hi
    s = shape(nc)
    patches = -(-gx // s["PX"]) * -(-gy // s["PY"])
    chunks = -(-nc // (2 * s["LPR"]))
    seglen, nseg = segments(patches * chunks, z_hi - z_lo, num_cu)
    return dict(LPR=s["LPR"], RW=s["RW"], WX=s["WX"], WY=s["WY"], PX=s["PX"], PY=s["PY"], patches=patches, chunks=chunks, seglen=seglen, nseg=nseg)


def find_grid(nc, num_cu, min_seglen, multi_segment, max_rows=400_000):
    """The grid (gx, gy, gz) with the fewest rows (ties: the smallest tuple) among gx > PX, gy > PY (a whole patch and more in both
    directions), 3 <= gz <= GZ_MAX, at most NP_MAX patches per direction and max_rows rows, whose plan has seglen >= min_seglen,
    nseg >= 2 (multi_segment) or nseg == 1 (not), and gx % PX != 0 and gy % PY != 0.  None if there is none."""
    s = shape(nc)
    PX, PY = s["PX"], s["PY"]
    sides = sorted((((npx - 1) * PX + 1) * ((npy - 1) * PY + 1), (npx - 1) * PX + 1, (npy - 1) * PY + 1)
                   for npx in range(2, NP_MAX + 1) for npy in range(2, NP_MAX + 1))
    gz0 = max(3, min_seglen)
    best = None
    for area, gx, gy in sides:
        if area * gz0 > (max_rows if best is None else min(max_rows, best[0])):
            break
        assert gx % PX != 0 and gy % PY != 0
        for gz in range(gz0, GZ_MAX + 1):
            cand = (area * gz, gx, gy, gz)
            if cand[0] > max_rows or (best is not None and cand >= best):
                break
            p = plan((gx, gy, gz), nc, num_cu)
            if p["seglen"] >= min_seglen and (p["nseg"] >= 2 if multi_segment else p["nseg"] == 1):
                best = cand
                break
    return None if best is None else best[1:]


def cross7_random(gx, gy, gz, seed):
    """The complete 7-point stencil on a gx x gy x gz grid with every value drawn per entry (the axis neighbours and the diagonal of
    problems.stencil27's random form): A != A', no two coefficients of a row are equal, rows sorted by column."""
    from rails_amd import problems as P

    rowptr, col, val = P.stencil27(gx, gy, gz, random_values=True, seed=seed)
    m = rowptr.size - 1
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptr))
    c = col.astype(np.int64)
    off_axis = ((c % gx != row % gx).astype(int) + ((c // gx) % gy != (row // gx) % gy) + (c // (gx * gy) != row // (gx * gy)))
    keep = off_axis <= 1
    rp = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(row[keep], minlength=m), out=rp[1:])
    return rp, np.ascontiguousarray(col[keep]), np.ascontiguousarray(val[keep])
