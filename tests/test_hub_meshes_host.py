"""The hub meshes of tests/hub_meshes.py are what test_gpu_hub_meshes.py says they are: one row of the stated length on the stated
row, every other row short, all cells with volume, the cones of a ball disjoint.  No GPU."""
import numpy as np
import pytest

import hub_meshes as hm
from oracle import fem_oracle as fo

# every other row stays below the smallest limit the hub sizes straddle - 16 stored entries in CG1 (the first register look-up
# of k_inc_fill), 125 in CG2 (the smallest CG2 hub under test) - so the hub alone decides the path.  What the ballast has:
OTHER_ROWS_MAX = {1: 15, 2: 65}


def _p2_table(co, ce):
    return (fo.p2_cell_dofs if co.shape[1] == 3 else fo.tri_p2_cell_dofs)(len(co), ce)


def test_row_length_formulas_of_the_issue():
    table = {("ball", 27): (28, 130), ("ball", 31): (32, 150), ("ball", 32): (33, 155), ("ball", 127): (128, 630),
             ("ball", 260): (261, 1295), ("spindle", 40): (42, 163)}
    for (gen, size), (l1, l2) in table.items():
        assert hm.hub_row_length(gen, 1, size) == l1 and hm.hub_row_length(gen, 2, size) == l2
        co, ce, hub = getattr(hm, gen)(size)
        rp, _ = fo.csr_pattern(len(co), ce)
        assert np.diff(rp)[hub] == l1
        cd, edges = fo.p2_cell_dofs(len(co), ce)
        assert hm.row_lengths(len(co) + len(edges), cd)[hub] == l2


@pytest.mark.parametrize("size", [4, 15, 27, 260])
def test_ball_is_a_star_around_its_hub(size):
    co, ce, hub = hm.ball(size)
    assert len(ce) == 2 * size - 4 and np.all(ce[:, 0] == hub)
    vol = hm.volumes(co, ce)
    assert vol.min() > 1e-6
    # the cones from the ORIGIN over the hull triangles tile the polyhedron; those from the hub fill the same volume only if
    # the hub sees every triangle from inside, i.e. no two cells overlap
    from_origin = np.abs(np.linalg.det(co[ce[:, 1:].astype(np.int64)])) / 6.0
    assert abs(vol.sum() - from_origin.sum()) <= 1e-12 * vol.sum()


@pytest.mark.parametrize("family,size,hub_row", hm.cases())
def test_hub_mesh_has_one_long_row_where_requested(family, size, hub_row):
    gen, degree, _, _ = hm.FAMILIES[family]
    co, ce, row = hm.build(family, size, hub_row)
    n = len(co)
    assert ce.dtype == np.int32 and np.all(np.diff(ce, axis=1) > 0) and ce.min() == 0 and ce.max() == n - 1
    assert row == (n - 1 if hub_row < 0 else hub_row) and n > 64
    assert hm.volumes(co, ce).min() > 1e-6
    want = hm.hub_row_length(gen, degree, size)
    rp, ci = fo.csr_pattern(n, ce)
    len1 = np.diff(rp)
    assert np.array_equal(len1, hm.row_lengths(n, ce))
    if degree == 1:
        lengths = len1
    else:
        cd, edges = _p2_table(co, ce)
        lengths = hm.row_lengths(n + len(edges), cd)
    assert lengths[row] == want == lengths.max()
    assert len(lengths) % 64 != 0                    # a partial last slice
    long_rows = np.flatnonzero(lengths > OTHER_ROWS_MAX[degree])
    if gen == "spindle":
        # the other pole and the node of the axis edge see the same m cells
        assert len(long_rows) == 3 and np.all(lengths[long_rows] == want) and row in long_rows
        assert np.sum(long_rows >= n) == 1
    else:
        assert np.array_equal(long_rows, [row])
    # (a spindle is used for CG2 spaces only: its poles are two long CG1 rows)
    assert np.sort(len1)[-2 if gen != "spindle" else -3] <= OTHER_ROWS_MAX[1]


def test_with_ballast_only_renumbers():
    co0, ce0, hub = hm.ball(16)
    vol0 = np.sort(hm.volumes(co0, ce0))
    for r in hm.HUB_ROWS:
        co, ce, row = hm.with_ballast(co0, ce0, r, hub)
        assert np.allclose(co[row], co0[hub], rtol=0, atol=0)
        vol = np.sort(hm.volumes(co, ce))
        assert len(vol) == len(vol0) + 6 * 4 * 4 * 3
        touching = np.any(ce == row, axis=1)
        assert np.allclose(np.sort(hm.volumes(co, ce[touching])), vol0, rtol=1e-12, atol=0)      # (the vertex order inside a cell changed)
