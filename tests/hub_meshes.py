"""Meshes with ONE very long matrix row (a "hub"): what the row-length-dependent paths of the symbolic phase and of the assembly are
tested on (test_hub_meshes_host.py, test_gpu_hub_meshes.py).  numpy + scipy.spatial.ConvexHull; the ballast is a regular mesh of the
oracle.

    ball(S)      a hub vertex near the origin joined to every triangle of the convex hull of S points on a sphere:
                 2S - 4 tetrahedra; hub row length S + 1 (CG1), 5S - 5 (CG2)
    spindle(m)   m tetrahedra around one edge (two poles, a ring of m): the poles AND the CG2 node of the axis edge have rows of
                 4m + 3 entries (CG2); the poles m + 2 in CG1
    fan(m)       m triangles around one vertex: hub row length m + 1 (CG1), 3m + 1 (CG2)

Every generator returns (coords, cells, hub) with the hub vertex 0; with_ballast() appends a regular mesh whose rows are short and
moves the hub to a chosen row.  Cells hold ascending vertex ids (int32)."""
import numpy as np
from scipy.spatial import ConvexHull

from oracle import fem_oracle as fo

HUB_ROWS = (0, 63, 64, -1)      # first / last lane of a full 64-row slice, first lane of the next slice, the partial last slice

# family -> (generator name, degree of the space, hub sizes: the one just below and the one just above every limit of
# fs_symbolic.hip / fs_assemble.hip, the size that runs at all four hub rows: the one just above the first limit)
FAMILIES = {
    "cg1_tet": ("ball", 1, (15, 16, 31, 32, 127, 128, 254, 255, 260), 16),
    "cg1_tri": ("fan", 1, (31, 32, 127, 128, 254, 255), 32),
    "cg2_tet_ball": ("ball", 2, (26, 27, 33, 34, 52, 53), 27),
    "cg2_tet_spindle": ("spindle", 2, (31, 32, 39, 40), 32),
    "cg2_tri": ("fan", 2, (42, 43, 53, 54), 43),
}


def hub_row_length(generator, degree, size):
    return {("ball", 1): size + 1, ("ball", 2): 5 * size - 5, ("spindle", 1): size + 2, ("spindle", 2): 4 * size + 3,
            ("fan", 1): size + 1, ("fan", 2): 3 * size + 1}[(generator, degree)]


def cases():
    """(family, size, hub row) of every case: all sizes with the hub on row 63, one size per family on the other three rows too"""
    out = []
    for fam, (_, _, sizes, all_rows) in FAMILIES.items():
        out += [(fam, s, 63) for s in sizes]
        out += [(fam, all_rows, r) for r in HUB_ROWS if r != 63]
    return out


def build(family, size, hub_row):
    """the mesh of a case with its ballast: (coords, cells, hub row)"""
    gen = {"ball": ball, "spindle": spindle, "fan": fan}[FAMILIES[family][0]]
    co, ce, hub = gen(size)
    return with_ballast(co, ce, hub_row, hub)


def _radii(n, seed):
    """radii 1 +- 10 %, fixed seed: no two cells congruent, so that a contribution taken from the wrong cell shows"""
    return 1.0 + 0.1 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def ball(S, seed=7):
    """Fibonacci lattice of S points on the unit sphere; the hull is taken of the points ON the sphere (every one of them is a hull
    vertex), the radii are jittered afterwards: the cones hub - triangle stay disjoint under a radial scaling."""
    assert S >= 4
    i = np.arange(S) + 0.5
    z = 1.0 - 2.0 * i / S
    phi = np.pi * (1.0 + np.sqrt(5.0)) * i
    rho = np.sqrt(1.0 - z * z)
    unit = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    tri = ConvexHull(unit).simplices
    assert len(tri) == 2 * S - 4 and len(np.unique(tri)) == S
    hub = np.array([[0.01, -0.02, 0.015]])
    co = np.vstack([hub, unit * _radii(S, seed)[:, None]])
    ce = np.concatenate([np.zeros((len(tri), 1), dtype=np.int64), 1 + tri], axis=1)
    return co, np.sort(ce, axis=1).astype(np.int32), 0


def spindle(m, seed=8):
    """poles 0 and 1 on the z axis, ring vertices 2 .. m + 1 around it; cell i = (pole, pole, ring i, ring i + 1)"""
    assert m >= 3
    ang = 2.0 * np.pi * np.arange(m) / m
    r = _radii(m, seed)
    ring = np.stack([r * np.cos(ang), r * np.sin(ang), 0.05 * np.sin(3.0 * ang)], axis=1)
    co = np.vstack([[0.0, 0.0, -0.8], [0.0, 0.0, 1.1], ring])
    k = np.arange(m)
    ce = np.stack([np.zeros(m, dtype=np.int64), np.ones(m, dtype=np.int64), 2 + k, 2 + (k + 1) % m], axis=1)
    return co, np.sort(ce, axis=1).astype(np.int32), 0


def fan(m, seed=9):
    """the triangle fan of tests/pattern_worker.py (centre 0, ring 1 .. m), with jittered radii"""
    assert m >= 3
    ang = 2.0 * np.pi * np.arange(m) / m
    r = _radii(m, seed)
    co = np.vstack([[0.0, 0.0], np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)])
    k = np.arange(m)
    ce = np.stack([np.zeros(m, dtype=np.int64), 1 + k, 1 + (k + 1) % m], axis=1)
    return co, np.sort(ce, axis=1).astype(np.int32), 0


def with_ballast(co, ce, hub_row, hub=0, seed=11):
    """Appends a disjoint mesh of short rows - a 4 x 4 x 3 box of 100 vertices with jittered interior vertices, in 2-D a 9 x 8
    rectangle of 90 - and renumbers the vertices with a fixed permutation that puts the hub on row `hub_row` (-1: the last vertex).
    Returns (coords, cells, hub_row >= 0)."""
    co, ce = np.asarray(co, dtype=np.float64), np.asarray(ce, dtype=np.int64)
    rng = np.random.default_rng(seed)
    if co.shape[1] == 3:
        bco, bce = fo.box_mesh((0, 0, 0), (1, 1, 1), 4, 4, 3)
        h = np.array([1.0 / 4, 1.0 / 4, 1.0 / 3])
        inner = np.all((bco > 1e-12) & (bco < 1.0 - 1e-12), axis=1)
        bco = bco + 0.1 * h * rng.uniform(-1.0, 1.0, bco.shape) * inner[:, None]
        bco = bco + np.array([co[:, 0].max() + 0.5, 0.0, 0.0])
    else:
        bco, bce = fo.rectangle_mesh((0, 0), (2, 0.5), 9, 8)
        bco = bco + np.array([co[:, 0].max() + 0.5, 0.0])
    n0, n = len(co), len(co) + len(bco)
    allco = np.vstack([co, bco])
    allce = np.vstack([ce, bce + n0])
    row = n - 1 if hub_row < 0 else int(hub_row)
    assert 0 <= row < n
    new = rng.permutation(n)                         # new id of every old vertex
    other = int(np.flatnonzero(new == row)[0])
    new[other], new[hub] = new[hub], row
    out = np.empty_like(allco)
    out[new] = allco
    return out, np.sort(new[allce], axis=1).astype(np.int32), row


def volumes(co, ce):
    """unsigned cell volumes (areas in 2-D)"""
    p = np.asarray(co, dtype=np.float64)[np.asarray(ce, dtype=np.int64)]
    d = np.linalg.det(p[:, 1:] - p[:, :1])
    return np.abs(d) / (6.0 if p.shape[2] == 3 else 2.0)


def row_lengths(n, cell_dofs):
    """entries per row of the sparsity pattern of a space given by its cell-dof table"""
    cd = np.asarray(cell_dofs, dtype=np.int64)
    nd = cd.shape[1]
    key = np.unique(np.repeat(cd, nd, axis=1).ravel() * n + np.tile(cd, (1, nd)).ravel())
    return np.bincount(key // n, minlength=n)
