"""Run by tests/test_gpu_stream_variants.py, one process per setting of FS_SPMV_PAIRS / FS_SPMV_NT / FS_PAIR_BLOCKS (the library reads
them once per process): the streaming product (kind 0) of small operators whose rows do not repeat, at every spmv_unroll and at
spmv_blocks 8 and 1024, against the extended-precision host product, and the Krylov solves whose products carry the fused dots.
Everything that has to be compared ACROSS processes goes into the .npz file argv[1]; what one process can decide it asserts itself.

Output lines the caller reads: "case NAME" ahead of each operator (the library's FS_SPACE_DEBUG lines that follow belong to it),
"worst NAME VARIANT RATIO" = the largest err / (eps |A| |x|) of a product, "plain NAME RATIO" the same for a plain fp64 row sum on
the host."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fenicssolver_amd import backend as B  # noqa: E402
from oracle import fem_oracle as fo, ns_oracle as ns  # noqa: E402
from spmv_reference import _check_against_host, _host_product, _poison, _vector_from_cache  # noqa: E402

UNROLLS = (2, 4, 8, 16)
BLOCKS = (8, 1024)
PAIRS_ON = os.environ.get("FS_SPMV_PAIRS") == "1"
DATA = os.path.join(ROOT, "tests", "golden", "data")

B.init(0)
out = {}


def say(*a):
    print(*a, flush=True)


def plain_row_sums(A, xv):
    """Plain fp64 row sums (one rounding per product and per addition, no FMA) in the order of the CSR copy: ascending columns, the
    order in which the DIA offset lists and the SELL columns hold a row."""
    rp, ci, va, (nr, _) = A.to_csr()
    rp = rp.astype(np.int64)
    lens = np.diff(rp)
    acc = np.zeros(nr)
    for k in range(int(lens.max())):
        live = np.flatnonzero(lens > k)
        e = rp[live] + k
        acc[live] = acc[live] + va[e] * xv[ci[e]]
    return acc


def products(name, A, V, seed, scalar=True, block4=False):
    """Every variant of the product of A twice (same bits), finite and within 4 eps |A| |x| of the host, kind 0."""
    say("case", name)
    n_local, n_owned = V.n_local, V.n_owned
    xv = np.random.default_rng(seed).standard_normal(n_local)
    y_ref, ax = _host_product(A, xv)
    # the bound is a condition on the inputs too: a plain fp64 sum has to stay inside it for this operator and this seed
    say("plain", name, "%.3f" % _check_against_host(plain_row_sums(A, xv), y_ref, ax, (name, "plain fp64 row sums on the host")))
    x = B.DeviceVector(n_local, xv)
    y = B.DeviceVector(n_owned)
    unroll_option = "spmv_unroll4" if block4 else "spmv_unroll"
    for v1, v2 in [(u, nb) for u in ((1, 2, 4) if block4 else UNROLLS) for nb in BLOCKS]:
        B.set_option(unroll_option, v1)
        B.set_option("spmv_blocks", v2)
        tag = "%s/u%d/b%d" % (name, v1, v2)
        ys = []
        for _ in range(2):
            y.fill(np.nan)                       # a row that no launch writes stays NaN
            if block4:
                A.spmv(x, y)                     # (fs_spmv_dictionary would take the Taylor-Hood kernels: kind 4)
            else:
                assert A.spmv_dictionary(x, y) == 0, (tag, "the rows repeat")
            assert B.last_product_kind() == 0, (tag, B.last_product_kind())
            ys.append(y.get())
        assert np.array_equal(ys[0], ys[1]), (tag, "two runs differ", int((ys[0] != ys[1]).sum()))
        say("worst", name, "u%d/b%d" % (v1, v2), "%.3f" % _check_against_host(ys[0], y_ref, ax, tag))
        out["y/" + tag] = ys[0]
    B.set_option(unroll_option, 2 if block4 else 4)
    B.set_option("spmv_blocks", 1024)
    x.close()
    y.close()
    if scalar and PAIRS_ON:
        # x in a block of the cache that held NaN / all-ones bits: the two-rows-per-lane kernel reads x in clamped pairs too
        runs = {}
        for pattern in ("zero", "nan", "ones"):
            y = B.DeviceVector(n_owned)
            _poison(B, (n_local + 1, n_local + 2), pattern, seed)
            x = _vector_from_cache(B, n_local)
            x.set(xv)
            assert A.spmv_dictionary(x, y) == 0 and B.last_product_kind() == 0
            runs[pattern] = y.get()
            x.close()
            y.close()
        for pattern, yp in runs.items():
            _check_against_host(yp, y_ref, ax, (name, "poisoned", pattern))
            assert np.array_equal(yp, runs["zero"]), (name, "poisoned", pattern, int((yp != runs["zero"]).sum()))
        assert np.array_equal(runs["zero"], out["y/%s/u4/b1024" % name]), (name, "poisoned: zero-filled cache")
        say("poisoned", name, "n", n_local, "odd" if n_local % 2 else "even")


def scalar_operator(mesh, degree, seed):
    V = B.DeviceSpace(mesh, 1, degree)
    A = B.DeviceMatrix(V)
    kc = np.random.default_rng(seed).uniform(0.5, 1.5, mesh.info()[1])
    A.assemble(stiffness=("cell", kc), mass=0.7)
    return V, A


def vector_operator(mesh, seed):
    V = B.DeviceSpace(mesh, 3)
    A = B.DeviceMatrix(V)
    rng = np.random.default_rng(seed)
    nc = mesh.info()[1]
    A.assemble(lame=("cell", np.stack([rng.uniform(0.8, 1.2, nc), rng.uniform(1.2, 1.8, nc)], axis=1)), mass=0.7)
    return V, A


def shuffled_cube():
    """The cube of pattern_worker.py: vertices and cells in random order, as a mesh file delivers them (SELL slices)."""
    co, ce = fo.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), 9, 8, 7)
    rng = np.random.default_rng(4)
    perm = rng.permutation(len(co))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(co))
    return B.DeviceMesh(co[perm], inv[ce][rng.permutation(len(ce))].astype(np.int32))


def file_mesh():
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(DATA, "mesh.xml"))
    return B.DeviceMesh(co, ce)


# ---- products ----------------------------------------------------------------------------------------------------------------------
# 1: lines of 201 rows, 3015 rows (odd, the last slice partial): slices straddle lines - pairs AND single slices
V, A = scalar_operator(B.DeviceMesh.box(200, 4, 2), 1, 11)
assert V.n_owned == 3015
products("p1_200x4x2", A, V, 101)
# 2: lines of 256 rows, 48 complete slices, pairs inside lines
V, A = scalar_operator(B.DeviceMesh.box(255, 3, 2), 1, 12)
assert V.n_owned == 3072
products("p1_255x3x2", A, V, 102)
# 2b: 200 complete slices: with 8 workgroups every one of them walks several chunks of four (pairs of) slices, and the range of the
# last XCD is cut short by the end of the list (xcd_chunks)
V, A = scalar_operator(B.DeviceMesh.box(255, 4, 9), 1, 13)
assert V.n_owned == 12800
products("p1_255x4x9", A, V, 103)
# 3: SELL slices
V, A = scalar_operator(file_mesh(), 1, 14)
assert V.n_owned == 1069
products("p1_file", A, V, 104)
V, A = scalar_operator(shuffled_cube(), 1, 15)
products("p1_shuffled", A, V, 105)
# 4: CG2: split DIA slices, rows of up to 65 entries (five 16-entry rounds, a remainder at every unroll)
V, A = scalar_operator(B.DeviceMesh.box(20, 3, 3), 2, 16)
assert V.n_owned == 41 * 7 * 7
products("p2_20x3x3", A, V, 106)
V, A = scalar_operator(file_mesh(), 2, 17)
products("p2_file", A, V, 107)
# 4b: CG2 with lines of 200 and 201 rows: whole slices inside a line, which the two-rows-per-lane kernel takes in pairs - the one
# place where its rows span several 16-entry rounds (a P1 row has 15 entries at most)
V, A = scalar_operator(B.DeviceMesh.box(200, 2, 2), 2, 20)
assert V.n_owned == 401 * 5 * 5
rp = A.to_csr()[0].astype(np.int64)
longest = np.maximum.reduceat(np.diff(rp), np.arange(0, V.n_owned, 64))
say("slices p2_200x2x2", len(longest), "longest row <= 16:", int((longest <= 16).sum()), "> 32:", int((longest > 32).sum()), "> 48:", int((longest > 48).sum()))
products("p2_200x2x2", A, V, 112)
# 5: vector spaces: 3 x 3 blocks (rounds of FS_BLOCK_ROUND block entries and a tail), 2 x 2 blocks (plane strain)
V, A = vector_operator(B.DeviceMesh.box(7, 6, 5), 18)
products("v3_7x6x5", A, V, 108, scalar=False)
V, A = vector_operator(file_mesh(), 19)
products("v3_file", A, V, 109, scalar=False)
co2, ce2 = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 40, 11)
rng = np.random.default_rng(5)
inner = (co2[:, 0] > 0) & (co2[:, 0] < 2) & (co2[:, 1] > 0) & (co2[:, 1] < 0.5)
co2 = co2 + 0.004 * rng.standard_normal(co2.shape) * inner[:, None]
V = B.DeviceSpace(B.DeviceMesh(co2, ce2.astype(np.int32)), ncomp=2)
A = B.DeviceMatrix(V)
A.assemble(lame=(1.0, 1.5), mass=0.7)
products("v2_rectangle", A, V, 110, scalar=False)
# 6: 4 x 4 blocks: the linearised Navier-Stokes operator of test_linearised_system_matches_oracle (Newton, 1 / dt = 7)
co, ce = fo.box_mesh((0, 0, 0), (1.0, 0.8, 1.3), 3, 3, 3)
th = ns.TaylorHood(co, ce)
W = B.DeviceSpace(B.DeviceMesh(co, ce), ncomp=4, degree=2)
rng = np.random.default_rng(1)
w0 = 0.3 * rng.standard_normal(th.n)
wp = 0.3 * rng.standard_normal(th.n)
w0[th.dummy_dofs()] = 0.0
J = B.DeviceMatrix(W)
g = B.DeviceVector(W.n_owned)
B.assemble_navier_stokes(J, g, B.DeviceVector(W.n_local, w0), B.DeviceVector(W.n_local, wp), nu=0.07, rho=1.7, inv_dt=7.0,
                         body_force=(0.1, -0.2, -9.8), convection=True, newton=True)
products("th_3x3x3", J, W, 111, scalar=False, block4=True)

# ---- solves: the products with fused dots (DOTS 3 / 1 / 4 / 2) -----------------------------------------------------------------------
# Operator 1 with the plane x = 0 held.  The caller compares iteration counts between settings that sum the dot partials in another
# order, which says something only while a last-bit change of a dot has not grown to the size of the residual: CG carries it along
# unchanged (measured: histories of 1091 entries agree to 1e-12), BiCGStab multiplies it by 10 about every 2.5 iterations, with the
# pair kernel or without (histories equal to 1e-16 for five entries, 1e-10 apart at entry 20, unrelated from entry 40).  So the mass
# term is chosen for the length of the solve: 1e4 for the CG recurrences (81 iterations on the host, the first 20 entries of the
# history far above round-off), 1e5 for BiCGStab (fewer than 25).
RTOL = 1e-10


def held_operator(dims, mass):
    mesh = B.DeviceMesh.box(*dims)
    V = B.DeviceSpace(mesh, 1)
    A = B.DeviceMatrix(V)
    A.assemble(stiffness=("cell", np.random.default_rng(11).uniform(0.5, 1.5, mesh.info()[1])), mass=mass)
    b = B.DeviceVector(V.n_owned)
    B.assemble_vector(V, b, source=1.0)
    face = np.flatnonzero(np.arange(V.n_owned) % (dims[0] + 1) == 0).astype(np.int32)
    A.apply_dirichlet(b, face, np.full(len(face), 2.0), True)
    return V, A, b


CG = {"cg_scaled": dict(method="cg", diagonal_scale=True), "cg_unscaled": dict(method="cg", diagonal_scale=False),
      "pipelined": dict(method="cg", pipelined=True)}
# name, box, mass, solves, spmv_unroll, spmv_blocks.  The last group: the 200 slices of operator 2b on 8 workgroups, each of which sums
# its dots over several chunks (on operator 1 no workgroup has more than one)
GROUPS = (("solve", (200, 4, 2), 1e4, CG, (4, 16), 1024),
          ("solve", (200, 4, 2), 1e5, {"bicgstab": dict(method="bicgstab", diagonal_scale=True)}, (4, 16), 1024),
          ("solve8", (255, 4, 9), 1e4, CG, (4,), 8))
B.set_option("cg_fused", 0)
for group, dims, mass, solves, unrolls, blocks in GROUPS:
    say("case", "%s_mass_%g" % (group, mass))
    V, A, b = held_operator(dims, mass)
    B.set_option("spmv_blocks", blocks)
    if solves is CG:
        rp, ci, va, _ = A.to_csr()
        out[group + "/A_rp"], out[group + "/A_ci"], out[group + "/A_va"], out[group + "/b"] = rp, ci, va, b.get()
    for unroll in unrolls:
        B.set_option("spmv_unroll", unroll)
        for kind, kw in solves.items():
            tag = "%s/%s/u%d" % (group, kind, unroll)
            x = B.DeviceVector(V.n_owned)
            st = B.krylov_solve(A, b, x, rtol=RTOL, max_iter=5000, **kw)
            hist = B.krylov_history().copy()
            assert st["converged"] == 1, (tag, st)
            assert st["product_kind"] == 0 and st["row_classes"] == 0, (tag, st["product_kind"], st["row_classes"])
            assert st["true_rel_residual"] <= 5 * RTOL, (tag, st["true_rel_residual"])
            assert np.all(np.isfinite(hist)), tag
            say(tag, "iterations", st["iterations"], "true_rel_residual %.3e" % st["true_rel_residual"])
            out[tag + "/iterations"], out[tag + "/hist"], out[tag + "/x"] = np.int64(st["iterations"]), hist, x.get()
            x.close()
B.set_option("spmv_blocks", 1024)
B.set_option("spmv_unroll", 4)
B.set_option("cg_fused", -1)
np.savez(sys.argv[1], **out)
say("ok")
