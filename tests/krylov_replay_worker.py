"""The device side of test_gpu_krylov_replay.py: the operators of krylov_reference.CASES on the device and one solve with its
history, imported by the test; and, run as a script, one process per setting of FS_UPDATE_NT (read once per process): the four
solve kinds on the four sizes with one workgroup of the update kernels, at the tolerances argv[2] holds, into the .npz file argv[1].
Last output line "ok"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import krylov_reference as kr  # noqa: E402

SIZE_KINDS = ("cg_scaled", "cg_unscaled", "pipelined", "bicgstab")


def case_of(n, kind):
    """the operator a solve kind runs on at size n: SPD for the CG recurrences, with advection for BiCGStab"""
    return ("adv%d" if kind.startswith("bicgstab") else "box%d") % n


def device_operator(B, name):
    """{"A", "b", "csr", "bh", "keep"}: the operator of a case assembled on the device, its right-hand side, and both as the host
    sees them (to_csr, get)."""
    import scipy.sparse as sp
    co, ce = kr.mesh_of(name)
    form = kr.CASES[name][1]
    mesh = B.DeviceMesh(co, ce)
    V = B.DeviceSpace(mesh, 3 if "lame" in form else 1)
    A = B.DeviceMatrix(V)
    A.assemble(**form)
    assert V.n_owned == kr.ROWS[name], (name, V.n_owned)
    b = B.DeviceVector(V.n_owned, kr.rhs_of(name))
    rp, ci, va, shape = A.to_csr()
    return {"A": A, "b": b, "csr": sp.csr_matrix((va, ci, rp), shape=shape), "bh": b.get(), "n": V.n_owned, "keep": (mesh, V)}


def device_solve(B, op, kind, x0=None, **kw):
    """One krylov_solve of a kind of krylov_reference.DEVICE_KW -> (stats, history, x).  None of these operators takes the row
    dictionary: streaming products, two or more launches per iteration."""
    x = B.DeviceVector(op["n"], x0) if x0 is not None else B.DeviceVector(op["n"])
    st = B.krylov_solve(op["A"], op["b"], x, nonzero_guess=x0 is not None, **dict(kr.DEVICE_KW[kind], **kw))
    hist = B.krylov_history().copy()
    xs = x.get()
    x.close()
    assert st["row_classes"] == 0 and st["product_kind"] == 0 and st["fused_iteration"] == 0, (kind, st)
    return st, hist, xs


def main():
    from fenicssolver_amd import backend as B
    B.init(0)
    out = {}
    with np.load(sys.argv[2]) as z:
        rtols = {k: float(z[k]) for k in z.files}
    B.set_option("cg_fused", 0)
    B.set_option("update_blocks", 1)
    for n in kr.SIZES:
        ops = {}
        for kind in SIZE_KINDS:
            name = case_of(n, kind)
            if name not in ops:
                ops[name] = device_operator(B, name)
                out[name + "/values"] = ops[name]["csr"].data
            tag = "%d/%s" % (n, kind)
            st, hist, xs = device_solve(B, ops[name], kind, rtol=rtols[tag], max_iter=kr.PLACE_ITERATIONS)
            assert st["converged"] == 1 and np.all(np.isfinite(hist)) and np.all(np.isfinite(xs)), (tag, st)
            print(tag, "iterations", st["iterations"], flush=True)
            out[tag + "/iterations"], out[tag + "/hist"], out[tag + "/x"] = np.int64(st["iterations"]), hist, xs
    B.set_option("update_blocks", 1024)
    B.set_option("cg_fused", -1)
    np.savez(sys.argv[1], **out)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
