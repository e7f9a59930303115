"""Host restatements of the recurrences of fs_krylov_solve (fs_krylov_iter.inc, begin_pass in fs_krylov_solve.inc), in extended
precision or float64, shared by test_krylov_reference_host.py and test_gpu_krylov_replay.py.

cg_replay        the single-reduction recurrence of cg_scalars_from - unscaled (k_cg_update: z = D^-1 r) or on the symmetrically
                 scaled system (k_cg_update_scaled: z == r, rho = sum d r^2 or sum r^2 / d) - and the pipelined one of k_pcg_update
bicgstab_replay  the right-preconditioned BiCGStab of k_bicg_p / k_bicg_s / k_bicg_x (K1 to K5)
envelope         how far a history moves when the last bit of its dots does: two float64 replays, one with the terms of every dot
                 permuted, against the extended one

Both replays stop as the device does: entry k of the history is written, then `<= threshold` is tested (status 1), then the
iteration limit (status 3: iteration max_iter only checks), then the scalars (status 2: breakdown).  One pass only: the
true-residual restart of restart_wanted is not replayed.

CASES are the operators of both test files, assembled on the host by the oracle here (operator) and on the device there."""
import numpy as np
import scipy.sparse as sp

from oracle import fem_oracle as fo

LD = np.longdouble
EPS = np.finfo(np.float64).eps
QUALIFY = 1e-8            # a history entry qualifies for a device comparison while envelope()[k] <= QUALIFY


class _Op:
    """A CSR matrix (every row has an entry) in the dtype of the replay, rows summed in the order of the columns."""

    def __init__(self, A, dtype):
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.n = A.shape[0]
        self.rp = A.indptr.astype(np.int64)
        self.ci = A.indices.astype(np.int64)
        self.va = A.data.astype(dtype)
        assert A.shape[0] == A.shape[1] and np.all(np.diff(self.rp) > 0), "a row without entries"
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rp))

    def diagonal(self):
        d = np.zeros(self.n, self.va.dtype)
        on = self.rows == self.ci
        d[self.rows[on]] = self.va[on]
        return d

    def scaled(self, sc):
        """D^-1/2 A D^-1/2 as k_scale_copy forms it: (a_ij sc_i) sc_j"""
        B = object.__new__(_Op)
        B.__dict__.update(self.__dict__)
        B.va = (self.va * sc[self.rows]) * sc[self.ci]
        return B

    def __matmul__(self, x):
        return np.add.reduceat(self.va * x[self.ci], self.rp[:-1])


def _dot_for(perm):
    if perm is None:
        return lambda t: t.sum()
    perm = np.asarray(perm)
    return lambda t: t[perm].sum()


def _cg_scalars(k, gamma, delta, rho, gamma_old, alpha_old):
    """cg_scalars_from: (alpha, beta, ok)"""
    with np.errstate(all="ignore"):
        if k == 0:
            beta, alpha = gamma * 0, gamma / delta
        else:
            beta = gamma / gamma_old
            alpha = gamma / (delta - beta * gamma / alpha_old)
    return alpha, beta, bool(alpha > 0.0) and bool(alpha < 1e300) and bool(rho == rho)


def threshold(A, b, rtol, atol, norm="unpreconditioned", dtype=LD):
    """(max(rtol^2 bb, atol^2), bb) of k_set_threshold with bb = ||b||^2 or ||D^-1 b||^2, in `dtype`."""
    b = np.asarray(b).astype(dtype)
    if norm == "preconditioned":
        sc = 1 / np.sqrt(_Op(A, dtype).diagonal())
        b = (sc * sc) * b
    bb = (b * b).sum()
    return max(dtype(rtol) * dtype(rtol) * bb, dtype(atol) * dtype(atol)), bb


def cg_replay(A, b, x0=None, jacobi=True, diagonal_scale=True, norm="unpreconditioned", pipelined=False, rtol=1e-8, atol=0.0,
              max_iter=10000, dtype=LD, perm=None):
    """-> (history, iterations, status, x)"""
    dot = _dot_for(perm)
    op = _Op(A, dtype)
    n = op.n
    b = np.asarray(b).astype(dtype)
    scaled = jacobi and diagonal_scale
    pnorm = norm == "preconditioned"
    assert scaled or not (pipelined or pnorm), "the pipelined recurrence and the preconditioned norm need the scaled system"
    d = op.diagonal() if jacobi else np.ones(n, dtype)
    if scaled:
        sc = 1 / np.sqrt(d)                           # ws.dinv in scaled mode
        wgt = sc * sc if pnorm else d                 # ws.dvec: the dot weights of rho
        op = op.scaled(sc)
        rhs = sc * b
        bn = wgt * b if pnorm else b
    else:
        dinv = 1 / d
        rhs = bn = b
    bb = dot(bn * bn)
    thr = max(dtype(rtol) * dtype(rtol) * bb, dtype(atol) * dtype(atol))
    if x0 is None:
        x = np.zeros(n, dtype)
        r = rhs.copy()
    else:
        x = np.asarray(x0).astype(dtype)
        if scaled:
            x = x / sc
        r = rhs - op @ x
    p = np.zeros(n, dtype)
    s = np.zeros(n, dtype)
    if pipelined:
        w = op @ r
        zz = np.zeros(n, dtype)
    elif not scaled:
        z = dinv * r
    hist = []
    gamma_old = alpha_old = dtype(0)
    k, status = 0, 0
    while True:
        if pipelined:
            gamma, delta, rho = dot(r * r), dot(w * r), dot(wgt * r * r)
        elif scaled:
            w = op @ r
            gamma, delta, rho = dot(r * r), dot(w * r), dot(wgt * r * r)
        else:
            w = op @ z
            gamma, delta, rho = dot(r * z), dot(w * z), dot(r * r)
        hist.append(rho)
        if rho <= thr:
            status = 1
            break
        if k == max_iter:
            status = 3
            break
        alpha, beta, ok = _cg_scalars(k, gamma, delta, rho, gamma_old, alpha_old)
        if not ok:
            status = 2
            break
        if pipelined:
            nv = op @ w
            zz = nv + beta * zz
            s = w + beta * s
            p = r + beta * p
            x = x + alpha * p
            r = r - alpha * s
            w = w - alpha * zz
        else:
            p = (r if scaled else z) + beta * p
            s = w + beta * s
            x = x + alpha * p
            r = r - alpha * s
            if not scaled:
                z = dinv * r
        gamma_old, alpha_old = gamma, alpha
        k += 1
    if scaled:
        x = sc * x
    return np.array(hist, dtype), k, status, x


def bicgstab_replay(A, b, x0=None, jacobi=True, rtol=1e-8, atol=0.0, max_iter=10000, dtype=LD, perm=None):
    """-> (history of r.r, iterations, status, x)"""
    dot = _dot_for(perm)
    op = _Op(A, dtype)
    n = op.n
    b = np.asarray(b).astype(dtype)
    dinv = 1 / op.diagonal() if jacobi else np.ones(n, dtype)
    bb = dot(b * b)
    thr = max(dtype(rtol) * dtype(rtol) * bb, dtype(atol) * dtype(atol))
    if x0 is None:
        x = np.zeros(n, dtype)
        r = b.copy()
    else:
        x = np.asarray(x0).astype(dtype)
        r = b - op @ x
    rhat = r.copy()
    p = np.zeros(n, dtype)
    v = np.zeros(n, dtype)
    rho_new, rr = dot(rhat * r), dot(r * r)
    rho_old = alpha = omega = dtype(0)
    hist = []
    k, status = 0, 0

    def finite(t):
        return bool(t == t) and bool(abs(t) < 1e300)

    while True:
        # K1
        hist.append(rr)
        if rr <= thr:
            status = 1
            break
        if k == max_iter:
            status = 3
            break
        beta = dtype(0)
        with np.errstate(all="ignore"):
            if k > 0:
                beta = (rho_new / rho_old) * (alpha / omega)
        if not (rho_new == rho_new) or rho_new == 0 or not finite(beta):
            status = 2
            break
        p = r.copy() if k == 0 else r + beta * (p - omega * v)
        y = dinv * p
        # K2, K3
        v = op @ y
        rv = dot(rhat * v)
        with np.errstate(all="ignore"):
            alpha = rho_new / rv
        if rv == 0 or not finite(alpha):
            status = 2
            break
        s = r - alpha * v
        z = dinv * s
        # K4, K5
        t = op @ z
        ts, tt = dot(t * s), dot(t * t)
        omega = ts / tt if tt > 0 else dtype(0)
        if not (omega == omega):
            status = 2
            break
        x = x + (alpha * y + omega * z)
        r = s - omega * t
        rho_old = rho_new
        rho_new, rr = dot(rhat * r), dot(r * r)
        k += 1
    return np.array(hist, dtype), k, status, x


def envelope(h_ld, h_64, h_perm):
    """env[k]: the running maximum over j <= k of the relative deviation of the two float64 histories from the extended one, never
    below eps; over the entries all three have."""
    m = min(len(h_ld), len(h_64), len(h_perm))
    ref = np.asarray(h_ld[:m], LD)
    dev = np.maximum(np.abs(np.asarray(h_64[:m], LD) - ref), np.abs(np.asarray(h_perm[:m], LD) - ref)) / np.abs(ref)
    return np.maximum(np.maximum.accumulate(dev.astype(np.float64)), EPS)


def replays(kind, A, b, seed=1, **kw):
    """The three replays of a solve kind ("cg_scaled", "cg_unscaled", "cg_none", "pipelined", "bicgstab", "bicgstab_none") and
    their envelope: {"ld", "f64", "perm": (history, iterations, status, x), "env"}."""
    fn, fixed = KINDS[kind]
    perm = np.random.default_rng(seed).permutation(sp.csr_matrix(A).shape[0])
    out = {"ld": fn(A, b, dtype=LD, **fixed, **kw), "f64": fn(A, b, dtype=np.float64, **fixed, **kw),
           "perm": fn(A, b, dtype=np.float64, perm=perm, **fixed, **kw)}
    out["env"] = envelope(out["ld"][0], out["f64"][0], out["perm"][0])
    return out


KINDS = {
    "cg_scaled": (cg_replay, dict(jacobi=True, diagonal_scale=True)),
    "cg_unscaled": (cg_replay, dict(jacobi=True, diagonal_scale=False)),
    "cg_none": (cg_replay, dict(jacobi=False, diagonal_scale=False)),
    "pipelined": (cg_replay, dict(jacobi=True, diagonal_scale=True, pipelined=True)),
    "bicgstab": (bicgstab_replay, dict(jacobi=True)),
    "bicgstab_none": (bicgstab_replay, dict(jacobi=False)),
}
# the same kinds as arguments of backend.krylov_solve
DEVICE_KW = {
    "cg_scaled": dict(method="cg", precond="jacobi", diagonal_scale=True),
    "cg_unscaled": dict(method="cg", precond="jacobi", diagonal_scale=False),
    "cg_none": dict(method="cg", precond="none", diagonal_scale=False),
    "pipelined": dict(method="cg", precond="jacobi", diagonal_scale=True, pipelined=True),
    "bicgstab": dict(method="bicgstab", precond="jacobi"),
    "bicgstab_none": dict(method="bicgstab", precond="none"),
}


def stopping_points(hist, env, k_min=3):
    """[(k, threshold, factor)], largest factor first: for every qualifying entry k >= k_min in front of which the history drops
    in one iteration - counted from the smallest entry before it, since the device stops at the FIRST entry at or below the
    threshold - the threshold in the middle of that drop: hist[k] * factor == threshold == min(hist[:k]) / factor, factor > 1."""
    h = np.asarray(hist, LD)
    out = []
    for k in range(max(k_min, 1), min(len(h), len(env))):
        if env[k] > QUALIFY or not h[k] > 0:
            break
        factor = np.sqrt(h[:k].min() / h[k])
        if factor > 1:
            out.append((k, h[k] * factor, factor))
    return sorted(out, key=lambda t: -t[2])


# fewest history entries a device comparison has to cover (test_krylov_reference_host.py holds every case to them)
MIN_ENTRIES = {"cg_scaled": 20, "cg_unscaled": 20, "cg_none": 20, "pipelined": 20, "bicgstab": 12, "bicgstab_none": 12}
PLACE_ITERATIONS = 80          # length of the replay with rtol = atol = 0 in which the stopping point is looked for
PLACE_FACTOR = 1.1             # least distance of a placed threshold from its two neighbours (2.0 where the stopping rule is asserted)
PLACE_RTOL_MIN = 1e-10         # no threshold below this relative tolerance: the recurrence residual goes on falling where b - A x cannot
                               # follow in float64, and the solver would answer with a true-residual restart (not replayed)


def placed(kind, A, b, k_min=None, **kw):
    """A solve of `kind` that ends inside the qualifying part of its history: the replays with rtol = atol = 0 over PLACE_ITERATIONS
    iterations, the stopping points at entry k_min (default MIN_ENTRIES[kind]) or later, largest drop first, none below PLACE_RTOL_MIN, and bb.
    -> {"free": replays, "points": [(k, threshold, factor)], "bb": ||b||^2 (or ||D^-1 b||^2) in extended precision}"""
    free = replays(kind, A, b, rtol=0.0, atol=0.0, max_iter=PLACE_ITERATIONS, **kw)
    bb = threshold(A, b, 0.0, 0.0, kw.get("norm", "unpreconditioned"))[1]
    points = stopping_points(free["ld"][0], free["env"], MIN_ENTRIES[kind] if k_min is None else k_min)
    points = [pt for pt in points if pt[1] >= LD(PLACE_RTOL_MIN) ** 2 * bb]
    return {"free": free, "points": points, "bb": bb}


def rtol_for(thr, bb):
    """rtol with rtol^2 bb == thr to the rounding of a double"""
    return float(np.sqrt(LD(thr) / LD(bb)))


# ---- the operators ---------------------------------------------------------------------------------------------------------------
VELOCITY = (3.0, -2.0, 1.0)
# name: (mesh, form).  Boxes (nx, ny, nz) of the unit cube with the inner vertices moved by up to a tenth of the spacing; the
# triangle mesh is the rectangle (0, 2) x (0, 0.5) in 24 x 14, moved the same way.  The mass terms keep the solves short enough to
# qualify (a last-bit change of a dot grows tenfold every 2.5 BiCGStab iterations from entry 13 on, the faster the smaller the
# mass term) and long enough for MIN_ENTRIES: measured on the host, see test_krylov_reference_host.py.
#   box*   SPD: the CG recurrences            adv*   the same boxes with advection: BiCGStab
#   tri375 triangles with advection           lame390 the SPD 3 x 3-block operator, lame = (mu, lambda)


def _spd(mass):
    return dict(stiffness=1.7, mass=mass)


def _adv(mass, velocity=VELOCITY):
    return dict(stiffness=1.7, mass=mass, advection=velocity)


CASES = {
    "box343": ((6, 6, 6), _spd(100.0)), "box729": ((8, 8, 8), _spd(200.0)), "box1859": ((12, 12, 10), _spd(200.0)),
    "box1984": ((30, 7, 7), _spd(200.0)),
    "adv343": ((6, 6, 6), _adv(200.0)), "adv729": ((8, 8, 8), _adv(200.0)), "adv1859": ((12, 12, 10), _adv(200.0)),
    "adv1984": ((30, 7, 7), _adv(200.0)),
    "adv390": ((12, 5, 4), _adv(500.0)), "adv1176": ((27, 6, 5), _adv(500.0)),
    "tri375": ("triangles", _adv(200.0, VELOCITY[:2] + (0.0,))),
    "lame390": ((12, 5, 4), dict(lame=(1.3, 0.8), mass=200.0)),
}
ROWS = {"box343": 343, "box729": 729, "box1859": 1859, "box1984": 1984, "adv343": 343, "adv729": 729, "adv1859": 1859, "adv1984": 1984,
        "adv390": 390, "adv1176": 1176, "tri375": 375, "lame390": 1170}
SIZES = (343, 729, 1859, 1984)


def mesh_of(name):
    """(coordinates, cells) of a case: the jittered box of test_gpu_assemble_dispatch.py, or the jittered rectangle."""
    dims = CASES[name][0]
    rng = np.random.default_rng(11)
    if dims == "triangles":
        co, ce = fo.rectangle_mesh((0, 0), (2, 0.5), 24, 14)
        h = np.array([2.0 / 24, 0.5 / 14])
        inner = (co[:, 0] > 1e-12) & (co[:, 0] < 2 - 1e-12) & (co[:, 1] > 1e-12) & (co[:, 1] < 0.5 - 1e-12)
    else:
        co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), *dims)
        h = 1.0 / np.array(dims, dtype=np.float64)
        inner = np.all((co > 1e-12) & (co < 1.0 - 1e-12), axis=1)
    assert inner.any()
    return co + 0.1 * h * rng.uniform(-1.0, 1.0, co.shape) * inner[:, None], ce.astype(np.int32)


def host_operator(name):
    """The operator of a case assembled by the oracle (vertex order of mesh_of)."""
    co, ce = mesh_of(name)
    form = CASES[name][1]
    n = len(co)
    if "lame" in form:
        mu, lm = form["lame"]
        E, nu = mu * (3 * lm + 2 * mu) / (lm + mu), lm / (2 * (lm + mu))
        M = fo.assemble_matrix(n, ce, fo.p1_mass_local(co, ce, form["mass"]))
        return (fo.assemble_p1_elasticity(co, ce, E, nu) + sp.kron(M, sp.identity(3))).tocsr()
    if co.shape[1] == 2:
        Ke = fo.tri_stiffness_local(co, ce, form["stiffness"]) + fo.tri_mass_local(co, ce, form["mass"])
        if "advection" in form:
            Ke = Ke + fo.tri_advection_local(co, ce, np.array(form["advection"][:2]))
    else:
        Ke = fo.p1_stiffness_local(co, ce, form["stiffness"]) + fo.p1_mass_local(co, ce, form["mass"])
        if "advection" in form:
            Ke = Ke + fo.p1_advection_local(co, ce, np.array(form["advection"]))
    return fo.assemble_matrix(n, ce, Ke)


def rhs_of(name):
    return np.random.default_rng(3).standard_normal(ROWS[name])
