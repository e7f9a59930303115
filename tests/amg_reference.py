"""Host replay of one V-cycle of fs_amg.hip (smooth() and vcycle() there, step for step) with a componentwise forward-error bound
carried next to every vector.  Shared by test_amg_reference_host.py (the replay against an explicit dense cycle in extended
precision), amg_vcycle_worker.py (the device cycle against the replay) and test_gpu_amg_vcycle.py.  Plain numpy / scipy, no GPU.

The replay computes every sparse or dense product with extended-precision row sums rounded once (_host_product of
spmv_reference.py) and every element-wise update in extended precision rounded once, so its own error is half an ulp of each
result.  The bound e of a vector is a bound for |device - replay| in each component, to first order in eps:
  y = Op x                         e_y = |Op| e_x + t_row eps (|Op| |x|)_row, t_row the scalar terms of the row: a dot product of t
                                   terms in ANY order of summation (one thread, 16 lanes, a wave, fused or not) is within
                                   t eps / 2 of its exact value relative to the sum of the magnitudes of its terms; the other half
                                   pays for the replay's one rounding
  r = b - t, x += d, x += P xc,    e = the bounds of the inputs, each times the magnitude of its coefficient, + 2 eps (sum of the
  d = c1 d + c2 dinv r             magnitudes of the terms)
The roundings of every operation enter exactly so.  What differs from chaining the rules blindly is how the bound that a vector
ARRIVES with is carried through the smoother.  smooth() is a linear map, x <- E x + S b with E = I - S A and S a polynomial in
D^-1 A: perturbations dx, db of its inputs leave it as E dx + S db - the same dx in every place it is read - so the bounds leave as
|E| e_x + |S| e_b, entry by entry, and those of the residual behind a pre-smoothing as |I - A S| e_b.  Chaining product,
subtraction, scaling and addition instead gives (I + c |D^-1| |A|) e_x per step where the step does (I - c D^-1 A) dx - on the
diagonal 1 + c for |1 - c| - which is valid too, but grows by a factor of 3 to 4 per step whatever the operator: measured on the
hierarchies of test_gpu_amg_vcycle.py 1e-9 to 1e-8 relative to the result for three levels, 4e-7 with three steps per sweep and
1e-7 with the ten steps of a Chebyshev coarsest level, all above the tightness condition with the device two orders inside.
The moduli of the maps are narrower and as valid, so they are what the device is held to.  The roundings made INSIDE a call of
smooth() (the part g) go from step to step with the modulus of the step, |I - c2 D^-1 A| g_x + |c1| g_d for x and
|c1| g_d + c2 |D^-1| |A| g_x for d.
The constants of the smoother (theta, delta, sigma, rho) are the same IEEE double operations in the same order as in smooth(), the
inverse diagonal is 1 / diag(A_l) (1 where the diagonal is zero) as k_amg_diag_grp forms it: both carry no bound of their own."""
import numpy as np
import scipy.sparse as sp

from spmv_reference import EPS, _host_product

LD = np.longdouble
TIGHT = 1e-9                  # every case: max(e_z) <= TIGHT max|z_ref| (two orders below an accidental fp32 accumulation)


# ---- what the library decides per level (coarse_level_spmv, level_operator_to_f32, level_transfers_to_f32) ----------------------
def product_family(bs, nnz_blocks, n_nodes, node_waves=True, row_groups=True):
    """The kernel family of a level product below level 0: "node" (k_bcsr_spmv_node, a wave per node), "grp" (k_bcsr_spmv_grp, 16
    lanes per scalar row) or "row" (k_bcsr_spmv, a thread per scalar row)."""
    if node_waves and bs == 6 and n_nodes > 0 and nnz_blocks >= 4 * n_nodes:
        return "node"
    if row_groups and n_nodes > 0 and nnz_blocks >= 8 * n_nodes:
        return "grp"
    return "row"


def operator_is_fp32(bs, nnz_blocks, n_nodes, fp32=True, node_waves=True):
    """A_l (l >= 1) is streamed rounded to fp32 only where the wave-per-node product streams it."""
    return bool(fp32) and product_family(bs, nnz_blocks, n_nodes, node_waves) == "node"


def transfers_are_fp32(br, bc, fp32=True):
    """P and R = P^T are streamed rounded to fp32 for the block shapes with a templated restriction and prolongation."""
    return bool(fp32) and br in (3, 6) and bc == 6


def rounded_to_fp32(Op):
    """The operator with every value rounded to fp32 and widened again: what the kernels load."""
    Op = sp.csr_matrix(Op, copy=True)
    Op.data = Op.data.astype(np.float32).astype(np.float64)
    return Op


# ---- the replay ---------------------------------------------------------------------------------------------------------------
def _round(v):
    return np.asarray(v, dtype=np.float64)


class _Level:
    """The operators of a level as the cycle reads them, and their moduli for the bounds."""

    def __init__(self, level):
        A = sp.csr_matrix(level["A"])
        d = A.diagonal()
        self.n = A.shape[0]
        self.dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
        self.lmax = float(level["lmax"])
        self.A = rounded_to_fp32(A) if level.get("a32") else A
        self.absA = abs(self.A)
        self._moduli, self._maps = {}, {}
        self.P = self.R = None
        if level.get("P") is not None:
            P = sp.csr_matrix(level["P"])
            self.P = rounded_to_fp32(P) if level.get("p32") else P
            self.R = sp.csr_matrix(self.P.T)           # R holds the SAME rounded numbers: it stays the exact transpose
            self.absP, self.absR = abs(self.P), abs(self.R)

    def step_modulus(self, c):
        """|I - c D^-1 A|, entry by entry: what a smoother step x <- x + c D^-1 (b - A x) does to a perturbation of x."""
        if c not in self._moduli:
            self._moduli[c] = abs(sp.identity(self.n, format="csr") - sp.diags(c * self.dinv) @ self.A).tocsr()
        return self._moduli[c]


    def smoother_maps(self, steps):
        """(|E|, |S|, |I - A S|) of the `steps` steps of smooth() as the linear map they are, x <- E x + S b: polynomials in
        D^-1 A, formed as sparse matrices by the recurrence of the steps themselves."""
        if steps not in self._maps:
            scale, later = _constants(self.lmax, steps)
            I, Dinv, A = sp.identity(self.n, format="csr"), sp.diags(self.dinv), self.A
            Sd, Ed = scale * Dinv, -scale * (Dinv @ A)                   # d = Sd b + Ed x0
            Sx, Ex = Sd, I + Ed                                          # x = Sx b + Ex x0
            for c1, c2 in later:
                Sd, Ed = c1 * Sd + c2 * (Dinv @ (I - A @ Sx)), c1 * Ed - c2 * (Dinv @ (A @ Ex))
                Sx, Ex = Sx + Sd, Ex + Ed
            self._maps[steps] = (abs(sp.csr_matrix(Ex)), abs(sp.csr_matrix(Sx)), abs(sp.csr_matrix(I - A @ Sx)))
        return self._maps[steps]


def _product(Op, absOp, x, ex):
    y, ax = _host_product(Op, x)
    return y, absOp @ ex + np.diff(Op.indptr) * EPS * ax


def _sub(b, eb, t, et):
    return _round(b.astype(LD) - t.astype(LD)), eb + et + 2.0 * EPS * (np.abs(b) + np.abs(t))


def _add(x, ex, d, ed):
    return _round(x.astype(LD) + d.astype(LD)), ex + ed + 2.0 * EPS * (np.abs(x) + np.abs(d))


def _constants(lmax, steps):
    """(scale of the first step, [(c1, c2) of the later steps]): the IEEE double operations of smooth(), in its order."""
    up, lo = 1.1 * lmax, 0.1 * lmax
    theta, delta = 0.5 * (up + lo), 0.5 * (up - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    later = []
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        later.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return 1.0 / theta, later


def _smooth(L, x, ex, b, eb, zero_guess, steps):
    """smooth(): `steps` Chebyshev steps with Jacobi on [0.1, 1.1] lmax; x is None for a zero guess.  Returns x, its bound
    |E| e_x + |S| e_b + g and g alone, the part that the roundings of these steps leave in x (see the module's header)."""
    scale, later = _constants(L.lmax, steps)
    zero = np.zeros(L.n)
    # k_cheb_first: d = scale dinv r; x = (x +) d.  l*: the roundings of one operation; gd, gx: what all of them so far leave in d, x
    if zero_guess:
        term = LD(scale) * L.dinv.astype(LD) * b.astype(LD)
        d = _round(term)
        gd = 2.0 * EPS * np.abs(d)
        x, gx = d.copy(), gd.copy()
    else:
        t, lt = _product(L.A, L.absA, x, zero)
        r, lr = _sub(b, zero, t, lt)
        term = LD(scale) * L.dinv.astype(LD) * r.astype(LD)
        d = _round(term)
        ld = 2.0 * EPS * np.abs(d)
        x, lx = _add(x, zero, d, zero)
        gd = np.abs(scale * L.dinv) * lr + ld
        gx = gd + lx
    for c1, c2 in later:
        t, lt = _product(L.A, L.absA, x, zero)
        r, lr = _sub(b, zero, t, lt)
        # k_cheb_next: d = c1 d + c2 dinv r; x += d
        t1, t2 = LD(c1) * d.astype(LD), LD(c2) * L.dinv.astype(LD) * r.astype(LD)
        ld = 2.0 * EPS * (np.abs(_round(t1)) + np.abs(_round(t2)))
        d = _round(t1 + t2)
        x, lx = _add(x, zero, d, zero)
        gx, gd = (L.step_modulus(c2) @ gx + abs(c1) * gd + np.abs(c2 * L.dinv) * lr + ld + lx,
                  abs(c1) * gd + np.abs(c2 * L.dinv) * (lr + L.absA @ gx) + ld)
    absE, absS, _ = L.smoother_maps(steps)
    e = gx + absS @ eb
    if not zero_guess:
        e = e + absE @ ex
    return x, e, gx


def _vcycle(lv, l, b, eb, steps, coarse):
    L = lv[l]
    last = len(lv) - 1
    if l == last:
        if coarse is not None and l > 0:                # k_dense_apply: a row of n terms
            y = _round(coarse[0] @ b.astype(LD))
            return y, coarse[1] @ eb + L.n * EPS * (coarse[1] @ np.abs(b))
        x, ex, _ = _smooth(L, None, None, b, eb, True, steps)
        for _ in range(4 if l > 0 else 0):
            x, ex, _ = _smooth(L, x, ex, b, eb, False, steps)
        return x, ex
    x, ex, gx = _smooth(L, None, None, b, eb, True, steps)
    # r = b - A x with x = S b + (roundings): a perturbation db of b leaves as (I - A S) db
    t, lt = _product(L.A, L.absA, x, np.zeros(L.n))
    r, lr = _sub(b, np.zeros(L.n), t, lt)
    er = L.smoother_maps(steps)[2] @ eb + L.absA @ gx + lr
    bc, ebc = _product(L.R, L.absR, r, er)
    xc, exc = _vcycle(lv, l + 1, bc, ebc, steps, coarse)
    px, epx = _product(L.P, L.absP, xc, exc)
    x, ex = _add(x, ex, px, epx)
    x, ex, _ = _smooth(L, x, ex, b, eb, False, steps)
    return x, ex


def prepare(levels):
    """The levels in the form the replay works on (built once per hierarchy, reused for every right-hand side)."""
    return [L if isinstance(L, _Level) else _Level(L) for L in levels]


def vcycle_replay(levels, r, smoother_steps=2, coarse=None, e_r=None):
    """z = M r and the bound e_z of |z_device - z|.  e_r: the bound that r itself arrives with where the device's right-hand side is
    the result of earlier kernels (None: the device reads the same r, bit for bit).  levels[l]: {"A": A_l, "P": prolongator from level l + 1 (None on the last
    level), "lmax": lambda_max, "a32" / "p32": the level operator / the transfers are streamed rounded to fp32}, fp64 scipy
    matrices as AMG.level_matrix returns them, or the output of prepare().  coarse: the dense inverse applied on the last level
    (AMG.coarse_inverse()), None = Chebyshev sweeps there."""
    lv = prepare(levels)
    r = np.asarray(r, dtype=np.float64)
    if coarse is not None:
        c = np.asarray(coarse, dtype=np.float64)
        coarse = (c.astype(LD), np.abs(c))
    return _vcycle(lv, 0, r, np.zeros(len(r)) if e_r is None else np.asarray(e_r, dtype=np.float64), int(smoother_steps), coarse)


def check_cycle(z, z_ref, e_z, what):
    """The device result finite and within the bound in every component; returns (largest err / e_z, max(e_z) / max|z_ref|), the
    second of which the caller holds to TIGHT."""
    assert np.all(np.isfinite(z)), (what, "non-finite entries", np.flatnonzero(~np.isfinite(z))[:8], int((~np.isfinite(z)).sum()))
    err = np.abs(z - z_ref)
    ratio = float((err / np.maximum(e_z, 1e-300)).max())
    tight = float(e_z.max() / np.abs(z_ref).max())
    bad = err > e_z
    assert not bad.any(), (what, "outside the bound", int(bad.sum()), np.flatnonzero(bad)[:8], ratio)
    return ratio, tight


# ---- the eigenvalue bound of a level ------------------------------------------------------------------------------------------------
def gershgorin_bound(A):
    """max_i (|d_i| + sum_{j != i} |a_ij|) / |d_i| over the rows with a diagonal entry: k_amg_diag_grp's bound of D^-1 A."""
    A = sp.csr_matrix(A)
    d = np.abs(A.diagonal())
    off = np.asarray(abs(A).sum(axis=1)).ravel() - d
    return float(((d[d > 0] + off[d > 0]) / d[d > 0]).max())


def largest_jacobi_eigenvalue(A):
    """The largest eigenvalue of D^-1 A (of D^-1/2 A D^-1/2, the same spectrum) of a level operator, D = 1 where A has no diagonal."""
    from scipy.sparse.linalg import eigsh
    A = sp.csr_matrix(A)
    d = A.diagonal()
    s = sp.diags(1.0 / np.sqrt(np.abs(np.where(d != 0.0, d, 1.0))))
    S = (s @ (0.5 * (A + A.T)) @ s).tocsr()
    if S.shape[0] <= 600:
        return float(np.linalg.eigvalsh(S.toarray())[-1])
    return float(eigsh(S, k=1, which="LA", tol=1e-13, v0=np.ones(S.shape[0]))[0][0])
