"""Host replay of the AMG set-up of fs_amg.hip (coarsen() and estimate_lmax() there, stage by stage).  Shared by
test_amg_setup_reference_host.py (the replay against the properties that define the method, in float64, in np.longdouble and with
every sum reversed), amg_setup_worker.py (the device's hierarchy against the replay, level by level) and test_gpu_amg_setup.py.
Plain numpy, no GPU; scipy only multiplies 0/1 patterns (integers) and never touches a value.

Given the strength graph, the set-up is an integer algorithm - MIS(2) with hashed keys, two aggregation passes, the symbolic
patterns of A T and P^T (A P) - plus a few short floating-point stages: the block diagonal, the per-aggregate Gram-Schmidt QR, the
power iteration and the prolongator smoothing.  The integer stages are replayed exactly; the floating-point ones in a STATED order
of summation: every sum runs over its terms in the order of the block row (of the members of the aggregate, of the products of an
output block), first to last, or last to first with reverse=True.  The device sums the same terms in other orders (16 lanes and a
butterfly, a wave, copies per lane group), so it agrees to rounding, not bit for bit.

The floating-point comparisons that DECIDE something are few - the strength test f > theta^2 dnorm_i dnorm_j, the pass-2 test
sw > best (1 + 1e-6) and the test nrm > 1e-16 orig of the QR - and the replay reports how far each was from flipping
(`margins`).  A decision is ambiguous if a relative change of AMBIGUOUS = 1e-9 of a compared quantity flips it (for the QR: if
nrm / orig lies in [1e-20, 1e-12]); every case of the tests has none, so that the integer stages compare exactly, without a list of
exceptions.  Exact ties of the pass-2 test (equal weights on uniform meshes) sit 1e-6 from flipping: the smaller index keeps it.

dtype: np.float64 or np.longdouble, the type every floating-point stage computes in (the inputs are float64 either way)."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -52
AMBIGUOUS = 1e-9
LIVE_BAND = (1e-20, 1e-12)
QR_C = 8.0                    # the constant of the QR tolerance (see qr_tolerance and the header of test_gpu_amg_setup.py)
LMAX_SPREAD = 4e-15           # relative; the largest the host test measures between two orders of summation stays below it (see there)
U64 = np.uint64


# ---- the library's hash and keys ------------------------------------------------------------------------------------------------
def amg_hash(x):
    x = np.asarray(x, dtype=U64) & U64(0xffffffff)
    x ^= x >> U64(16)
    x = (x * U64(0x7feb352d)) & U64(0xffffffff)
    x ^= x >> U64(15)
    x = (x * U64(0x846ca68b)) & U64(0xffffffff)
    x ^= x >> U64(16)
    return x


def default_theta(option):
    """fs_amg_setup: 0 = 0.05, anything else max(option, 1e-8)."""
    return 0.05 if option == 0.0 else max(float(option), 1e-8)


# ---- a near-null space with nearly dependent columns (a case of the tests) --------------------------------------------------------
FAR = 100.0


def far_rigid_body_modes(co, far=FAR):
    """The six rigid-body modes with the rotations about a point `far` box widths away and scaled by 1 / far, [6, 3 n_nodes]: over
    an aggregate such a rotation is a translation up to (radius of the aggregate / far)^2 of its norm - columns that are nearly
    dependent and still live (nrm / orig between the 1e-16 of the QR and 1e-6)."""
    x, y, z = (co + far).T / far
    raw = np.zeros((6, len(co), 3))
    raw[0, :, 0] = raw[1, :, 1] = raw[2, :, 2] = 1.0
    raw[3, :, 0], raw[3, :, 1] = -y, x
    raw[4, :, 0], raw[4, :, 2] = z, -x
    raw[5, :, 2], raw[5, :, 1] = y, -z
    return raw.reshape(6, -1)


# ---- sums in a stated order -----------------------------------------------------------------------------------------------------
def _seq(terms, reverse=False):
    """The sum of a vector of terms, first to last (last to first with reverse): cumsum adds one term after the other."""
    terms = np.asarray(terms)
    if terms.size == 0:
        return terms.dtype.type(0)
    return np.cumsum(terms[::-1] if reverse else terms)[-1]


def _row_sums(terms, rowptr, reverse=False):
    """out[i] = terms[rowptr[i]] + ... + terms[rowptr[i + 1] - 1] in that order (reversed with reverse); terms may carry further axes."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    out = np.zeros((n,) + terms.shape[1:], dtype=terms.dtype)
    length = np.diff(rowptr)
    for k in range(int(length.max()) if n else 0):
        rows = np.flatnonzero(length > k)
        out[rows] += terms[(rowptr[rows + 1] - 1 - k) if reverse else (rowptr[rows] + k)]
    return out


def _rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _accumulate(n_out, slot, terms, reverse=False):
    """out[slot[t]] += terms[t], t in order (np.add.at is unbuffered: one addition after the other), or from the last t to the first."""
    out = np.zeros((n_out,) + terms.shape[1:], dtype=terms.dtype)
    if reverse:
        slot, terms = slot[::-1], terms[::-1]
    np.add.at(out, slot, terms)
    return out


def block_product(lptr, lcol, lval, rptr, rcol, rval, n_cols, reverse=False):
    """C = L R of two block CSR matrices as the row-wise SpGEMM forms it: the pattern of a row is the sorted set of the columns its
    products reach (structural zeros kept), a block the sum of its products in the order (entry of the left row, entry of the right
    row)."""
    lptr, rptr = np.asarray(lptr, dtype=np.int64), np.asarray(rptr, dtype=np.int64)
    n_out = len(lptr) - 1
    lrow = _rows_of(lptr)
    cnt = (rptr[1:] - rptr[:-1])[lcol]
    q = np.repeat(np.arange(len(lcol)), cnt)                                   # left entry of every product
    start = np.cumsum(cnt) - cnt
    p = rptr[lcol][q] + (np.arange(len(q)) - start[q])                         # right entry
    key = lrow[q] * np.int64(n_cols) + rcol[p]
    uniq, slot = np.unique(key, return_inverse=True)
    crow, ccol = uniq // n_cols, uniq % n_cols
    cptr = np.zeros(n_out + 1, dtype=np.int64)
    np.add.at(cptr, crow + 1, 1)
    cptr = np.cumsum(cptr)
    cval = _accumulate(len(uniq), slot.ravel(), np.matmul(lval[q], rval[p]), reverse)
    return cptr.astype(np.int32), ccol.astype(np.int32), cval


def block_transpose(rowptr, col, val, n_cols):
    """The transpose as build_p_transpose orders it: entries sorted by column, stable (ascending row inside a column)."""
    order = np.argsort(col, kind="stable")
    ptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.add.at(ptr, np.asarray(col, dtype=np.int64) + 1, 1)
    return np.cumsum(ptr).astype(np.int32), _rows_of(rowptr)[order].astype(np.int32), np.swapaxes(val[order], 1, 2).copy()


def blocks_from_csr(K, bs):
    """(rowptr, col, val[nnz, bs, bs]) of a scipy matrix, columns ascending."""
    M = sp.bsr_matrix(sp.csr_matrix(K), blocksize=(bs, bs))
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), np.array(M.data, dtype=np.float64)


def blocks_to_csr(rowptr, col, val, n_cols):
    val = np.asarray(val, dtype=np.float64)
    return sp.bsr_matrix((val, col, rowptr), shape=((len(rowptr) - 1) * val.shape[1], n_cols * val.shape[2])).tocsr()


def columns_strictly_ascending(rowptr, col):
    col = np.asarray(col, dtype=np.int64)
    inner = np.ones(len(col), dtype=bool)
    inner[np.asarray(rowptr[:-1], dtype=np.int64)[np.diff(rowptr) > 0]] = False       # first entry of a row: nothing before it
    return bool(np.all(col[1:][inner[1:]] > col[:-1][inner[1:]]))


# ---- the stages -----------------------------------------------------------------------------------------------------------------
def diagonal(rp, ci, val, reverse=False):
    """k_amg_diag_grp: dinv = 1/d (1 where d == 0), ident iff the off-diagonal absolute row sum is 0, dnorm = ||A_ii||_F,
    gersh = max (|d| + off) / |d| over the rows with d != 0 (2.0 if that is not positive)."""
    nn, bs = len(rp) - 1, val.shape[1]
    row = _rows_of(rp)
    isd = ci == row
    offv = np.abs(val)
    offv[isd] *= (1.0 - np.eye(bs)).astype(val.dtype)
    off = _row_sums(_inner(offv, reverse), rp, reverse)                               # [nn, bs]: the columns of a block, then the blocks
    d = np.zeros((nn, bs), dtype=val.dtype)
    d[row[isd]] = np.einsum("eii->ei", val[isd])
    dn = np.zeros(nn, dtype=val.dtype)
    dn[row[isd]] = np.sqrt(_seq_blocks(val[isd] * val[isd], reverse))
    nz = d != 0
    dinv = np.where(nz, 1.0 / np.where(nz, d, 1), 1).astype(val.dtype)
    ratio = np.where(nz, (np.abs(d) + off) / np.where(nz, np.abs(d), 1), 0)
    gersh = ratio.max() if ratio.size else 0.0
    if not gersh > 0:
        gersh = val.dtype.type(2.0)
    return dinv.reshape(-1), (off == 0).reshape(-1), dn, gersh, off.reshape(-1)


def _inner(x, reverse=False, axis=2):
    """Sum over an axis of a small array (the columns of a block, then its rows), one term after the other."""
    idx = range(x.shape[axis])
    out = np.zeros(np.delete(x.shape, axis), dtype=x.dtype)
    for k in (reversed(idx) if reverse else idx):
        out = out + np.take(x, k, axis=axis)
    return out


def strength(rp, ci, val, dnorm, theta, reverse=False):
    """k_strength_grp: (sptr, scol, sw, margin) - j != i strong iff f = ||A_ij||_F^2 > 0 and f > theta^2 dnorm_i dnorm_j, the
    strong entries in the order of the block row, sw = f.  margin: the smallest |f / threshold - 1| over the off-diagonal blocks with
    f > 0 (None without one), coupled: nodes with an off-diagonal block of f > 0."""
    row = _rows_of(rp)
    t = val.dtype.type
    f = _seq_blocks(val * val, reverse)
    theta2 = t(theta) * t(theta)
    thr = theta2 * dnorm[row] * dnorm[ci]
    off = (ci != row) & (f > 0)
    strong = off & (f > thr)
    rel = np.abs(f[off] / np.where(thr[off] > 0, thr[off], t(1e-300)) - 1)
    cnt = np.zeros(len(rp), dtype=np.int64)
    np.add.at(cnt, row[strong] + 1, 1)
    coupled = np.zeros(len(rp) - 1, dtype=bool)
    coupled[row[off]] = True
    return (np.cumsum(cnt).astype(np.int32), ci[strong].astype(np.int32), f[strong], float(rel.min()) if rel.size else None, coupled)


def _seq_blocks(x, reverse=False):
    """The entries of every block summed in row-major order."""
    flat = x.reshape(x.shape[0], -1)
    out = np.zeros(x.shape[0], dtype=x.dtype)
    idx = range(flat.shape[1])
    for k in (reversed(idx) if reverse else idx):
        out = out + flat[:, k]
    return out


def mis2(sptr, scol):
    """k_mis_init / _max / _update: (root flags, rounds).  key = state << 62 | (hash(i) & 0x3fffffff) << 32 | i, state 2 root,
    1 undecided, 0 out; a round is two max-propagations over the strong couplings and the update."""
    nn = len(sptr) - 1
    i = np.arange(nn, dtype=U64)
    srow = _rows_of(sptr)
    state = (np.diff(sptr) > 0).astype(U64)
    key = (state << U64(62)) | ((amg_hash(i) & U64(0x3fffffff)) << U64(32)) | i
    low, clear = U64(0xffffffff), ~(U64(3) << U64(62))
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= 200, "MIS(2) did not terminate"
        m1 = key.copy()
        np.maximum.at(m1, srow, key[scol])
        m2 = m1.copy()
        np.maximum.at(m2, srow, m1[scol])
        und = (key >> U64(62)) == U64(1)
        root = und & ((m2 & low) == i)
        out = und & ~root & ((m2 >> U64(62)) == U64(2))
        key[root] = (key[root] & clear) | (U64(2) << U64(62))
        key[out] = key[out] & clear
        if not (und & ~root & ~out).any():
            break
    return (key >> U64(62)) == U64(2), rounds


def aggregate(sptr, scol, sw, root):
    """k_agg_rootflag, the scan, k_agg_pass1 / _pass2: (agg, n_agg, figures).  Pass 1: a root, or the first root among the strong
    neighbours; pass 2: over the aggregated strong neighbours in row order, the one with sw > best (1 + 1e-6)."""
    nn = len(sptr) - 1
    rootid = np.cumsum(root) - root
    n_agg = int(root.sum())
    agg1 = np.full(nn, -1, dtype=np.int64)
    for i in range(nn):
        if root[i]:
            agg1[i] = rootid[i]
        else:
            for e in range(sptr[i], sptr[i + 1]):
                if root[scol[e]]:
                    agg1[i] = rootid[scol[e]]
                    break
    agg = agg1.copy()
    margin, pass2, ties = None, 0, 0
    factor = sw.dtype.type(1.0) + sw.dtype.type(1e-6)
    for i in np.flatnonzero(agg1 < 0):
        best, a = sw.dtype.type(-1.0), -1
        for e in range(sptr[i], sptr[i + 1]):
            aj = agg1[scol[e]]
            if aj < 0:
                continue
            if best > 0:
                m = abs(float(sw[e] / (best * factor)) - 1.0)
                margin = m if margin is None else min(margin, m)
                if sw[e] == best and aj != a:
                    ties += 1
            if sw[e] > best * factor:
                best, a = sw[e], aj
        agg[i] = a
        pass2 += a >= 0
    return agg.astype(np.int32), n_agg, {"pass2_margin": margin, "pass2_nodes": int(pass2), "ties_by_index": int(ties)}


def tentative(agg, n_agg, bs, nb, B, ident, dtype=np.float64, reverse=False):
    """k_tentative: per aggregate (members in ascending node order, rows with ident zeroed) column-by-column modified Gram-Schmidt.
    Returns T [n, nb], R [n_agg, nb, nb] (= B of the next level), live [n_agg, nb], the ratios nrm / orig of every column with
    orig > 0, and per aggregate (rows, condition of the live columns, max|B_a|)."""
    n = len(agg) * bs
    T = np.zeros((n, nb), dtype=dtype)
    R = np.zeros((n_agg, nb, nb), dtype=dtype)
    live = np.zeros((n_agg, nb), dtype=bool)
    ratios, rows_a, kappa, bmax = [], np.zeros(n_agg, dtype=np.int64), np.ones(n_agg), np.zeros(n_agg)
    order = np.argsort(np.where(agg >= 0, agg, n_agg), kind="stable")
    bounds = np.searchsorted(np.where(agg >= 0, agg, n_agg)[order], np.arange(n_agg + 1))
    B = np.asarray(B, dtype=np.float64).reshape(n, nb)
    for a in range(n_agg):
        nodes = order[bounds[a]:bounds[a + 1]]
        rows = (nodes[:, None] * bs + np.arange(bs)).ravel()
        Q = np.where(ident[rows][:, None], 0.0, B[rows]).astype(dtype)
        Q0 = np.array(Q, dtype=np.float64)
        for c in range(nb):
            orig = _seq(Q[:, c] * Q[:, c], reverse)
            for k in range(c):
                dot = _seq(Q[:, k] * Q[:, c], reverse)
                R[a, k, c] = dot
                Q[:, c] = Q[:, c] - dot * Q[:, k]
            nrm = _seq(Q[:, c] * Q[:, c], reverse)
            if orig > 0:
                ratios.append(float(nrm / orig))
            ok = bool(nrm > dtype(1e-16) * orig and nrm > 0)
            live[a, c] = ok
            nrm = np.sqrt(nrm)
            R[a, c, c] = nrm if ok else 0
            if not ok:
                R[a, :c, c] = 0
            Q[:, c] = Q[:, c] * ((dtype(1.0) / nrm) if ok else dtype(0.0))
        T[rows] = Q
        rows_a[a], bmax[a] = len(rows), np.abs(Q0).max() if len(rows) else 0.0
        if live[a].any():
            s = np.linalg.svd(Q0[:, live[a]], compute_uv=False)
            kappa[a] = s[0] / s[-1]
    return T, R, live, np.array(ratios), (rows_a, kappa, bmax)


def qr_tolerance(rows, kappa, bmax, c=QR_C):
    """|R_device - R| <= c eps m kappa_a max|B_a| per aggregate: two runs of modified Gram-Schmidt on m rows that differ in the order
    of their sums differ by a small multiple of m eps in every product, amplified by the condition of the (live) columns."""
    return c * EPS * rows * kappa * bmax


def power_iteration(rp, ci, val, dinv, gersh, eig_steps, fp32=False, dtype=np.float64, reverse=False):
    """estimate_lmax: (lambda_max, lam, bound).  v seeded from the hash, v <- dinv (A v) eig_steps - 1 times,
    lam = (v, A v) / (v, v / dinv), lambda_max = min(1.1 lam, gersh) or gersh if lam is not positive and finite.  fp32: the products
    read the values rounded to fp32.  bound: of |lambda_max_device - lambda_max| to first order, carried through the recurrence -
    a row sum of t terms in any order is within t eps of the replay's relative to the sum of the magnitudes of its terms, an
    element-wise product within 2 eps."""
    nn, bs = len(rp) - 1, val.shape[1]
    n = nn * bs
    vals = (val.astype(np.float32).astype(np.float64) if fp32 else np.asarray(val, dtype=np.float64)).astype(dtype)
    absv = np.abs(np.asarray(vals, dtype=np.float64))
    t_row = np.repeat(np.diff(rp) * bs, bs).astype(np.float64)

    def product(x, scalar_vals):
        terms = scalar_vals * x.reshape(nn, bs)[ci][:, None, :]                 # [nnz, bs(r), bs(c)]
        return _row_sums(_inner(terms, reverse), rp, reverse).reshape(-1)

    i = np.arange(n, dtype=U64)
    seed = (amg_hash((i * U64(2654435761) + U64(12345)) & U64(0xffffffff)) & U64(0xffffff)).astype(np.float64) / 8388608.0 - 1.0
    v = seed.astype(dtype)
    e = np.zeros(n)
    growth = float(gersh) if gersh > 1.0 else 1.0
    safe = int(eig_steps)
    while safe > 1 and safe * np.log10(growth) > 250.0:
        safe -= 1
    adinv = np.abs(np.asarray(dinv, dtype=np.float64))
    for _ in range(safe - 1):
        w = product(v, vals)
        ew = product(e, absv) + t_row * EPS * product(np.abs(np.asarray(v, dtype=np.float64)), absv)
        v = w * (dtype(1.0) * dinv.astype(dtype))
        e = adinv * ew + 2.0 * EPS * np.abs(np.asarray(v, dtype=np.float64))
    w = product(v, vals)
    av, aw = np.abs(np.asarray(v, dtype=np.float64)), np.abs(np.asarray(w, dtype=np.float64))
    ew = product(e, absv) + t_row * EPS * product(av, absv)
    num = _seq(v * w, reverse)
    e_num = float((av * ew + e * aw).sum() + (n + 2) * EPS * (av * aw).sum())
    w2 = v / dinv.astype(dtype)
    den = _seq(v * w2, reverse)
    aw2 = av / adinv
    e_den = float((2.0 * e * aw2).sum() + (n + 4) * EPS * (av * aw2).sum())
    lam = num / den if den > 0 else dtype(0.0)
    if lam > 0 and np.isfinite(lam) and lam < 1e300:
        lmax = min(dtype(1.1) * lam, dtype(gersh))
        e_lam = 1.1 * float(lam) * (e_num / abs(float(num)) + e_den / float(den) + 3.0 * EPS)
    else:
        lmax, e_lam = dtype(gersh), 0.0
    e_gersh = (int(np.diff(rp).max()) * bs + 3) * EPS * float(gersh)
    return lmax, lam, max(e_lam, e_gersh)


def smooth_prolongator(rp, ci, val, dinv, agg, n_agg, T, lmax, reverse=False):
    """The SpGEMM A T and k_smooth_p_grp: P = T - omega dinv (A T) on the symbolic pattern of A T (columns ascending, structural
    zeros kept), omega = 4 / (3 lambda_max).  Returns (prow, pcol, pval, tptr, tcol, tval, omega)."""
    nn, bs = len(rp) - 1, val.shape[1]
    nb = T.shape[1]
    has = agg >= 0
    tptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    tcol = agg[has].astype(np.int32)
    tval = T.reshape(nn, bs, nb)[has]
    pptr, pcol, at = block_product(rp, ci, val.astype(T.dtype), tptr, tcol, tval, n_agg, reverse)
    omega = T.dtype.type(4.0) / (T.dtype.type(3.0) * T.dtype.type(lmax))
    prow = _rows_of(pptr)
    pval = (-omega * dinv.astype(T.dtype).reshape(nn, bs)[prow])[:, :, None] * at
    own = pcol == agg[prow]
    pval[own] = pval[own] + T.reshape(nn, bs, nb)[prow[own]]
    return pptr, pcol, pval, tptr, tcol, tval, omega


def prolongator_bound(rp, ci, val, dinv, agg, n_agg, T, e_T_of_aggregate, lmax):
    """|P_device - P| <= (I + omega |dinv| |A|) e_T + (k + 3) eps (|T| + omega |dinv| |A| |T|) on the pattern of P, k the scalar
    terms of the longest block row of A, e_T the bound of the tentative prolongator (per aggregate, every entry of its blocks)."""
    nn, bs = len(rp) - 1, val.shape[1]
    nb = T.shape[1]
    has = agg >= 0
    tptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    tcol = agg[has].astype(np.int32)
    absT = np.abs(np.asarray(T, dtype=np.float64)).reshape(nn, bs, nb)
    eT = np.broadcast_to(np.asarray(e_T_of_aggregate, dtype=np.float64)[np.where(has, agg, 0)][:, None, None], absT.shape) * has[:, None, None]
    absA = np.abs(np.asarray(val, dtype=np.float64))
    pptr, pcol, a_abs_t = block_product(rp, ci, absA, tptr, tcol, absT[has], n_agg)
    _, _, a_e_t = block_product(rp, ci, absA, tptr, tcol, eT[has], n_agg)
    omega = 4.0 / (3.0 * float(lmax))
    prow = _rows_of(pptr)
    scale = (omega * np.abs(np.asarray(dinv, dtype=np.float64)).reshape(nn, bs)[prow])[:, :, None]
    own = pcol == agg[prow]
    k = int(np.diff(rp).max()) * bs
    bound = scale * a_e_t + (k + 3) * EPS * scale * a_abs_t
    bound[own] += eT[prow[own]] + (k + 3) * EPS * absT[prow[own]]
    return bound


def galerkin(rp, ci, val, pptr, pcol, pval, n_agg, reverse=False):
    """A_c = P^T (A P) by the two row-wise products, then k_fix_dead: a diagonal entry that is exactly 0.0 becomes 1.0.  Returns
    (rowptr, col, val, dead dofs)."""
    aptr, acol, aval = block_product(rp, ci, val.astype(pval.dtype), pptr, pcol, pval, n_agg, reverse)
    tptr, tcol, tval = block_transpose(pptr, pcol, pval, n_agg)
    cptr, ccol, cval = block_product(tptr, tcol, tval, aptr, acol, aval, n_agg, reverse)
    dead = []
    crow = _rows_of(cptr)
    for e in np.flatnonzero(ccol == crow):
        for r in range(cval.shape[1]):
            if cval[e, r, r] == 0.0:
                cval[e, r, r] = 1.0
                dead.append(int(crow[e]) * cval.shape[1] + r)
    return cptr, ccol, cval, np.array(sorted(dead), dtype=np.int64)


def coarse_pattern(rp, ci, pptr, pcol, n_agg):
    """The symbolic pattern of P^T (A P) alone (0/1 integer products)."""
    nn = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci), dtype=np.int64), ci, rp), shape=(nn, nn))
    P = sp.csr_matrix((np.ones(len(pcol), dtype=np.int64), pcol, pptr), shape=(nn, n_agg))
    C = (P.T @ (A @ P)).tocsr()
    C.sort_indices()
    return C.indptr.astype(np.int32), C.indices.astype(np.int32)


# ---- one coarsening step, and the whole set-up -----------------------------------------------------------------------------------
def coarsen_step(rp, ci, val, B, theta, nb, eig_steps=15, fp32=False, lmax=None, dtype=np.float64, reverse=False, want_coarse=True):
    """coarsen() of a level that is not the last by the level rules: every intermediate in a dict.  out["stop"] names the rule that
    ends the hierarchy here (None: a coarser level follows).  lmax: the lambda_max the prolongator is smoothed with (None: the
    replay's own) - the device test passes the library's, so that an error of one stage does not blur the next."""
    rp, ci = np.asarray(rp, dtype=np.int32), np.asarray(ci, dtype=np.int32)
    val64 = np.asarray(val, dtype=np.float64)
    v = val64.astype(dtype)
    nn, bs = len(rp) - 1, v.shape[1]
    out = {"nn": nn, "bs": bs, "nb": nb, "stop": None}
    dinv, ident, dnorm, gersh, off = diagonal(rp, ci, v, reverse)
    out.update(dinv=dinv, ident=ident, dnorm=dnorm, gersh=gersh)
    out["lmax"], out["lam"], out["lmax_bound"] = power_iteration(rp, ci, val64, dinv, gersh, eig_steps, fp32, dtype, reverse)
    sptr, scol, sw, s_margin, coupled = strength(rp, ci, v, dnorm, theta, reverse)
    out.update(sptr=sptr, scol=scol, sw=sw, coupled_not_strong=int((coupled & (np.diff(sptr) == 0)).sum()))
    out["margins"] = margins = {"strength": s_margin, "pass2": None, "live_ratios": np.zeros(0)}
    out["nearly_dead"] = 0
    if len(scol) == 0:
        out["stop"] = "no strong coupling"
        return _judge(out)
    root, rounds = mis2(sptr, scol)
    agg, n_agg, fig = aggregate(sptr, scol, sw, root)
    out.update(root=root, mis_rounds=rounds, agg=agg, n_agg=n_agg, **fig)
    margins["pass2"] = fig["pass2_margin"]
    if n_agg == 0 or n_agg * nb >= nn * bs:
        out["stop"] = "no reduction"
        return _judge(out)
    T, R, live, ratios, per_agg = tentative(agg, n_agg, bs, nb, B, ident, dtype, reverse)
    margins["live_ratios"] = ratios
    out["nearly_dead"] = int(((ratios > LIVE_BAND[1]) & (ratios < 1e-6)).sum())       # live, and dead with a threshold of 1e-6
    out.update(T=T, R=R, live=live, agg_rows=per_agg[0], agg_kappa=per_agg[1], agg_bmax=per_agg[2])
    use = out["lmax"] if lmax is None else lmax
    pptr, pcol, pval, tptr, tcol, tval, omega = smooth_prolongator(rp, ci, v, dinv, agg, n_agg, T, use, reverse)
    out.update(pptr=pptr, pcol=pcol, pval=pval, omega=omega, lmax_used=use)
    out["dead"] = np.flatnonzero(~live.reshape(-1))
    if want_coarse:
        cptr, ccol, cval, dead = galerkin(rp, ci, v, pptr, pcol, pval, n_agg, reverse)
        out.update(cptr=cptr, ccol=ccol, cval=cval, dead_by_value=dead)
    else:
        out["cptr"], out["ccol"] = coarse_pattern(rp, ci, pptr, pcol, n_agg)
    return _judge(out)


def _judge(out):
    m = out["margins"]
    r = m["live_ratios"]
    out["ambiguous"] = {"strength": m["strength"] is not None and m["strength"] < AMBIGUOUS,
                        "pass2": m["pass2"] is not None and m["pass2"] < AMBIGUOUS,
                        "live": int(((r >= LIVE_BAND[0]) & (r <= LIVE_BAND[1])).sum())}
    out["n_ambiguous"] = int(out["ambiguous"]["strength"]) + int(out["ambiguous"]["pass2"]) + out["ambiguous"]["live"]
    return out


def is_last_level(n_levels_so_far, n_rows, max_levels=0, coarse_size=0):
    """fs_amg_setup: a level is the last when the hierarchy has max_levels (default 10) or the level at most coarse_size (default
    500) rows."""
    return n_levels_so_far >= (max_levels if max_levels > 0 else 10) or n_rows <= (coarse_size if coarse_size > 0 else 500)


def has_dense_inverse(n_levels, n_rows_last):
    return n_levels > 1 and n_rows_last <= 2500


def setup_replay(rp, ci, val, B, nb, strength_threshold=0.0, max_levels=0, coarse_size=0, eig_steps=0, fp32_of_level=None,
                 dtype=np.float64, reverse=False):
    """The whole of fs_amg_setup on the host: a list of levels {"rp", "ci", "val", "B", "bs", "step": coarsen_step() or None on the
    last level, "lmax", "stop"} and whether the last level gets a dense inverse.  fp32_of_level(level, bs, nnz, nn): whether the
    power iteration of a level >= 1 reads fp32 values."""
    theta = default_theta(strength_threshold)
    steps = eig_steps if eig_steps > 0 else 15
    levels = []
    B = np.asarray(B, dtype=np.float64)
    while True:
        bs = val.shape[1]
        nn = len(rp) - 1
        lev = {"rp": rp, "ci": ci, "val": val, "B": B, "bs": bs, "nn": nn, "step": None, "stop": None}
        levels.append(lev)
        l = len(levels) - 1
        fp32 = bool(l > 0 and fp32_of_level is not None and fp32_of_level(l, bs, len(ci), nn))
        if is_last_level(len(levels), nn * bs, max_levels, coarse_size):
            dinv, _, _, gersh, _ = diagonal(rp, ci, val.astype(dtype), reverse)
            lev["lmax"], lev["lam"], lev["lmax_bound"] = power_iteration(rp, ci, val, dinv, gersh, steps, fp32, dtype, reverse)
            lev["stop"] = "level rule"
            break
        step = coarsen_step(rp, ci, val, B, theta, nb, steps, fp32, None, dtype, reverse)
        lev.update(step=step, lmax=step["lmax"], lam=step["lam"], lmax_bound=step["lmax_bound"])
        if step["stop"] is not None:
            lev["stop"] = step["stop"]
            break
        rp, ci, val = step["cptr"], step["ccol"], np.asarray(step["cval"], dtype=np.float64)
        B = np.asarray(step["R"], dtype=np.float64).reshape(-1, nb)
    return levels, has_dense_inverse(len(levels), levels[-1]["nn"] * levels[-1]["bs"])
