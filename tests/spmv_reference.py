"""Shared by test_gpu_tails.py and stream_variants_worker.py: the extended-precision host product with the bound every sparse
product is held to (4 eps |A| |x| per row), and the block-cache poisoning that puts chosen bits behind the end of a vector."""
import math
import os

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
K_BLOCKS = 16                        # poisoned blocks per length: more than the vectors of a solve's workspace


def _fill(v, m, pattern, rng):
    if pattern == "zero":
        v.fill(0.0)
    elif pattern == "finite":
        v.set(rng.standard_normal(m))
    elif pattern == "nan":
        v.fill(np.nan)
    elif pattern == "inf":
        v.fill(np.inf)
    elif pattern == "ones":
        v.set(np.full(m, -1, np.int64).view(np.float64))
    else:
        raise ValueError(pattern)


def _poison(gpu, lengths, pattern, seed=0):
    """Empty the block cache, then leave in it K_BLOCKS blocks of each length (in doubles) filled with the pattern.  The cache serves
    a request from the smallest idle block that holds it and wastes at most a quarter (below 1 MiB: half), so vectors of the lengths
    the library allocates for an n-row operator - n, n + 2 - land in these blocks.  The lengths are n + 1 and n + 2: a block filled
    to n entries only would keep whatever the driver's recycled memory held at entry n."""
    if os.environ.get("FS_POOL_MAX_MB") == "0":
        pytest.skip("the block cache is switched off (FS_POOL_MAX_MB=0)")
    rng = np.random.default_rng(seed)
    gpu.trim_memory()
    before = gpu.memory_info()["cached_bytes"]
    vs, released = [], 0
    for m in lengths:
        for _ in range(K_BLOCKS):
            v = gpu.DeviceVector(m)
            _fill(v, m, pattern, rng)
            vs.append(v)
            released += 8 * m
    gpu.synchronize()
    for v in vs:
        v.close()
    assert gpu.memory_info()["cached_bytes"] - before >= released


def _vector_from_cache(gpu, n):
    """A vector of n entries whose block comes out of the (poisoned) cache."""
    before = gpu.memory_info()["cached_bytes"]
    v = gpu.DeviceVector(n)
    assert before - gpu.memory_info()["cached_bytes"] >= 8 * n, "the vector did not come out of the block cache"
    return v


def _host_product(A, x):
    """y = A x from the assembled CSR in float64 with the row sums rounded once (extended precision: 64-bit products and sums, ~2^-60
    relative to |A| |x| for the row lengths here, then one rounding), and |A| |x|.  A: a device matrix (to_csr(); every row has an
    entry) or a scipy CSR matrix, whose rows without entries give 0."""
    if hasattr(A, "to_csr"):
        rp, ci, va, (nr, _) = A.to_csr()
        assert np.all(np.diff(rp) > 0), "a row without entries"
    else:
        rp, ci, va, nr = A.indptr, A.indices, A.data, A.shape[0]
    rp = rp.astype(np.int64)
    y = np.zeros(nr)
    ax = np.zeros(nr)
    if np.finfo(np.longdouble).nmant >= 63:
        step = 1 << 18
        for r0 in range(0, nr, step):
            r1 = min(nr, r0 + step)
            e0, e1 = rp[r0], rp[r1]
            rows = r0 + np.flatnonzero(rp[r0 + 1:r1 + 1] > rp[r0:r1])      # (reduceat takes the starts of the rows that have entries)
            if len(rows) == 0:
                continue
            off = rp[rows] - e0
            prod = va[e0:e1].astype(np.longdouble) * x[ci[e0:e1]].astype(np.longdouble)
            y[rows] = np.add.reduceat(prod, off).astype(np.float64)
            ax[rows] = np.add.reduceat(np.abs(prod), off).astype(np.float64)
    else:
        for i in range(nr):
            sl = slice(rp[i], rp[i + 1])
            t = va[sl] * x[ci[sl]]
            y[i] = math.fsum(t)
            ax[i] = math.fsum(np.abs(t))
    return y, ax


def _check_against_host(y, y_ref, ax, what):
    """Every row finite and within 4 eps (|A| |x|)_row of the host product; returns the largest err / (eps |A| |x|) met."""
    assert np.all(np.isfinite(y)), (what, "non-finite rows", np.flatnonzero(~np.isfinite(y))[:8], int((~np.isfinite(y)).sum()))
    err = np.abs(y - y_ref)
    bad = err > 4.0 * EPS * ax
    worst = float((err / np.maximum(ax, 1e-300)).max() / EPS)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8], worst)
    return worst
