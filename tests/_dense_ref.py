"""
Float64 numpy references of the dense batched SGD step, kernel by kernel
(skdist_amd/ops/csrc/sgd_kernels.hip).  Every function takes the buffers
its kernel takes, as numpy arrays holding the VALUES of those buffers
(bf16 buffers as float64 of their bf16 values), and returns float64.
Rounding to bf16 is left to the caller (``bf16_rne``), so the same
functions compose into an unrounded fp64 step for the CPU check against
``_sgd._sgd_step_torch`` (tests/test_dense_ref.py).

A plain helper module, not a conftest.
"""

import numpy as np

LOSS_LOG, LOSS_HINGE, LOSS_SQUARED = 0, 1, 2
PAD_SENTINEL = -1e30  # y of a pad row in the scoring buffers
EPS32 = 2.0 ** -24    # fp32 unit roundoff (half an ulp of 1.0)


def ceil_to(x, q):
    return (x + q - 1) // q * q


def bf16_rne(x):
    """Round float64 values to bf16 (8-bit significand, round to nearest,
    ties to even), returned as float64.  Works on the float64 bit pattern:
    52 - 7 = 45 significand bits are dropped.  Finite inputs in bf16's
    normal range only (the tests stay far inside it)."""
    shape = np.shape(x)
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    drop = np.uint64(45)
    lsb = (b >> drop) & np.uint64(1)
    r = b + np.uint64((1 << 44) - 1) + lsb
    r &= ~np.uint64((1 << 45) - 1)
    return r.view(np.float64).reshape(shape)


def bf16_step(x):
    """Spacing of bf16 values in the binade of |x| (x != 0)."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    return 2.0 ** (e - 7)


def to_bf16_bits(x):
    """uint16 bf16 bit patterns of float64 values that ARE bf16 values."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(x, np.float64))
    bits = f.view(np.uint32)
    assert not np.any(bits & np.uint32(0xFFFF)), "not a bf16 value"
    return (bits >> np.uint32(16)).astype(np.uint16)


def dloss(loss_id, z, t):
    """common.h dloss in float64."""
    if loss_id == LOSS_LOG:
        zc = np.clip(z, -30.0, 30.0)
        return 1.0 / (1.0 + np.exp(-zc)) - t
    if loss_id == LOSS_HINGE:
        s = 2.0 * t - 1.0
        return np.where(s * z < 1.0, -s, 0.0)
    return z - t


def ref_gt(Xs, WbfT, y, fold, col_class, col_fold, col_class2, row_w,
           start, m, loss_id):
    """K1 (k_fwd_gt).  Xs [n_pad, fa], WbfT [ncols_pad, fa], y/fold [n],
    column vectors [ncols_pad], row_w [n] or None.

    Returns (z, g, train), each [m_pad, ncols_pad] (row-major by batch
    row; the kernel stores g transposed): z = Xs[start:start+m_pad]·WbfTᵀ,
    g = dloss(z, target) * row_w where the element trains, else 0.
    An element trains when the row is below m, the row's fold differs from
    the column's, and, for a one-vs-one column (col_class2 >= 0), y is one
    of the pair.  Rows at or past n read y = 0, fold = -9, row_w = 1."""
    Xs = np.asarray(Xs, np.float64)
    WbfT = np.asarray(WbfT, np.float64)
    n = len(y)
    m_pad = ceil_to(m, 128)
    rows = start + np.arange(m_pad)
    ok = rows < n
    rc = np.minimum(rows, n - 1)
    yv = np.where(ok, np.asarray(y, np.float64)[rc], 0.0)
    fv = np.where(ok, np.asarray(fold)[rc], -9)
    rw = np.ones(m_pad)
    if row_w is not None:
        rw = np.where(ok, np.asarray(row_w, np.float64)[rc], 1.0)
    cls = np.asarray(col_class).astype(np.int64)
    cfo = np.asarray(col_fold).astype(np.int64)
    c2 = np.asarray(col_class2).astype(np.int64)

    z = Xs[start:start + m_pad] @ WbfT.T
    is_cls = yv[:, None] == cls[None, :].astype(np.float64)
    t = np.where(cls[None, :] < 0, yv[:, None], is_cls.astype(np.float64))
    g = dloss(loss_id, z, t) * rw[:, None]
    train = (fv[:, None] != cfo[None, :]) & (np.arange(m_pad) < m)[:, None]
    pair = is_cls | (yv[:, None] == c2[None, :].astype(np.float64))
    train = train & ((c2[None, :] < 0) | pair)
    return z, np.where(train, g, 0.0), train


def ref_partial_sum(XsT, GT, start, m_pad):
    """K2 (k_grad_partial), summed over the split-K slabs:
    XsT[:, start:start+m_pad] · GT[:, :m_pad]ᵀ -> [rows of XsT, ncols_pad].
    GT is [ncols_pad, gt_stride] as the kernel stores it."""
    XsT = np.asarray(XsT, np.float64)
    GT = np.asarray(GT, np.float64)
    return XsT[:, start:start + m_pad] @ GT[:, :m_pad].T


def slab_bounds(m_pad, splitk):
    """[k0, k1) of every split-K slab, as the launcher cuts them."""
    k_chunk = ceil_to(m_pad // splitk, 32)
    return [(min(z * k_chunk, m_pad), min(m_pad, (z + 1) * k_chunk))
            for z in range(splitk)]


def ref_update(psum, W, V, col_lr, col_l2, fmask, inv_m, lr_scale,
               momentum, intercept_row):
    """K3 (k_reduce_update).  psum [fa, ncols_pad] is Σ_z partial[z];
    W/V [fa, ncols_pad] (V None when momentum == 0); fmask [fa,
    ncols_pad] of 0/1 or None.  Returns (W', V', terms): terms holds the
    magnitudes the fp32 rounding bound of the test is built from."""
    W = np.asarray(W, np.float64)
    psum = np.asarray(psum, np.float64)
    lr = np.asarray(col_lr, np.float64)[None, :]
    l2 = np.broadcast_to(np.asarray(col_l2, np.float64)[None, :],
                         W.shape).copy()
    l2[intercept_row] = 0.0
    a = psum * float(inv_m)
    b = l2 * W
    step = lr * float(lr_scale) * (a + b)
    S = np.abs(lr * float(lr_scale)) * (np.abs(a) + np.abs(b))
    M = np.zeros_like(W)
    Vn = None
    if momentum > 0.0:
        mv = np.asarray(V, np.float64) * float(momentum)
        M = np.abs(mv)
        step = mv + step
        Vn = step.copy()
    Wn = W - step
    if fmask is not None:
        keep = np.asarray(fmask) != 0
        Wn = np.where(keep, Wn, 0.0)
        if Vn is not None:
            Vn = np.where(keep, Vn, 0.0)
    return Wn, Vn, {"S": S, "M": M, "W": np.abs(W)}


def ref_score(Xf, WbfT, yf, mode):
    """K5 (k_score).  Rows whose y is the pad sentinel are skipped.
    mode 0 -> (hits, valid) per column: hits counts (z >= 0) == (y != 0);
    mode 1 -> (sse, z, y_valid_mask)."""
    Xf = np.asarray(Xf, np.float64)
    WbfT = np.asarray(WbfT, np.float64)
    yf = np.asarray(yf, np.float64)
    valid = yf > -1e29
    z = Xf @ WbfT.T
    if mode == 0:
        hit = (z >= 0.0) == (yf != 0.0)[:, None]
        hits = (hit & valid[:, None]).sum(axis=0).astype(np.float64)
        return hits, np.full(z.shape[1], float(valid.sum())), z
    e = np.where(valid[:, None], z - yf[:, None], 0.0)
    return (e * e).sum(axis=0), z, valid


def ref_standardize(X, mean, inv_std, fa):
    """K4 (k_standardize): [(x - mean) * inv_std | 1 | 0-pad] in fp32
    (a subtraction feeding a product cannot contract to an FMA, so fp32
    numpy is the kernel's arithmetic), then bf16 RNE; as float64."""
    X = np.asarray(X, np.float32)
    n, f = X.shape
    v = (X - np.asarray(mean, np.float32)[None, :]) * \
        np.asarray(inv_std, np.float32)[None, :]
    assert v.dtype == np.float32
    out = np.zeros((n, fa), np.float64)
    out[:, :f] = bf16_rne(v.astype(np.float64))
    out[:, f] = 1.0
    return out


def make_case(seed, n, f, fa, ncols, loss_id, dyadic=True, ovo=True,
              row_w=False, fmask=False, momentum=0.9, n_pad=None,
              w_scale=1.0):
    """Hand-built buffers of one step, as numpy arrays of buffer values.

    dyadic: x in {-1, -.5, 0, .5, 1}, w a multiple of 1/8 in [-.5, .5],
    V a multiple of 1/64, row_w in {.5, 1, 2}, lr and l2 powers of two --
    every product in K1 and K2 is then a multiple of a fixed power of two.
    Otherwise x is a sparse bf16-rounded normal and w a bf16 value of size
    about w_scale/16, with one column 64x larger to reach the +-30 clamp.

    Columns cycle through CV columns of folds 0..2 (class 1), a full-data
    column (fold -2), one-vs-one columns (class 0 vs 2) when ``ovo``, and,
    for squared loss, regression columns (class -1).  Pad columns carry
    what hip_sgd_solve pads with (class -99, fold -9, lr = l2 = 0)."""
    rng = np.random.default_rng(seed)
    n_pad = ceil_to(n, 128) if n_pad is None else n_pad
    ncp = ceil_to(ncols, 128)
    assert f < fa and fa % 32 == 0

    Xs = np.zeros((n_pad, fa))
    if dyadic:
        Xs[:n, :f] = rng.integers(-2, 3, size=(n, f)) / 2.0
    else:
        x = rng.standard_normal((n, f)) * (rng.random((n, f)) < 0.5)
        Xs[:n, :f] = bf16_rne(x)
    Xs[:n, f] = 1.0
    fa_store = ceil_to(fa, 128)
    XsT = np.zeros((fa_store, n_pad))
    XsT[:fa] = Xs.T

    y = rng.integers(0, 3, size=n).astype(np.float64)
    fold = rng.integers(0, 3, size=n).astype(np.int32)

    kinds = [(1, 0, -1), (1, 1, -1), (1, 2, -1), (1, -2, -1)]
    if ovo:
        kinds += [(0, 0, 2), (0, -2, 2), (2, 1, 0)]
    if loss_id == LOSS_SQUARED:
        kinds += [(-1, 0, -1), (-1, -2, -1)]
    col_class = np.full(ncp, -99, np.int32)
    col_fold = np.full(ncp, -9, np.int32)
    col_class2 = np.full(ncp, -1, np.int32)
    for c in range(ncols):
        col_class[c], col_fold[c], col_class2[c] = kinds[c % len(kinds)]
    col_lr = np.zeros(ncp)
    col_l2 = np.zeros(ncp)
    col_lr[:ncols] = 2.0 ** -rng.integers(1, 4, size=ncols)
    col_l2[:ncols] = np.array([0.0, 2.0 ** -6, 2.0 ** -4])[
        rng.integers(0, 3, size=ncols)]

    W = np.zeros((fa, ncp))
    V = np.zeros((fa, ncp))
    if dyadic:
        W[:f + 1, :ncols] = rng.integers(-4, 5, size=(f + 1, ncols)) / 8.0
    else:
        w = rng.standard_normal((f + 1, ncols)) * (w_scale / 16.0)
        if ncols > 5:
            w[:, 5] *= 64.0
        W[:f + 1, :ncols] = bf16_rne(w)
    V[:f + 1, :ncols] = rng.integers(-8, 9, size=(f + 1, ncols)) / 64.0

    rw = None
    if row_w:
        rw = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, size=n)]
    fm = None
    if fmask:
        fm = np.ones((fa, ncp), np.uint8)
        fm[:f, :ncols] = rng.random((f, ncols)) < 0.7
    return dict(
        n=n, n_pad=n_pad, f=f, fa=fa, fa_store=fa_store, ncols=ncols,
        ncols_pad=ncp, loss_id=loss_id, momentum=momentum,
        Xs=Xs, XsT=XsT, y=y, fold=fold, col_class=col_class,
        col_fold=col_fold, col_class2=col_class2, col_lr=col_lr,
        col_l2=col_l2, W=W, V=V if momentum > 0.0 else None,
        row_w=rw, fmask=fm, intercept_row=f)


def inv_m_of(case, start, m):
    """float32 1/m, or 1/sum(row_w) over the batch, as the solver passes."""
    if case["row_w"] is None:
        return np.float32(1.0 / m)
    return np.float32(1.0 / max(float(case["row_w"][start:start + m].sum()),
                                1e-30))
