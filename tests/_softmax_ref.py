"""
Float64 numpy reference of the multinomial forward kernel
(k_fwd_gt_softmax, skdist_amd/ops/csrc/sgd_kernels.hip), the column layout
it expects, and the sklearn comparison the CPU and GPU tests share.

A plain helper module beside ``_dense_ref`` (imported, not edited); not a
conftest.
"""

import functools

import numpy as np

import _dense_ref as R

LOSS_SOFTMAX = 3
TILE = 128


def tile_columns(n_models, gk):
    """Kernel column of every (model, class), model-major, and ncols_pad:
    model j, class c at (j // gpt) * 128 + (j % gpt) * gk + c with
    gpt = 128 // gk groups per tile.  Written out here on its own, not
    imported from the package, so the test pins the layout."""
    gpt = TILE // gk
    cols = np.array([(j // gpt) * TILE + (j % gpt) * gk + c
                     for j in range(n_models) for c in range(gk)])
    return cols, R.ceil_to(n_models, gpt) // gpt * TILE


def make_softmax_case(seed, n, f, fa, n_tiles, gk, row_w, momentum,
                      w_scale=1.0):
    """One step's buffers in the tile layout: ``_dense_ref.make_case``
    inputs (non-dyadic, no one-vs-one), columns re-labelled into groups of
    ``gk``, W and V zeroed on dead and pad columns, y uniform in 0..gk-1.

    The first ``n_tiles - 1`` tiles are full; the last holds about half its
    groups, so pad groups (class -99) sit between live groups and the dead
    tail.  Model j trains against fold (0, 1, 2, -2)[j % 4]."""
    ncp = n_tiles * TILE
    c = R.make_case(seed, n, f, fa, ncp, R.LOSS_LOG, dyadic=False,
                    ovo=False, row_w=row_w, momentum=momentum,
                    w_scale=w_scale)
    assert c["ncols_pad"] == ncp
    gpt = TILE // gk
    n_models = (n_tiles - 1) * gpt + max(1, gpt // 2)
    cols, ncp2 = tile_columns(n_models, gk)
    assert ncp2 == ncp
    live = np.zeros(ncp, bool)
    live[cols] = True
    col_class = np.full(ncp, -99, np.int32)
    col_fold = np.full(ncp, -9, np.int32)
    col_class[cols] = np.tile(np.arange(gk), n_models)
    col_fold[cols] = np.repeat(
        np.array([0, 1, 2, -2])[np.arange(n_models) % 4], gk)
    c["col_class"], c["col_fold"] = col_class, col_fold
    c["col_class2"] = np.full(ncp, -1, np.int32)
    for k in ("col_lr", "col_l2"):
        c[k] = np.where(live, c[k], 0.0)
    c["W"] = np.where(live[None, :], c["W"], 0.0)
    if c["V"] is not None:
        c["V"] = np.where(live[None, :], c["V"], 0.0)
    rng = np.random.default_rng(seed + 1000)
    c["y"] = rng.integers(0, gk, size=n).astype(np.float64)
    c.update(gk=gk, n_models=n_models, live=live, cols=cols,
             loss_id=LOSS_SOFTMAX, ncols=ncp)
    return c


def ref_gt_softmax(c, start, m):
    """Float64 K1 of the softmax loss on a ``make_softmax_case`` case.

    Returns z, g, train [m_pad, ncols_pad] and rw [m_pad]: z = Xs·W,
    p = max-shifted softmax over each live group, g = (p - t) * row_w where
    the element trains (row < m, row < n, row fold != column fold, live
    column), else 0 -- masked like ``_dense_ref.ref_gt``."""
    Xs = np.asarray(c["Xs"], np.float64)
    n, gk = len(c["y"]), c["gk"]
    m_pad = R.ceil_to(m, TILE)
    rows = start + np.arange(m_pad)
    ok = rows < n
    rc = np.minimum(rows, n - 1)
    yv = np.where(ok, c["y"][rc], 0.0)
    fv = np.where(ok, c["fold"][rc], -9)
    rw = np.ones(m_pad)
    if c["row_w"] is not None:
        rw = np.where(ok, c["row_w"][rc], 1.0)
    z = Xs[start:start + m_pad] @ np.asarray(c["W"], np.float64)
    g = np.zeros_like(z)
    cols = c["cols"].reshape(-1, gk)
    for grp in cols:
        zg = z[:, grp]
        e = np.exp(zg - zg.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        t = (yv[:, None] == c["col_class"][grp][None, :]).astype(np.float64)
        g[:, grp] = (p - t) * rw[:, None]
    train = ((fv[:, None] != c["col_fold"][None, :])
             & ((np.arange(m_pad) < m) & ok)[:, None] & c["live"][None, :])
    return z, np.where(train, g, 0.0), train, rw


def softmax_delta(c, start, m, train, rw):
    """The interval half-width of the GPU test, per element:
    (dzg / 2 + 2^-19 + (K + 3) 2^-24) * row_w on trained elements, 0
    elsewhere; dzg = max over the group's live columns of
    dz = fa 2^-24 (|Xs| |W|)."""
    gk, fa = c["gk"], c["fa"]
    m_pad = R.ceil_to(m, TILE)
    dz = fa * R.EPS32 * (np.abs(c["Xs"][start:start + m_pad])
                         @ np.abs(c["W"]))
    dzg = np.zeros_like(dz)
    for grp in c["cols"].reshape(-1, gk):
        dzg[:, grp] = dz[:, grp].max(axis=1, keepdims=True)
    delta = (dzg / 2 + 2.0 ** -19 + (gk + 3) * R.EPS32) * rw[:, None]
    return np.where(train, delta, 0.0)


# ------------------------------------------------------------------ #
# the sklearn comparison (CPU test 1, GPU test 10)
# ------------------------------------------------------------------ #

def load(name):
    from sklearn import datasets

    return getattr(datasets, f"load_{name}")(return_X_y=True)


@functools.lru_cache(maxsize=None)
def sklearn_probas(name):
    """(P_multinomial, P_ovr) of sklearn's LogisticRegression(C=0.1,
    tol=1e-12, max_iter=50000) on the population-standardised data set,
    on the training rows.  Computed once per session; callers must not
    modify the arrays."""
    from sklearn.linear_model import LogisticRegression as SkLR
    from sklearn.multiclass import OneVsRestClassifier

    X, y = load(name)
    Xs = (X - X.mean(axis=0)) / X.std(axis=0)
    kw = dict(C=0.1, tol=1e-12, max_iter=50000)
    multi = SkLR(**kw).fit(Xs, y).predict_proba(Xs)
    ovr = OneVsRestClassifier(SkLR(**kw)).fit(Xs, y).predict_proba(Xs)
    multi.setflags(write=False)
    ovr.setflags(write=False)
    return multi, ovr
