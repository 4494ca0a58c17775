"""Sparse (CSR) input for the tree family — GPU tier.

k_bin_csr is asserted against the dense constructor's codes, and
k_forest_predict_csr / k_forest_apply_csr against the dense kernels on a
separately held ndarray.  Every sparse matrix handed to the code under
test is a ``NoDensify`` (any ``toarray`` / ``todense`` fails the test).
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_sparse_trees import (
    BIN_CASES,
    NoDensify,
    assert_same_trees,
    binned_pair,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skdist_amd import Cluster
    from skdist_amd.distribute.ensemble import DistExtraTreesClassifier
    from skdist_amd.distribute.predict import DistPredictor
    from skdist_amd.models.boosting import HistGradientBoostingClassifier
    from skdist_amd.models.forest import (
        BinnedDataset,
        FlatForest,
        ForestBuilder,
        HistTree,
        flat_forest_for,
    )


# --------------------------------------------------------------------- #
# 7 / 8: binning kernel and the device builder on its codes
# --------------------------------------------------------------------- #

@pytest.mark.parametrize("n,f,mbs", BIN_CASES)
def test_binning_identity_kernel(n, f, mbs):
    a, b, _, _, _ = binned_pair(n, f, mbs, "cuda")
    assert a.codes.is_cuda and a.codes.shape == (n, (f + 3) // 4 * 4)
    np.testing.assert_array_equal(a.edges.cpu().numpy(),
                                  b.edges.cpu().numpy())
    np.testing.assert_array_equal(a.codes.cpu().numpy(),
                                  b.codes.cpu().numpy())


def test_builder_identity_device():
    a, b, _, _, _ = binned_pair(1237, 9, 200_000, "cuda")
    kw = dict(max_depth=6, bootstrap=False)
    ta = ForestBuilder(a, "gini", **kw).build([3, 17, 42])
    tb = ForestBuilder(b, "gini", **kw).build([3, 17, 42])
    assert max(t.node_count for t in tb) > 3
    assert_same_trees(ta, tb)


# --------------------------------------------------------------------- #
# 9: CSR traversal against the dense kernels
# --------------------------------------------------------------------- #

F9 = 37
ROOT_EQ_FEAT, ROOT_EQ_THR = 5, 2.0      # a stored 2.0 must go LEFT
ROOT_NEG_FEAT, ROOT_NEG_THR = 3, -1.0   # an absent cell (0.0) goes RIGHT


def _stump(feat, thr, f):
    return HistTree(
        np.array([feat, -1, -1], dtype=np.int32),
        np.array([thr, 0, 0], dtype=np.float32),
        np.array([1, 0, 1], dtype=np.int32),
        np.array([2, 0, 0], dtype=np.int32),
        np.zeros((2, 1), dtype=np.float32), None, f, None)


def _with_payload(t, vs, rng):
    """Same structure, random [n_leaves, vs] payload."""
    n_leaves = int((t.feature < 0).sum())
    v = rng.standard_normal((n_leaves, vs)).astype(np.float32)
    return HistTree(t.feature, t.threshold, t.left, t.right, v, None,
                    t.n_features_in_, None)


@pytest.fixture(scope="module")
def case9():
    """(NoDensify [257, 37], the same matrix dense, base tree list)."""
    rng = np.random.default_rng(9)
    n = 257
    Xd = rng.integers(-2, 4, size=(n, F9)).astype(np.float32)
    stored = rng.random((n, F9)) < 0.3
    stored[0] = True                 # row 0: fully stored, zeros explicit
    stored[1] = False                # row 1: empty
    stored[2, 7] = True              # row 2: a stored explicit zero
    Xd[2, 7] = 0.0
    stored[3, ROOT_EQ_FEAT] = True   # row 3: value == a root threshold
    Xd[3, ROOT_EQ_FEAT] = ROOT_EQ_THR
    stored[4, ROOT_NEG_FEAT] = False  # row 4: root feature absent
    Xd = np.where(stored, Xd, 0).astype(np.float32)
    data, indices, indptr = [], [], [0]
    for i in range(n):
        cols = np.flatnonzero(stored[i])
        indices.extend(cols)
        data.extend(Xd[i, cols])
        indptr.append(len(indices))
    X = NoDensify(
        (np.asarray(data, dtype=np.float32),
         np.asarray(indices, dtype=np.int32),
         np.asarray(indptr, dtype=np.int64)), shape=(n, F9))
    assert (X.data == 0).any()       # explicit zeros really are stored

    # fitted structures: thresholds are quantile edges of small-integer
    # columns, so x == thr happens all over the data
    y = (Xd[:, 0] + Xd[:, 1] - Xd[:, 2] > 0).astype(np.int64)
    ds = BinnedDataset(Xd, y, "cpu", is_cls=True)
    fitted = ForestBuilder(ds, "gini", max_depth=6,
                           bootstrap=False).build([1, 2, 3])
    leaf = HistTree(
        np.array([-1], dtype=np.int32), np.zeros(1, dtype=np.float32),
        np.array([0], dtype=np.int32), np.array([0], dtype=np.int32),
        np.zeros((1, 1), dtype=np.float32), None, F9, None)
    base = fitted[:1] + [
        _stump(ROOT_EQ_FEAT, ROOT_EQ_THR, F9),
        _stump(ROOT_NEG_FEAT, ROOT_NEG_THR, F9), leaf] + fitted[1:]
    return X, Xd, base


@pytest.mark.parametrize("vs", [1, 2, 32])
@pytest.mark.parametrize("n_trees", [1, 65])
@pytest.mark.parametrize("rows", [1, 257])
def test_traversal_matches_dense_kernel(case9, rows, n_trees, vs):
    X, Xd, base = case9
    rng = np.random.default_rng(vs)
    trees = [_with_payload(t, vs, rng)
             for t in (base * 11)[:n_trees]]
    ff = FlatForest(trees, "cuda")
    Xs, Xn = X[:rows], Xd[:rows]
    assert isinstance(Xs, NoDensify)
    np.testing.assert_array_equal(ff.apply(Xs), ff.apply(Xn))
    # trees are walked in order t = 0..T-1 by one thread per row, as in
    # the dense kernel: the sums are bit-identical
    np.testing.assert_array_equal(ff.predict_value(Xs),
                                  ff.predict_value(Xn))


def test_traversal_edge_rows(case9):
    X, Xd, base = case9
    rng = np.random.default_rng(0)
    base = [_with_payload(t, 1, rng) for t in base]
    ff = FlatForest(base, "cuda")
    leaves = ff.apply(X)
    np.testing.assert_array_equal(leaves, ff.apply(Xd))
    # base[1]: root "x[5] <= 2.0"; row 3 stores exactly 2.0 → left (1)
    assert leaves[3, 1] == 1
    # base[2]: root "x[3] <= -1.0"; row 4 has no entry (0.0) → right (2),
    # and so does the empty row
    assert leaves[4, 2] == 2 and leaves[1, 2] == 2
    # base[3] is a single leaf
    assert (leaves[:, 3] == 0).all()
    # host traversal of the same CSR agrees
    for k, t in enumerate(base):
        np.testing.assert_array_equal(t.apply(X), leaves[:, k])


def test_traversal_long_row():
    """One fully stored row of f = 5000 entries.  The CSR kernels stage
    nothing in LDS — every row, whatever its length, takes the same
    global-memory binary search — so there is no staging cap to exceed;
    5000 stays as the long-row case."""
    f = 5000
    rng = np.random.default_rng(5)
    depth = 8
    n_int = 2 ** depth - 1
    trees = []
    for _ in range(9):
        feature = np.full(2 * n_int + 1, -1, dtype=np.int32)
        feature[:n_int] = rng.integers(0, f, n_int)
        feature[0] = f - 1               # the last column is looked up
        thr = rng.integers(-2, 4, 2 * n_int + 1).astype(np.float32)
        left = np.zeros(2 * n_int + 1, dtype=np.int32)
        right = np.zeros(2 * n_int + 1, dtype=np.int32)
        left[:n_int] = 2 * np.arange(n_int) + 1
        right[:n_int] = 2 * np.arange(n_int) + 2
        left[n_int:] = np.arange(n_int + 1)
        value = rng.standard_normal((n_int + 1, 3)).astype(np.float32)
        trees.append(HistTree(feature, thr, left, right, value, None, f,
                              None))
    Xd = rng.integers(-2, 4, size=(3, f)).astype(np.float32)
    Xd[1] = 0
    Xd[2, 10:] = 0
    data = np.concatenate([Xd[0], Xd[2, :10]])
    indices = np.concatenate([np.arange(f), np.arange(10)])
    X = NoDensify((data, indices.astype(np.int32),
                   np.array([0, f, f, f + 10], dtype=np.int64)),
                  shape=(3, f))
    ff = FlatForest(trees, "cuda")
    np.testing.assert_array_equal(ff.apply(X), ff.apply(Xd))
    np.testing.assert_array_equal(ff.predict_value(X),
                                  ff.predict_value(Xd))
    np.testing.assert_array_equal(
        ff.apply(X), np.column_stack([t.apply(Xd) for t in trees]))


def test_traversal_rejects_wrong_width(case9):
    X, _, base = case9
    rng = np.random.default_rng(0)
    ff = FlatForest([_with_payload(t, 1, rng) for t in base], "cuda")
    wide = NoDensify(sp.hstack([X, X]).tocsr())
    with pytest.raises(ValueError, match="features"):
        ff.predict_value(wide)
    with pytest.raises(ValueError, match="features"):
        ff.apply(wide)


# --------------------------------------------------------------------- #
# 10: sklearn-fitted ensembles on a wide hashed-text-like matrix
# --------------------------------------------------------------------- #

@pytest.fixture(scope="module")
def wide_counts():
    rng = np.random.default_rng(10)
    n, f = 400, 2 ** 18
    rows = np.repeat(np.arange(n), 30)
    cols = np.concatenate([
        rng.integers(0, 64, size=(n, 10)),       # informative block
        rng.integers(64, f, size=(n, 20)),       # hashed tail
    ], axis=1).ravel()
    vals = rng.integers(1, 4, size=n * 30).astype(np.float32)
    X = sp.csr_matrix((vals, (rows, cols)), shape=(n, f))
    X.sum_duplicates()
    head = np.asarray(X[:, :64].sum(axis=1)).ravel()
    lo = np.asarray(X[:, :32].sum(axis=1)).ravel()
    y = (2 * lo > head).astype(np.int64)
    assert 0.2 < y.mean() < 0.8
    return X, NoDensify(X), y


def test_sklearn_forests_wide(wide_counts):
    from sklearn.ensemble import (
        RandomForestClassifier,
        RandomForestRegressor,
    )

    X, Xg, y = wide_counts
    rf = RandomForestClassifier(n_estimators=8, max_depth=6,
                                random_state=0).fit(X, y)
    ff = flat_forest_for(rf, "cuda")
    np.testing.assert_array_equal(ff.apply(Xg), rf.apply(X))
    np.testing.assert_allclose(ff.predict_proba(Xg), rf.predict_proba(X),
                               atol=1e-5, rtol=0)
    out = DistPredictor(rf, sc=None, method="predict_proba")(Xg)
    np.testing.assert_allclose(out, rf.predict_proba(X), atol=1e-5,
                               rtol=0)

    rr = RandomForestRegressor(n_estimators=8, max_depth=6,
                               random_state=0).fit(X, y.astype(float))
    fr = flat_forest_for(rr, "cuda")
    np.testing.assert_array_equal(fr.apply(Xg), rr.apply(X))
    np.testing.assert_allclose(fr.predict(Xg), rr.predict(X), atol=1e-5,
                               rtol=0)


def test_sklearn_gbt_wide(wide_counts):
    from sklearn.ensemble import GradientBoostingClassifier

    X, Xg, y = wide_counts
    gbt = GradientBoostingClassifier(n_estimators=10,
                                     random_state=0).fit(X, y)
    fg = flat_forest_for(gbt, "cuda")
    np.testing.assert_allclose(fg.predict_proba(Xg), gbt.predict_proba(X),
                               atol=1e-4, rtol=0)
    out = DistPredictor(gbt, sc=None, method="predict_proba")(Xg)
    np.testing.assert_allclose(out, gbt.predict_proba(X), atol=1e-4,
                               rtol=0)


def test_dist_extratrees_scores_csr(wide_counts):
    X, Xg, y = wide_counts
    clf = DistExtraTreesClassifier(n_estimators=4, sc=None,
                                   random_state=0).fit(X, y)
    proba = clf.predict_proba(Xg)
    assert clf._device_forest() is not None   # scored by the CSR kernel
    host = np.mean([t.predict_proba(X) for t in clf.estimators_], axis=0)
    np.testing.assert_allclose(proba, host, atol=1e-5, rtol=0)


# --------------------------------------------------------------------- #
# 11: boosted fit with the CSR resident on the device
# --------------------------------------------------------------------- #

def test_boosted_fit_device():
    rng = np.random.default_rng(0)
    Xd = rng.standard_normal((3000, 24)).astype(np.float32)
    Xd[rng.random((3000, 24)) < 0.85] = 0
    y = (Xd[:, 0] - Xd[:, 1] + 0.5 * Xd[:, 2] > 0.2).astype(int)
    Xtr = NoDensify(sp.csr_matrix(Xd[:2400]))
    Xte, Xte_d = NoDensify(sp.csr_matrix(Xd[2400:])), Xd[2400:]
    m = HistGradientBoostingClassifier(
        n_estimators=20, random_state=0, sc=Cluster(require_gpu=True))
    m.fit(Xtr, y[:2400])
    assert m.n_features_in_ == 24 and len(m.stages_) == 20
    acc = (m.predict(Xte) == y[2400:]).mean()
    print("held-out accuracy", acc)
    assert acc >= 0.95, acc
    # host scorer, sparse vs dense: the same traversal, equal bits
    ps = m.predict_proba(Xte)
    np.testing.assert_array_equal(ps, m.predict_proba(Xte_d))
    np.testing.assert_allclose(ps.sum(axis=1), 1.0, atol=1e-6, rtol=0)
    # device scorer, CSR kernel vs dense kernel: tree order is kept, so
    # the bound of the traversal test (exact equality) holds here too
    pred = DistPredictor(m, sc=None, method="predict_proba")
    np.testing.assert_array_equal(pred(Xte), pred(Xte_d))
