"""Missing values (NaN) in the tree stack, CPU tier: binning with a missing
bin, the split scan's learned direction (eager mirror of k_tree_split_m),
the partition, host traversal and the sklearn flatten."""

import pickle

import numpy as np
import pytest
import scipy.sparse as sp

from skdist_amd.models import (
    HistGradientBoostingClassifier,
    HistGradientBoostingRegressor,
)
from skdist_amd.models.forest import (
    BinnedDataset,
    ForestBuilder,
    HistTree,
    _sklearn_tree_to_hist_tree,
)

LEVELS = np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32)


def stump_data(n=3000, seed=0):
    """x0 in {-3..3} with 40 % NaN, x1 noise; y = 0 if missing else x0 > 0:
    the one perfect depth-1 split is x0 <= -1 with the missing rows left."""
    rng = np.random.default_rng(seed)
    x0 = rng.choice(LEVELS, n)
    miss = rng.random(n) < 0.4
    y = np.where(miss, 0.0, x0 > 0).astype(np.float64)
    x0[miss] = np.nan
    X = np.column_stack([x0, rng.standard_normal(n)]).astype(np.float32)
    return X, y


def missing_vs_rest_data(n=3000, seed=1):
    """y = 1 if x0 is missing else x1 > 0 (x0 normal, x1 in {-3..3})."""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal(n).astype(np.float32)
    x1 = rng.choice(LEVELS, n)
    miss = rng.random(n) < 0.3
    y = np.where(miss, 1, x1 > 0).astype(np.int64)
    x0[miss] = np.nan
    return np.column_stack([x0, x1]).astype(np.float32), y


def holes(X, frac, seed):
    X = np.array(X, dtype=np.float32)
    X[np.random.default_rng(seed).random(X.shape) < frac] = np.nan
    return X


def trees_of(model):
    return [t for stage in model.stages_ for t in stage]


# ---------------------------------------------------------------------- #
# binning
# ---------------------------------------------------------------------- #
def test_binning_reserves_the_top_code_for_nan():
    rng = np.random.default_rng(0)
    X = holes(rng.standard_normal((4000, 5)), 0.2, 1)
    X[:, 3] = np.nan                                  # an all-NaN column
    ds = BinnedDataset(X, np.zeros(len(X)), "cpu", is_cls=False,
                       allow_missing=True)
    assert ds.missing_bin == ds.nbins - 1 == 255
    codes = ds.codes.numpy()[:, : ds.f]
    np.testing.assert_array_equal(codes == ds.missing_bin, np.isnan(X))
    edges = ds.edges.numpy()
    assert edges.shape == (5, 255)
    assert np.isposinf(edges[:, -1]).all()
    assert np.isposinf(edges[3]).all()
    assert np.isfinite(edges[[0, 1, 2, 4], :-1]).all()
    # the finite edges are the non-NaN quantiles, ascending
    assert (np.diff(edges[0, :-1]) >= 0).all()
    q = np.nanquantile(X[:, 0].astype(np.float64),
                       np.linspace(0, 1, 256)[1:-1])
    np.testing.assert_allclose(edges[0, :-1], q, rtol=0, atol=1e-5)
    # code = number of edges below the value; the +inf edge caps it
    present = ~np.isnan(X[:, 0])
    ref = (edges[0][None, :] < X[present, 0][:, None]).sum(axis=1)
    np.testing.assert_array_equal(codes[present, 0], ref)
    assert codes[present, 0].max() <= 254
    # pad columns stay zero
    assert ds.fp == 8 and not ds.codes.numpy()[:, 5:].any()


def test_binning_without_nan_is_todays():
    X = np.random.default_rng(2).standard_normal((3000, 6)).astype(
        np.float32)
    y = np.zeros(len(X))
    a = BinnedDataset(X, y, "cpu", is_cls=False)
    b = BinnedDataset(X, y, "cpu", is_cls=False, allow_missing=True)
    assert a.missing_bin is None and b.missing_bin is None
    np.testing.assert_array_equal(a.edges.numpy(), b.edges.numpy())
    np.testing.assert_array_equal(a.codes.numpy(), b.codes.numpy())
    assert a.nbins == b.nbins


def test_binning_rejections():
    X = np.zeros((10, 2), dtype=np.float32)
    X[3, 1] = np.nan
    y = np.zeros(10)
    with pytest.raises(ValueError, match="NaN or infinity"):
        BinnedDataset(X, y, "cpu", is_cls=False)
    Xi = X.copy()
    Xi[4, 0] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        BinnedDataset(Xi, y, "cpu", is_cls=False, allow_missing=True)
    Xi[3, 1] = 0.0                                     # inf alone
    with pytest.raises(ValueError, match="infinity"):
        BinnedDataset(Xi, y, "cpu", is_cls=False, allow_missing=True)
    # a stored NaN in a sparse X raises in either mode, with its own text
    with pytest.raises(ValueError, match="sparse"):
        BinnedDataset(sp.csr_matrix(X), y, "cpu", is_cls=False,
                      allow_missing=True)
    with pytest.raises(ValueError, match="NaN or infinity"):
        BinnedDataset(sp.csr_matrix(X), y, "cpu", is_cls=False)


def test_extra_mode_rejected_on_a_missing_bin():
    X, y = stump_data(200)
    ds = BinnedDataset(X, y, "cpu", is_cls=False, allow_missing=True)
    with pytest.raises(ValueError, match="extra_mode"):
        ForestBuilder(ds, "squared_error", extra_mode=True)


# ---------------------------------------------------------------------- #
# learned direction
# ---------------------------------------------------------------------- #
def test_stump_sends_missing_left_like_sklearn():
    from sklearn.tree import DecisionTreeRegressor

    X, y = stump_data()
    m = HistGradientBoostingRegressor(
        n_estimators=1, learning_rate=1, max_depth=1, allow_nan=True,
        random_state=0).fit(X, y)
    t = m.stages_[0][0]
    assert t.feature[0] == 0
    assert t.missing_left[0] == 1
    assert -1.0 <= t.threshold[0] < 1.0
    pred = m.predict(X)
    # leaf means come from f32 sums of <= 3000 residuals: n * eps ~ 2e-4
    assert np.abs(pred - y).max() < 2e-4
    np.testing.assert_array_equal(np.round(pred), y)

    # sklearn 1.7 finds this split under every feature order, but its leaf
    # means are exact only when the NaN feature is the last one visited
    # (otherwise one row's target is booked to the other child: 4.9e-4
    # instead of 0); the seed fixes such an order
    sk = DecisionTreeRegressor(max_depth=1, random_state=0).fit(X, y)
    assert sk.tree_.feature[0] == 0
    assert sk.tree_.missing_go_to_left[0] == 1
    np.testing.assert_array_equal(sk.predict(X), y)


def test_missing_vs_rest_split():
    X, y = missing_vs_rest_data()
    m = HistGradientBoostingClassifier(
        n_estimators=20, max_depth=3, allow_nan=True,
        random_state=0).fit(X[:2000], y[:2000])
    acc = (m.predict(X[2000:]) == y[2000:]).mean()
    assert acc >= 0.99, acc
    t = m.stages_[0][0]
    inner = t.feature >= 0
    assert (inner & (t.feature == 0) & np.isposinf(t.threshold)).any()
    # everything that reads the trees takes NaN
    assert m.decision_function(X[2000:]).shape == (1000,)
    last = list(m.staged_predict(X[2000:]))[-1]
    np.testing.assert_array_equal(last, m.predict(X[2000:]))


def test_no_nan_fit_is_identical_and_flags_follow_majority():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((1500, 5)).astype(np.float32)
    y = (X[:, 0] + X[:, 1] ** 2 > 0.5).astype(np.int64)
    kw = dict(n_estimators=5, random_state=3)
    a = HistGradientBoostingClassifier(**kw).fit(X, y)
    b = HistGradientBoostingClassifier(allow_nan=True, **kw).fit(X, y)
    seen = set()
    for ta, tb in zip(trees_of(a), trees_of(b)):
        for name in ("feature", "threshold", "left", "right", "value"):
            np.testing.assert_array_equal(getattr(ta, name),
                                          getattr(tb, name))
        assert ta.missing_left is None
        assert tb.missing_left.dtype == np.uint8
        assert tb.missing_left.shape == (tb.node_count,)
        # majority: count the training rows on each side of every split
        node = tb.apply(X)                 # leaf per row -> walk up
        n_at = np.bincount(node, minlength=tb.node_count).astype(float)
        for i in reversed(range(tb.node_count)):     # children after parent
            if tb.feature[i] >= 0:
                n_at[i] = n_at[tb.left[i]] + n_at[tb.right[i]]
        for i in range(tb.node_count):
            if tb.feature[i] >= 0:
                want = int(n_at[tb.left[i]] > n_at[tb.right[i]])
                assert tb.missing_left[i] == want, (i, n_at)
                seen.add(want)
            else:
                assert tb.missing_left[i] == 0
    assert seen == {0, 1}
    np.testing.assert_array_equal(a.predict_proba(X), b.predict_proba(X))


def test_default_still_raises_and_inf_always_raises():
    X, y = stump_data(300)
    with pytest.raises(ValueError, match="NaN or infinity"):
        HistGradientBoostingRegressor(n_estimators=2).fit(X, y)
    with pytest.raises(ValueError, match="NaN or infinity"):
        HistGradientBoostingClassifier(n_estimators=2).fit(
            X, (y > 0).astype(int))
    X[5, 1] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        HistGradientBoostingRegressor(n_estimators=2, allow_nan=True).fit(
            X, y)
    with pytest.raises(ValueError, match="sparse"):
        HistGradientBoostingRegressor(n_estimators=2, allow_nan=True).fit(
            sp.csr_matrix(stump_data(300)[0]), y)


# ---------------------------------------------------------------------- #
# composition
# ---------------------------------------------------------------------- #
def test_composes_with_weights_subsample_and_early_stopping():
    X, y = missing_vs_rest_data(1500, seed=4)
    Xh, yh = missing_vs_rest_data(800, seed=5)
    sw = np.random.default_rng(0).uniform(0.5, 2.0, len(y))
    kw = dict(n_estimators=12, max_depth=3, allow_nan=True, random_state=0)
    fits = {
        "sample_weight": HistGradientBoostingClassifier(**kw).fit(
            X, y, sample_weight=sw),
        "class_weight": HistGradientBoostingClassifier(
            class_weight="balanced", **kw).fit(X, y),
        "subsample": HistGradientBoostingClassifier(
            subsample=0.7, **kw).fit(X, y),
        "early_stop": HistGradientBoostingClassifier(
            n_iter_no_change=3, **kw).fit(X, y),
    }
    for name, m in fits.items():
        assert (m.predict(Xh) == yh).mean() >= 0.97, name
        assert all(t.missing_left is not None for t in trees_of(m))
    r = HistGradientBoostingRegressor(**kw).fit(
        X, y.astype(float), sample_weight=sw)
    assert np.isfinite(r.predict(Xh)).all()


def test_params_clone_pickle_and_grid_search():
    from sklearn.base import clone

    from skdist_amd.distribute.search import DistGridSearchCV

    X, y = missing_vs_rest_data(600, seed=6)
    m = HistGradientBoostingClassifier(n_estimators=5, allow_nan=True,
                                       random_state=0)
    assert m.get_params()["allow_nan"] is True
    assert HistGradientBoostingRegressor().get_params()["allow_nan"] is False
    assert clone(m).allow_nan is True
    m.fit(X, y)
    m2 = pickle.loads(pickle.dumps(m))
    np.testing.assert_array_equal(m2.predict_proba(X), m.predict_proba(X))
    gs = DistGridSearchCV(
        HistGradientBoostingClassifier(n_estimators=5, random_state=0),
        {"allow_nan": [True], "max_depth": [1, 2]}, cv=2).fit(X, y)
    assert gs.best_params_["allow_nan"] is True
    assert gs.best_score_ > 0.9
    assert gs.predict(X).shape == y.shape


def test_tree_without_the_attribute_still_walks():
    """A HistTree pickled before missing_left existed has no such
    attribute: NaN goes right, as it did."""
    t = HistTree(np.array([0, -1, -1], dtype=np.int32),
                 np.array([0.0, 0, 0], dtype=np.float32),
                 np.array([1, 0, 1], dtype=np.int32),
                 np.array([2, 0, 0], dtype=np.int32),
                 np.array([[1.0], [2.0]], dtype=np.float32), None, 1, None)
    del t.missing_left
    X = np.array([[-1.0], [1.0], [np.nan]], dtype=np.float32)
    np.testing.assert_array_equal(t.apply(X), [1, 2, 2])
    t.missing_left = np.array([1, 0, 0], dtype=np.uint8)
    np.testing.assert_array_equal(t.apply(X), [1, 2, 1])


# ---------------------------------------------------------------------- #
# host traversal, sklearn flatten
# ---------------------------------------------------------------------- #
def test_host_apply_dense_and_csr_agree():
    X, y = missing_vs_rest_data(1500, seed=7)
    X = np.column_stack([X, holes(np.random.default_rng(8).standard_normal(
        (len(X), 3)), 0.25, 9)]).astype(np.float32)
    m = HistGradientBoostingClassifier(
        n_estimators=6, max_depth=4, allow_nan=True,
        random_state=0).fit(X, y)
    # CSR keeps every NaN as a stored entry (and drops the zeros)
    Xs = sp.csr_matrix(X)
    assert np.isnan(Xs.data).sum() == np.isnan(X).sum() > 0
    went_left = 0
    for t in trees_of(m):
        a, b = t.apply(X), t.apply(Xs)
        np.testing.assert_array_equal(a, b)
        flagless = HistTree(t.feature, t.threshold, t.left, t.right, t.value,
                            None, t.n_features_in_, None)
        went_left += int((flagless.apply(X) != a).sum())
    assert went_left > 0          # the flags changed some row's path
    np.testing.assert_array_equal(m.predict_proba(X), m.predict_proba(Xs))


def test_sklearn_flatten_carries_missing_go_to_left():
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(0)
    X = rng.standard_normal((800, 6)).astype(np.float32)
    y = ((X[:, 0] > 0) ^ (X[:, 2] > 0.5)).astype(np.int64)
    X = holes(X, 0.2, 1)
    y[np.isnan(X[:, 0])] = 1
    rf = RandomForestClassifier(n_estimators=6, max_depth=5,
                                random_state=0).fit(X, y)
    rows = np.isnan(X).any(axis=1)
    assert rows.sum() > 100
    n_left = n_wrong = 0
    for est in rf.estimators_:
        mg = est.tree_.missing_go_to_left
        inner = est.tree_.feature >= 0
        n_left += int(mg[inner].sum())
        ht = _sklearn_tree_to_hist_tree(est, "proba")
        np.testing.assert_array_equal(ht.missing_left[inner], mg[inner])
        np.testing.assert_allclose(ht.predict_proba(X[rows]),
                                   est.predict_proba(X[rows]),
                                   atol=1e-6, rtol=0)
        np.testing.assert_array_equal(ht.apply(X), est.apply(X))
        ht.missing_left = None     # what the flatten did before
        n_wrong += int((ht.apply(X) != est.apply(X)).sum())
    assert n_left > 0              # precondition: some node sends NaN left
    assert n_wrong > 0             # ... and dropping the flags shows
