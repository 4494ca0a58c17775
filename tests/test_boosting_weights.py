"""sample_weight / class_weight for the boosted family (CPU tier).

Every fit here is pinned to the CPU (``sc=Cluster(device="cpu")``), also
on a machine with a GPU: the CPU path runs the builder's eager mirror,
which is sequential and deterministic, so exact comparisons are legitimate
here and nowhere else.  The bars against
sklearn are the margins tests/test_boosting.py already uses (0.03) and the
class-weight effect margin of test_class_weight_through_hip_weight_plane
(0.05)."""

import functools
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.ensemble import GradientBoostingClassifier as SkGBC
from sklearn.ensemble import GradientBoostingRegressor as SkGBR
from sklearn.metrics import balanced_accuracy_score, r2_score, recall_score
from sklearn.utils.class_weight import compute_sample_weight

from skdist_amd import Cluster
from skdist_amd.distribute.search import DistGridSearchCV
from skdist_amd.models import (
    HistGradientBoostingClassifier,
    HistGradientBoostingRegressor,
)


def _cpu():
    return Cluster(device="cpu")


def _label(X, noise):
    return (2 * X[:, 0] - 2.8 + 0.5 * noise > 0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _imbalanced():
    """The imbalanced data set (~8% positives) and a 4000-row holdout."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((3000, 8)).astype(np.float32)
    y = _label(X, rng.standard_normal(3000))
    Xh = rng.standard_normal((4000, 8)).astype(np.float32)
    yh = _label(Xh, rng.standard_normal(4000))
    return X, y, Xh, yh


@functools.lru_cache(maxsize=None)
def _unweighted_fit():
    X, y, _, _ = _imbalanced()
    return HistGradientBoostingClassifier(
        n_estimators=30, random_state=0, sc=_cpu()).fit(X, y)


def _clf(**kw):
    kw.setdefault("n_estimators", 12)
    kw.setdefault("random_state", 0)
    kw.setdefault("sc", _cpu())
    return HistGradientBoostingClassifier(**kw)


def _sparse_informative(m, seed):
    """Zero-inflated rows whose label depends on EVERY feature, so that
    no split has to choose among pure-noise candidates."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, 8)).astype(np.float32)
    X[np.abs(X) < 0.6] = 0.0
    w = np.array([2.0, 1.5, -1.2, 1.0, -0.8, 0.7, -0.6, 0.5])
    y = (X @ w + 0.3 * rng.standard_normal(m) > 2.5).astype(np.int64)
    return X, y


# ---------------------------------------------------------------------- #
# 1-3: quality against sklearn with the same weights
# ---------------------------------------------------------------------- #
def test_weighted_classifier_matches_sklearn_recall():
    X, y, Xh, yh = _imbalanced()
    assert 0.05 < y.mean() < 0.12
    sw = compute_sample_weight("balanced", y)
    ours = HistGradientBoostingClassifier(
        n_estimators=30, random_state=0, sc=_cpu()).fit(
            X, y, sample_weight=sw)
    sk = SkGBC(n_estimators=30, random_state=0).fit(X, y, sample_weight=sw)
    r_ours = recall_score(yh, ours.predict(Xh))
    r_sk = recall_score(yh, sk.predict(Xh))
    r_unw = recall_score(yh, _unweighted_fit().predict(Xh))
    print("recall ours", r_ours, "sklearn", r_sk, "ours unweighted", r_unw)
    assert r_ours >= r_sk - 0.03, (r_ours, r_sk)
    assert r_ours >= r_unw + 0.05, (r_ours, r_unw)


def test_weighted_regressor_matches_sklearn_r2():
    X = _imbalanced()[0]
    n = len(X)
    half = np.arange(n) < n // 2
    t = np.where(half, 2 * X[:, 0] + np.abs(X[:, 1]), -X[:, 0] + X[:, 2])
    sw = np.where(half, 8.0, 0.125)
    ours = HistGradientBoostingRegressor(
        n_estimators=40, random_state=0, sc=_cpu()).fit(
            X, t, sample_weight=sw)
    sk = SkGBR(n_estimators=40, random_state=0).fit(X, t, sample_weight=sw)
    r_ours = r2_score(t, ours.predict(X), sample_weight=sw)
    r_sk = r2_score(t, sk.predict(X), sample_weight=sw)
    print("weighted R2 ours", r_ours, "sklearn", r_sk)
    assert r_ours >= r_sk - 0.03, (r_ours, r_sk)


def test_weighted_multiclass_matches_sklearn_balanced_accuracy():
    rng = np.random.default_rng(0)

    def make(m):
        X = rng.standard_normal((m, 8)).astype(np.float32)
        s = X[:, 0] + 0.5 * X[:, 1] + 0.5 * rng.standard_normal(m)
        return X, s

    X, s = make(3000)
    cuts = np.quantile(s, [0.70, 0.95])      # shares 70 / 25 / 5
    y = np.searchsorted(cuts, s)
    Xh, sh = make(4000)
    yh = np.searchsorted(cuts, sh)
    sw = compute_sample_weight("balanced", y)
    ours = HistGradientBoostingClassifier(
        n_estimators=30, random_state=0, sc=_cpu()).fit(
            X, y, sample_weight=sw)
    sk = SkGBC(n_estimators=30, random_state=0).fit(X, y, sample_weight=sw)
    b_ours = balanced_accuracy_score(yh, ours.predict(Xh))
    b_sk = balanced_accuracy_score(yh, sk.predict(Xh))
    print("balanced accuracy ours", b_ours, "sklearn", b_sk)
    assert b_ours >= b_sk - 0.03, (b_ours, b_sk)


# ---------------------------------------------------------------------- #
# 4: exact invariances
# ---------------------------------------------------------------------- #
@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_uniform_weight_equals_unweighted(scale):
    X, y, Xh, _ = _imbalanced()
    m = HistGradientBoostingClassifier(
        n_estimators=30, random_state=0, sc=_cpu()).fit(
            X, y, sample_weight=np.full(len(X), scale))
    d = np.abs(m.predict_proba(Xh) - _unweighted_fit().predict_proba(Xh))
    assert d.max() == 0.0, d.max()


def test_zero_weight_rows_do_not_matter():
    X, y, Xh, _ = _imbalanced()
    rng = np.random.default_rng(1)
    n = len(X)
    sw = rng.integers(1, 9, n) / 4.0
    zero = rng.random(n) < 0.3
    sw[zero] = 0.0
    y2 = y.copy()
    y2[zero] = 1 - y2[zero]
    a = _clf().fit(X, y, sample_weight=sw)
    b = _clf().fit(X, y2, sample_weight=sw)
    d = np.abs(a.predict_proba(Xh) - b.predict_proba(Xh))
    assert d.max() == 0.0, d.max()
    # and the weights are not ignored
    c = _clf().fit(X, y)
    assert np.abs(a.predict_proba(Xh) - c.predict_proba(Xh)).max() > 0


# ---------------------------------------------------------------------- #
# 5: class_weight
# ---------------------------------------------------------------------- #
def test_class_weight_balanced_equals_sample_weight():
    X, y, Xh, _ = _imbalanced()
    a = _clf(class_weight="balanced").fit(X, y)
    b = _clf().fit(X, y, sample_weight=compute_sample_weight("balanced", y))
    np.testing.assert_array_equal(a.predict_proba(Xh), b.predict_proba(Xh))
    assert a.get_params()["class_weight"] == "balanced"
    assert "class_weight" not in HistGradientBoostingRegressor().get_params()


def test_class_weight_dict_times_sample_weight():
    X, y, Xh, _ = _imbalanced()
    sw = np.random.default_rng(2).uniform(0.5, 2.0, len(X))
    cw = {0: 1.0, 1: 6.0}
    a = _clf(class_weight=cw).fit(X, y, sample_weight=sw)
    b = _clf().fit(X, y, sample_weight=sw * compute_sample_weight(cw, y))
    np.testing.assert_array_equal(a.predict_proba(Xh), b.predict_proba(Xh))


# ---------------------------------------------------------------------- #
# 6: CSR input
# ---------------------------------------------------------------------- #
def test_csr_with_weights_equals_dense():
    Xs, y = _sparse_informative(3000, 3)
    Xhs, _ = _sparse_informative(4000, 4)
    assert 0.03 < y.mean() < 0.3
    sw = compute_sample_weight("balanced", y)
    a = _clf().fit(Xs, y, sample_weight=sw)
    b = _clf().fit(sp.csr_matrix(Xs), y, sample_weight=sw)
    np.testing.assert_array_equal(a.predict_proba(Xhs),
                                  b.predict_proba(sp.csr_matrix(Xhs)))
    np.testing.assert_array_equal(a.predict_proba(Xhs),
                                  b.predict_proba(Xhs))


# ---------------------------------------------------------------------- #
# 7: search + pickling
# ---------------------------------------------------------------------- #
def test_weighted_search_and_pickle():
    X, y, Xh, _ = _imbalanced()
    sw = compute_sample_weight("balanced", y)
    gs = DistGridSearchCV(
        HistGradientBoostingClassifier(n_estimators=10),
        {"max_depth": [2, 3]}, cv=3,
    ).fit(X, y, sample_weight=sw)
    assert np.isfinite(gs.best_score_)
    m = gs.best_estimator_
    m2 = pickle.loads(pickle.dumps(m))
    np.testing.assert_array_equal(m.predict_proba(Xh), m2.predict_proba(Xh))
    np.testing.assert_array_equal(m.predict(Xh), m2.predict(Xh))


# ---------------------------------------------------------------------- #
# 8: validation and early stopping
# ---------------------------------------------------------------------- #
@pytest.mark.parametrize("bad", ["negative", "nan", "length", "zero"])
def test_bad_sample_weight_raises(bad):
    X, y, _, _ = _imbalanced()
    sw = np.ones(len(X))
    if bad == "negative":
        sw[3] = -1.0
    elif bad == "nan":
        sw[3] = np.nan
    elif bad == "length":
        sw = sw[:-1]
    else:
        sw[:] = 0.0
    with pytest.raises(ValueError):
        _clf(n_estimators=2).fit(X, y, sample_weight=sw)
    with pytest.raises(ValueError):
        HistGradientBoostingRegressor(n_estimators=2, sc=_cpu()).fit(
            X, y.astype(np.float64), sample_weight=sw)


def test_weighted_early_stopping():
    X, y, _, _ = _imbalanced()
    sw = compute_sample_weight("balanced", y)
    m = HistGradientBoostingClassifier(
        n_estimators=200, n_iter_no_change=5, random_state=0, sc=_cpu(),
    ).fit(X, y, sample_weight=sw)
    assert 5 <= m.n_estimators_ < 200, m.n_estimators_


def test_zero_weight_validation_slice_raises():
    X, y, _, _ = _imbalanced()
    n = len(X)
    # the held-out rows are the first entries of the fit's own permutation
    from sklearn.utils import check_random_state

    rng = check_random_state(0)
    rng.randint(1 << 31)            # the binning seed is drawn first
    val = rng.permutation(n)[: int(round(0.1 * n))]
    sw = np.ones(n)
    sw[val] = 0.0
    with pytest.raises(ValueError, match="validation"):
        HistGradientBoostingClassifier(
            n_estimators=5, n_iter_no_change=2, random_state=0, sc=_cpu(),
        ).fit(X, y, sample_weight=sw)
