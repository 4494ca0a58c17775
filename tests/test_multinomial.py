"""
Multinomial (softmax) LogisticRegression on the CPU path: the eager solver
is the numerics reference of the HIP kernel (tests/test_multinomial_gpu.py).
"""

import pickle

import numpy as np
import pytest
import torch
from sklearn.datasets import load_breast_cancer, load_digits, load_iris

import _softmax_ref as S

from skdist_amd.distribute.eliminate import DistFeatureEliminator
from skdist_amd.distribute.search import DistGridSearchCV
from skdist_amd.models import LogisticRegression
from skdist_amd.models._sgd import (
    LOSS_SOFTMAX,
    ColumnSpec,
    DeviceDataset,
    batched_sgd_fit,
)
from skdist_amd.parallel import Cluster


def _fit(name, multi_class):
    X, y = S.load(name)
    return LogisticRegression(
        C=0.1, multi_class=multi_class, epochs=400, batch_size=8192,
        random_state=0).fit(X, y)


# ---- 1. agreement with sklearn ------------------------------------- #

@pytest.mark.parametrize("name", ["iris", "wine"])
def test_matches_sklearn_multinomial(name):
    X, y = S.load(name)
    P_sk, P_sk_ovr = S.sklearn_probas(name)
    # what is being told apart, from sklearn alone
    assert np.abs(P_sk - P_sk_ovr).max() >= 0.115

    est = _fit(name, "multinomial")
    P = est.predict_proba(X)
    K, f = len(np.unique(y)), X.shape[1]
    assert est.coef_.shape == (K, f) and est.intercept_.shape == (K,)
    d = np.abs(P - P_sk).max()
    print(f"{name}: max|P - P_sklearn| = {d:.3e}")
    assert d <= 1e-4, d
    np.testing.assert_allclose(P.sum(axis=1), 1.0, atol=1e-6)
    assert np.array_equal(est.predict(X), est.classes_[P.argmax(axis=1)])
    np.testing.assert_allclose(
        est.predict_log_proba(X), np.log(P), atol=1e-12)
    P_ovr = _fit(name, "ovr").predict_proba(X)
    assert np.abs(P - P_ovr).max() > 0.05


# ---- 2. default and binary unchanged ------------------------------- #

def test_default_is_ovr_bit_for_bit():
    X, y = load_digits(return_X_y=True)
    a = LogisticRegression(epochs=5, random_state=0).fit(X, y)
    b = LogisticRegression(epochs=5, random_state=0,
                           multi_class="ovr").fit(X, y)
    assert a.get_params()["multi_class"] == "ovr"
    assert np.array_equal(a.coef_, b.coef_)
    assert np.array_equal(a.intercept_, b.intercept_)
    assert np.array_equal(a.predict_proba(X), b.predict_proba(X))


def test_binary_multinomial_is_the_sigmoid_column():
    X, y = load_breast_cancer(return_X_y=True)
    a = LogisticRegression(epochs=5, random_state=0).fit(X, y)
    b = LogisticRegression(epochs=5, random_state=0,
                           multi_class="multinomial").fit(X, y)
    assert b.coef_.shape == (1, X.shape[1])
    assert np.array_equal(a.coef_, b.coef_)
    assert np.array_equal(a.intercept_, b.intercept_)
    assert np.array_equal(a.predict_proba(X), b.predict_proba(X))


# ---- 3. groups are independent models ------------------------------ #

def _eager_solve(ds, folds, l2s, K, l1=None):
    nm = len(folds)
    spec = ColumnSpec(
        ds.device,
        col_fold=np.repeat(np.asarray(folds, np.int32), K),
        col_class=np.tile(np.arange(K, dtype=np.int32), nm),
        col_lr=np.full(nm * K, 0.5, np.float32),
        col_l2=np.repeat(np.asarray(l2s, np.float32), K),
        col_l1=None if l1 is None else np.full(nm * K, l1, np.float32),
        group_k=K)
    return batched_sgd_fit(ds, spec, LOSS_SOFTMAX, epochs=3, batch_size=64,
                           seed=0, momentum=0.9,
                           force_eager=True).numpy()


def test_groups_in_one_solve_are_independent():
    X, y = load_iris(return_X_y=True)
    ds = DeviceDataset(X, y, device="cpu")
    ds.fold_id = torch.as_tensor(np.arange(len(y)) % 3, dtype=torch.int32)
    both = _eager_solve(ds, [0, 2], [1e-3, 1e-1], 3)
    one = _eager_solve(ds, [0], [1e-3], 3)
    two = _eager_solve(ds, [2], [1e-1], 3)
    assert both.shape == (ds.fa, 6)
    np.testing.assert_allclose(both[:, :3], one, atol=1e-6)
    np.testing.assert_allclose(both[:, 3:], two, atol=1e-6)
    assert np.abs(one - two).max() > 1e-2     # they are different models
    # softmax gradients of a group sum to 0 over its classes, and so does
    # the L2 term of a solve started at 0: the columns of a model cancel
    assert np.abs(one.sum(axis=1)).max() < 1e-5


# ---- 4. search path ------------------------------------------------ #

def test_grid_search_batched_matches_generic():
    """The batched path is not the generic path's objective to the letter,
    for any loss: it standardises on all rows where a generic task
    standardises on its training fold, and it divides a batch's gradient
    by the batch's row count, held-out rows included, which at cv=3 makes
    its C act like 2/3 C.  The two agree where the CV curve is flat against
    a factor 1.5 in C, so the grid brackets the log-loss optimum of digits
    (C about 0.5 in standardised space) within a factor 2 each way, and
    both paths run to convergence (300 full-batch steps)."""
    X, y = load_digits(return_X_y=True)
    grid = {"C": [0.25, 0.5, 1.0]}
    est = LogisticRegression(multi_class="multinomial", epochs=300,
                             random_state=0)
    generic = DistGridSearchCV(est, grid, cv=3, scoring="neg_log_loss")
    generic.fit(X, y)
    batched = DistGridSearchCV(est, grid, cv=3, scoring="neg_log_loss",
                               sc=Cluster())
    batched.fit(X, y)
    a = generic.cv_results_["mean_test_score"]
    b = batched.cv_results_["mean_test_score"]
    print("generic", a, "batched", b)
    assert np.allclose(a, b, atol=0.02), (a, b)
    best = batched.best_estimator_
    assert best.multi_class == "multinomial"
    assert best.coef_.shape == (10, 64)
    direct = LogisticRegression(
        multi_class="multinomial", epochs=300, random_state=0,
        **batched.best_params_).fit(X, y)
    np.testing.assert_allclose(best.predict_proba(X),
                               direct.predict_proba(X), atol=1e-4)
    assert np.array_equal(best.predict(X), direct.predict(X))
    # the refit column came out of the joint solve: softmax probabilities,
    # not row-normalised sigmoids
    z = best.decision_function(X)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    np.testing.assert_allclose(best.predict_proba(X),
                               e / e.sum(axis=1, keepdims=True), atol=1e-12)


def test_multi_class_in_a_grid_takes_the_generic_path():
    from skdist_amd.models.linear import FallbackToGeneric

    X, y = load_iris(return_X_y=True)
    est = LogisticRegression(epochs=20, random_state=0)
    grid = {"multi_class": ["ovr", "multinomial"]}
    with pytest.raises(FallbackToGeneric, match="multi_class"):
        est.batched_cv_fit_score(
            X, y, [{"multi_class": "ovr"}, {"multi_class": "multinomial"}],
            [], "neg_log_loss", None, None)
    gs = DistGridSearchCV(est, grid, cv=3, scoring="neg_log_loss",
                          sc=Cluster())
    gs.fit(X, y)
    scores = gs.cv_results_["mean_test_score"]
    assert len(scores) == 2 and np.isfinite(scores).all()
    assert scores[0] != scores[1]


# ---- 5. eliminate path --------------------------------------------- #

def test_feature_eliminator_with_a_multinomial_base():
    X, y = load_iris(return_X_y=True)
    rng = np.random.default_rng(0)
    X = np.hstack([X, rng.standard_normal((len(y), 3))])
    out = {}
    for mc in ("ovr", "multinomial"):
        el = DistFeatureEliminator(
            LogisticRegression(epochs=20, random_state=0, multi_class=mc),
            sc=Cluster(), min_features_to_select=2, step=2, cv=3)
        el.fit(X, y)
        out[mc] = el
    a, b = out["ovr"], out["multinomial"]
    assert type(b.best_features_) is type(a.best_features_)
    assert np.asarray(b.scores_).shape == np.asarray(a.scores_).shape
    assert np.isfinite(np.asarray(b.scores_, dtype=float)).all()
    assert b.best_estimator_.multi_class == "multinomial"
    assert b.best_estimator_.coef_.shape == (3, len(b.best_features_))
    assert b.predict(X).shape == (len(y),)
    assert b.best_score_ > 0.8


# ---- 6. composition ------------------------------------------------ #

def test_l1_gives_exact_zeros():
    X, y = load_digits(return_X_y=True)
    est = LogisticRegression(C=0.02, penalty="l1", epochs=60,
                             multi_class="multinomial",
                             random_state=0).fit(X, y)
    zeros = (est.coef_ == 0.0).mean()
    alive = X.std(axis=0) > 0
    assert (est.coef_[:, alive] == 0.0).any() and zeros < 1.0
    assert (est.predict(X) == y).mean() > 0.85


def test_sample_weight_zero_rows_have_no_influence():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((900, 8)).astype(np.float32)
    y = (X[:, :3] @ rng.standard_normal((3, 4))).argmax(axis=1)
    w = np.ones(900)
    w[::5] = 0.0
    y_bad = y.copy()
    y_bad[::5] = (y_bad[::5] + 1) % 4
    kw = dict(epochs=8, random_state=0, multi_class="multinomial")
    a = LogisticRegression(**kw).fit(X, y, sample_weight=w)
    b = LogisticRegression(**kw).fit(X, y_bad, sample_weight=w)
    np.testing.assert_allclose(a.coef_, b.coef_, atol=1e-7)
    np.testing.assert_allclose(a.intercept_, b.intercept_, atol=1e-7)
    c = LogisticRegression(**kw).fit(X, y)
    assert np.abs(a.coef_ - c.coef_).max() > 1e-4


def test_class_weight_and_lr_decay_compose():
    X, y = S.load("wine")
    est = LogisticRegression(multi_class="multinomial", epochs=40,
                             class_weight="balanced", lr_decay=0.05,
                             momentum=0.5, random_state=0).fit(X, y)
    assert (est.predict(X) == y).mean() > 0.95


def test_pickle_round_trip_and_old_pickles():
    X, y = load_iris(return_X_y=True)
    est = LogisticRegression(multi_class="multinomial", epochs=30,
                             random_state=0).fit(X, y)
    back = pickle.loads(pickle.dumps(est))
    assert back.multi_class == "multinomial"
    assert np.array_equal(back.predict_proba(X), est.predict_proba(X))
    # an estimator pickled before the parameter existed has no attribute
    old = LogisticRegression(epochs=30, random_state=0).fit(X, y)
    want = old.predict_proba(X)
    del old.__dict__["multi_class"]
    old = pickle.loads(pickle.dumps(old))
    assert np.array_equal(old.predict_proba(X), want)
    old.fit(X, y)
    assert np.array_equal(old.predict_proba(X), want)


@pytest.mark.parametrize("bad", ["auto", "softmax", None, 3])
def test_bad_multi_class_raises_at_fit(bad):
    X, y = load_iris(return_X_y=True)
    est = LogisticRegression(multi_class=bad)     # not at construction
    with pytest.raises(ValueError, match="multi_class"):
        est.fit(X, y)


def test_column_spec_rejects_malformed_groups():
    def spec(fold, cls, gk, cls2=None):
        n = len(fold)
        return ColumnSpec("cpu", np.asarray(fold, np.int32),
                          np.asarray(cls, np.int32), np.ones(n, np.float32),
                          np.zeros(n, np.float32), col_class2=cls2,
                          group_k=gk)

    ok = spec([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2], 3)
    assert ok.group_k == 3 and ok.ncols == 6
    assert spec([0], [1], None).group_k is None
    with pytest.raises(ValueError, match="multiple"):
        spec([0, 0, 0, 1], [0, 1, 2, 0], 3)
    with pytest.raises(ValueError, match="col_class"):
        spec([0, 0, 0], [0, 2, 1], 3)
    with pytest.raises(ValueError, match="col_class"):
        spec([0, 0, 0], [1, 2, 3], 3)
    with pytest.raises(ValueError, match="col_fold"):
        spec([0, 0, 1], [0, 1, 2], 3)
    with pytest.raises(ValueError, match="one-vs-one"):
        spec([0, 0, 0], [0, 1, 2], 3, cls2=np.array([-1, 0, -1], np.int32))
    with pytest.raises(ValueError, match="group_k"):
        spec([0, 0], [0, 1], 1)
    with pytest.raises(ValueError, match="group_k"):
        spec([0, 0], [0, 1], 2.0)
    # loss and groups go together
    X, y = load_iris(return_X_y=True)
    ds = DeviceDataset(X, y, device="cpu")
    ds.set_cv_partition([])
    with pytest.raises(ValueError, match="group_k"):
        batched_sgd_fit(ds, spec([-2] * 3, [0, 1, 2], None), LOSS_SOFTMAX,
                        1, 64, force_eager=True)
    with pytest.raises(ValueError, match="softmax"):
        batched_sgd_fit(ds, spec([-2] * 3, [0, 1, 2], 3), "log", 1, 64,
                        force_eager=True)


def test_sparse_native_route_raises(monkeypatch):
    import scipy.sparse as sp

    monkeypatch.setenv("SKDIST_AMD_FORCE_SPARSE", "1")
    X, y = load_iris(return_X_y=True)
    Xs = sp.csr_matrix(X)
    est = LogisticRegression(multi_class="multinomial", epochs=2)
    with pytest.raises(ValueError, match="not supported on the "
                                         "sparse-native solver yet"):
        est.fit(Xs, y)
    # two classes are the sigmoid column: served as before
    keep = y < 2
    est.fit(Xs[keep], y[keep])
    assert est.coef_.shape == (1, 4)
    # a small sparse input that densifies is supported
    monkeypatch.delenv("SKDIST_AMD_FORCE_SPARSE")
    est.fit(Xs, y)
    assert est.coef_.shape == (3, 4)
