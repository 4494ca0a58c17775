"""
Multilabel and ``max_negatives`` one-vs-rest on the batched solver:
``DistOneVsRestClassifier(native estimator, sc=Cluster())`` trains every
label as one column of one solve (per-element targets and train masks)
instead of one task per label.
"""

import pickle

import numpy as np
import pytest
import scipy.sparse as sp

from skdist_amd import Cluster
from skdist_amd.distribute.multiclass import (
    DistOneVsRestClassifier,
    _ConstantPredictor,
    _negatives_mask,
)
from skdist_amd.models import LinearSVC, LogisticRegression


def _wide_margin_data(n=600, f=8, labels=3, seed=0):
    """Label j is ``X[:, j] > 0`` with ``|X[:, j]| >= 0.5``: every margin
    is wide.  Rows carry 0 to ``labels`` labels."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f))
    sign = rng.integers(0, 2, size=(n, labels)) * 2 - 1
    X[:, :labels] = sign * rng.uniform(0.5, 2.0, size=(n, labels))
    X = X.astype(np.float32)
    Y = (X[:, :labels] > 0).astype(int)
    return X, Y


@pytest.fixture(scope="module")
def wide():
    X, Y = _wide_margin_data()
    per_row = Y.sum(axis=1)
    assert {0, 1, 3} <= set(per_row.tolist())
    return X, Y


class _Spy:
    """Counts ``run_tasks`` calls and keeps the specs the solver saw."""

    def __init__(self, monkeypatch):
        import skdist_amd.models.linear as lin

        self.specs, self.run_tasks = [], 0
        real_fit, real_run = lin.batched_sgd_fit, Cluster.run_tasks

        def fit(ds, spec, *a, **kw):
            self.specs.append(spec)
            return real_fit(ds, spec, *a, **kw)

        def run(cluster, fn, tasks):
            self.run_tasks += 1
            return real_run(cluster, fn, tasks)

        monkeypatch.setattr(lin, "batched_sgd_fit", fit)
        monkeypatch.setattr(Cluster, "run_tasks", run)


def _est(**kw):
    return LogisticRegression(epochs=30, batch_size=128, random_state=0, **kw)


# ------------------------------------------------------------------ #
# routing
# ------------------------------------------------------------------ #

def _tag_sets(Y):
    return [tuple(f"t{j}" for j in np.flatnonzero(r)) for r in Y]


@pytest.mark.parametrize("kind", ["indicator", "sparse", "sets",
                                  "1d_max_negatives"])
def test_batched_path_is_taken(wide, monkeypatch, kind):
    X, Y = wide
    spy = _Spy(monkeypatch)
    kw = {}
    if kind == "indicator":
        y = Y
    elif kind == "sparse":
        y = sp.csr_matrix(Y)
    elif kind == "sets":
        y = _tag_sets(Y)
    else:
        y = Y[:, 0] + 2 * Y[:, 1]          # 4 classes
        kw = dict(max_negatives=0.5, random_state=1)
    clf = DistOneVsRestClassifier(_est(), sc=Cluster(), **kw).fit(X, y)
    assert spy.run_tasks == 0
    assert len(spy.specs) == 1 and spy.specs[0].targets is not None
    assert clf.multilabel_ == (kind != "1d_max_negatives")
    assert len(clf.estimators_) == (4 if kind == "1d_max_negatives" else 3)
    if kind == "1d_max_negatives":
        assert spy.specs[0].train_mask is not None
        assert clf.label_binarizer_ is None
        assert (clf.predict(X) == y).mean() > 0.9
    else:
        assert list(clf.classes_) == [0, 1, 2]
        # the binarizer is in the state a fit on all of y leaves
        from sklearn.preprocessing import LabelBinarizer

        full = LabelBinarizer(sparse_output=True).fit(
            clf.mlb_.transform(y) if kind == "sets" else y)
        lb = clf.label_binarizer_
        assert lb.y_type_ == full.y_type_ == "multilabel-indicator"
        assert lb.sparse_input_ == full.sparse_input_
        assert np.array_equal(lb.classes_, full.classes_)
        assert np.array_equal(lb.transform(Y).toarray(),
                              full.transform(Y).toarray())


def test_class_weight_keeps_the_generic_path(wide, monkeypatch):
    X, Y = wide
    spy = _Spy(monkeypatch)
    clf = DistOneVsRestClassifier(
        _est(class_weight="balanced"), sc=Cluster()).fit(X, Y)
    assert spy.run_tasks == 1
    assert all(s.targets is None for s in spy.specs)
    assert clf.multilabel_ and len(clf.estimators_) == 3


# ------------------------------------------------------------------ #
# results
# ------------------------------------------------------------------ #

def test_one_hot_indicator_equals_the_class_target_fit_bitwise():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((500, 6)).astype(np.float32)
    y = rng.integers(0, 4, size=500)
    onehot = (y[:, None] == np.arange(4)[None, :]).astype(int)
    a = DistOneVsRestClassifier(_est(momentum=0.9), sc=Cluster()).fit(X, y)
    b = DistOneVsRestClassifier(_est(momentum=0.9), sc=Cluster()).fit(
        X, onehot)
    assert not a.multilabel_ and b.multilabel_
    for ea, eb in zip(a.estimators_, b.estimators_):
        assert np.abs(ea.coef_).max() > 1e-3
        assert np.array_equal(ea.coef_, eb.coef_)
        assert np.array_equal(ea.intercept_, eb.intercept_)
        assert list(eb.classes_) == [0, 1]


@pytest.mark.parametrize("make", [
    lambda: LogisticRegression(epochs=30, batch_size=128, random_state=0),
    lambda: LinearSVC(epochs=30, batch_size=128, random_state=0),
], ids=["logistic", "svc"])
def test_genuine_multilabel_predict_equals_the_generic_fit(wide, make):
    X, Y = wide
    generic = DistOneVsRestClassifier(make(), sc=None).fit(X, Y)
    want = generic.predict(X)
    # the generic path alone is 100% right on this data
    assert np.array_equal(want, Y)
    batched = DistOneVsRestClassifier(make(), sc=Cluster()).fit(X, Y)
    got = batched.predict(X)
    assert got.shape == Y.shape and got.dtype.kind == "i"
    assert np.array_equal(got, want)


def test_degenerate_labels_become_constant_predictors(wide):
    X, Y = wide
    n = len(Y)
    Yd = np.column_stack([Y[:, 0], np.zeros(n, int), Y[:, 1],
                          np.ones(n, int), Y[:, 2]])
    clf = DistOneVsRestClassifier(_est(), sc=Cluster()).fit(X, Yd)
    kinds = [isinstance(e, _ConstantPredictor) for e in clf.estimators_]
    assert kinds == [False, True, False, True, False]
    assert clf.estimators_[1].y_.tolist() == [0]
    assert clf.estimators_[3].y_.tolist() == [1]
    got = clf.predict(X)
    assert (got[:, 1] == 0).all() and (got[:, 3] == 1).all()
    assert np.array_equal(got, Yd)


# ------------------------------------------------------------------ #
# max_negatives
# ------------------------------------------------------------------ #

def _unbalanced(n=800, f=6, seed=2):
    """3 labels with 10%, 25% and 50% positives."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f)).astype(np.float32)
    q = np.quantile(X[:, :3], [0.9, 0.75, 0.5], axis=0)
    Y = np.column_stack([X[:, j] > q[j, j] for j in range(3)]).astype(int)
    return X, Y


@pytest.mark.parametrize("max_negatives,method", [
    (100, "ratio"), (0.3, "ratio"), (1.5, "multiplier")])
def test_max_negatives_masks_step_size_and_penalty(monkeypatch,
                                                   max_negatives, method):
    X, Y = _unbalanced()
    n = len(Y)
    spy = _Spy(monkeypatch)
    est = _est(C=2.0, lr=0.25)
    DistOneVsRestClassifier(
        est, sc=Cluster(), max_negatives=max_negatives, method=method,
        random_state=7).fit(X, Y)
    assert spy.run_tasks == 0 and len(spy.specs) == 1
    spec = spy.specs[0]
    tm = spec.train_mask.cpu().numpy()
    assert tm.shape == (n, 3)
    assert np.array_equal(spec.targets.cpu().numpy(), Y)
    lr = spec.col_lr.cpu().numpy()
    masked = 0
    for c in range(3):
        want = _negatives_mask(Y[:, c], max_negatives, method, 7)
        assert np.array_equal(tm[:, c] != 0, want), c
        assert want[Y[:, c] == 1].all()            # positives always train
        n_t = int(want.sum())
        masked += n_t < n
        assert lr[c] == np.float32(0.25 * n / n_t), c
    assert masked >= 2                             # the masks are live
    l2 = np.float32(est._lam(n)[0])
    assert (spec.col_l2.cpu().numpy() == l2).all() and l2 > 0


def test_a_cap_above_every_negative_count_needs_no_mask(monkeypatch):
    X, Y = _unbalanced()
    spy = _Spy(monkeypatch)
    DistOneVsRestClassifier(_est(lr=0.25), sc=Cluster(), max_negatives=10 ** 6,
                            random_state=7).fit(X, Y)
    spec = spy.specs[0]
    assert spec.targets is not None and spec.train_mask is None
    assert (spec.col_lr.cpu().numpy() == np.float32(0.25)).all()


# ------------------------------------------------------------------ #
# MultiLabelBinarizer round trip
# ------------------------------------------------------------------ #

def test_tag_sets_round_trip_and_pickle(wide):
    X, Y = wide
    tags = _tag_sets(Y)
    sc = Cluster()
    clf = DistOneVsRestClassifier(_est(), sc=sc).fit(X, tags)
    assert clf.sc is None and clf.mlb_ is not None
    assert all(getattr(e, "sc", None) is None for e in clf.estimators_)
    got = clf.predict(X)
    assert isinstance(got[0], tuple)
    assert [tuple(sorted(t)) for t in got] == [tuple(sorted(t)) for t in tags]
    clone = pickle.loads(pickle.dumps(clf))
    assert clone.predict(X) == got

    ind = DistOneVsRestClassifier(_est(), sc=sc, mlb_override=True).fit(X, Y)
    assert ind.mlb_ is None and ind.multilabel_
    assert np.array_equal(ind.predict(X), Y)
