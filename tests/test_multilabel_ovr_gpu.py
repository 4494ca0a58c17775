"""
Multilabel one-vs-rest end to end on the device: the HIP solve (bit planes,
k_fwd_gt_bits) against the eager mirror of the same fit, device multilabel
``predict`` against the host loop, and sparse X.
"""

import numpy as np
import pytest
import scipy.sparse as sp

from skdist_amd import Cluster
from skdist_amd.distribute.multiclass import (
    DistOneVsRestClassifier,
    _ConstantPredictor,
)
from skdist_amd.models import LinearSVC, LogisticRegression

pytestmark = pytest.mark.gpu

N, F, L = 4000, 16, 6


@pytest.fixture(scope="module")
def data():
    """6 labels of different frequency, label 4 all-zero; noisy linear."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N, F)).astype(np.float32)
    Wt = rng.standard_normal((F, L))
    bias = np.array([0.0, 1.0, -1.0, 0.5, 0.0, -1.5]) * np.sqrt(F)
    Y = ((X @ Wt + 0.5 * rng.standard_normal((N, L)) + bias) > 0).astype(int)
    Y[:, 4] = 0
    assert all(0 < Y[:, j].sum() < N for j in (0, 1, 2, 3, 5))
    return X, Y


def _fit(make, X, Y, **kw):
    return DistOneVsRestClassifier(make(), sc=Cluster(), **kw).fit(X, Y)


def _fit_eager(monkeypatch, make, X, Y, **kw):
    import skdist_amd.models._sgd as sgd_mod

    with monkeypatch.context() as mp:
        mp.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
        mp.setattr(sgd_mod, "_use_hip", lambda d: False)
        return _fit(make, X, Y, **kw)


def _host_indicator(clf, X):
    """The host loop of DistOneVsRestClassifier.predict, and its scores."""
    scores = clf._scores(X)
    thr = np.array([0.5 if hasattr(e, "predict_proba") else 0.0
                    for e in clf.estimators_])
    return (scores > thr[None, :]).astype(int), scores - thr[None, :]


def _compare(hip, ref, X):
    """The project's tolerance for a HIP fit against the eager mirror
    (tests/test_gpu_kernels.py, test_sample_weight_hip_matches_eager)."""
    assert isinstance(hip.estimators_[4], _ConstantPredictor)
    assert isinstance(ref.estimators_[4], _ConstantPredictor)
    a, _ = _host_indicator(hip, X)
    b, _ = _host_indicator(ref, X)
    agree = (a == b).mean()
    print(f"indicator agreement {agree:.5f}")
    assert agree > 0.995
    for j in (0, 1, 2, 3, 5):
        np.testing.assert_allclose(hip.estimators_[j].coef_,
                                   ref.estimators_[j].coef_,
                                   rtol=0.1, atol=0.02)
    return a


def _logistic():
    return LogisticRegression(epochs=8, random_state=0)


@pytest.fixture(scope="module")
def hip_fit(data):
    X, Y = data
    return _fit(_logistic, X, Y)


def test_hip_fit_matches_the_eager_mirror(data, hip_fit, monkeypatch):
    X, Y = data
    ref = _fit_eager(monkeypatch, _logistic, X, Y)
    ind = _compare(hip_fit, ref, X)
    assert (ind[:, 4] == 0).all()
    assert (ind == Y).mean() > 0.9             # the fit learned the labels


def test_max_negatives_hip_fit_matches_the_eager_mirror(data, monkeypatch):
    X, Y = data
    kw = dict(max_negatives=0.25, random_state=3)
    seen = []
    import skdist_amd.models.linear as lin

    real = lin.batched_sgd_fit
    monkeypatch.setattr(
        lin, "batched_sgd_fit",
        lambda ds, spec, *a, **k: (seen.append(spec),
                                   real(ds, spec, *a, **k))[1])
    hip = _fit(_logistic, X, Y, **kw)
    ref = _fit_eager(monkeypatch, _logistic, X, Y, **kw)
    assert len(seen) == 2 and all(s.train_mask is not None for s in seen)
    assert 0.2 < float(seen[0].train_mask.float().mean()) < 0.9
    _compare(hip, ref, X)


def test_linear_svc_hip_fit_matches_the_eager_mirror(data, monkeypatch):
    X, Y = data
    make = lambda: LinearSVC(epochs=8, random_state=0)
    _compare(_fit(make, X, Y), _fit_eager(monkeypatch, make, X, Y), X)


def test_device_multilabel_predict_equals_the_host_loop(data, hip_fit):
    X, Y = data
    want, margin = _host_indicator(hip_fit, X)
    sure = np.abs(margin) > 1e-4
    # on the host scores alone: rows near a threshold are rare
    unsure_rows = (~sure).any(axis=1).mean()
    assert unsure_rows < 0.01, unsure_rows
    fn = hip_fit._device_predict_fn("predict", "cuda")
    assert fn is not None
    got = fn(X)
    assert got.shape == want.shape and got.dtype.kind == "i"
    assert np.array_equal(got[sure], want[sure])
    assert (got[:, 4] == 0).all()
    # predict takes the device route and returns the same indicator
    assert np.array_equal(hip_fit.predict(X), got)


def test_sparse_x_densifies_or_falls_back(data, monkeypatch):
    X, Y = data
    Xs = sp.csr_matrix(np.where(np.abs(X[:600]) > 0.5, X[:600], 0.0)
                       .astype(np.float32))
    Ys = Y[:600]
    calls = {"run": 0, "specs": []}
    import skdist_amd.models.linear as lin

    real_fit, real_run = lin.batched_sgd_fit, Cluster.run_tasks
    monkeypatch.setattr(
        lin, "batched_sgd_fit",
        lambda ds, spec, *a, **k: (calls["specs"].append(spec),
                                   real_fit(ds, spec, *a, **k))[1])

    def run(cluster, fn, tasks):
        calls["run"] += 1
        return real_run(cluster, fn, tasks)

    monkeypatch.setattr(Cluster, "run_tasks", run)
    a = _fit(_logistic, Xs, Ys)
    assert calls["run"] == 0 and calls["specs"][0].targets is not None
    assert (a.predict(Xs) == Ys).mean() > 0.8

    monkeypatch.setenv("SKDIST_AMD_FORCE_SPARSE", "1")
    b = _fit(_logistic, Xs, Ys)
    assert calls["run"] == 1                   # the generic path, no error
    assert b.multilabel_ and len(b.estimators_) == L
    assert (b.predict(Xs) == Ys).mean() > 0.8
