"""average_precision as a device metric: the _MetricState route and the
batched search path, against sklearn's average_precision_score."""

import types

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score

import skdist_amd.models.linear as linear_mod
from skdist_amd.models import LogisticRegression
from skdist_amd.models._sgd import _MetricState

EPS = 2.0 ** -53


@pytest.mark.parametrize("tied", [False, True])
def test_metric_state_average_precision_matches_sklearn(tied):
    rng = np.random.default_rng(0)
    m, nm = 2000, 7
    z = rng.standard_normal((m, nm))
    Z = torch.as_tensor(np.round(z * 3) / 3 if tied else z,
                        dtype=torch.float32)
    y = (rng.random(m) < 0.2).astype(np.float32)
    spec = types.SimpleNamespace(col_class=torch.ones(nm, dtype=torch.int32))
    fid, mf = torch.zeros(m, dtype=torch.int32), torch.zeros(nm)
    for yy in (y, np.zeros_like(y)):    # no positives: 0.0, as in sklearn
        st = _MetricState("average_precision", nm, 2, torch.device("cpu"))
        for s in (slice(0, 900), slice(900, m)):    # two chunks accumulate
            st.update(Z[s], torch.as_tensor(yy[s]), fid[s], spec, mf, 2)
        expect = [average_precision_score(yy, Z[:, c].numpy()) if yy.any()
                  else 0.0 for c in range(nm)]
        assert np.abs(st.finalize() - expect).max() <= 2 * yy.sum() * EPS


def test_search_average_precision_batched(monkeypatch):
    """The batched solve scores every (candidate, fold) column as sklearn
    scores that column's decision values on the fold's rows; 3 classes take
    the generic path."""
    rng = np.random.default_rng(1)
    n, f = 600, 8
    X = rng.standard_normal((n, f)).astype(np.float32)
    y = (X @ rng.standard_normal(f) + rng.standard_normal(n) > 1.0).astype(int)
    fold = np.arange(n) % 3
    splits = [(np.flatnonzero(fold != k), np.flatnonzero(fold == k))
              for k in range(3)]
    seen = {}
    real = linear_mod.batched_scores_by_fold

    def spy(ds, W, model_folds, *a, **k):
        seen.update(ds=ds, W=W.to(ds.comp_dtype), mf=model_folds,
                    scores=real(ds, W, model_folds, *a, **k))
        return seen["scores"]
    monkeypatch.setattr(linear_mod, "batched_scores_by_fold", spy)
    est = LogisticRegression(epochs=5, random_state=0)
    out = est.batched_cv_fit_score(
        X, y, [{"C": 0.1}, {"C": 10.0}], splits, "average_precision", None,
        None)
    got = sorted(t["test_scores"]["score"] for t in out["tasks"])
    ds, mf = seen["ds"], seen["mf"]
    assert got == sorted(seen["scores"][mf >= 0]) and got[0] > y.mean() + 0.2
    for k in range(3):      # the scorer's own forward, fold by fold
        mids = np.flatnonzero(mf == k)
        rows = torch.nonzero(ds.fold_id == k).flatten()
        Wf = seen["W"].index_select(
            1, torch.as_tensor(mids, device=ds.device)).contiguous()
        Z = (ds.Xaug.index_select(0, rows) @ Wf).float().cpu().numpy()
        yk = y[rows.cpu().numpy()]
        expect = [average_precision_score(yk, Z[:, j]) for j in range(2)]
        assert np.abs(seen["scores"][mids] - expect).max() \
            <= 2 * yk.sum() * EPS
    with pytest.raises(linear_mod.FallbackToGeneric,
                       match="average_precision is binary only"):
        est.batched_cv_fit_score(X, np.arange(n) // 3 % 3, [{"C": 1.0}],
                                 splits, "average_precision", None, None)
