"""Sparse (CSR) input for the tree family — CPU tier.

A scipy-sparse X is binned, fitted on and traversed from its CSR arrays.
Every result is asserted equal to the dense path on a separately held
ndarray, and every sparse matrix handed to the code under test is a
``NoDensify``: any ``toarray`` / ``todense`` on it fails the test.
"""

import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from skdist_amd.models.boosting import (
    HistGradientBoostingClassifier,
    HistGradientBoostingRegressor,
)
from skdist_amd.models.forest import BinnedDataset, ForestBuilder


class NoDensify(sp.csr_matrix):
    def toarray(self, *a, **k):
        raise AssertionError("densified")

    todense = toarray


def messy_csr(n, f, density=0.1, seed=0):
    """(NoDensify built from raw arrays, equivalent dense float32 array).

    The raw arrays hold an all-empty column (0; its one stored entry is
    the fully stored row's explicit 0.0), a positive-only column
    (1), a negative-only column (2), an all-empty row (5), a fully stored
    row (7), a stored explicit 0.0, an unsummed duplicate entry, rows with
    unsorted indices, and int64 ``indices``."""
    rng = np.random.default_rng(seed)
    Xd = rng.standard_normal((n, f)).astype(np.float32)
    Xd[rng.random((n, f)) >= density] = 0
    Xd[:, 0] = 0
    Xd[:, 1] = np.abs(Xd[:, 1])
    Xd[:, 2] = -np.abs(Xd[:, 2])
    Xd[5] = 0
    Xd[7] = rng.standard_normal(f).astype(np.float32)
    Xd[7, 0] = 0
    Xd[7, 1] = abs(Xd[7, 1])
    Xd[7, 2] = -abs(Xd[7, 2])
    Xd[9, 3] = 0.75          # rows 9..11 carry the hand-made entries
    Xd[10, 4] = 0.0
    data, indices, indptr = [], [], [0]
    for i in range(n):
        cols = list(np.flatnonzero(Xd[i]))
        vals = [float(Xd[i, j]) for j in cols]
        if i == 7:           # fully stored row, zero in column 0 explicit
            cols = list(range(f))
            vals = [float(v) for v in Xd[7]]
        if i == 9:           # unsummed duplicate: 0.5 + 0.25 = 0.75
            k = cols.index(3)
            vals[k] = 0.5
            cols.append(3)
            vals.append(0.25)
        if i == 10:          # stored explicit zero
            cols.append(4)
            vals.append(0.0)
        if i % 3 == 0:       # unsorted indices
            cols, vals = cols[::-1], vals[::-1]
        indices.extend(cols)
        data.extend(vals)
        indptr.append(len(indices))
    X = NoDensify(
        (np.asarray(data, dtype=np.float32),
         np.asarray(indices, dtype=np.int64),
         np.asarray(indptr, dtype=np.int64)),
        shape=(n, f))
    return X, Xd


def labels(Xd, seed=0):
    rng = np.random.default_rng(seed)
    s = Xd[:, 1] + Xd[:, 2] + Xd[:, 3] - Xd[:, 4]
    return (s + 0.1 * rng.standard_normal(len(Xd)) > 0).astype(np.int64)


BIN_CASES = [
    # (n, f, max_bin_sample)
    (1237, 9, 200_000),
    (1237, 9, 500),        # the subsample branch
    (130, 4101, 200_000),  # wide: fp = 4104
]


def binned_pair(n, f, mbs, device):
    X, Xd = messy_csr(n, f)
    y = labels(Xd)
    raw = (X.data.tobytes(), X.indices.tobytes(), X.indptr.tobytes())
    a = BinnedDataset(X, y, device, is_cls=True, max_bin_sample=mbs,
                      seed=3)
    assert raw == (X.data.tobytes(), X.indices.tobytes(),
                   X.indptr.tobytes()), "caller's matrix was mutated"
    b = BinnedDataset(Xd, y, device, is_cls=True, max_bin_sample=mbs,
                      seed=3)
    return a, b, X, Xd, y


def assert_same_trees(ta, tb):
    assert len(ta) == len(tb)
    for a, b in zip(ta, tb):
        for name in ("feature", "threshold", "left", "right", "value"):
            np.testing.assert_array_equal(
                getattr(a, name), getattr(b, name), err_msg=name)


@pytest.mark.parametrize("n,f,mbs", BIN_CASES)
def test_binning_identity(n, f, mbs):
    a, b, _, _, _ = binned_pair(n, f, mbs, "cpu")
    assert a.fp == b.fp == (f + 3) // 4 * 4
    np.testing.assert_array_equal(a.edges.numpy(), b.edges.numpy())
    np.testing.assert_array_equal(a.codes.numpy(), b.codes.numpy())


@pytest.fixture(scope="module")
def cpu_trees():
    a, b, X, Xd, _ = binned_pair(1237, 9, 200_000, "cpu")
    kw = dict(max_depth=6, bootstrap=False)
    ta = ForestBuilder(a, "gini", **kw).build([3, 17, 42])
    tb = ForestBuilder(b, "gini", **kw).build([3, 17, 42])
    return ta, tb, X, Xd


def test_builder_identity(cpu_trees):
    ta, tb, _, _ = cpu_trees
    assert max(t.node_count for t in tb) > 3
    assert_same_trees(ta, tb)


def test_host_traversal(cpu_trees):
    ta, _, X, Xd = cpu_trees
    for t in ta:
        np.testing.assert_array_equal(t.apply(X), t.apply(Xd))
        np.testing.assert_array_equal(t.predict_proba(X),
                                      t.predict_proba(Xd))


def boost_data():
    rng = np.random.default_rng(0)
    Xd = rng.standard_normal((1500, 24)).astype(np.float32)
    Xd[rng.random((1500, 24)) < 0.85] = 0
    yc = (Xd[:, 0] - Xd[:, 1] + 0.5 * Xd[:, 2] > 0.2).astype(int)
    yr = (Xd[:, 0] - Xd[:, 1] + 0.5 * Xd[:, 2]).astype(np.float32)
    return NoDensify(sp.csr_matrix(Xd)), Xd, yc, yr


@pytest.mark.parametrize("kind", ["classifier", "regressor"])
def test_boosted_fit_identity(kind):
    X, Xd, yc, yr = boost_data()
    if kind == "classifier":
        make = lambda: HistGradientBoostingClassifier(
            n_estimators=8, random_state=0)
        y = yc
    else:
        make = lambda: HistGradientBoostingRegressor(
            n_estimators=8, random_state=0)
        y = yr
    ms = make().fit(X, y)
    md = make().fit(Xd, y)
    assert ms.n_features_in_ == md.n_features_in_ == 24
    assert len(ms.stages_) == len(md.stages_) == 8
    for sa, sb in zip(ms.stages_, md.stages_):
        assert_same_trees(sa, sb)
    if kind == "classifier":
        np.testing.assert_array_equal(ms.predict_proba(X),
                                      ms.predict_proba(Xd))
    np.testing.assert_array_equal(ms.predict(X), md.predict(Xd))
    for pa, pb in zip(ms.staged_predict(X), md.staged_predict(Xd)):
        np.testing.assert_array_equal(pa, pb)


def test_size_guard():
    X = NoDensify((70_000, 2 ** 20), dtype=np.float32)
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="SKDIST_AMD_DENSIFY_GB"):
        BinnedDataset(X, np.zeros(70_000), "cpu", is_cls=False)
    # raised before anything of that size was allocated or filled
    assert time.perf_counter() - t0 < 1.0


def test_out_of_range_column():
    X = NoDensify((3, 4), dtype=np.float32)
    X.data = np.array([1.0, 2.0], dtype=np.float32)
    X.indices = np.array([1, 4], dtype=np.int32)   # 4 >= f
    X.indptr = np.array([0, 1, 2, 2], dtype=np.int32)
    with pytest.raises(ValueError, match="column index"):
        BinnedDataset(X, np.zeros(3), "cpu", is_cls=False)


def test_feature_count_mismatch_raises():
    X, Xd, yc, _ = boost_data()
    m = HistGradientBoostingClassifier(n_estimators=2, random_state=0)
    m.fit(X, yc)
    with pytest.raises(ValueError, match="features"):
        m.predict_proba(NoDensify(sp.csr_matrix(Xd[:, :20])))
