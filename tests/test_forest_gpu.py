"""GPU tests for the HIP histogram forest builder + inference kernels.

The HIP engine is asserted against the eager torch mirror (same weights,
same hash-driven feature subsampling) and against sklearn-level quality;
the flattened inference kernel is asserted against the host traversal.
"""

import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skdist_amd import Cluster
    from skdist_amd.distribute.ensemble import (
        DistExtraTreesClassifier,
        DistRandomForestClassifier,
        DistRandomForestRegressor,
        DistRandomTreesEmbedding,
    )
    from skdist_amd.distribute.predict import DistPredictor
    from skdist_amd.models.forest import (
        BinnedDataset,
        FlatForest,
        ForestBuilder,
        HistTree,
    )


def _cls_data(n=4000, f=12, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f)).astype(np.float32)
    w = rng.standard_normal(f)
    y = ((X @ w + 0.3 * rng.standard_normal(n)) > 0).astype(np.int64)
    return X, y


def test_hip_builder_matches_eager(monkeypatch):
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    X, y = _cls_data(3000, 10)
    ds = BinnedDataset(X, y, "cuda", is_cls=True)
    kw = dict(max_depth=8, max_features="sqrt", bootstrap=True,
              tree_batch=4)
    th = ForestBuilder(ds, "gini", engine="hip", **kw).build([3, 17, 42])
    te = ForestBuilder(ds, "gini", engine="eager", **kw).build([3, 17, 42])
    for a, b in zip(th, te):
        # identical split decisions up to fp32-vs-fp64 gain ties
        pa, pb = a.predict(X), b.predict(X)
        assert (pa == pb).mean() > 0.99, (a.node_count, b.node_count)
        assert abs(a.node_count - b.node_count) <= 0.1 * b.node_count


def test_hip_builder_regression_matches_eager(monkeypatch):
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    rng = np.random.default_rng(5)
    X = rng.standard_normal((2500, 8)).astype(np.float32)
    yr = (X @ rng.standard_normal(8)).astype(np.float32)
    ds = BinnedDataset(X, yr, "cuda", is_cls=False)
    kw = dict(max_depth=7, max_features=1.0, bootstrap=True, tree_batch=2)
    th = ForestBuilder(ds, "squared_error", engine="hip", **kw).build([9])
    te = ForestBuilder(ds, "squared_error", engine="eager",
                       **kw).build([9])
    pa, pb = th[0].predict(X), te[0].predict(X)
    # fp32 atomic-order rounding can flip near-tie splits
    assert np.corrcoef(pa, pb)[0, 1] > 0.99


def test_dist_forest_gpu_end_to_end():
    X, y = _cls_data()
    Xtr, Xte, ytr, yte = X[:3000], X[3000:], y[:3000], y[3000:]
    clf = DistRandomForestClassifier(
        sc=Cluster(require_gpu=True), n_estimators=24, random_state=0)
    clf.fit(Xtr, ytr)
    assert all(isinstance(t, HistTree) for t in clf.estimators_)
    acc = (clf.predict(Xte) == yte).mean()
    assert acc > 0.85, acc
    blob = pickle.dumps(clf)
    clf2 = pickle.loads(blob)
    np.testing.assert_array_equal(clf.predict(Xte), clf2.predict(Xte))
    proba = clf.predict_proba(Xte)
    np.testing.assert_allclose(proba.sum(axis=1), 1.0, atol=1e-5)


def test_dist_extratrees_gpu():
    X, y = _cls_data(3000, 10, seed=2)
    clf = DistExtraTreesClassifier(
        sc=Cluster(require_gpu=True), n_estimators=24, random_state=0)
    clf.fit(X, y)
    assert all(isinstance(t, HistTree) for t in clf.estimators_)
    assert (clf.predict(X) == y).mean() > 0.9


def test_dist_forest_regressor_gpu():
    rng = np.random.default_rng(7)
    X = rng.standard_normal((3000, 10)).astype(np.float32)
    y = (X @ rng.standard_normal(10)).astype(np.float32)
    reg = DistRandomForestRegressor(
        sc=Cluster(require_gpu=True), n_estimators=24, random_state=0)
    reg.fit(X, y)
    pred = reg.predict(X)
    r2 = 1 - ((pred - y) ** 2).sum() / ((y - y.mean()) ** 2).sum()
    assert r2 > 0.7, r2


def test_oob_score_gpu():
    X, y = _cls_data(2500, 10, seed=3)
    clf = DistRandomForestClassifier(
        sc=Cluster(require_gpu=True), n_estimators=30, oob_score=True,
        random_state=0)
    clf.fit(X, y)
    assert 0.7 < clf.oob_score_ <= 1.0


def test_flat_forest_matches_host():
    X, y = _cls_data(2000, 8, seed=4)
    clf = DistRandomForestClassifier(
        sc=Cluster(require_gpu=True), n_estimators=12, random_state=0)
    clf.fit(X, y)
    ff = FlatForest(clf.estimators_, "cuda")
    host = clf.predict_proba(X)
    dev = ff.predict_proba(X)
    np.testing.assert_allclose(dev, host, atol=1e-5)
    np.testing.assert_array_equal(ff.predict(X), clf.predict(X))
    # apply: tree-local leaf ids match the host traversal
    host_apply = clf.apply(X)
    np.testing.assert_array_equal(ff.apply(X), host_apply)


def test_flat_forest_matches_host_tree_walk():
    """The dense kernels against the numpy HistTree walk, tree by tree
    (257 rows: two blocks, the second with one row; 65 trees; vs = 2).

    predict sums 65 payloads in [0, 1] in f32: each add rounds by at most
    half an ulp of 64 (2^-18) and the mean divides the total by 65, so the
    worst case is 2^-18 = 3.8e-6 from the fp64 mean; atol = 1e-5."""
    X, y = _cls_data(257, 8, seed=11)
    ds = BinnedDataset(X, y, "cuda", is_cls=True)
    trees = ForestBuilder(ds, "gini", max_depth=5, bootstrap=True,
                          tree_batch=65, engine="hip").build(list(range(65)))
    assert len(trees) == 65 and trees[0].value.shape[1] == 2
    assert len({len(t.feature) for t in trees}) > 1     # trees differ
    ff = FlatForest(trees, "cuda")
    host = np.mean([t.predict_proba(X).astype(np.float64) for t in trees],
                   axis=0)
    np.testing.assert_allclose(ff.predict_value(X), host, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(
        ff.apply(X), np.column_stack([t.apply(X) for t in trees]))


def _one_split_node_arrays():
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device="cuda")
    return (t([0, -1, -1], torch.int32), t([0.0, 0.0, 0.0], torch.float32),
            t([1, 0, 1], torch.int32), t([2, 0, 0], torch.int32),
            t([0], torch.int32))


def test_forest_apply_rejects_wrong_out_width():
    from skdist_amd.ops import require_hip

    X = torch.zeros(5, 2, device="cuda")
    out = torch.empty(5, 2, dtype=torch.int32, device="cuda")   # 1 tree
    with pytest.raises(RuntimeError, match="out_leaf"):
        require_hip().forest_apply(X, *_one_split_node_arrays(), out)


def test_part_count_rejects_int64_split_feat():
    from skdist_amd.ops import require_hip

    n = 8
    dev = "cuda"
    codes = torch.zeros(n, 4, dtype=torch.uint8, device=dev)
    si = torch.arange(n, dtype=torch.int32, device=dev).view(1, n)
    chunks = torch.tensor([[0, 0, 0, n]], dtype=torch.int32, device=dev)
    split_bin = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="split_feat"):
        require_hip().part_count(
            codes, si, chunks, torch.zeros(1, dtype=torch.int64, device=dev),
            split_bin, n, counts)


def test_dist_predictor_uses_device_forest():
    X, y = _cls_data(2000, 8, seed=6)
    clf = DistRandomForestClassifier(
        sc=Cluster(require_gpu=True), n_estimators=12, random_state=0)
    clf.fit(X, y)
    pred = DistPredictor(clf, sc=None, method="predict_proba")
    out = pred(X)
    assert pred._flat is not False and pred._flat is not None
    np.testing.assert_allclose(out, clf.predict_proba(X), atol=1e-5)


def test_tree_embedding_gpu():
    rng = np.random.default_rng(8)
    X = rng.standard_normal((1500, 6)).astype(np.float32)
    emb = DistRandomTreesEmbedding(
        sc=Cluster(require_gpu=True), n_estimators=10, max_depth=4,
        random_state=0)
    T = emb.fit_transform(X)
    assert T.shape[0] == 1500
    assert all(isinstance(t, HistTree) for t in emb.estimators_)
    T2 = emb.transform(X)
    assert (T != T2).nnz == 0


def test_sklearn_forest_and_gbt_on_device():
    """Host-fitted sklearn ensembles score through the traversal kernel
    (BASELINE config 5's GBT batch-inference path)."""
    from sklearn.ensemble import (
        GradientBoostingClassifier,
        RandomForestClassifier,
    )

    from skdist_amd.models.forest import flat_forest_for

    X, y = _cls_data(3000, 10, seed=9)
    rf = RandomForestClassifier(n_estimators=20, random_state=0).fit(X, y)
    ff = flat_forest_for(rf, "cuda")
    np.testing.assert_allclose(
        ff.predict_proba(X), rf.predict_proba(X), atol=1e-5)

    gbt = GradientBoostingClassifier(
        n_estimators=25, random_state=0).fit(X, y)
    fg = flat_forest_for(gbt, "cuda")
    np.testing.assert_allclose(
        fg.predict_proba(X), gbt.predict_proba(X), atol=1e-4)
    assert (fg.predict(X) == gbt.predict(X)).mean() > 0.999

    pred = DistPredictor(gbt, sc=None, method="predict_proba")
    np.testing.assert_allclose(
        pred(X), gbt.predict_proba(X), atol=1e-4)


def test_subtraction_trick_identical_trees():
    """Sibling-subtraction histograms are exact for classification: the
    built trees must match the direct-histogram path bit-for-bit."""
    X, y = _cls_data(5000, 12, seed=11)
    ds = BinnedDataset(X, y, "cuda", is_cls=True)
    kw = dict(max_depth=9, max_features="sqrt", bootstrap=True,
              tree_batch=4)
    a = ForestBuilder(ds, "gini", subtract=True, **kw).build([5, 21])
    b = ForestBuilder(ds, "gini", subtract=False, **kw).build([5, 21])
    for ta, tb in zip(a, b):
        assert ta.node_count == tb.node_count
        np.testing.assert_array_equal(ta.feature, tb.feature)
        np.testing.assert_array_equal(ta.threshold, tb.threshold)
        np.testing.assert_array_equal(ta.left, tb.left)
        np.testing.assert_allclose(ta.value, tb.value, atol=1e-6)


def test_device_forest_sample_weight_matches_eager(monkeypatch):
    """Real-valued sample_weight through the quantized uint8 plane: HIP
    builder vs the eager mirror must produce identical trees."""
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    from skdist_amd.models.forest import BinnedDataset, ForestBuilder

    X, y = _cls_data(n=6000, f=10, seed=11)
    rng = np.random.default_rng(0)
    sw = rng.random(len(y)) + 0.5

    def build(engine):
        ds = BinnedDataset(X, y, "cuda", is_cls=True)
        b = ForestBuilder(ds, "gini", max_depth=7, min_samples_split=4,
                          min_samples_leaf=2, max_features=None,
                          extra_mode=False, bootstrap=True,
                          engine=engine)
        return b.build([5, 6], sample_weight=sw)

    t_hip = build("hip")
    t_hip2 = build("hip")
    t_eag = build("eager")
    Xq = _cls_data(n=2000, f=10, seed=12)[0]
    for a, a2, b in zip(t_hip, t_hip2, t_eag):
        # HIP is deterministic vs itself
        np.testing.assert_array_equal(a.feature, a2.feature)
        np.testing.assert_array_equal(a.value, a2.value)
        # vs eager: quantized weights make split GAINS large integers
        # squared — fp32 (kernel) vs fp64 (mirror) rounding flips
        # near-tie splits occasionally, so identity is node-level-close
        # rather than exact (integer-weight identity is asserted by
        # test_hip_builder_matches_eager)
        m = min(len(a.feature), len(b.feature))
        agree = (a.feature[:m] == b.feature[:m]).mean()
        assert agree > 0.9, agree
        pa = a.predict_proba(Xq)
        pb = b.predict_proba(Xq)
        assert (np.abs(pa - pb) < 0.05).mean() > 0.97


def test_dist_forest_class_weight_device_path():
    """class_weight='balanced' stays on the device path and shifts
    minority-class recall up (round-1: silent CPU fallback)."""
    from sklearn.metrics import recall_score

    from skdist_amd import Cluster
    from skdist_amd.distribute.ensemble import DistRandomForestClassifier

    rng = np.random.default_rng(0)
    n = 60_000
    X = rng.standard_normal((n, 16)).astype(np.float32)
    y = ((X[:, 0] * 2 - 2.6 + 0.5 * rng.standard_normal(n)) > 0).astype(
        np.int64)
    sc = Cluster(require_gpu=True)
    m0 = DistRandomForestClassifier(
        n_estimators=20, max_depth=6, random_state=0, sc=sc).fit(X, y)
    import warnings as _w

    sc2 = Cluster(require_gpu=True)
    m1 = DistRandomForestClassifier(
        n_estimators=20, max_depth=6, class_weight="balanced",
        random_state=0, sc=sc2)
    with _w.catch_warnings(record=True) as rec:
        _w.simplefilter("always")
        m1.fit(X, y)
    # stayed on the device path: no CPU-fallback warning fired
    assert not any("falling back" in str(r.message) for r in rec)
    r0 = recall_score(y, m0.predict(X))
    r1 = recall_score(y, m1.predict(X))
    assert r1 > r0
