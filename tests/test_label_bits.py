"""
Per-element targets and train masks of the batched solver
(``ColumnSpec(targets=..., train_mask=...)``) on the CPU: the eager mirror
must compute, from a one-hot target matrix, exactly what it computes from
class targets, and from a pair mask exactly what a one-vs-one column
computes -- same matmul shapes, same G values, so the same bits.
"""

import numpy as np
import pytest
import torch

from skdist_amd.models._sgd import (
    ColumnSpec,
    DeviceDataset,
    batched_sgd_fit,
)

N, F, K = 300, 7, 4


def _data():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, F)).astype(np.float32)
    y = rng.integers(0, K, size=N)
    ds = DeviceDataset(X, y, device="cpu")
    ds.set_cv_partition([])
    return ds, y


def _spec(ncols, col_class, col_class2=None, **kw):
    return ColumnSpec(
        "cpu",
        col_fold=np.full(ncols, -2, np.int32),
        col_class=np.asarray(col_class, np.int32),
        col_lr=np.linspace(0.2, 0.5, ncols).astype(np.float32),
        col_l2=np.full(ncols, 1e-3, np.float32),
        col_class2=col_class2, **kw)


def _fit(ds, spec, loss):
    return batched_sgd_fit(ds, spec, loss, epochs=2, batch_size=128,
                           seed=0, momentum=0.9)


@pytest.mark.parametrize("loss", ["log", "hinge"])
def test_one_hot_targets_equal_class_targets_bitwise(loss):
    ds, y = _data()
    onehot = y[:, None] == np.arange(K)[None, :]
    W_cls = _fit(ds, _spec(K, np.arange(K)), loss)
    # col_class is ignored once targets are set: give it a wrong class
    W_bits = _fit(ds, _spec(K, np.full(K, 1), targets=onehot), loss)
    assert W_cls.abs().max() > 1e-2
    assert (W_cls[:, 0] - W_cls[:, 1]).abs().max() > 1e-3
    assert torch.equal(W_cls, W_bits)


@pytest.mark.parametrize("loss", ["log", "hinge"])
def test_pair_mask_equals_one_vs_one_column_bitwise(loss):
    ds, y = _data()
    pairs = [(0, 1), (2, 0), (3, 1)]
    a = np.array([p[0] for p in pairs])
    b = np.array([p[1] for p in pairs])
    W_ovo = _fit(ds, _spec(len(pairs), a, col_class2=b.astype(np.int32)),
                 loss)
    targets = np.stack([y == p[0] for p in pairs], axis=1)
    mask = np.stack([(y == p[0]) | (y == p[1]) for p in pairs], axis=1)
    assert 0 < mask.mean() < 1
    W_bits = _fit(ds, _spec(len(pairs), np.full(len(pairs), -1),
                            targets=targets.astype(np.uint8),
                            train_mask=mask), loss)
    assert torch.equal(W_ovo, W_bits)
    # the mask is live: without it the result differs
    W_nomask = _fit(ds, _spec(len(pairs), np.full(len(pairs), -1),
                              targets=targets), loss)
    assert not torch.equal(W_ovo, W_nomask)


def test_none_planes_leave_the_spec_as_it_was():
    spec = _spec(K, np.arange(K))
    assert spec.targets is None and spec.train_mask is None


def test_validation_errors(monkeypatch):
    ds, y = _data()
    onehot = (y[:, None] == np.arange(K)[None, :])
    with pytest.raises(ValueError, match="train_mask needs targets"):
        _spec(K, np.arange(K), train_mask=onehot)
    with pytest.raises(ValueError, match="targets must be"):
        _spec(K, np.arange(K), targets=onehot[:, :3])
    with pytest.raises(ValueError, match="targets must be"):
        _spec(K, np.arange(K), targets=onehot.ravel())
    with pytest.raises(ValueError, match="shape of targets"):
        _spec(K, np.arange(K), targets=onehot, train_mask=onehot[:-1])
    with pytest.raises(ValueError, match="group_k"):
        ColumnSpec("cpu", np.full(K, -2, np.int32), np.arange(K, dtype=np.int32),
                   np.full(K, 0.1, np.float32), np.zeros(K, np.float32),
                   group_k=K, targets=onehot)
    # a row count that is not the data's is caught at the solve
    with pytest.raises(ValueError, match="rows"):
        _fit(ds, _spec(K, np.arange(K), targets=onehot[:-1]), "log")


def test_targets_on_the_sparse_native_solver_raise(monkeypatch):
    import scipy.sparse as sp

    from skdist_amd.models.linear import _make_dataset

    monkeypatch.setenv("SKDIST_AMD_FORCE_SPARSE", "1")
    rng = np.random.default_rng(0)
    X = sp.random(60, 12, density=0.3, format="csr", random_state=0,
                  dtype=np.float32)
    y = rng.integers(0, 2, size=60)
    ds = _make_dataset(X, y, device="cpu")
    assert getattr(ds, "is_sparse", False)
    spec = ColumnSpec("cpu", np.full(1, -2, np.int32),
                      np.ones(1, np.int32), np.full(1, 0.1, np.float32),
                      np.zeros(1, np.float32),
                      targets=(y == 1)[:, None])
    with pytest.raises(ValueError,
                       match="not supported on the sparse-native solver yet"):
        batched_sgd_fit(ds, spec, "log", 1, 32)
