"""k_ap_sums (average precision fold scoring) against float64 numpy."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from sklearn.metrics import average_precision_score

import skdist_amd.models._sgd as sgd_mod
import skdist_amd.models._sparse_sgd as sparse_mod
from skdist_amd.ops import require_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -53
SHAPES = [(1, 1), (2, 1), (5, 0), (5, 5), (513, 256), (513, 257), (512, 256),
          (1400, 1025), (1400, 3)]
CASES = [(M, P, kind) for M, P in SHAPES for kind in ("normal", "grid")] + [
    (1400, 1025, "inf")]


def _ref(col, n_neg):      # AP of one float64 column, negatives first
    neg, pos = np.sort(col[:n_neg]), np.sort(col[n_neg:])
    tp = len(pos) - np.searchsorted(pos, pos, "left")
    fp = len(neg) - np.searchsorted(neg, pos, "left")
    return (tp / (tp + fp)).sum() / len(pos) if len(pos) else 0.0


def _run(z, n_neg):
    """The kernel on z [nm, M]: S per model, a canary behind every buffer."""
    nm, M = z.shape
    zt = torch.full((nm * M + 8,), 12345.0, device=DEV)
    zt[:nm * M] = torch.tensor(z, device=DEV).flatten()
    scr = torch.full((nm * M + 8,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((nm + 8,), -7.0, dtype=torch.float64, device=DEV)
    require_hip().ap_sums(zt[:nm * M].view(nm, M), n_neg,
                          scr[:nm * M].view(nm, M), out[:nm])
    assert zt[nm * M:].eq(12345.0).all() and scr[nm * M:].eq(-7).all() \
        and out[nm:].eq(-7).all()
    return out[:nm].cpu().numpy()


@pytest.mark.parametrize("M,P,kind", CASES)
def test_ap_sums_match_numpy(M, P, kind):
    """Empty and one-element segments; one 256-key tile, one more, both
    full; more positives than one batch of the count loop (1024) over fewer
    negatives; 3 positives.  Measured: at most 2.2e-16 from the reference."""
    rng = np.random.default_rng(M * 7 + P)
    n_neg = M - P
    z = rng.standard_normal((3, M)).astype(np.float32)
    if kind == "grid":      # heavy ties within and across the classes
        z = np.round(z * 2) / 2
        z[z == 0] = rng.choice(np.float32([0.0, -0.0]), size=(z == 0).sum())
        bits = z.view(np.uint32)
        assert M < 500 or ((bits == 0x80000000).any() and (bits == 0).any())
    if kind == "inf":       # both infinities in both classes
        z[:, [0, 1, n_neg, n_neg + 1]] = [np.inf, -np.inf, np.inf, -np.inf]
    got = _run(z, n_neg)
    ap = got / max(P, 1)
    ref = np.array([_ref(col.astype(np.float64), n_neg) for col in z])
    assert np.abs(ap - ref).max() <= 2 * P * EPS, (ap, ref)
    if (M, P, kind) == (1400, 1025, "grid"):    # sklearn takes no infinity
        skl = [average_precision_score(np.arange(M) >= n_neg, c) for c in z]
        assert np.abs(ap - skl).max() <= 2 * P * EPS, (ap, skl)
    assert np.array_equal(_run(z, n_neg), got)   # same bits on a fresh copy


@pytest.mark.parametrize("sparse", [False, True])
def test_average_precision_search_scoring_route(monkeypatch, sparse):
    """Integer X and W: z is an exact integer on every path, with ties."""
    rng = np.random.default_rng(7)
    n, f, folds, per = (2000, 300, 2, 4) if sparse else (3000, 20, 3, 4)
    X = rng.integers(-2, 3, size=(n, f)).astype(np.float32)
    y = rng.integers(0, 2, size=n)
    fold, nm = np.arange(n) % folds, folds * per
    if sparse:
        X[rng.random((n, f)) < 0.9] = 0
        ds = sparse_mod.SparseDeviceDataset(sp.csr_matrix(X), y, device=DEV)
        W = rng.integers(-2, 3, size=(f + 1, nm)).astype(np.float32)
        Z = X @ W[:f] + W[f]
    else:
        ds = sgd_mod.DeviceDataset(X, y, device=DEV, standardize=False)
        W = np.zeros((ds.fa, nm), dtype=np.float32)
        W[:f + 1] = rng.integers(-2, 3, size=(f + 1, nm))
        Z = ds.Xaug.float().cpu().numpy() @ W
    assert ds.set_cv_partition([(np.flatnonzero(fold != k),
                                 np.flatnonzero(fold == k))
                                for k in range(folds)])
    model_folds = np.repeat(np.arange(folds), per)
    tol = 2 * EPS * np.repeat([y[fold == k].sum() for k in range(folds)], per)
    skl = [average_precision_score(y[fold == k], Z[fold == k, j])
           for j, k in enumerate(model_folds)]

    def score(kernel):
        monkeypatch.setattr(sgd_mod, "_ap_kernel_pays", lambda m, k: kernel)
        return sgd_mod.batched_scores_by_fold(
            ds, torch.tensor(W, device=DEV), model_folds,
            np.ones(nm, dtype=np.int32), 2, "average_precision")
    ref = score(False)      # the _MetricState route
    for mod in (sgd_mod, sparse_mod):   # which from here on cannot be taken
        monkeypatch.setattr(mod, "_MetricState", None)
    got = score(True)
    assert len(np.unique(Z)) < 200 and len(np.unique(got)) > 1
    assert (np.abs(got - skl) <= tol).all(), (got, skl)
    assert (np.abs(got - ref) <= tol).all(), (got, ref)
