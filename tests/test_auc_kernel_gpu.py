"""k_auc_counts (exact ROC AUC fold scoring) against numpy, for equality."""

import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from sklearn.metrics import roc_auc_score

import skdist_amd.models._sgd as sgd_mod
import skdist_amd.models._sparse_sgd as sparse_mod
from skdist_amd.ops import require_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
PI = 0x40490FDB     # no zero byte; a top byte of 0x7f or 0xff stays finite
F = np.finfo(np.float32)
SPECIALS = np.array(
    [0.0, -0.0, np.inf, -np.inf, F.smallest_subnormal, -F.smallest_subnormal,
     F.tiny - F.smallest_subnormal, F.smallest_subnormal - F.tiny, F.tiny,
     -F.tiny, F.max, -F.max, 1.0, -1.0, 0.5, -2.5, 3.25], dtype=np.float32)
PATTERNS = ("normal", "thirds", "equal", "byte0", "byte1", "byte2", "byte3",
            "specials")


def _values(pattern, rng, nm, M):
    if pattern == "equal":
        return np.full((nm, M), 1.5, dtype=np.float32)
    if pattern == "specials":
        return rng.choice(SPECIALS, size=(nm, M))
    if pattern.startswith("byte"):  # only radix pass b orders anything
        sh = 8 * int(pattern[4])
        r = rng.integers(0, 256, size=(nm, M), dtype=np.uint32) << sh
        return ((np.uint32(PI) & ~np.uint32(255 << sh)) | r).view(np.float32)
    z = rng.standard_normal((nm, M)).astype(np.float32)
    return np.round(z * 3) / 3 if pattern == "thirds" else z


def _run(z, n_neg):
    """The kernel on z [nm, M]: U2 per column, with a canary behind every
    buffer it writes and the positives' part of ZT left as it was."""
    nm, M = z.shape
    zt = torch.full((nm * M + 8,), 12345.0, device=DEV)
    zt[:nm * M] = torch.tensor(z, device=DEV).flatten()
    scr = torch.full((nm * n_neg + 8,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((nm + 8,), -7, dtype=torch.int64, device=DEV)
    require_hip().auc_counts(zt[:nm * M].view(nm, M), n_neg,
                             scr[:nm * n_neg].view(nm, n_neg), out[:nm])
    assert zt[nm * M:].eq(12345.0).all() and scr[nm * n_neg:].eq(-7).all()
    assert out[nm:].eq(-7).all()
    after = zt[:nm * M].view(nm, M)[:, n_neg:].cpu().numpy()
    assert np.array_equal(after.view(np.uint32), z[:, n_neg:].view(np.uint32))
    return out[:nm].cpu().numpy()


def _ref(z, n_neg):
    """(strict, ties) per column: U2 = 2 * strict + ties."""
    strict, ties = np.zeros(len(z), np.int64), np.zeros(len(z), np.int64)
    for c, col in enumerate(z):
        negs = np.sort(col[:n_neg])
        lo = np.searchsorted(negs, col[n_neg:], "left")
        hi = np.searchsorted(negs, col[n_neg:], "right")
        strict[c], ties[c] = lo.sum(), (hi - lo).sum()
    return strict, ties


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", [0, 1, 257])
@pytest.mark.parametrize("n_neg", [0, 1, 63, 64, 65, 255, 256, 257, 1029])
def test_auc_counts_equal_numpy(n_neg, P, pattern):
    """Wave (64) and tile (256 keys) edges, three tiles and a tail, the
    empty sides; 1, 5 and 70 columns of different data.  Over the 76
    columns of a case the reference must see ties where the pattern makes
    them, and a strict count elsewhere."""
    rng = np.random.default_rng(n_neg * 1000 + P + PATTERNS.index(pattern))
    strict_all = ties_all = 0
    for nm in (1, 5, 70):
        z = _values(pattern, rng, nm, n_neg + P)
        strict, ties = _ref(z, n_neg)
        got = _run(z, n_neg)
        # without rows nothing is launched: out keeps its fill
        want = 2 * strict + ties if n_neg + P else np.full(nm, -7)
        assert np.array_equal(got, want), (nm, got, strict, ties)
        strict_all, ties_all = strict_all + strict.sum(), ties_all + ties.sum()
    if pattern == "equal":
        assert ties_all == 76 * P * n_neg and strict_all == 0
    elif n_neg and P:
        assert (ties_all if pattern in ("thirds", "specials") else strict_all)


def test_auc_counts_past_32_bits():
    """40,000 positives all above 40,000 negatives: U2 = 3.2e9 > 2^32."""
    rng = np.random.default_rng(0)
    z = rng.standard_normal((2, 80_000)).astype(np.float32)
    z[:, :40_000] -= 100
    z[:, 40_000:] += 100
    assert _run(z, 40_000).tolist() == [3_200_000_000] * 2


@pytest.mark.parametrize("sparse", [False, True])
def test_roc_auc_search_scoring_route(monkeypatch, sparse):
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
    ref, skl = np.zeros(nm), np.zeros(nm)
    for k in range(folds):
        rows, mids = fold == k, np.flatnonzero(model_folds == k)
        st = sgd_mod._MetricState("roc_auc", per, 2, torch.device(DEV))
        st.update(torch.tensor(Z[rows][:, mids], device=DEV),
                  torch.tensor(y[rows], dtype=torch.float32, device=DEV),
                  torch.full((int(rows.sum()),), k, device=DEV),
                  types.SimpleNamespace(col_class=torch.ones(per, device=DEV)),
                  torch.full((per,), k, device=DEV), 2)
        ref[mids] = st.finalize()
        skl[mids] = [roc_auc_score(y[rows], Z[rows, j]) for j in mids]

    def boom(*a, **k):
        raise AssertionError("_MetricState constructed")
    monkeypatch.setattr(sgd_mod, "_MetricState", boom)
    monkeypatch.setattr(sparse_mod, "_MetricState", boom)
    got = sgd_mod.batched_scores_by_fold(
        ds, torch.tensor(W, device=DEV), model_folds,
        np.ones(nm, dtype=np.int32), 2, "roc_auc")
    assert len(np.unique(Z)) < 200 and len(np.unique(got)) > 1
    assert np.array_equal(got, ref), (got, ref)
    assert np.abs(got - skl).max() <= 1e-12


@pytest.mark.parametrize("name,bad", [
    ("ZT", lambda t: t.double()), ("out", lambda t: t.int()),
    ("ZT", lambda t: t.t().contiguous().t()),
    ("scratch", lambda t: t[:3].contiguous()),
    ("out", lambda t: t[:3].contiguous()), ("n_neg", lambda v: 9),
])
def test_auc_counts_rejects_bad_arguments(name, bad):
    a = dict(ZT=torch.arange(32., device=DEV).view(4, 8), n_neg=5,
             scratch=torch.zeros(4, 5, dtype=torch.int32, device=DEV),
             out=torch.full((4,), -7, dtype=torch.int64, device=DEV))
    a[name] = bad(a[name])
    with pytest.raises(RuntimeError, match="n_neg" if name == "n_neg" else name):
        require_hip().auc_counts(*a.values())
    torch.cuda.synchronize()
    assert a["out"].eq(-7).all()    # nothing was launched
