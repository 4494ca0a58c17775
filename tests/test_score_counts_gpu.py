"""k_score_counts (fused F1 fold scoring) against float64 numpy and sklearn."""

import types

import numpy as np
import pytest
import torch
from sklearn.metrics import f1_score

import skdist_amd.models._sgd as sgd_mod
from skdist_amd.ops import require_hip, softmax_columns

pytestmark = pytest.mark.gpu
DEV = "cuda"
F1_NAMES = ("f1", "f1_macro", "f1_weighted")


def _bf(a):
    return torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(DEV)


@pytest.mark.filterwarnings("ignore:The number of unique classes")
@pytest.mark.parametrize("fa", [32, 96])
@pytest.mark.parametrize("m", [1, 127, 129, 200])
@pytest.mark.parametrize("gk", [1, 3, 5, 10, 64, 65, 128])
def test_kernel_matches_float64(gk, m, fa):
    """Integer inputs: z is exact in fp32 in any order, so the counts admit
    no tolerance.  Duplicated class columns tie at the maximum; binary z
    reaches the z == 0 boundary.  Multiclass y never holds class gk-1; a
    binary y holds both classes, or tp would only repeat pc (or be 0), and
    its one-row case leaves a class without support."""
    rng = np.random.default_rng(gk * 1000 + m + fa)
    k = max(gk, 2)
    nm, m_pad = 128 // gk + 1, (m + 127) // 128 * 128
    Xf = rng.integers(-3, 4, size=(m_pad, fa)).astype(np.float64)
    W = rng.integers(-3, 4, size=(nm, gk, fa)).astype(np.float64)
    yf = np.full(m_pad, -1e30)    # pad rows hold data: only y excludes them
    yf[:m] = y = rng.integers(0, gk - 1 if gk > 1 else 2, size=m)
    if gk > 1:
        W[::2, 1] = W[::2, 0]
    z = np.einsum("if,jcf->ijc", Xf[:m], W)        # [m, nm, gk]
    if gk > 1:
        zs = np.sort(z, axis=2)
        assert m == 1 or (zs[:, :, -1] == zs[:, :, -2]).any()
        pred, cls = z.argmax(axis=2), np.arange(gk)
    else:
        assert m == 1 or (z == 0).any()
        pred, cls = (z[:, :, 0] >= 0).astype(np.int64), np.array([1])
    hit = pred[:, :, None] == cls                  # [m, nm, gk]
    ref = np.stack([hit.sum(axis=0),
                    (hit & (y[:, None, None] == cls)).sum(axis=0)])

    cols, ncp = softmax_columns(nm, gk)
    Wt = np.zeros((ncp, fa))
    Wt[cols] = W.reshape(nm * gk, fa)
    cnt = torch.zeros(2, ncp, dtype=torch.int32, device=DEV)
    yt = torch.tensor(yf, dtype=torch.float32, device=DEV)
    require_hip().score_fold_counts(_bf(Xf), _bf(Wt), yt, cnt, gk)
    got = cnt.cpu().numpy()[:, cols].reshape(2, nm, gk)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]

    ds = types.SimpleNamespace(device=torch.device(DEV), Xaug=_bf(Xf[:m]),
                               comp_dtype=torch.bfloat16, y_float=yt[:m])
    for metric in (F1_NAMES if gk == 1 else F1_NAMES[1:]):
        # "f1" is sklearn's default: binary, pos_label=1
        avg = {} if metric == "f1" else dict(average=metric[3:],
                                             labels=np.arange(k))
        res = sgd_mod._score_fold_hip_counts(
            ds, _bf(W.reshape(nm * gk, fa).T), torch.arange(m, device=DEV),
            k, metric)
        want = [f1_score(y, pred[:, j], zero_division=0, **avg)
                for j in range(nm)]
        assert res.shape == (nm,)
        assert np.abs(res - want).max() <= 1e-12, (metric, res, want)


@pytest.mark.parametrize("n_classes,gk", [(4, 4), (2, 1)])
def test_batched_scores_route(monkeypatch, n_classes, gk):
    """Integer X and W: z is exact on both paths (|z| <= 84, exact in the
    bf16 the torch path rounds to), so both see the same predictions."""
    rng = np.random.default_rng(5)
    n, f, nm = 600, 20, 7
    X = rng.integers(-2, 3, size=(n, f)).astype(np.float32)
    ds = sgd_mod.DeviceDataset(X, rng.integers(0, n_classes, size=n),
                               device=DEV, standardize=False)
    i = np.arange(n)
    assert ds.set_cv_partition(
        [(np.setdiff1d(i, i[k::3]), i[k::3]) for k in range(3)])
    W = np.zeros((ds.fa, nm * gk), dtype=np.float32)
    W[:f + 1] = rng.integers(-2, 3, size=(f + 1, nm * gk))
    col_class = np.tile(np.arange(gk), nm) if gk > 1 else np.ones(nm)
    args = (ds, torch.tensor(W, device=DEV), np.arange(nm) % 3,
            col_class.astype(np.int32), n_classes)
    ext, seen = require_hip(), []
    real = ext.score_fold_counts
    monkeypatch.setattr(ext, "score_fold_counts",
                        lambda *a: (seen.append(a[4]), real(*a))[1])
    sgd_mod.batched_scores_by_fold(*args, "accuracy")
    assert seen == []
    got = {mt: sgd_mod.batched_scores_by_fold(*args, mt) for mt in F1_NAMES}
    assert seen == [gk] * 9
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    monkeypatch.setattr(sgd_mod, "_use_hip", lambda d: False)
    for mt in F1_NAMES:
        ref = sgd_mod.batched_scores_by_fold(*args, mt)
        assert len(np.unique(got[mt])) > 1
        assert np.abs(got[mt] - ref).max() <= 1e-12, (mt, got[mt], ref)
    assert len(seen) == 9


@pytest.mark.parametrize("name,bad,text", [
    ("gk", 0, "gk"), ("gk", 2, "gk"), ("gk", 129, "gk"),
    ("cnt", lambda t: t.float(), "cnt"),
    ("cnt", lambda t: t[:, :64].contiguous(), "cnt"),
    ("cnt", lambda t: t.cpu(), "cnt"), ("Xf", lambda t: t.cpu(), "Xf"),
    ("WbfT", lambda t: t.t().contiguous().t(), "WbfT"),
])
def test_score_fold_counts_rejects_bad_arguments(name, bad, text):
    a = dict(Xf=torch.zeros(128, 32, dtype=torch.bfloat16, device=DEV),
             WbfT=torch.zeros(128, 32, dtype=torch.bfloat16, device=DEV),
             yf=torch.zeros(128, device=DEV),
             cnt=torch.zeros(2, 128, dtype=torch.int32, device=DEV), gk=10)
    require_hip().score_fold_counts(*a.values())            # a good call
    # z == 0 everywhere: every row goes to class 0 of its group, and is right
    assert a["cnt"].cpu().view(2, 128)[:, :120:10].eq(128).all()
    assert int(a["cnt"].sum()) == 2 * 12 * 128
    a[name] = bad(a[name]) if callable(bad) else bad
    with pytest.raises(RuntimeError, match=text):
        require_hip().score_fold_counts(*a.values())
    torch.cuda.synchronize()
