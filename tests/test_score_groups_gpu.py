"""k_score_groups (fused multiclass fold scoring) against float64 numpy."""

import types

import numpy as np
import pytest
import torch

import skdist_amd.models._sgd as sgd_mod
from skdist_amd.ops import require_hip, softmax_columns

pytestmark = pytest.mark.gpu
DEV = "cuda"
# max |mean nll - float64 reference| over the mode-1 cases below, measured
# on an MI355X on 2026-11-26: reached at gk = 3, m = 1, fa = 96, where the
# one row is the 60-unit one and nll is up to 57
NLL_MEASURED = 5.4e-6


def _bf(a):
    return torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("fa", [32, 96])
@pytest.mark.parametrize("m", [1, 127, 129, 200])
@pytest.mark.parametrize("gk,mode", [(g, 0) for g in (3, 5, 10, 64, 65, 128)]
                         + [(g, 1) for g in (3, 10, 65)])
def test_kernel_matches_float64(gk, mode, m, fa):
    """mode 0: integer inputs, z exact in fp32 in any order, so the hit
    counts admit no tolerance; duplicated class columns tie at the maximum.
    mode 1: real inputs rounded to bf16, row 0 with z spread over 60."""
    rng = np.random.default_rng(gk * 1000 + m + fa)
    nm, m_pad = 128 // gk + 1, (m + 127) // 128 * 128
    if mode == 0:
        Xf = rng.integers(-3, 4, size=(m_pad, fa)).astype(np.float64)
        W = rng.integers(-3, 4, size=(nm, gk, fa)).astype(np.float64)
        W[::2, 1] = W[::2, 0]
    else:
        Xf = rng.standard_normal((m_pad, fa))
        W = rng.standard_normal((nm, gk, fa)) / 4.0
        z0 = W @ Xf[0]
        Xf[0] *= 60.0 / (z0.max(axis=1) - z0.min(axis=1)).max()
        Xf, W = (torch.tensor(a).to(torch.bfloat16).double().numpy()
                 for a in (Xf, W))
    yf = np.full(m_pad, -1e30)    # pad rows hold data: only y excludes them
    yf[:m] = y = rng.integers(0, gk - 1, size=m)   # class gk-1 is absent
    z = np.einsum("if,jcf->ijc", Xf[:m], W)        # [m, nm, gk]
    zs = np.sort(z, axis=2)
    if mode == 0:
        assert m == 1 or (zs[:, :, -1] == zs[:, :, -2]).any()
        ref = (z.argmax(axis=2) == y[:, None]).sum(axis=0) / m
    else:
        assert 55.0 <= (zs[0, :, -1] - zs[0, :, 0]).max() <= 65.0
        lse = zs[:, :, -1] + np.log(np.exp(z - zs[:, :, -1:]).sum(axis=2))
        ref = -(lse - z[np.arange(m), :, y]).mean(axis=0)

    cols, ncp = softmax_columns(nm, gk)
    Wt = np.zeros((ncp, fa))
    Wt[cols] = W.reshape(nm * gk, fa)
    part = torch.full((m_pad // 128, ncp // 128 * (128 // gk)), 777.0,
                      dtype=torch.float32, device=DEV)
    yt = torch.tensor(yf, dtype=torch.float32, device=DEV)
    require_hip().score_fold_groups(_bf(Xf), _bf(Wt), yt, part, gk, mode)
    got = part.double().sum(dim=0).cpu().numpy()[:nm] / m * (1 - 2 * mode)
    ds = types.SimpleNamespace(device=torch.device(DEV), Xaug=_bf(Xf[:m]),
                               comp_dtype=torch.bfloat16, y_float=yt[:m])
    res = sgd_mod._score_fold_hip_groups(
        ds, _bf(W.reshape(nm * gk, fa).T), torch.arange(m, device=DEV), gk,
        mode)
    # dead groups never reach the caller; pad rows of zeros change nothing
    assert res.shape == (nm,) and np.array_equal(res, got)
    err = np.abs(got - ref).max()
    print(f"gk={gk} mode={mode} m={m} fa={fa}: max|got - ref| = {err:.3e}")
    assert err <= (0.0 if mode == 0 else min(4 * NLL_MEASURED, 1e-4)), err


@pytest.mark.parametrize("n_classes,calls", [(4, 3), (2, 0)])
def test_batched_scores_route(monkeypatch, n_classes, calls):
    """Integer X and W: z is exact on both paths (|z| <= 84, exact in the
    bf16 the torch path rounds to), so accuracy is equal, not close."""
    rng = np.random.default_rng(5)
    n, f, nm, cpm = 600, 20, 7, (n_classes if n_classes > 2 else 1)
    X = rng.integers(-2, 3, size=(n, f)).astype(np.float32)
    ds = sgd_mod.DeviceDataset(X, rng.integers(0, n_classes, size=n),
                               device=DEV, standardize=False)
    i = np.arange(n)
    assert ds.set_cv_partition(
        [(np.setdiff1d(i, i[k::3]), i[k::3]) for k in range(3)])
    W = np.zeros((ds.fa, nm * cpm), dtype=np.float32)
    W[:f + 1] = rng.integers(-2, 3, size=(f + 1, nm * cpm))
    col_class = np.tile(np.arange(cpm), nm) if cpm > 1 else np.ones(nm)
    args = (ds, torch.tensor(W, device=DEV), np.arange(nm) % 3,
            col_class.astype(np.int32), n_classes, "accuracy")
    ext, seen = require_hip(), []
    real = ext.score_fold_groups
    monkeypatch.setattr(ext, "score_fold_groups",
                        lambda *a: (seen.append(a[4:]), real(*a))[1])
    got = sgd_mod.batched_scores_by_fold(*args)
    assert seen == [(4, 0)] * calls
    monkeypatch.setenv("SKDIST_AMD_ALLOW_EAGER", "1")
    monkeypatch.setattr(sgd_mod, "_use_hip", lambda d: False)
    ref = sgd_mod.batched_scores_by_fold(*args)
    assert len(seen) == calls and len(np.unique(got)) > 1
    # k_score's binary route divides in fp32
    assert np.abs(got - ref).max() <= (0.0 if calls else 1e-6), (got, ref)


@pytest.mark.parametrize("name,bad,text", [
    ("gk", 2, "gk"), ("gk", 129, "gk"), ("mode", 2, "mode"),
    ("part", lambda t: t[:, :11].contiguous(), "part"),
    ("part", lambda t: t.repeat(2, 1), "part"),
    ("Xf", lambda t: t.cpu(), "Xf"), ("part", lambda t: t.cpu(), "part"),
    ("WbfT", lambda t: t.t().contiguous().t(), "WbfT"),
])
def test_score_fold_groups_rejects_bad_arguments(name, bad, text):
    a = dict(Xf=torch.zeros(128, 32, dtype=torch.bfloat16, device=DEV),
             WbfT=torch.zeros(128, 32, dtype=torch.bfloat16, device=DEV),
             yf=torch.full((128,), -1e30, device=DEV),
             part=torch.full((1, 12), 5.0, device=DEV), gk=10, mode=0)
    require_hip().score_fold_groups(*a.values())            # a good call
    assert float(a["part"].abs().sum()) == 0.0      # written; all pad rows
    a[name] = bad(a[name]) if callable(bad) else bad
    with pytest.raises(RuntimeError, match=text):
        require_hip().score_fold_groups(*a.values())
    torch.cuda.synchronize()
