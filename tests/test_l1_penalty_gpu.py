"""GPU tests of the L1 / elastic-net kernels (k_reduce_update_l1 in
sgd_kernels.hip; k_sp_l1_catchup, k_sp_bias_scale_l1, k_sp_update_l1,
k_sp_l1_flush, k_sp_renorm_l1 in sparse_sgd_kernels.hip) against the
eager mirrors of the same arithmetic (test_l1_penalty.py tests those on
CPU).  Each test prints the figures it asserts on."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skdist_amd.models._sgd import (
        ColumnSpec,
        DeviceDataset,
        batched_sgd_fit,
    )
    from skdist_amd.models._sparse_sgd import (
        SparseDeviceDataset,
        sparse_sgd_fit,
    )

# 3 x 3: every col_l1 against every col_l2
COL_L1 = np.array([0, 1e-3, 1e-2] * 3, dtype=np.float32)
COL_L2 = np.repeat(np.array([0, 1e-3, 1e-2], dtype=np.float32), 3)


def _bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _dense_case(loss_id, feat_mask=None, col_l1=COL_L1):
    """n=400 rows on 128-row batches (a 16-row tail), f=37 (fa pads to
    64) and 9 columns (pad to 128): pad rows, pad columns, a tail batch."""
    torch.manual_seed(0)
    n, f, ncols = 400, 37, 9
    X = _bf16_round(torch.randn(n, f))
    y = (torch.rand(n) < 0.3).float()
    fold = torch.randint(0, 3, (n,), dtype=torch.int32)
    ds = DeviceDataset(X.numpy(), y.numpy().astype(np.float32),
                       device="cuda", standardize=False)
    ds.fold_id = fold.to(ds.device)
    cls = -1 if loss_id == 2 else 1
    kw = dict(
        col_fold=np.array([0, 1, 2, -2, 0, 1, 2, 0, 1], dtype=np.int32),
        col_class=np.full(ncols, cls, dtype=np.int32),
        col_lr=np.array([0.4, 0.3, 0.2] * 3, dtype=np.float32),
        col_l2=COL_L2, feat_mask=feat_mask)
    Xref = torch.zeros(n, ds.Xaug.shape[1])
    Xref[:, :f] = X
    Xref[:, ds.intercept_row] = 1.0
    return {"ds": ds, "spec": ColumnSpec(ds.device, col_l1=col_l1, **kw),
            "spec_l2": ColumnSpec(ds.device, **kw), "Xref": Xref, "y": y,
            "fold": fold, "loss_id": loss_id}


def _mirror_solve(case, epochs, bs, seed, momentum, lr_decay):
    """The eager mirror on CPU in the kernels' number flow, as
    test_gpu_kernels._ref_solve does it (bf16 operands into fp32-
    accumulated GEMMs, G rounded to bf16), with the solver's own eager
    L1 step `_l1_clip_torch` after each update."""
    from skdist_amd.models._sgd import _l1_clip_torch

    spec, ds = case["spec"], case["ds"]
    Xs, y, fold, loss_id = case["Xref"], case["y"], case["fold"], \
        case["loss_id"]
    col_class, col_fold = spec.col_class.cpu(), spec.col_fold.cpu()
    col_lr, col_l2 = spec.col_lr.cpu(), spec.col_l2.cpu()
    col_l1 = spec.col_l1.cpu()
    fmask = (None if spec.feat_mask is None
             else spec.feat_mask.cpu().float())
    ir = ds.intercept_row
    n, fa = Xs.shape
    ncols = len(col_class)
    W = torch.zeros(fa, ncols)
    V = torch.zeros_like(W)
    cpos, cneg = torch.zeros_like(W), torch.zeros_like(W)
    perm = np.random.default_rng(seed).permutation(n)
    Xs, ys, fs = Xs[perm], y[perm], fold[perm]
    for epoch in range(epochs):
        lr_scale = 1.0 / (1.0 + lr_decay * epoch)
        for s in range(0, n, bs):
            Xm, ym, fm = Xs[s:s + bs], ys[s:s + bs], fs[s:s + bs]
            m = Xm.shape[0]
            Z = Xm @ _bf16_round(W)
            t = torch.where(
                col_class.unsqueeze(0) < 0,
                ym.unsqueeze(1).expand(m, ncols),
                (ym.unsqueeze(1) == col_class.unsqueeze(0).float()).float())
            if loss_id == 0:
                G = torch.sigmoid(Z.clamp(-30, 30)) - t
            elif loss_id == 1:
                sgn = 2 * t - 1
                G = torch.where(sgn * Z < 1, -sgn, torch.zeros_like(Z))
            else:
                G = Z - t
            mask = (fm.unsqueeze(1) != col_fold.unsqueeze(0)).float()
            G = _bf16_round(G * mask)
            grad = Xm.t() @ G / m
            l2 = col_l2.unsqueeze(0) * W
            l2[ir] = 0
            step = col_lr.unsqueeze(0) * lr_scale * (grad + l2)
            if momentum > 0:
                V.mul_(momentum).add_(step)
                W.sub_(V)
            else:
                W.sub_(step)
            delta = col_lr * lr_scale * col_l1 * (1.0 / (1.0 - momentum))
            _l1_clip_torch(W, cpos, cneg, delta, ir)
            if fmask is not None:
                for t_ in (W, V, cpos, cneg):
                    t_.mul_(fmask)
    return W


def _check_against_mirror(got, ref):
    """The criterion of test_gpu_kernels.test_sgd_step_matches_reference,
    plus: where exactly one side is 0 the other is below the tolerance
    (implied by it, asserted apart so a failure names the cause)."""
    diff = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    tol = max(2e-3, 2e-3 * scale)
    one_zero = (got == 0) ^ (ref == 0)
    worst = torch.maximum(got.abs(), ref.abs())[one_zero]
    worst = worst.max().item() if len(worst) else 0.0
    print(f"diff={diff:.2e} scale={scale:.2f} one-sided zeros="
          f"{int(one_zero.sum())} worst={worst:.2e}")
    assert diff < tol, (diff, scale)
    assert worst < tol


@pytest.mark.parametrize("loss_id", [0, 1, 2])
@pytest.mark.parametrize("lr_decay", [0.0, 0.5])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_dense_l1_kernel_matches_eager_mirror(momentum, lr_decay, loss_id):
    case = _dense_case(loss_id)
    ds = case["ds"]
    kw = dict(epochs=2, batch_size=128, seed=0, momentum=momentum,
              lr_decay=lr_decay)
    W_hip = batched_sgd_fit(ds, case["spec"], loss_id, **kw).float().cpu()
    W_ref = _mirror_solve(case, 2, 128, 0, momentum, lr_decay)
    assert W_hip.shape == W_ref.shape == (64, 9)
    _check_against_mirror(W_hip, W_ref)
    # L1 did something, and the strong columns hold exact zeros
    ir = ds.intercept_row
    assert (W_hip[:37, COL_L1 > 5e-3] == 0).any()
    assert (W_hip[ir] != 0).all()               # intercept never clipped
    assert (W_hip[38:] == 0).all()              # pad rows
    # columns without L1 ran the same arithmetic as the L2-only kernel
    W_l2 = batched_sgd_fit(ds, case["spec_l2"], loss_id,
                           **kw).float().cpu()
    keep = torch.as_tensor(COL_L1 == 0)
    assert torch.equal(W_hip[:, keep], W_l2[:, keep])
    assert not torch.equal(W_hip[:, ~keep], W_l2[:, ~keep])


def test_dense_l1_intercept_row_is_unshrunk():
    """An L1 strong enough to zero every feature weight leaves the
    intercept where the penalty-free intercept-only model puts it."""
    case = _dense_case(0, col_l1=np.full(9, 1.0, dtype=np.float32))
    ds = case["ds"]
    W_hip = batched_sgd_fit(ds, case["spec"], 0, epochs=2, batch_size=128,
                            seed=0, momentum=0.9).float().cpu()
    W_ref = _mirror_solve(case, 2, 128, 0, 0.9, 0.0)
    ir = ds.intercept_row
    assert (W_hip[:ir] == 0).all() and (W_hip[ir + 1:] == 0).all()
    assert (W_hip[ir] < -0.3).all()             # P(y=1) = 0.3
    _check_against_mirror(W_hip, W_ref)


def test_dense_l1_kernel_with_feat_mask():
    mask = np.ones((64, 9), dtype=np.uint8)
    mask[[0, 5, 20], 1::2] = 0
    case = _dense_case(0, feat_mask=mask)
    W_hip = batched_sgd_fit(case["ds"], case["spec"], 0, epochs=2,
                            batch_size=128, seed=0,
                            momentum=0.9).float().cpu()
    W_ref = _mirror_solve(case, 2, 128, 0, 0.9, 0.0)
    _check_against_mirror(W_hip, W_ref)
    assert (W_hip[[0, 5, 20], 1::2] == 0).all()
    assert (W_hip[[0, 5, 20], 0] != 0).all()


# ------------------------------------------------------------------ #
# sparse
# ------------------------------------------------------------------ #

# feature -> (positions in the shuffled order, values); with 1024-row
# batches: 7 in batches 0, 2, 4; 8 in 1, 3; 9 in 0, 2, 4
RARE = {7: ([100, 2300, 4500], [1.5, -1.0, 2.0]),
        8: ([1500, 3500], [-2.0, 1.0]),
        9: ([700, 2900, 4900], [1.0, 1.0, -1.5])}


def _sparse_case(seed=0, lr=0.3, l2=1e-4, n=5000, f=400, ncols=24,
                 folds=3):
    """Shape of test_sparse_gpu._ds_and_spec with mixed col_l1; feature 5
    has no stored entry, feature 6 is stored in a single row, and the
    RARE features in two or three rows that the solver's shuffle (seed
    0) puts into different batches with batches between them: their
    weights wait several steps for the catch-up, and feature 8, last
    seen in the fourth of five batches, for the end-of-fit flush."""
    rng = np.random.default_rng(seed)
    Xd = rng.standard_normal((n, f)).astype(np.float32)
    Xd[np.abs(Xd) < 1.1] = 0
    Xd[:, 5] = 0
    Xd[:, 6] = 0
    Xd[17, 6] = 1.5
    perm = np.random.default_rng(0).permutation(n)   # the solver's shuffle
    for j, (positions, v) in RARE.items():
        Xd[:, j] = 0
        Xd[perm[positions], j] = v
    X = sp.csr_matrix(Xd)
    w = rng.standard_normal(f) * (rng.random(f) < 0.2)
    y = ((Xd @ w) > 0).astype(np.int64)
    ds = SparseDeviceDataset(X, y)
    fold = np.arange(n) % folds
    assert ds.set_cv_partition([
        (np.flatnonzero(fold != k), np.flatnonzero(fold == k))
        for k in range(folds)])
    l1 = np.tile(np.array([0, 0, 0, 1e-4, 1e-4, 1e-4, 1e-3, 1e-3, 1e-3,
                           1e-2, 1e-2, 1e-2], dtype=np.float32), 2)
    spec = ColumnSpec(
        ds.device,
        col_fold=np.tile(np.arange(folds, dtype=np.int32), ncols // folds),
        col_class=np.ones(ncols, dtype=np.int32),
        col_lr=np.full(ncols, lr, dtype=np.float32),
        col_l2=np.full(ncols, l2, dtype=np.float32), col_l1=l1)
    return ds, spec, l1


@pytest.mark.parametrize("adaptive", [True, False])
def test_sparse_l1_kernels_match_eager_mirror(adaptive):
    ds, spec, l1 = _sparse_case()
    kw = dict(epochs=5, batch_size=1024, seed=0, adaptive=adaptive)
    W_hip = sparse_sgd_fit(ds, spec, "log", **kw).cpu().numpy()
    W_eag = sparse_sgd_fit(ds, spec, "log", force_eager=True,
                           **kw).cpu().numpy()
    # tolerances of test_sparse_gpu.test_hip_solve_matches_eager_mirror
    corr = np.corrcoef(W_hip.ravel(), W_eag.ravel())[0, 1]
    print(f"adaptive={adaptive} corr={corr:.6f} "
          f"maxdiff={np.abs(W_hip - W_eag).max():.2e} zeros hip/eager="
          f"{(W_hip == 0).sum()}/{(W_eag == 0).sum()}")
    assert corr > 0.9999, corr
    np.testing.assert_allclose(W_hip, W_eag, atol=2e-2, rtol=0.05)
    # exact zeros appear, more of them under the stronger penalty
    nz = [(W_hip[:400, m] == 0).mean()
          for m in (l1 == 0, (l1 > 5e-4) & (l1 < 5e-3), l1 > 5e-3)]
    assert nz[0] < nz[1] < nz[2], nz
    # a feature with no stored entry stays 0 in every column
    assert (W_hip[5] == 0).all()
    # a feature stored in one row is touched twice per epoch; the rest
    # of its penalty arrives in the end-of-fit flush
    trained = spec.col_fold.cpu().numpy() != 17 % 3   # row 17's fold
    assert (W_hip[6, (l1 == 0) & trained] != 0).all()
    assert (W_hip[6, ~trained] == 0).all()
    np.testing.assert_allclose(W_hip[6], W_eag[6], atol=2e-3, rtol=0.05)
    # rare features: gaps of one or two steps between touches, so their
    # weights show whether the catch-up accrued the skipped steps
    sh = ds.shuffled(0, 1024)
    for j, (positions, _) in RARE.items():
        batches = [b for b in range(5) if j in sh["ufeat"][
            int(sh["ub_ptr"][b]):int(sh["ub_ptr"][b + 1])].tolist()]
        assert batches == sorted({p // 1024 for p in positions}), batches
        assert (W_hip[j, l1 == 0] != 0).any()
        print(f"feature {j} batches {batches} max|hip-eager|="
              f"{np.abs(W_hip[j] - W_eag[j]).max():.2e} "
              f"max|w|={np.abs(W_eag[j]).max():.2e}")
        # feature 6's tolerance, tightened to 2% of the row's largest
        # weight where that is less (adaptive off: weights of ~1e-3)
        atol = min(2e-3, 0.02 * np.abs(W_eag[j]).max())
        np.testing.assert_allclose(W_hip[j], W_eag[j], atol=atol,
                                   rtol=0.05)
    # two runs are bitwise equal
    W_again = sparse_sgd_fit(ds, spec, "log", **kw).cpu().numpy()
    np.testing.assert_array_equal(W_hip, W_again)


@pytest.mark.parametrize("adaptive", [True, False])
def test_sparse_l1_heavy_l2_renorm_matches_eager(adaptive):
    """test_sparse_gpu.test_hip_heavy_l2_renorm_matches_eager with
    l1 > 0: the renorm rescales W together with every L1 table."""
    ds, spec, _ = _sparse_case(seed=4, lr=1.0, l2=0.08)
    kw = dict(epochs=10, batch_size=512, seed=0, adaptive=adaptive)
    W_hip = sparse_sgd_fit(ds, spec, "log", **kw).cpu().numpy()
    W_eag = sparse_sgd_fit(ds, spec, "log", force_eager=True,
                           **kw).cpu().numpy()
    assert np.isfinite(W_hip).all()
    corr = np.corrcoef(W_hip.ravel(), W_eag.ravel())[0, 1]
    print(f"adaptive={adaptive} renorm corr={corr:.6f}")
    assert corr > 0.99, corr


# ------------------------------------------------------------------ #
# end to end
# ------------------------------------------------------------------ #

def test_hashed_text_search_over_l1_ratio(monkeypatch):
    """Hashed text through DistGridSearchCV on the sparse HIP path: the
    l1_ratio=1 model is sparser than the l1_ratio=0 one and its CV
    accuracy is no further below sklearn saga's than saga's own
    fold-to-fold spread (max - min of its three fold accuracies, taken
    at run time; measured 0.8058 / 0.8095 / 0.8057, spread 0.0038, with
    this solver at 0.8258 and 1499 nonzeros against 2930).  Half-overlapping
    vocabularies, 12 tokens per document and 10% flipped labels keep the
    problem off 100% accuracy, where the spread would be 0."""
    from sklearn.feature_extraction.text import HashingVectorizer
    from sklearn.linear_model import LogisticRegression as SkLogReg
    from sklearn.model_selection import StratifiedKFold, cross_val_score

    from skdist_amd import Cluster
    from skdist_amd.distribute.search import DistGridSearchCV
    from skdist_amd.models import LogisticRegression

    monkeypatch.setenv("SKDIST_AMD_FORCE_SPARSE", "1")
    # every solve must be the batched one on the sparse HIP path: a
    # fall-back to the generic per-task search would fit 6 + 1 models
    import skdist_amd.models.linear as lin

    solves = []
    real_fit = lin.batched_sgd_fit

    def spy(ds, spec, *a, **kw):
        assert not kw.get("force_eager")
        solves.append((getattr(ds, "is_sparse", False), ds.device.type,
                       spec.ncols, spec.col_l1 is not None))
        return real_fit(ds, spec, *a, **kw)

    monkeypatch.setattr(lin, "batched_sgd_fit", spy)
    rng = np.random.default_rng(0)
    v0 = [f"tok{i}" for i in range(2000)]
    v1 = [f"tok{i}" for i in range(1000, 3000)]
    n = 4000
    y = np.arange(n) % 2
    docs = [" ".join(rng.choice(v1 if c else v0, size=12)) for c in y]
    y = np.where(rng.random(n) < 0.1, 1 - y, y)
    X = HashingVectorizer(n_features=2 ** 16).transform(docs)
    C = 3.0
    cv = StratifiedKFold(3)
    gs = DistGridSearchCV(
        LogisticRegression(penalty="elasticnet", C=C, epochs=20,
                           batch_size=256, momentum=0.0, random_state=0),
        {"l1_ratio": [0.0, 1.0]}, cv=cv, scoring="accuracy",
        sc=Cluster(require_gpu=True))
    gs.fit(X, y)
    # one solve: 2 candidates x (3 folds + the refit column)
    assert solves == [(True, "cuda", 8, True)], solves
    res = gs.cv_results_
    score = {p["l1_ratio"]: s
             for p, s in zip(res["params"], res["mean_test_score"])}

    nnz = {}
    for rho in (0.0, 1.0):
        est = LogisticRegression(**{**gs.estimator.get_params(),
                                    "l1_ratio": rho, "sc": None})
        nnz[rho] = int((est.fit(X, y).coef_ != 0).sum())
    assert solves[1:] == [(True, "cuda", 1, False), (True, "cuda", 1, True)]
    saga = cross_val_score(
        SkLogReg(penalty="l1", solver="saga", C=C, max_iter=200), X, y,
        cv=cv, scoring="accuracy")
    margin = saga.max() - saga.min()
    print(f"nnz={nnz} ours={score} saga={saga} margin={margin:.4f}")
    assert 0 < nnz[1.0] < nnz[0.0]
    assert score[1.0] > saga.mean() - margin, (score, saga)
