"""
The multinomial forward kernel (k_fwd_gt_softmax) and everything above it
on the device: one staged step against the float64 reference of
tests/_softmax_ref.py, graph replay, the solve against the eager solver,
end-to-end fits against sklearn, and the binding's argument checks.
"""

import numpy as np
import pytest
import torch

import _dense_ref as R
import _softmax_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = R.EPS32
CANARY = 12345.0   # finite, and no kernel result equals it
STALE = 7.0        # pre-fill of GT; past m_pad it must stay
LOSS_SOFTMAX = S.LOSS_SOFTMAX


def _ext():
    from skdist_amd.ops import require_hip

    return require_hip()


# the helpers of tests/test_dense_sgd_kernels_gpu.py, copied

def _bf(a):
    """float64 bf16 VALUES -> bf16 device tensor (exact)."""
    a = np.asarray(a, np.float64)
    assert np.array_equal(R.bf16_rne(a), a), "not bf16 values"
    return torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(DEV)


def _f32(a):
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return torch.tensor(a, dtype=torch.float32, device=DEV)


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)


def _np(t):
    return t.detach().cpu().to(torch.float64).numpy()


def _guarded(values, dtype, extra_rows):
    v = torch.tensor(np.asarray(values, np.float64), dtype=torch.float32)
    big = torch.full((v.shape[0] + extra_rows,) + tuple(v.shape[1:]),
                     CANARY, dtype=torch.float32)
    big[: v.shape[0]] = v
    big = big.to(dtype).to(DEV)
    view = big.narrow(0, 0, v.shape[0])
    assert view.is_contiguous()
    return view, big.narrow(0, v.shape[0], extra_rows)


def _canary_intact(t):
    return bool((t.to(torch.float32) == torch.tensor(
        CANARY).to(t.dtype).to(torch.float32)).all())


def _device_step_buffers(c, m, splitk):
    fa, ncp = c["fa"], c["ncols_pad"]
    m_pad = R.ceil_to(m, 128)
    d = {}
    d["Xs"] = _bf(c["Xs"])
    d["XsT"] = _bf(c["XsT"])
    d["GT"], d["GT_can"] = _guarded(
        np.full((ncp, m_pad + 128), STALE), torch.bfloat16, 8)
    d["W"], d["W_can"] = _guarded(c["W"], torch.float32, fa)
    if c["V"] is not None:
        d["V"], d["V_can"] = _guarded(c["V"], torch.float32, fa)
    else:
        d["V"] = torch.empty(0, dtype=torch.float32, device=DEV)
    d["WbfT"], d["WbfT_can"] = _guarded(c["W"].T, torch.bfloat16, 8)
    d["partial"], d["partial_can"] = _guarded(
        np.full((splitk, fa, ncp), CANARY), torch.float32, 1)
    d["y"] = _f32(c["y"])
    d["fold"] = _i32(c["fold"])
    for k in ("col_class", "col_fold", "col_class2"):
        d[k] = _i32(c[k])
    d["col_lr"] = _f32(c["col_lr"])
    d["col_l2"] = _f32(c["col_l2"])
    d["fmask"] = torch.empty(0, dtype=torch.uint8, device=DEV)
    d["row_w"] = (
        _f32(c["row_w"]) if c["row_w"] is not None
        else torch.empty(0, dtype=torch.float32, device=DEV))
    return d


def _step_args(d):
    return (d["Xs"], d["XsT"], d["GT"], d["W"], d["V"], d["WbfT"],
            d["partial"], d["y"], d["fold"], d["col_class"], d["col_fold"],
            d["col_class2"], d["col_lr"], d["col_l2"], d["fmask"],
            d["row_w"])


# ------------------------------------------------------------------ #
# 7. the kernel: one staged step
# ------------------------------------------------------------------ #

# name -> start, m, n, f, fa, column tiles (see test_dense_sgd_kernels_gpu:
# two row tiles and 5 K-tiles; rows >= m and >= n in the only row tile; a
# single K-tile).  w_scale: make_case's weight scale.  At 1 the largest
# spread of z inside a group is about 128 on `tiles`; `tail` has 16 live
# rows to find its extreme in and `onek` 21 terms per dot product where the
# others have 151, so their weights are scaled up to spread z as far.
_SHAPES = {
    "tiles": dict(start=128, m=256, n=400, f=150, fa=160, tiles=2,
                  w_scale=1.0),
    "tail": dict(start=384, m=16, n=400, f=150, fa=160, tiles=1,
                 w_scale=2.0),
    "onek": dict(start=0, m=128, n=128, f=20, fa=32, tiles=1, w_scale=4.0),
}

# (shape, gk, row_w, momentum).  gk: 3 = 42 groups and 2 dead columns per
# tile, groups across the 16-lane fragment and the 64-column wave
# boundaries; 10 a middle case; 43 = 2 groups, 42 dead columns; 64 = groups
# on the wave split; 128 = one group over both column waves.
_STEP_CASES = [
    ("tiles", 3, True, 0.9),
    ("tiles", 10, False, 0.0),
    ("tiles", 43, True, 0.0),
    ("tiles", 64, False, 0.9),
    ("tiles", 128, True, 0.9),
    ("tail", 3, False, 0.9),
    ("tail", 128, True, 0.0),
    ("onek", 10, True, 0.0),
    ("onek", 64, False, 0.9),
]


def _case_id(p):
    shape, gk, rw, mom = p
    return f"{shape}-gk{gk}-mom{mom}{'-roww' if rw else ''}"


@pytest.mark.parametrize("p", _STEP_CASES, ids=_case_id)
def test_staged_softmax_step(p):
    shape, gk, row_w, momentum = p
    s = _SHAPES[shape]
    start, m, n, f, fa = (s[k] for k in ("start", "m", "n", "f", "fa"))
    splitk = 8
    c = S.make_softmax_case(11, n, f, fa, s["tiles"], gk, row_w, momentum,
                            w_scale=s["w_scale"])
    ncp, m_pad = c["ncols_pad"], R.ceil_to(m, 128)
    live = c["live"]
    inv_m = R.inv_m_of(c, start, m)
    lr_scale = 0.5
    mom32 = float(np.float32(momentum))

    # ---- everything the reference alone decides, before any GPU call
    z, g, train, rw = S.ref_gt_softmax(c, start, m)
    assert not train[m:].any() and not train[:, ~live].any()
    assert train[:m][:, live].any() and (~train[:m][:, live]).any()
    assert (~live).any() or gk == 128   # dead or pad columns exist
    spread = max((z[:m, grp].max(axis=1) - z[:m, grp].min(axis=1)).max()
                 for grp in c["cols"].reshape(-1, gk))
    print(f"largest max z - min z in a group: {spread:.1f}")
    assert spread > 88, spread     # an unshifted exp would overflow
    # delta: see the issue's derivation, kept as stated.  The kernel's
    # chain is z - max (rounding of at most |d| 2^-24 on an exponent d,
    # i.e. |d| e^d 2^-24 <= 0.37 * 2^-24 on e, as much again on the sum's
    # share), __expf twice (numerator and sum: 2^-19), K - 1 adds, one
    # correctly rounded divide, one subtract, one multiply: 0.74 + K + 2
    # roundings, within the (K + 3) 2^-24 of the bound.
    delta = S.softmax_delta(c, start, m, train, rw)
    lo, hi = R.bf16_rne(g - delta), R.bf16_rne(g + delta)
    want_gt = R.bf16_rne(g)
    # the sigmoid gradient of the same z is a different number
    t = (np.where(start + np.arange(m_pad) < n,
                  c["y"][np.minimum(start + np.arange(m_pad), n - 1)],
                  0.0)[:, None] == c["col_class"][None, :])
    g_sig = R.dloss(R.LOSS_LOG, z, t.astype(np.float64)) * rw[:, None]
    far = (np.abs(g - g_sig) > 10 * delta)[train].mean()
    print(f"trained elements far from the sigmoid gradient: {far:.3f}")
    assert far > 0.5, far
    # transpose detection: g differs between columns and between rows
    assert np.abs(g[:, 0] - g[:, 2]).max() > 0.1
    assert np.abs(g[0] - g[3]).max() > 0.1

    # ---- one step on the device
    d = _device_step_buffers(c, m, splitk)
    _ext().sgd_step(*_step_args(d), start, m, LOSS_SOFTMAX, lr_scale,
                    momentum, c["intercept_row"], float(inv_m), gk)
    torch.cuda.synchronize()
    GT = _np(d["GT"])
    partial = _np(d["partial"])
    W_got, WbfT_got = _np(d["W"]), _np(d["WbfT"])

    # ---- canaries, stale GT
    for k in ("GT_can", "W_can", "WbfT_can", "partial_can", "V_can"):
        if k in d:
            assert _canary_intact(d[k]), k
    assert (GT[:, m_pad:] == STALE).all(), "K1 wrote past m_pad"

    # ---- K1
    got = GT[:, :m_pad].T                                  # [m_pad, ncp]
    assert np.isfinite(got).all()
    assert (got[~train] == 0).all(), "masked element or dead column not 0"
    bad = np.argwhere((got < lo) | (got > hi))
    err = np.abs(got - g)[train]
    print(f"max |got - g| = {err.max():.3e}, off bf16_rne(g): "
          f"{(got != want_gt)[train].mean():.4%}")
    assert len(bad) == 0, ("GT (row, col)", bad[:8], len(bad))

    # ---- K2, from the GT the device wrote; slab by slab
    xt = c["XsT"][:, start:start + m_pad]
    for zi, (k0, k1) in enumerate(R.slab_bounds(m_pad, splitk)):
        want = xt[:fa, k0:k1] @ GT[:, k0:k1].T
        tol = (k1 - k0) * EPS * (np.abs(xt[:fa, k0:k1])
                                 @ np.abs(GT[:, k0:k1]).T)
        bad = np.argwhere(np.abs(partial[zi] - want) > tol)
        assert len(bad) == 0, ("partial slab", zi, bad[:8], len(bad))
    psum = partial.sum(axis=0)

    # ---- K3, from the slabs the device wrote (bounds: see
    # test_dense_sgd_kernels_gpu.test_staged_step)
    Wn, Vn, tm = R.ref_update(psum, c["W"], c["V"], c["col_lr"],
                              c["col_l2"], None, inv_m,
                              np.float32(lr_scale), mom32,
                              c["intercept_row"])
    tol_w = EPS * (8 * tm["S"] + 3 * tm["M"] + tm["W"]) * (1 + 2.0 ** -10)
    tol_v = EPS * (7 * tm["S"] + 2 * tm["M"]) * (1 + 2.0 ** -10)
    ds = (splitk * EPS * np.abs(partial).sum(axis=0) * float(inv_m)
          * np.abs(c["col_lr"])[None, :] * lr_scale)
    tol_w, tol_v = tol_w + ds, tol_v + ds
    bad = np.argwhere(np.abs(W_got - Wn) > tol_w)
    assert len(bad) == 0, ("W (row, col)", bad[:8], len(bad))
    assert tol_w.max() < 1e-4 * np.abs(Wn - c["W"]).max()
    if momentum > 0:
        bad = np.argwhere(np.abs(_np(d["V"]) - Vn) > tol_v)
        assert len(bad) == 0, ("V (row, col)", bad[:8], len(bad))
    assert np.array_equal(WbfT_got, R.bf16_rne(W_got).T), "WbfT != bf16(W)ᵀ"
    # dead and pad columns and pad feature rows stay exactly 0
    assert (W_got[:, ~live] == 0).all() and (W_got[f + 1:] == 0).all()
    dW = W_got - c["W"]
    assert np.abs(dW[:, 0] - dW[:, 2]).max() > 1e-3
    assert np.abs(dW[0] - dW[3]).max() > 1e-3


# ------------------------------------------------------------------ #
# 8. graph replay
# ------------------------------------------------------------------ #

def test_graph_replay_equals_eager_epochs():
    """sgd_solve(epochs=3) with the softmax loss against three sgd_epoch
    calls, bit for bit in W, V and WbfT (no atomics anywhere)."""
    n, bs, f, fa, gk = 400, 256, 150, 160, 10
    c = S.make_softmax_case(5, n, f, fa, 2, gk, True, 0.9)
    inv_m = torch.tensor([R.inv_m_of(c, s, min(bs, n - s))
                          for s in range(0, n, bs)], dtype=torch.float32)
    outs = []
    for solve in (True, False):
        d = _device_step_buffers(c, bs, 8)
        a = _step_args(d)
        if solve:
            _ext().sgd_solve(*a, inv_m, bs, LOSS_SOFTMAX, 0.9,
                             c["intercept_row"], 3, gk)
        else:
            for _ in range(3):
                _ext().sgd_epoch(*a, inv_m, bs, LOSS_SOFTMAX, 1.0, 0.9,
                                 c["intercept_row"], gk)
        torch.cuda.synchronize()
        for k in ("W_can", "V_can", "WbfT_can", "partial_can", "GT_can"):
            assert _canary_intact(d[k]), k
        outs.append((d["W"].clone(), d["V"].clone(), d["WbfT"].clone()))
    for x, y in zip(*outs):
        assert torch.isfinite(x.float()).all()
        assert torch.equal(x, y)
    moved = outs[0][0].cpu().double().numpy() - c["W"]
    assert np.abs(moved[: f + 1, c["live"]]).max() > 1e-2
    assert (outs[0][0].cpu().numpy()[:, ~c["live"]] == 0).all()


# ------------------------------------------------------------------ #
# 9. solve level
# ------------------------------------------------------------------ #

@pytest.mark.parametrize("K,masked", [(3, False), (10, False), (10, True)])
def test_solve_matches_eager_solver(K, masked):
    """hip_sgd_solve against the eager fp32 solver on the same
    bf16-rounded data, under test_solve_at_tiles_shape_matches_reference's
    criterion.  29 models: the columns fill more than one tile for K = 10
    (12 groups per tile) and leave the last tile part empty for both.
    ``masked`` adds a per-model feature mask (the eliminator's solve),
    which has to follow its columns into the tile layout."""
    from skdist_amd.models._sgd import (
        ColumnSpec, DeviceDataset, batched_sgd_fit)
    from skdist_amd.ops import hip_sgd_solve

    rng = np.random.default_rng(0)
    n, f, nm = 400, 150, 29
    X = R.bf16_rne(rng.standard_normal((n, f))).astype(np.float32)
    y = rng.integers(0, K, size=n)
    fold = torch.as_tensor(rng.integers(0, 3, size=n), dtype=torch.int32)
    mfold = np.array([0, 1, 2, -2])[np.arange(nm) % 4]
    mlr = np.array([0.4, 0.3, 0.2])[np.arange(nm) % 3]
    ml2 = np.array([0.0, 1e-3, 1e-2, 0.0, 1e-4])[np.arange(nm) % 5]
    fmask = None
    if masked:
        fmask = np.ones((160, nm), np.uint8)
        fmask[:f] = rng.random((f, nm)) < 0.7
        fmask = np.repeat(fmask, K, axis=1)

    def solve(device, hip):
        ds = DeviceDataset(X, y, device=device, standardize=False)
        ds.fold_id = fold.to(ds.device)
        spec = ColumnSpec(
            ds.device, np.repeat(mfold, K).astype(np.int32),
            np.tile(np.arange(K, dtype=np.int32), nm),
            np.repeat(mlr, K).astype(np.float32),
            np.repeat(ml2, K).astype(np.float32), group_k=K,
            feat_mask=None if fmask is None else fmask[: ds.fa])
        if hip:
            assert ds.Xaug.shape[1] == 160
            return hip_sgd_solve(ds, spec, LOSS_SOFTMAX, epochs=2,
                                 batch_size=256, seed=0, momentum=0.9,
                                 lr_decay=0.0), f
        W = batched_sgd_fit(ds, spec, LOSS_SOFTMAX, 2, 256, seed=0,
                            momentum=0.9, force_eager=True)
        return W, f

    W_hip, _ = solve("cuda", True)
    W_ref, _ = solve("cpu", False)
    assert tuple(W_hip.shape) == (160, nm * K)     # compact, model-major
    got = W_hip.cpu().float()
    assert (got[f + 1:] == 0).all()
    got = got[: f + 1]
    if masked:
        off = torch.as_tensor(fmask[: f + 1] == 0)
        assert off.any() and (got[off] == 0).all() and (W_ref[off] == 0).all()
        assert (got[~off] != 0).float().mean() > 0.99
    diff = (got - W_ref).abs().max().item()
    scale = W_ref.abs().max().item()
    print(f"softmax solve K={K} masked={masked}: diff={diff:.3e} "
          f"scale={scale:.3e}")
    assert diff < max(2e-3, 2e-3 * scale), (K, diff, scale)
    # order: every model against its own fold, lr and l2
    assert (W_ref[:, 0] - W_ref[:, K]).abs().max() > 1e-3
    assert (W_ref[0] - W_ref[3]).abs().max() > 1e-3


# ------------------------------------------------------------------ #
# 10. end to end
# ------------------------------------------------------------------ #

# max |P - P_sklearn| of the device fit on iris, measured on an MI355X
# (docs/BENCHMARKS.md, "Multinomial"): the fit holds X in bf16
IRIS_MEASURED = 7.8e-4


def test_device_fit_matches_sklearn_on_iris():
    from skdist_amd.models import LogisticRegression

    X, y = S.load("iris")
    P_sk, P_sk_ovr = S.sklearn_probas("iris")
    est = LogisticRegression(C=0.1, multi_class="multinomial", epochs=400,
                             batch_size=8192, random_state=0).fit(X, y)
    P = est.predict_proba(X)
    d = np.abs(P - P_sk).max()
    print(f"iris on device: max|P - P_sklearn| = {d:.3e}")
    assert d <= min(4 * IRIS_MEASURED, 0.02), d
    assert est.coef_.shape == (3, 4)
    assert np.abs(P_sk - P_sk_ovr).max() >= 0.115
    # the device inference hook has the same softmax split
    fn = est._device_predict_fn("predict_proba", "cuda")
    np.testing.assert_allclose(fn(X), P, atol=1e-5)
    np.testing.assert_allclose(fn(X).sum(axis=1), 1.0, atol=1e-6)


def test_device_grid_search_matches_cpu_batched_path():
    from sklearn.datasets import load_digits

    from skdist_amd.distribute.search import DistGridSearchCV
    from skdist_amd.models import LogisticRegression
    from skdist_amd.parallel import Cluster

    X, y = load_digits(return_X_y=True)
    grid = {"C": [0.1, 0.5, 2.0]}
    est = LogisticRegression(multi_class="multinomial", epochs=100,
                             random_state=0)
    sc = Cluster()
    assert sc.device.type == "cuda"
    gpu = DistGridSearchCV(est, grid, cv=3, scoring="neg_log_loss", sc=sc)
    gpu.fit(X, y)
    cpu = DistGridSearchCV(est, grid, cv=3, scoring="neg_log_loss",
                           sc=Cluster(device="cpu"))
    cpu.fit(X, y)
    a = gpu.cv_results_["mean_test_score"]
    b = cpu.cv_results_["mean_test_score"]
    print("device", a, "cpu", b)
    assert np.allclose(a, b, atol=0.02), (a, b)
    assert gpu.best_estimator_.multi_class == "multinomial"
    assert gpu.best_estimator_.coef_.shape == (10, 64)


def test_more_than_128_classes_is_refused_on_device():
    from skdist_amd.models import LogisticRegression

    rng = np.random.default_rng(0)
    X = rng.standard_normal((260, 8)).astype(np.float32)
    y = np.arange(260) % 130
    est = LogisticRegression(multi_class="multinomial", epochs=1)
    with pytest.raises(ValueError, match="128"):
        est.fit(X, y)


# ------------------------------------------------------------------ #
# 11. binding rejects
# ------------------------------------------------------------------ #

def test_bindings_reject_bad_group_and_loss():
    ext = _ext()
    c = S.make_softmax_case(3, 128, 20, 32, 1, 10, False, 0.9)
    d = _device_step_buffers(c, 128, 8)
    a = _step_args(d)
    ir = c["intercept_row"]
    inv_m = torch.tensor([1 / 128.0], dtype=torch.float32)
    before = {k: d[k].clone() for k in ("GT", "W", "V", "WbfT", "partial")}

    def unchanged():
        torch.cuda.synchronize()
        return all(torch.equal(d[k], v) for k, v in before.items())

    bad = [(3, 0), (3, 1), (3, 129), (3, -1), (0, 10), (1, 2), (2, 128),
           (4, 0), (-1, 0), (7, 10)]
    for loss_id, gk in bad:
        with pytest.raises(RuntimeError):
            ext.sgd_step(*a, 0, 128, loss_id, 1.0, 0.9, ir, 1 / 128.0, gk)
        with pytest.raises(RuntimeError):
            ext.sgd_epoch(*a, inv_m, 128, loss_id, 1.0, 0.9, ir, gk)
        with pytest.raises(RuntimeError):
            ext.sgd_solve(*a, inv_m, 128, loss_id, 0.9, ir, 2, gk)
        assert unchanged(), (loss_id, gk)
    l1 = (torch.zeros(c["ncols_pad"], device=DEV),
          torch.zeros_like(d["W"]), torch.zeros_like(d["W"]))
    for loss_id, gk in [(3, 0), (0, 10), (5, 0)]:
        with pytest.raises(RuntimeError):
            ext.sgd_epoch_l1(*a, inv_m, 128, loss_id, 1.0, 0.9, ir, *l1, gk)
        with pytest.raises(RuntimeError):
            ext.sgd_solve_l1(*a, inv_m, 128, loss_id, 0.9, ir, 2, *l1, gk)
        assert unchanged(), (loss_id, gk)
    # softmax without the trailing argument is a rejected call, not a
    # squared-loss step
    with pytest.raises(RuntimeError):
        ext.sgd_step(*a, 0, 128, 3, 1.0, 0.9, ir, 1 / 128.0)
    assert unchanged()

    # every positional form of tests/test_dense_sgd_kernels_gpu.py still
    # runs, and group_k may be named
    ext.sgd_step(*a, 0, 128, 0, 1.0, 0.9, ir, 1 / 128.0)
    ext.sgd_epoch(*a, inv_m, 128, 0, 1.0, 0.9, ir)
    ext.sgd_solve(*a, inv_m, 128, 0, 0.9, ir, 3)
    ext.sgd_epoch_l1(*a, inv_m, 128, 0, 1.0, 0.9, ir, *l1)
    ext.sgd_solve_l1(*a, inv_m, 128, 0, 0.9, ir, 2, *l1)
    ext.sgd_step(*a, 0, 128, 3, 1.0, 0.9, ir, 1 / 128.0, group_k=10)
    ext.sgd_solve_l1(*a, inv_m, 128, 3, 0.9, ir, 2, *l1, 10)
    torch.cuda.synchronize()
    assert not unchanged()
    assert torch.isfinite(d["W"]).all()
    for k in ("W_can", "V_can", "WbfT_can", "partial_can", "GT_can"):
        assert _canary_intact(d[k]), k
