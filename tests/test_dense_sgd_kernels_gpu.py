"""
The dense batched SGD kernels (ops/csrc/sgd_kernels.hip), one kernel at a
time against the float64 references of tests/_dense_ref.py.

One ``ext.sgd_step`` call runs K1 (k_fwd_gt), K2 (k_grad_partial) and K3
(k_reduce_update).  Each kernel is compared with the reference fed with
what the previous kernel actually wrote, so a failure names one kernel.
With dyadic inputs (hinge, squared loss) every fp32 sum is exact in any
order and the comparison is bit for bit; with random inputs (log loss) an
element may leave the reference's bf16 value only where the reference lies
within a derived distance of a bf16 rounding boundary.

Shapes are the smallest that reach each tile edge; see ``_SHAPES``.
"""

import numpy as np
import pytest
import torch

import _dense_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = R.EPS32
CANARY = 12345.0   # finite, and no kernel result equals it
STALE = 7.0        # pre-fill of GT; past m_pad it must stay


def _ext():
    from skdist_amd.ops import require_hip

    return require_hip()


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
    """``values`` [r, ...] as the leading rows of a larger allocation whose
    trailing ``extra_rows`` rows hold CANARY; narrowing dim 0 of a
    contiguous tensor keeps it contiguous.  Returns (view, canary view)."""
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
    """Upload one case.  GT, partial, W, V and WbfT sit in front of canary
    rows; GT is 128 columns wider than m_pad and pre-filled with STALE."""
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
    d["fmask"] = (
        torch.tensor(c["fmask"], dtype=torch.uint8, device=DEV)
        if c["fmask"] is not None
        else torch.empty(0, dtype=torch.uint8, device=DEV))
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
# staged single-step tests
# ------------------------------------------------------------------ #

# name -> start, m, n, f (fa), ncols.  What each reaches:
#  tiles: 2 row tiles in K1; 2 column tiles in K1/K2/K3; 2 feature tiles in
#         K2 with the `row < fa` guard live (fa = 160 < fa_store = 256);
#         5 K-tiles in K1
#  tail:  rows >= m and >= n masked in the only row tile; with splitk = 8
#         slabs 4..7 are empty (k0 >= k1)
#  deepk: slabs of 64 rows (K2's own double buffering) at splitk 8; an
#         uneven last slab (192/192/128) at 3; one slab of 512 at 1
#  onek:  fa = 32, a single K-tile in K1 (nk == 1, nothing prefetched)
_SHAPES = {
    "tiles": dict(start=128, m=256, n=400, f=150, fa=160, ncols=130),
    "tail": dict(start=384, m=16, n=400, f=150, fa=160, ncols=130),
    "deepk": dict(start=0, m=512, n=512, f=37, fa=64, ncols=9),
    "onek": dict(start=0, m=128, n=128, f=20, fa=32, ncols=9),
}

# (shape, splitk, loss, momentum, ovo, row_w, fmask).  Every option, on and
# off, and every loss appears on `tiles`; the other shapes take each loss
# and both momenta once and vary the rest.
_STEP_CASES = [
    ("tiles", 8, 0, 0.9, True, True, True),
    ("tiles", 8, 1, 0.9, True, True, True),
    ("tiles", 8, 2, 0.9, True, True, True),
    ("tiles", 8, 0, 0.0, False, False, False),
    ("tiles", 8, 1, 0.0, True, False, False),
    ("tiles", 8, 2, 0.0, False, False, False),
    ("tail", 8, 0, 0.9, True, True, False),
    ("tail", 8, 1, 0.0, True, False, True),
    ("tail", 8, 2, 0.9, True, True, False),
    ("deepk", 8, 0, 0.9, True, True, True),
    ("deepk", 8, 1, 0.0, True, False, False),
    ("deepk", 8, 2, 0.9, True, True, True),
    ("deepk", 3, 0, 0.0, True, False, False),
    ("deepk", 3, 2, 0.9, True, True, False),
    ("deepk", 1, 1, 0.9, True, False, True),
    ("deepk", 1, 2, 0.0, True, True, False),
    ("onek", 8, 0, 0.9, True, False, True),
    ("onek", 8, 1, 0.9, True, True, False),
    ("onek", 8, 2, 0.0, True, False, False),
]


def _case_id(p):
    shape, splitk, loss, mom, ovo, rw, fm = p
    return (f"{shape}-k{splitk}-loss{loss}-mom{mom}"
            f"{'-ovo' if ovo else ''}{'-roww' if rw else ''}"
            f"{'-fmask' if fm else ''}")


def _assert_exact_preconditions(c, start, m_pad, z):
    """Dyadic inputs: x is a multiple of 1/2, w of 1/8, row_w of 1/2, so
    every K1 product is a multiple of 2^-4, g (and its bf16 rounding, a
    coarser dyadic grid) a multiple of 2^-5, and every K2 product a
    multiple of 2^-6.  When the largest sum of magnitudes is below 2^24
    grid units, every partial sum in any order is an integer below 2^24 in
    grid units, hence an fp32 value: accumulation is exact."""
    xb = c["Xs"][start:start + m_pad]
    assert np.array_equal(xb * 2, np.round(xb * 2))
    assert np.array_equal(c["W"] * 8, np.round(c["W"] * 8))
    k1 = (np.abs(xb) @ np.abs(c["W"])).max() / 2.0 ** -4
    assert k1 < 2 ** 24, k1
    # g = (z - t) * row_w: |z| + 2 bounds |z - t|, row_w <= 2
    gmax = (np.abs(z).max() + 2.0) * 2.0
    assert gmax / 2.0 ** -5 < 2 ** 24
    # K2, all slabs together (covers each slab and K3's sum of slabs)
    k2 = np.abs(xb).sum(axis=0).max() * gmax / 2.0 ** -6
    assert k2 < 2 ** 24, k2


@pytest.mark.parametrize("p", _STEP_CASES, ids=_case_id)
def test_staged_step(p):
    shape, splitk, loss_id, momentum, ovo, row_w, fmask = p
    s = _SHAPES[shape]
    start, m, n, f, fa, ncols = (s[k] for k in
                                 ("start", "m", "n", "f", "fa", "ncols"))
    exact = loss_id != R.LOSS_LOG
    c = R.make_case(11, n, f, fa, ncols, loss_id, dyadic=exact, ovo=ovo,
                    row_w=row_w, fmask=fmask, momentum=momentum)
    ncp, m_pad = c["ncols_pad"], R.ceil_to(m, 128)
    inv_m = R.inv_m_of(c, start, m)
    lr_scale = 0.5
    mom32 = float(np.float32(momentum))

    # ---- everything the reference alone decides, before any GPU call
    z, g, train = R.ref_gt(c["Xs"], c["W"].T, c["y"], c["fold"],
                           c["col_class"], c["col_fold"], c["col_class2"],
                           c["row_w"], start, m, loss_id)
    assert not train[m:].any() and train[:m, :ncols].any()
    assert (~train[:m, :ncols]).any()          # masks are live
    want_gt = R.bf16_rne(g)
    if exact:
        _assert_exact_preconditions(c, start, m_pad, z)
        lo = hi = want_gt
    else:
        # dz: fp32 accumulation of fa products, each add rounding a
        # running sum of at most sum|x||w|.  sigmoid' <= 1/4 carries dz/4
        # into g; 2^-20 stands for __expf and the three fp32 roundings
        # after it (no accuracy table for __expf ships with the ROCm
        # documentation available to this project, so the issue's fallback
        # figure is used); row_w scales both.  A kernel value is right
        # when it is the bf16 rounding of SOME value within delta of the
        # reference: lo <= got <= hi.  Where lo == hi that is equality
        # with bf16_rne(reference); elsewhere the reference lies within
        # delta of a rounding boundary, and such elements must be rare.
        dz = fa * EPS * (np.abs(c["Xs"][start:start + m_pad])
                         @ np.abs(c["W"]))
        rw = np.ones(m_pad)
        if c["row_w"] is not None:
            ok = start + np.arange(m_pad) < n
            rw[ok] = c["row_w"][start:start + m_pad][: ok.sum()]
        delta = np.where(train, (dz / 4 + 2.0 ** -20) * rw[:, None], 0.0)
        lo, hi = R.bf16_rne(g - delta), R.bf16_rne(g + delta)
        near = lo != hi
        print(f"near a bf16 boundary: {near.mean():.4%} of the tile")
        assert near.mean() <= 0.01, near.mean()
        assert (np.abs(z) > 30).any()          # the clamp is reached
    # transpose detection: g differs between columns and between rows
    assert np.abs(g[:, 0] - g[:, 2]).max() > 0.1
    assert np.abs(g[0] - g[3]).max() > 0.1

    # ---- one step on the device
    d = _device_step_buffers(c, m, splitk)
    _ext().sgd_step(*_step_args(d), start, m, loss_id, lr_scale, momentum,
                    c["intercept_row"], float(inv_m))
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
    assert (got[~train] == 0).all(), "masked element not 0"
    if exact:
        bad = np.argwhere(got != want_gt)
        assert len(bad) == 0, ("GT (row, col)", bad[:8], len(bad))
    else:
        bad = np.argwhere((got < lo) | (got > hi))
        assert len(bad) == 0, ("GT (row, col)", bad[:8], len(bad))
        # ... and a near-boundary element is at most one bf16 step off
        step1 = R.bf16_step(np.abs(g) + delta)
        assert (np.abs(got - want_gt) <= step1)[near].all()

    # ---- K2, from the GT the device wrote; slab by slab
    xt = c["XsT"][:, start:start + m_pad]
    for zi, (k0, k1) in enumerate(R.slab_bounds(m_pad, splitk)):
        want = xt[:fa, k0:k1] @ GT[:, k0:k1].T
        if exact:
            bad = np.argwhere(partial[zi] != want)
        else:
            # at most k1 - k0 adds, each rounding a running sum of at
            # most sum|x||g|
            tol = (k1 - k0) * EPS * (np.abs(xt[:fa, k0:k1])
                                     @ np.abs(GT[:, k0:k1]).T)
            bad = np.argwhere(np.abs(partial[zi] - want) > tol)
        assert len(bad) == 0, ("partial slab", zi, bad[:8], len(bad))
    psum = partial.sum(axis=0)
    want_sum = R.ref_partial_sum(c["XsT"], GT, start, m_pad)[:fa]
    if exact:
        assert np.array_equal(psum, want_sum)

    # ---- K3, from the slabs the device wrote
    Wn, Vn, t = R.ref_update(psum, c["W"], c["V"], c["col_lr"], c["col_l2"],
                             c["fmask"], inv_m, np.float32(lr_scale), mom32,
                             c["intercept_row"])
    # fp32 chain of K3 with eps = 2^-24, any FMA contraction allowed:
    #   grad = s*inv_m + l2*w      <= 3 eps (|a| + |b|)
    #   step = (lr*ls) * grad      <= |lr ls| err(grad) + 2 eps |step|
    #                              <= 5 eps S,  S = |lr ls| (|a| + |b|)
    #   v    = V*mom + step        <= err(step) + 2 eps (M + S), M = |V mom|
    #   w'   = w - v               <= err(v) + eps (|w| + M + S)
    # so err(v) <= eps (7 S + 2 M) and err(w') <= eps (8 S + 3 M + |w|).
    # s itself is exact with dyadic inputs; otherwise summing splitk
    # slabs in fp32 adds splitk roundings of at most sum|partial_z|.
    tol_w = EPS * (8 * t["S"] + 3 * t["M"] + t["W"]) * (1 + 2.0 ** -10)
    tol_v = EPS * (7 * t["S"] + 2 * t["M"]) * (1 + 2.0 ** -10)
    if not exact:
        ds = (splitk * EPS * np.abs(partial).sum(axis=0) * float(inv_m)
              * np.abs(c["col_lr"])[None, :] * lr_scale)
        tol_w, tol_v = tol_w + ds, tol_v + ds
    bad = np.argwhere(np.abs(W_got - Wn) > tol_w)
    assert len(bad) == 0, ("W (row, col)", bad[:8], len(bad))
    # a few ulps, not a loose number: far below the step itself
    assert tol_w.max() < 1e-4 * np.abs(Wn - c["W"]).max()
    if momentum > 0:
        bad = np.argwhere(np.abs(_np(d["V"]) - Vn) > tol_v)
        assert len(bad) == 0, ("V (row, col)", bad[:8], len(bad))
    assert np.array_equal(WbfT_got, R.bf16_rne(W_got).T), "WbfT != bf16(W)ᵀ"
    # pad columns and pad feature rows stay exactly 0; fmask pins to 0
    assert (W_got[:, ncols:] == 0).all() and (W_got[f + 1:] == 0).all()
    if c["fmask"] is not None:
        off = c["fmask"] == 0
        assert off.any() and (W_got[off] == 0).all()
        if momentum > 0:
            assert (_np(d["V"])[off] == 0).all()
    # the step moved W, differently across columns and across rows
    dW = W_got - c["W"]
    assert np.abs(dW[:, 0] - dW[:, 2]).max() > 1e-3
    assert np.abs(dW[0] - dW[3]).max() > 1e-3


# ------------------------------------------------------------------ #
# graph replay and solve level
# ------------------------------------------------------------------ #

def test_graph_replay_equals_eager_epochs():
    """sgd_solve(epochs=3) replays a captured epoch twice; three
    sgd_epoch(lr_scale=1) calls launch the same kernels eagerly.  No
    kernel uses atomics and the slabs are summed in a fixed order, so the
    two must agree bit for bit -- which they only do if the replay carries
    every batch's own start / m / 1/m."""
    n, bs, f, fa, ncols = 400, 256, 150, 160, 130
    c = R.make_case(5, n, f, fa, ncols, R.LOSS_LOG, dyadic=False,
                    row_w=True, fmask=True, momentum=0.9)
    inv_m = torch.tensor([R.inv_m_of(c, s, min(bs, n - s))
                          for s in range(0, n, bs)], dtype=torch.float32)
    outs = []
    for solve in (True, False):
        d = _device_step_buffers(c, bs, 8)
        a = _step_args(d)
        if solve:
            _ext().sgd_solve(*a, inv_m, bs, R.LOSS_LOG, 0.9,
                             c["intercept_row"], 3)
        else:
            for _ in range(3):
                _ext().sgd_epoch(*a, inv_m, bs, R.LOSS_LOG, 1.0, 0.9,
                                 c["intercept_row"])
        torch.cuda.synchronize()
        for k in ("W_can", "V_can", "WbfT_can", "partial_can", "GT_can"):
            assert _canary_intact(d[k]), k
        outs.append((d["W"].clone(), d["V"].clone(), d["WbfT"].clone()))
    for x, y in zip(*outs):
        assert torch.isfinite(x.float()).all()
        assert torch.equal(x, y)
    moved = (outs[0][0].cpu().double().numpy() - c["W"])
    assert np.abs(moved[: f + 1, :ncols]).max() > 1e-2


@pytest.mark.parametrize("loss_id", [0, 1, 2])
def test_solve_at_tiles_shape_matches_reference(loss_id):
    """hip_sgd_solve at the multi-tile shape (two row tiles, two column
    tiles, fa = 160) against the number flow of
    test_gpu_kernels._ref_solve, under that test's criterion."""
    from test_gpu_kernels import _bf16_round, _ref_solve

    from skdist_amd.models._sgd import ColumnSpec, DeviceDataset
    from skdist_amd.ops import hip_sgd_solve

    torch.manual_seed(0)
    n, f, ncols = 400, 150, 130
    X = _bf16_round(torch.randn(n, f))
    yb = (torch.rand(n) < 0.5).float()
    fold = torch.randint(0, 3, (n,), dtype=torch.int32)
    col_class = torch.tensor([1, 1, 1, -1, -1, 1, 1, 1, 1] * 15)[:ncols]
    col_class = col_class.to(torch.int32)
    col_fold = torch.tensor([0, 1, 2, -2, 0, 1, 2, 0, 1] * 15,
                            dtype=torch.int32)[:ncols]
    col_lr = torch.tensor([0.4, 0.3, 0.2] * 44)[:ncols]
    col_l2 = torch.tensor([0.0, 1e-3, 1e-2, 0.0, 1e-4] * 26)[:ncols]

    ds = DeviceDataset(X.numpy(), yb.numpy().astype(np.float32),
                       device="cuda", standardize=False)
    ds.fold_id = fold.to(ds.device)
    spec = ColumnSpec(ds.device, col_fold.numpy(), col_class.numpy(),
                      col_lr.numpy(), col_l2.numpy())
    W_hip = hip_sgd_solve(ds, spec, loss_id, epochs=2, batch_size=256,
                          seed=0, momentum=0.9, lr_decay=0.0)
    fa = ds.Xaug.shape[1]
    assert fa == 160
    Xref = torch.zeros(n, fa)
    Xref[:, :f] = X
    Xref[:, ds.intercept_row] = 1.0
    W_ref = _ref_solve(Xref, yb, fold, col_class, col_fold, col_lr, col_l2,
                       loss_id, 2, 256, 0, 0.9, ds.intercept_row)
    got = W_hip.cpu().float()
    diff = (got - W_ref).abs().max().item()
    scale = W_ref.abs().max().item()
    print(f"solve tiles loss={loss_id}: diff={diff:.3e} scale={scale:.3e}")
    assert diff < max(2e-3, 2e-3 * scale), (loss_id, diff, scale)
    assert (W_ref[:, 0] - W_ref[:, 2]).abs().max() > 1e-3
    assert (W_ref[0] - W_ref[3]).abs().max() > 1e-3


# ------------------------------------------------------------------ #
# k_score, called directly
# ------------------------------------------------------------------ #

def _score_inputs(seed, m, m_pad, f, fa, ncols, dyadic, y_kind):
    """Fold buffers as _score_fold_hip builds them, except that the pad
    rows of Xf hold data too: only the sentinel may exclude a row."""
    rng = np.random.default_rng(seed)
    ncp = R.ceil_to(ncols, 128)
    Xf = np.zeros((m_pad, fa))
    Wt = np.zeros((ncp, fa))
    if dyadic:
        Xf[:, :f] = rng.integers(-2, 3, size=(m_pad, f)) / 2.0
        Wt[:ncols, :f + 1] = rng.integers(-4, 5, size=(ncols, f + 1)) / 8.0
    else:
        Xf[:, :f] = R.bf16_rne(rng.standard_normal((m_pad, f)))
        Wt[:ncols, :f + 1] = R.bf16_rne(
            rng.standard_normal((ncols, f + 1)) / 4.0)
    Xf[:, f] = 1.0
    yf = np.full(m_pad, R.PAD_SENTINEL)
    if y_kind == "binary":
        yf[:m] = rng.integers(0, 2, size=m)
    else:
        yf[:m] = np.float32(rng.standard_normal(m) * 2.0 + 1.0)
    return Xf, Wt, yf.astype(np.float32).astype(np.float64)


_SCORE_SHAPES = [(m, m_pad, f, fa)
                 for (m, m_pad) in ((1, 128), (130, 384), (384, 384))
                 for (f, fa) in ((20, 32), (150, 160))]


def _run_score(Xf, Wt, yf, mode):
    nstat = 2 if mode == 0 else 1
    ncp = Wt.shape[0]
    stats, can = _guarded(np.zeros((ncp * nstat,)), torch.float32, 128)
    _ext().score_fold(_bf(Xf), _bf(Wt),
                      torch.tensor(yf, dtype=torch.float32, device=DEV),
                      stats, mode)
    torch.cuda.synchronize()
    assert _canary_intact(can)
    return _np(stats).reshape(ncp, nstat)


@pytest.mark.parametrize("m,m_pad,f,fa", _SCORE_SHAPES)
def test_score_fold_accuracy_counts_exact(m, m_pad, f, fa):
    ncols = 130
    Xf, Wt, yf = _score_inputs(1, m, m_pad, f, fa, ncols, True, "binary")
    hits, valid, z = R.ref_score(Xf, Wt, yf, 0)
    # dyadic inputs (grid 2^-4), sums below 2^24 grid units: z is exact in
    # fp32 whatever the order, so its sign -- 0 included -- is the
    # reference's and the counts admit no tolerance
    assert (np.abs(Xf) @ np.abs(Wt).T).max() / 2.0 ** -4 < 2 ** 24
    assert (z == 0).any() or m == 1
    got = _run_score(Xf, Wt, yf, 0)
    assert np.array_equal(got[:, 1], np.full(len(got), float(m)))
    assert np.array_equal(got[:, 0], hits)
    assert len(np.unique(hits[:ncols])) > 1 or m == 1


@pytest.mark.parametrize("m,m_pad,f,fa", _SCORE_SHAPES)
def test_score_fold_sse(m, m_pad, f, fa):
    ncols = 130
    Xf, Wt, yf = _score_inputs(2, m, m_pad, f, fa, ncols, False, "real")
    sse, z, valid = R.ref_score(Xf, Wt, yf, 1)
    got = _run_score(Xf, Wt, yf, 1)[:, 0]
    # e = z - y in fp32: z carries dz = fa eps sum|x||w| (fp32
    # accumulation), the subtraction eps |e|; e^2 then moves by at most
    # 2 |e| dz + dz^2, plus 3 eps e^2 for the subtraction (twice, through
    # the square) and the product.  Summing at most m_pad terms per
    # column in fp32, in any order and through the LDS and global atomics,
    # adds m_pad roundings of a running sum of at most sse.
    dz = fa * EPS * (np.abs(Xf) @ np.abs(Wt).T)
    e = np.abs(np.where(valid[:, None], z - yf[:, None], 0.0))
    tol = ((2 * e * dz + dz * dz) * valid[:, None]).sum(axis=0) \
        + (m_pad + 3) * EPS * sse
    err = np.abs(got - sse)
    print(f"sse m={m} fa={fa}: max err/tol = {(err / tol).max():.3f}, "
          f"max rel err = {(err / sse).max():.3e}")
    assert (err <= tol).all(), (err.max(), tol[err.argmax()])
    assert np.median(tol / sse) < 1e-3    # the bound itself is tight
    assert len(np.unique(sse[:ncols])) == ncols


# ------------------------------------------------------------------ #
# r2 / mse end to end: targets with an offset
# ------------------------------------------------------------------ #

def _offset_regression(ratio):
    """y = mu + x.w + noise with mu / std(y) = ratio; mu and sigma are
    chosen so that mu is a bf16 value (it becomes the intercept weight)."""
    sigma, mu = {0: (1.0, 0.0), 100: (1.28, 128.0),
                 10000: (1.024, 10240.0)}[ratio]
    rng = np.random.default_rng(4)
    n, f = 1203, 6
    X = R.bf16_rne(rng.standard_normal((n, f)))
    w = R.bf16_rne(rng.standard_normal(f) * 0.4)
    y = X @ w + 0.3 * rng.standard_normal(n)
    scale = sigma / y.std()
    y = mu + scale * (y - y.mean())
    W = np.zeros((f + 1, 3))
    W[:f, 0], W[f, 0] = R.bf16_rne(w * scale), mu
    W[:f, 1], W[f, 1] = R.bf16_rne(W[:f, 0] * 0.5), mu   # a worse model
    W[f, 2] = R.bf16_rne(mu + sigma / 8)                 # a constant
    return X.astype(np.float32), y.astype(np.float32), W


@pytest.mark.parametrize("metric", ["r2", "neg_mean_squared_error"])
@pytest.mark.parametrize("ratio", [0, 100, 10000])
def test_regression_scores_with_offset_targets(ratio, metric):
    """batched_scores_by_fold through k_score on targets mu + noise,
    against float64 from the same bf16 operands.

    Measured on an MI355X while r2's total sum of squares was still
    syy - sy*sy/m from fp32 atomic sums: r2 errors of 0.058 to 6e14 at
    mu/sigma = 1e4 (bound here: 8e-3 to 3e-2) and up to 7.2e-4 at 1e2
    (bound: 3.4e-4), so both cases failed.  With the float64 sum of
    squares: at most 3.9e-4 at 1e4 and 7.4e-7 at 1e2."""
    from skdist_amd.models._sgd import DeviceDataset, batched_scores_by_fold

    X, y, W = _offset_regression(ratio)
    n, f = X.shape
    ds = DeviceDataset(X, y, device=DEV, standardize=False, task="reg")
    fold = (np.arange(n) % 2).astype(np.int32)
    ds.fold_id = torch.tensor(fold, device=ds.device)
    fa = ds.Xaug.shape[1]
    Wfull = np.zeros((fa, 6))
    Wfull[: f + 1] = np.concatenate([W, W], axis=1)
    model_folds = np.array([0, 0, 0, 1, 1, 1])
    got = batched_scores_by_fold(
        ds, torch.tensor(Wfull, dtype=torch.float32, device=ds.device),
        model_folds, np.full(6, -1, np.int32), 1, metric)

    Xa = _np(ds.Xaug)
    yd = y.astype(np.float64)
    for k in range(6):
        rows = fold == model_folds[k]
        m = int(rows.sum())
        m_pad = R.ceil_to(m, 128)
        wk = R.bf16_rne(Wfull[:, k])
        zk = Xa[rows] @ wk
        e = np.abs(zk - yd[rows])
        sse = (e * e).sum()
        sst = ((yd[rows] - yd[rows].mean()) ** 2).sum()
        # the sse bound of test_score_fold_sse, carried through
        # 1 - sse/sst (sst is float64 on both sides) or -sse/m
        dz = fa * EPS * (np.abs(Xa[rows]) @ np.abs(wk))
        dsse = (2 * e * dz + dz * dz).sum() + (m_pad + 3) * EPS * sse
        if metric == "r2":
            want, tol = 1.0 - sse / sst, dsse / sst
        else:
            want, tol = -sse / m, dsse / m
        print(f"{metric} mu/sigma={ratio} model {k}: got={got[k]:.6g} "
              f"want={want:.6g} err={abs(got[k] - want):.3e} "
              f"tol={tol:.3e}")
        assert abs(got[k] - want) <= tol, (k, got[k], want, tol)
    if metric == "r2":
        assert got[0] > 0.8 and got[1] < got[0] - 0.1 and got[2] < 0.05


# ------------------------------------------------------------------ #
# k_standardize, called directly
# ------------------------------------------------------------------ #

@pytest.mark.parametrize("n,f,fa", [
    (1, 7, 8),        # one chunk
    (5, 31, 32),      # the intercept is the last element of a row
    (300, 32, 64),    # an intercept chunk, then chunks of pure pad
    (300, 37, 64),    # one chunk straddles real, intercept and pad
    (2051, 3, 8),     # chunk count not a multiple of the block size
])
def test_standardize_bits(n, f, fa):
    rng = np.random.default_rng(n)
    X = (rng.standard_normal((n, f)) * 3 + 1).astype(np.float32)
    mean = rng.standard_normal(f).astype(np.float32)
    inv_std = (1.0 / rng.uniform(0.5, 2.0, f)).astype(np.float32)
    # exact bf16 ties in column 0: truncation would give 1 + 2^-7 for the
    # second and round-half-up 1 + 2^-7 for the first; RNE gives 1 and
    # 1 + 2^-6
    mean[0], inv_std[0] = 0.0, 1.0
    X[0::2, 0] = 1.0 + 2.0 ** -8
    X[1::2, 0] = 1.0 + 3 * 2.0 ** -8
    want = R.ref_standardize(X, mean, inv_std, fa)
    assert want[0, 0] == 1.0 and (n == 1 or want[1, 0] == 1.0 + 2.0 ** -6)

    out, can = _guarded(np.full((n, fa), CANARY), torch.bfloat16, 4)
    t = lambda a: torch.tensor(a, device=DEV)
    _ext().standardize(t(X), t(mean), t(inv_std), out, f)
    torch.cuda.synchronize()
    assert _canary_intact(can)
    got = _np(out)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:8], len(bad))
    assert (got[:, f] == 1.0).all() and (got[:, f + 1:] == 0).all()


def test_standardize_rejects_bad_arguments():
    n, f = 16, 5
    t = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    out8 = t(n, 8, dt=torch.bfloat16)
    ext = _ext()
    ext.standardize(t(n, f), t(f), t(f), out8, f)           # the good call
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.standardize(t(n, f), t(f), t(f), t(n, 12, dt=torch.bfloat16), f)
    with pytest.raises(RuntimeError, match="mean"):
        ext.standardize(t(n, f), t(f + 8), t(f), out8, f)
    with pytest.raises(RuntimeError, match="inv_std"):
        ext.standardize(t(n, f), t(f), t(f, dt=torch.float64), out8, f)
    with pytest.raises(RuntimeError, match="X"):
        ext.standardize(t(n, f, dt=torch.float64), t(f), t(f), out8, f)
    with pytest.raises(RuntimeError, match="out"):
        ext.standardize(t(n, f), t(f), t(f), t(n, 8), f)
    with pytest.raises(RuntimeError, match="f must be"):
        ext.standardize(t(n, 8), t(8), t(8), out8, 8)       # no room for 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ #
# binding checks.  Every bad tensor is as large as the good one or larger
# (or a view into a larger allocation), so a missing check shows as "did
# not raise" and never as an access outside an allocation.
# ------------------------------------------------------------------ #

def _good_step_buffers():
    n, f, fa, ncols = 256, 20, 32, 9
    c = R.make_case(1, n, f, fa, ncols, R.LOSS_LOG, dyadic=False,
                    row_w=True, fmask=True, momentum=0.9)
    d = _device_step_buffers(c, 128, 2)
    # Xs / XsT as views into larger allocations: a batch past n_pad, if a
    # missing check let it launch, would still read allocated memory
    big = torch.zeros(c["n_pad"] * 2, fa, dtype=torch.bfloat16, device=DEV)
    big[: c["n_pad"]] = d["Xs"]
    d["Xs"] = big.narrow(0, 0, c["n_pad"])
    bigT = torch.zeros(c["fa_store"] + 128, c["n_pad"],
                       dtype=torch.bfloat16, device=DEV)
    bigT[: c["fa_store"]] = d["XsT"]
    d["XsT"] = bigT.narrow(0, 0, c["fa_store"])
    return c, d


def _z(shape, dt):
    return torch.zeros(*shape, dtype=dt, device=DEV)


# name of the replaced argument -> (builder of the bad tensor from the good
# buffers, text the error must carry)
_BAD_TENSORS = {
    "y_f64": ("y", lambda d: d["y"].double(), "y must"),
    "fold_i64": ("fold", lambda d: d["fold"].long(), "fold must"),
    "fold_long": ("fold", lambda d: _z((d["fold"].numel() + 128,),
                                       torch.int32), "fold must"),
    "col_class_i64": ("col_class", lambda d: d["col_class"].long(),
                      "col_class must"),
    "col_fold_long": ("col_fold", lambda d: _z((256,), torch.int32),
                      "col_fold must"),
    "col_class2_i64": ("col_class2", lambda d: d["col_class2"].long(),
                       "col_class2 must"),
    "col_lr_f64": ("col_lr", lambda d: d["col_lr"].double(), "col_lr must"),
    "col_l2_long": ("col_l2", lambda d: _z((256,), torch.float32),
                    "col_l2 must"),
    "fmask_tall": ("fmask", lambda d: torch.ones(
        64, 128, dtype=torch.uint8, device=DEV), "fmask must"),
    "fmask_i32": ("fmask", lambda d: d["fmask"].int(), "fmask must"),
    "row_w_f64": ("row_w", lambda d: d["row_w"].double(), "row_w must"),
    "row_w_long": ("row_w", lambda d: _z((d["row_w"].numel() + 128,),
                                         torch.float32), "row_w must"),
    "GT_f32": ("GT", lambda d: d["GT"].float(), "GT must"),
    "GT_rows": ("GT", lambda d: _z((256, d["GT"].shape[1]),
                                   torch.bfloat16), "GT must"),
    # a [ncols_pad, 64] view into a larger allocation: stride below m_pad
    "GT_narrow": ("GT", lambda d: _z((512, 64), torch.bfloat16)
                  .narrow(0, 0, 128), "GT must"),
    "WbfT_transposed": ("WbfT", lambda d: _z((32, 128), torch.bfloat16),
                        "WbfT must"),
    "WbfT_f32": ("WbfT", lambda d: d["WbfT"].float(), "WbfT must"),
    "partial_transposed": ("partial", lambda d: _z((2, 128, 32),
                                                   torch.float32),
                           "partial must"),
    "partial_f64": ("partial", lambda d: d["partial"].double(), "partial must"),
    "V_tall": ("V", lambda d: _z((64, 128), torch.float32), "V must"),
    "V_f64": ("V", lambda d: d["V"].double(), "V must"),
    "W_f64": ("W", lambda d: d["W"].double(), "W must"),
    "XsT_f32": ("XsT", lambda d: d["XsT"].float(), "XsT must"),
    "Xs_f32": ("Xs", lambda d: d["Xs"].float(), "Xs must"),
}


@pytest.fixture(scope="module")
def good():
    c, d = _good_step_buffers()
    # the good buffers pass every entry, so each raise below is the bad
    # tensor's doing
    inv_m = torch.tensor([1 / 128.0, 1 / 128.0], dtype=torch.float32)
    ext = _ext()
    ir = c["intercept_row"]
    a = _step_args(d)
    l1 = (_z((128,), torch.float32), torch.zeros_like(d["W"]),
          torch.zeros_like(d["W"]))
    ext.sgd_step(*a, 0, 128, 0, 1.0, 0.9, ir, 1 / 128.0)
    ext.sgd_epoch(*a, inv_m, 128, 0, 1.0, 0.9, ir)
    ext.sgd_solve(*a, inv_m, 128, 0, 0.9, ir, 1)
    ext.sgd_epoch_l1(*a, inv_m, 128, 0, 1.0, 0.9, ir, *l1)
    ext.sgd_solve_l1(*a, inv_m, 128, 0, 0.9, ir, 1, *l1)
    torch.cuda.synchronize()
    return c, d, inv_m, l1


def _call_entry(entry, d, inv_m, l1, ir, start=0, m=128):
    ext = _ext()
    a = _step_args(d)
    if entry == "sgd_step":
        ext.sgd_step(*a, start, m, 0, 1.0, 0.9, ir, 1 / 128.0)
    elif entry == "sgd_epoch":
        ext.sgd_epoch(*a, inv_m, 128, 0, 1.0, 0.9, ir)
    elif entry == "sgd_solve":
        ext.sgd_solve(*a, inv_m, 128, 0, 0.9, ir, 1)
    elif entry == "sgd_epoch_l1":
        ext.sgd_epoch_l1(*a, inv_m, 128, 0, 1.0, 0.9, ir, *l1)
    else:
        ext.sgd_solve_l1(*a, inv_m, 128, 0, 0.9, ir, 1, *l1)


_ENTRIES = ["sgd_step", "sgd_epoch", "sgd_solve", "sgd_epoch_l1",
            "sgd_solve_l1"]
# every bad tensor through sgd_step; a dtype, a length and a shape through
# the others (they share check_step_tensors)
_REJECTS = [("sgd_step", k) for k in _BAD_TENSORS] + [
    (e, k) for e in _ENTRIES[1:]
    for k in ("fold_i64", "col_lr_f64", "col_l2_long", "WbfT_transposed",
              "GT_narrow", "fmask_tall", "row_w_long", "y_f64")]


@pytest.mark.parametrize("entry,bad", _REJECTS)
def test_step_entries_reject_one_bad_tensor(good, entry, bad):
    c, d, inv_m, l1 = good
    key, make, text = _BAD_TENSORS[bad]
    d2 = dict(d)
    d2[key] = make(d).contiguous()
    with pytest.raises(RuntimeError, match=text):
        _call_entry(entry, d2, inv_m, l1, c["intercept_row"])


@pytest.mark.parametrize("entry", _ENTRIES[1:])
@pytest.mark.parametrize("kind", ["f64", "short"])
def test_epoch_entries_reject_bad_inv_m(good, entry, kind):
    c, d, inv_m, l1 = good
    if kind == "f64":
        bad = inv_m.double()
    else:
        bad = torch.ones(8, dtype=torch.float32)[:1]   # 1 < 2 batches
    with pytest.raises(RuntimeError, match="inv_m"):
        _call_entry(entry, d, bad, l1, c["intercept_row"])


@pytest.mark.parametrize("what", ["start_past_n_pad", "intercept_row_fa",
                                  "intercept_row_neg", "splitk_0"])
def test_sgd_step_rejects_bad_ranges(good, what):
    c, d, inv_m, l1 = good
    ir, start, d2 = c["intercept_row"], 0, dict(d)
    if what == "start_past_n_pad":
        start, text = 256, "n_pad"      # 256 + 128 > n_pad = 256
    elif what == "intercept_row_fa":
        ir, text = c["fa"], "intercept_row"
    elif what == "intercept_row_neg":
        ir, text = -1, "intercept_row"
    else:
        d2["partial"] = _z((0, 32, 128), torch.float32)
        text = "splitk"
    with pytest.raises(RuntimeError, match=text):
        _call_entry("sgd_step", d2, inv_m, l1, ir, start=start)


def test_score_fold_rejects_bad_arguments():
    ext = _ext()
    Xf = _z((128, 32), torch.bfloat16)
    Wt = _z((128, 32), torch.bfloat16)
    yf = _z((128,), torch.float32)
    s0, s1 = _z((256,), torch.float32), _z((128,), torch.float32)
    ext.score_fold(Xf, Wt, yf, s0, 0)                       # good calls
    ext.score_fold(Xf, Wt, yf, s1, 1)
    bad = [
        ((Xf, Wt, _z((256,), torch.float32), s0, 0), "yf"),
        ((Xf, Wt, yf.double(), s0, 0), "yf"),
        ((Xf, Wt, yf, _z((512,), torch.float32), 0), "stats"),
        ((Xf, Wt, yf, s0, 1), "stats"),      # mode 1 takes one statistic
        ((Xf, Wt, yf, s0.double(), 0), "stats"),
        ((Xf, Wt, yf, s0, 2), "mode"),
        ((Xf, Wt.float(), yf, s0, 0), "WbfT must"),
        ((Xf.float(), Wt, yf, s0, 0), "Xf"),
        ((Xf, _z((128, 64), torch.bfloat16), yf, s0, 0), "WbfT must"),
    ]
    for args, text in bad:
        with pytest.raises(RuntimeError, match=text):
            ext.score_fold(*args)
    torch.cuda.synchronize()
