"""
The float64 references of tests/_dense_ref.py, checked on the CPU: one
composed reference step (K1 -> K2 -> K3, nothing rounded to bf16) against
``_sgd._sgd_step_torch`` in fp32, so the reference the GPU tests compare
the HIP kernels with is itself tested wherever the suite runs.
"""

import numpy as np
import pytest
import torch

import _dense_ref as R
from skdist_amd.models._sgd import ColumnSpec, _sgd_step_torch


def test_bf16_rne_matches_torch_and_ties_to_even():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096),
        # exact ties: 1 + 2^-8 -> 1 (even), 1 + 3*2^-8 -> 1 + 2^-6 (even)
        [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 0.0],
    ]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy()
    got = R.bf16_rne(x.astype(np.float64))
    assert np.array_equal(got, want)
    assert got[4096] == 1.0 and got[4097] == 1.0 + 2.0 ** -6
    bits = R.to_bf16_bits(got)
    back = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    assert np.array_equal(back.to(torch.float64).numpy(), got)


def test_slab_bounds_cover_the_batch():
    assert R.slab_bounds(512, 3) == [(0, 192), (192, 384), (384, 512)]
    assert R.slab_bounds(128, 8)[3:] == [(96, 128)] + [(128, 128)] * 4
    assert R.slab_bounds(512, 1) == [(0, 512)]


# (ovo, row_w, regress); regression targets exist for squared loss only
_FEATURES = [(False, False, False), (True, False, False), (True, True, False)]
_STEP_CASES = [(l, mo) + ft for l in (0, 1, 2) for mo in (0.0, 0.9)
               for ft in _FEATURES]
_STEP_CASES += [(2, mo, False, rw, True) for mo in (0.0, 0.9)
                for rw in (False, True)]


@pytest.mark.parametrize("loss_id,momentum,ovo,row_w,regress", _STEP_CASES)
def test_composed_reference_step_matches_eager_fp32(loss_id, momentum, ovo,
                                                    row_w, regress):
    n, f, fa, ncols = 300, 37, 64, 11
    start, m = 128, 150
    c = R.make_case(7 + loss_id, n, f, fa, ncols, loss_id, dyadic=True,
                    ovo=ovo, row_w=row_w, momentum=momentum)
    if regress:
        # _sgd_step_torch regresses on y in every column or in none
        c["col_class"][:ncols] = -1
    elif loss_id == R.LOSS_SQUARED:
        c["col_class"][:ncols] = np.where(c["col_class"][:ncols] < 0, 1,
                                          c["col_class"][:ncols])
    inv_m = R.inv_m_of(c, start, m)
    lr_scale = 0.5

    z, g, train = R.ref_gt(c["Xs"], c["W"].T, c["y"], c["fold"],
                           c["col_class"], c["col_fold"], c["col_class2"],
                           c["row_w"], start, m, loss_id)
    m_pad = R.ceil_to(m, 128)
    # rows at or past m never train, whatever their fold
    assert not train[m:].any() and train[:m, :ncols].any()
    psum = R.ref_partial_sum(c["XsT"], g.T, start, m_pad)[:fa]
    Wn, Vn, terms = R.ref_update(psum, c["W"], c["V"], c["col_lr"],
                                 c["col_l2"], None, inv_m, lr_scale,
                                 momentum, c["intercept_row"])

    t32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    spec = ColumnSpec("cpu", c["col_fold"][:ncols], c["col_class"][:ncols],
                      c["col_lr"][:ncols], c["col_l2"][:ncols],
                      col_class2=c["col_class2"][:ncols])
    W = t32(c["W"][:, :ncols]).contiguous()
    V = t32(c["V"][:, :ncols]).contiguous() if momentum > 0 else None
    _sgd_step_torch(
        t32(c["Xs"][:n]), t32(c["y"]), torch.tensor(c["fold"]),
        torch.arange(start, start + m), W, V, spec, loss_id, lr_scale,
        momentum, c["intercept_row"],
        row_w=None if c["row_w"] is None else t32(c["row_w"]))

    # fp32 rounding of the eager step.  z is exact (dyadic inputs, sums far
    # below 2^24 grid units); g carries a few roundings of a value <= 2
    # (dg); the gradient GEMM adds at most m roundings of the running sum
    # and carries dg through |x|; K3's elementwise chain is bounded as in
    # the GPU test: eps * (8 S + 3 M + |w|).
    eps = R.EPS32
    ax = np.abs(c["Xs"][start:start + m_pad]).T          # [fa, m_pad]
    dg = 8 * eps * (np.abs(g) + 1.0)
    dgrad = (ax @ (dg + m * eps * np.abs(g))) * float(inv_m)
    lr = np.abs(c["col_lr"])[None, :] * lr_scale
    tol = lr * dgrad + eps * (8 * terms["S"] + 3 * terms["M"] + terms["W"])
    err = np.abs(W.numpy().astype(np.float64) - Wn[:, :ncols])
    assert (err <= tol[:, :ncols]).all(), (err.max(), tol.max())
    # the bound is fp32 rounding, not a loose number: far below one step
    assert tol.max() < 1e-4 * np.abs(Wn - c["W"]).max()
    if momentum > 0:
        errv = np.abs(V.numpy().astype(np.float64) - Vn[:, :ncols])
        assert (errv <= tol[:, :ncols]).all(), errv.max()
    # transpose detection: the step differs across columns and rows
    d = Wn - c["W"]
    assert np.abs(d[:, 0] - d[:, 2]).max() > 1e-3
    assert np.abs(d[0] - d[3]).max() > 1e-3


def test_ref_update_pins_masked_weights_and_skips_intercept_l2():
    c = R.make_case(3, 200, 20, 32, 6, R.LOSS_LOG, fmask=True)
    psum = np.zeros((32, 128))
    Wn, Vn, _ = R.ref_update(psum, c["W"], np.zeros_like(c["W"]),
                             c["col_lr"], np.full(128, 0.25), c["fmask"],
                             1.0, 1.0, 0.9, c["intercept_row"])
    off = c["fmask"] == 0
    assert off.any() and (Wn[off] == 0).all() and (Vn[off] == 0).all()
    ir = c["intercept_row"]
    assert np.array_equal(Wn[ir], c["W"][ir])          # no L2 there
    on = ~off[:20, :6] & (c["W"][:20, :6] != 0)
    assert (np.abs(Wn[:20, :6][on]) < np.abs(c["W"][:20, :6][on])).all()


def test_ref_score_skips_sentinel_rows():
    Xf = np.zeros((128, 32))
    Xf[:3, 0] = [1.0, -1.0, 2.0]
    Wt = np.zeros((128, 32))
    Wt[0, 0] = 1.0
    yf = np.full(128, R.PAD_SENTINEL)
    yf[:3] = [1.0, 1.0, 0.0]
    hits, valid, _ = R.ref_score(Xf, Wt, yf, 0)
    assert hits[0] == 1 and valid[0] == 3
    # z = 0 counts as the positive class
    assert hits[1] == 2
    sse, _, _ = R.ref_score(Xf, Wt, yf, 1)
    assert sse[0] == 0.0 + 4.0 + 4.0 and sse[1] == 2.0


def test_ref_standardize_layout_and_tie():
    X = np.array([[1.0 + 2.0 ** -8, 3.0]], np.float32)
    out = R.ref_standardize(X, np.zeros(2), np.ones(2), 8)
    assert out.tolist() == [[1.0, 3.0, 1.0, 0, 0, 0, 0, 0]]
