"""
The two code paths of k_fwd_gt's epilogue and the two tile heights of
k_grad_partial (ops/csrc/sgd_kernels.hip), against the float64 references
of tests/_dense_ref.py.

K1 takes a plain path for a column tile whose columns all have
col_class < 0 and col_class2 < 0 when there is no row_w, and the general
path otherwise; both must write the same GT for an element both can
express.  K2 runs a 96-row tile where ceil(fa/96)*96 < ceil(fa/128)*128
and the 128-row tile elsewhere; a slab of ``partial`` is the same sum
under either, so with dyadic inputs it equals the float64 product bit for
bit.

The buffers, canaries and criteria are those of
test_dense_sgd_kernels_gpu.py.
"""

import numpy as np
import pytest
import torch

import _dense_ref as R
import test_dense_sgd_kernels_gpu as K

pytestmark = pytest.mark.gpu

EPS = R.EPS32


def _step(c, d, start, m, loss_id):
    K._ext().sgd_step(*K._step_args(d), start, m, loss_id, 0.5,
                      c["momentum"], c["intercept_row"],
                      float(R.inv_m_of(c, start, m)))
    torch.cuda.synchronize()


def _canaries(d, m_pad):
    for k in ("GT_can", "W_can", "WbfT_can", "partial_can", "V_can"):
        if k in d:
            assert K._canary_intact(d[k]), k
    assert (K._np(d["GT"])[:, m_pad:] == K.STALE).all(), \
        "K1 wrote past m_pad"


def _gt_bounds(c, start, m, loss_id):
    """What the reference alone decides about GT: (train, g, lo, hi,
    near, delta), each [m_pad, ncols_pad].  Hinge and squared loss on
    dyadic inputs are exact (lo == hi == bf16(g)); log loss takes the
    bound derived in test_dense_sgd_kernels_gpu.test_staged_step."""
    fa, n = c["fa"], c["n"]
    m_pad = R.ceil_to(m, 128)
    z, g, train = R.ref_gt(c["Xs"], c["W"].T, c["y"], c["fold"],
                           c["col_class"], c["col_fold"], c["col_class2"],
                           c["row_w"], start, m, loss_id)
    assert not train[m:].any() and train[:m, :c["ncols"]].any()
    assert (~train[:m, :c["ncols"]]).any()          # masks are live
    want = R.bf16_rne(g)
    if loss_id != R.LOSS_LOG:
        K._assert_exact_preconditions(c, start, m_pad, z)
        return train, g, want, want, np.zeros_like(train), np.zeros_like(g)
    dz = fa * EPS * (np.abs(c["Xs"][start:start + m_pad]) @ np.abs(c["W"]))
    rw = np.ones(m_pad)
    if c["row_w"] is not None:
        ok = start + np.arange(m_pad) < n
        rw[ok] = c["row_w"][start:start + m_pad][: ok.sum()]
    delta = np.where(train, (dz / 4 + 2.0 ** -20) * rw[:, None], 0.0)
    lo, hi = R.bf16_rne(g - delta), R.bf16_rne(g + delta)
    near = lo != hi
    print(f"near a bf16 boundary: {near.mean():.4%} of the tile")
    assert near.mean() <= 0.01, near.mean()
    assert (np.abs(z) > 30).any()                   # the clamp is reached
    return train, g, lo, hi, near, delta


def _assert_gt(d, m_pad, bounds):
    train, g, lo, hi, near, delta = bounds
    got = K._np(d["GT"])[:, :m_pad].T                   # [m_pad, ncp]
    assert (got[~train] == 0).all(), "masked element not 0"
    bad = np.argwhere((got < lo) | (got > hi))
    assert len(bad) == 0, ("GT (row, col)", bad[:8], len(bad))
    if near.any():
        step1 = R.bf16_step(np.abs(g) + delta)
        assert (np.abs(got - R.bf16_rne(g)) <= step1)[near].all()
    return got


# ------------------------------------------------------------------ #
# K2: tile heights
# ------------------------------------------------------------------ #

# fa -> what it reaches (rows x tiles, guard):
#   96   one 96-row tile              288  three 96-row tiles, no padding
#   160  two 96-row tiles, rows 160..191 guarded
#   128  one 128-row tile             256  two 128-row tiles
#   224  two 128-row tiles, rows 224..255 guarded
_FA = [96, 288, 160, 128, 256, 224]


def _picks_96(fa):
    return R.ceil_to(fa, 96) < R.ceil_to(fa, 128)


def test_tile_rule_of_the_cases():
    assert [_picks_96(fa) for fa in _FA] == [True, True, True,
                                             False, False, False]
    # a 96-row tiling never reads XsT rows past fa_store
    for fa in range(32, 1025, 32):
        if _picks_96(fa):
            assert R.ceil_to(fa, 96) <= R.ceil_to(fa, 128)


@pytest.mark.parametrize("splitk", [8, 3])
@pytest.mark.parametrize("fa", _FA)
def test_grad_partial_tile_heights(fa, splitk):
    start, m, n, ncols = 128, 256, 400, 130
    f = fa - 11                       # pad feature rows f+1..fa-1 are live
    loss_id = R.LOSS_SQUARED
    c = R.make_case(23, n, f, fa, ncols, loss_id, dyadic=True, ovo=True,
                    momentum=0.0)
    m_pad = 256
    bounds = _gt_bounds(c, start, m, loss_id)
    slabs = R.slab_bounds(m_pad, splitk)
    assert [k1 - k0 for k0, k1 in slabs] == (
        [32] * 8 if splitk == 8 else [96, 96, 64])

    d = K._device_step_buffers(c, m, splitk)
    _step(c, d, start, m, loss_id)
    _canaries(d, m_pad)               # partial has no rows >= fa
    _assert_gt(d, m_pad, bounds)

    GT = K._np(d["GT"])
    partial = K._np(d["partial"])
    xt = c["XsT"][:, start:start + m_pad]
    for zi, (k0, k1) in enumerate(slabs):
        want = xt[:fa, k0:k1] @ GT[:, k0:k1].T
        bad = np.argwhere(partial[zi] != want)
        assert len(bad) == 0, ("partial slab", zi, bad[:8], len(bad))
    # the slabs carry a gradient in every feature tile and column tile
    psum = partial.sum(axis=0)
    assert np.abs(psum[:32, :ncols]).max() > 1
    assert np.abs(psum[f - 31:f + 1, 128:ncols]).max() > 1
    assert (psum[f + 1:] == 0).all()
    W_got = K._np(d["W"])
    assert (W_got[f + 1:] == 0).all(), "W above the intercept moved"
    assert (W_got[:, ncols:] == 0).all()
    assert np.abs(W_got - c["W"])[: f + 1, :ncols].max() > 1e-3


# ------------------------------------------------------------------ #
# K1: plain path
# ------------------------------------------------------------------ #

def _plain_case(loss_id, n=400):
    """fa = 32, two column tiles, binary y; every live column is plain
    (class -1, no partner), pad columns keep -99 / -1, no row_w."""
    c = R.make_case(31, n, 20, 32, 130, loss_id,
                    dyadic=loss_id != R.LOSS_LOG, ovo=False, momentum=0.0)
    c["y"] = np.minimum(c["y"], 1.0)
    assert set(np.unique(c["y"])) == {0.0, 1.0}
    c["col_class"][:130] = -1
    assert (c["col_class"] < 0).all() and (c["col_class2"] == -1).all()
    assert c["row_w"] is None
    return c


@pytest.mark.parametrize("loss_id", [0, 1, 2])
def test_fwd_plain_path(loss_id):
    start, m = 128, 256
    c = _plain_case(loss_id)
    bounds = _gt_bounds(c, start, m, loss_id)
    d = K._device_step_buffers(c, m, 8)
    _step(c, d, start, m, loss_id)
    _canaries(d, 256)
    got = _assert_gt(d, 256, bounds)
    # transposed store: g differs between columns and between rows
    assert np.abs(got[:, 0] - got[:, 2]).max() > 0.1
    assert np.abs(got[0] - got[3]).max() > 0.1


@pytest.mark.parametrize("loss_id", [0, 1, 2])
def test_fwd_paths_agree(loss_id):
    """Run 0: both column tiles plain.  Run 1: column 129 one-vs-one, so
    tile 1 takes the general path.  Run 2: as run 1 with row_w = 1, so
    tile 0 takes it too.  What both paths can express is equal bit for
    bit."""
    start, m = 128, 256
    gts = []
    for run in range(3):
        c = _plain_case(loss_id)
        if run >= 1:
            c["col_class"][129], c["col_class2"][129] = 0, 1
        if run == 2:
            c["row_w"] = np.ones(c["n"])
        d = K._device_step_buffers(c, m, 8)
        _step(c, d, start, m, loss_id)
        _canaries(d, 256)
        gts.append(d["GT"].clone())
    assert gts[0].float().abs().max() > 0.1
    for other in gts[1:]:
        assert torch.equal(gts[0][:128], other[:128])       # tile 0
        assert torch.equal(gts[0][128:129], other[128:129])  # tile 1, plain
        assert torch.equal(gts[0][130:], other[130:])        # pad columns
    # the one-vs-one column trains on y in {0, 1} against target y == 0:
    # it is not the plain column it replaced
    assert not torch.equal(gts[0][129], gts[1][129])
    assert torch.equal(gts[1][129], gts[2][129])


def test_fwd_plain_row_tail():
    start, m = 384, 16
    loss_id = R.LOSS_LOG
    c = _plain_case(loss_id)
    bounds = _gt_bounds(c, start, m, loss_id)
    d = K._device_step_buffers(c, m, 8)
    _step(c, d, start, m, loss_id)
    _canaries(d, 128)                  # GT past m_pad keeps its pre-fill
    got = _assert_gt(d, 128, bounds)
    assert (got[m:] == 0).all(), "rows >= m must be exactly 0"
    assert np.abs(got[:m]).max() > 0.1
