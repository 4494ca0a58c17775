"""
k_fwd_gt_bits (ops/csrc/sgd_kernels.hip) through ``ext.sgd_step_bits``:
the forward kernel whose targets and train masks come from int32 bit planes,
against the float64 reference of tests/_bits_ref.py, staged like
test_dense_sgd_kernels_gpu.py (canary rows around every written buffer),
and bit for bit against today's kernels where both can express the problem
(a one-hot plane is class targets; a pair-mask plane is a one-vs-one column).
"""

import numpy as np
import pytest
import torch

import _bits_ref as B
import _dense_ref as R
from test_dense_sgd_kernels_gpu import (
    CANARY,
    DEV,
    EPS,
    STALE,
    _assert_exact_preconditions,
    _canary_intact,
    _device_step_buffers,
    _ext,
    _f32,
    _np,
    _step_args,
)

pytestmark = pytest.mark.gpu

# name -> start, m, n, f (fa), ncols.  What each reaches:
#  tiles: 2 row tiles, 2 column tiles; ncols_pad = 256, 8 words per row: the
#         second column tile reads words 4..7, column 129 is bit 1 of word 4
#  tail:  rows past m and past n masked in the only row tile
#  onek:  fa = 32, a single K-tile (nothing prefetched), one column tile
_SHAPES = {
    "tiles": dict(start=128, m=256, n=400, f=150, fa=160, ncols=130),
    "tail": dict(start=384, m=16, n=400, f=150, fa=160, ncols=130),
    "onek": dict(start=0, m=128, n=128, f=20, fa=32, ncols=9),
}

# (shape, loss, momentum, mask plane, row_w, l1)
_CASES = [
    ("tiles", 0, 0.9, True, True, False),
    ("tiles", 1, 0.9, True, True, False),
    ("tiles", 2, 0.0, False, False, False),
    ("tiles", 1, 0.0, False, True, False),
    ("tiles", 1, 0.9, True, False, True),
    ("tail", 0, 0.9, False, False, False),
    ("tail", 1, 0.0, True, True, False),
    ("tail", 2, 0.9, True, False, False),
    ("onek", 0, 0.0, True, False, False),
    ("onek", 1, 0.9, False, True, False),
    ("onek", 2, 0.9, True, True, False),
]


def _case_id(p):
    shape, loss, mom, mask, rw, l1 = p
    return (f"{shape}-loss{loss}-mom{mom}{'-mask' if mask else ''}"
            f"{'-roww' if rw else ''}{'-l1' if l1 else ''}")


def _planes(seed, n, ncols, mask):
    rng = np.random.default_rng(seed)
    T = (rng.random((n, ncols)) < 0.3).astype(np.uint8)
    M = (rng.random((n, ncols)) < 0.7).astype(np.uint8) if mask else None
    return T, M


def _plane_t(a, n_pad, ncp):
    return torch.tensor(B.pack_plane(a, n_pad, ncp), dtype=torch.int32,
                        device=DEV)


def _no_plane():
    return torch.empty(0, dtype=torch.int32, device=DEV)


def _assert_planes_are_live(T, M, c, start, m):
    """Both planes carry set and clear bits in every word that holds real
    columns, on the rows of the batch: per (row, word) for a word of 32
    real columns, over the rows for a partly real word."""
    n, ncols, ncp, n_pad = c["n"], c["ncols"], c["ncols_pad"], c["n_pad"]
    rows = slice(start, min(start + m, n))
    for a in (T, M):
        if a is None:
            continue
        words = B.pack_plane(a, n_pad, ncp)[rows].view(np.uint32)
        for wi in range((ncols + 31) // 32):
            real = min(32, ncols - 32 * wi)
            full = np.uint32((1 << real) - 1)
            col = words[:, wi]
            if real == 32:
                assert (col != 0).all() and (col != full).all(), wi
            else:
                assert (col != 0).any() and ((col & full) != full).any(), wi
        assert (words[:, (ncols + 31) // 32:] == 0).all()   # pad words
    assert np.array_equal(B.unpack_plane(B.pack_plane(T, n_pad, ncp),
                                         ncp)[:n, :ncols], T)


def _assert_word_and_bit_order_matter(c, T, M, start, m, loss_id, g):
    """g changes when two words of the target plane, or the bit order
    inside its words, are swapped: a kernel reading the wrong word or
    counting bits from the top cannot pass."""
    n, ncp = c["n"], c["ncols_pad"]
    full = np.zeros((n, ncp), np.uint8)
    full[:, : T.shape[1]] = T
    words = full.reshape(n, ncp // 32, 32)
    swapped = words.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    reversed_ = words[:, :, ::-1]
    for other in (swapped, reversed_):
        _, g2, _ = B.ref_gt_bits(c["Xs"], c["W"].T, c["fold"], c["col_fold"],
                                 c["row_w"], other.reshape(n, ncp), M,
                                 start, m, loss_id)
        assert np.abs(g2[:, : c["ncols"]] - g[:, : c["ncols"]]).max() > 0.1


@pytest.mark.parametrize("p", _CASES, ids=_case_id)
def test_staged_step_bits(p):
    shape, loss_id, momentum, mask, row_w, l1 = p
    s = _SHAPES[shape]
    start, m, n, f, fa, ncols = (s[k] for k in
                                 ("start", "m", "n", "f", "fa", "ncols"))
    exact = loss_id != R.LOSS_LOG
    c = R.make_case(11, n, f, fa, ncols, loss_id, dyadic=exact, ovo=False,
                    row_w=row_w, fmask=False, momentum=momentum)
    ncp, n_pad, m_pad = c["ncols_pad"], c["n_pad"], R.ceil_to(m, 128)
    T, M = _planes(23, n, ncols, mask)
    inv_m = R.inv_m_of(c, start, m)
    lr_scale = 0.5
    mom32 = float(np.float32(momentum))

    # ---- everything the reference alone decides, before any GPU call
    _assert_planes_are_live(T, M, c, start, m)
    z, g, train = B.ref_gt_bits(c["Xs"], c["W"].T, c["fold"], c["col_fold"],
                                c["row_w"], T, M, start, m, loss_id)
    assert not train[m:].any() and train[:m, :ncols].any()
    assert (~train[:m, :ncols]).any()
    if mask:
        assert not train[:, ncols:].any()      # pad columns are masked
    _assert_word_and_bit_order_matter(c, T, M, start, m, loss_id, g)
    want_gt = R.bf16_rne(g)
    if exact:
        _assert_exact_preconditions(c, start, m_pad, z)
        lo = hi = want_gt
    else:
        # the bracket of test_dense_sgd_kernels_gpu.test_staged_step,
        # unchanged: dz is the fp32 accumulation error of z, sigmoid' <= 1/4
        # carries dz/4 into g, 2^-20 stands for __expf and the roundings
        # after it, row_w scales both; a kernel value is right when it is
        # the bf16 rounding of some value within delta of the reference
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
    assert np.abs(g[:, 0] - g[:, 2]).max() > 0.1
    assert np.abs(g[0] - g[3]).max() > 0.1

    # ---- one step on the device
    d = _device_step_buffers(c, m, 8)
    tb = _plane_t(T, n_pad, ncp)
    mb = _plane_t(M, n_pad, ncp) if mask else _no_plane()
    l1_args = ()
    if l1:
        col_l1 = np.zeros(ncp)
        col_l1[:ncols] = 2.0 ** -3
        l1_args = (_f32(col_l1), torch.zeros_like(d["W"]),
                   torch.zeros_like(d["W"]))
    _ext().sgd_step_bits(*_step_args(d), start, m, loss_id, lr_scale,
                         momentum, c["intercept_row"], float(inv_m), tb, mb,
                         *l1_args)
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
        step1 = R.bf16_step(np.abs(g) + delta)
        assert (np.abs(got - want_gt) <= step1)[near].all()

    # ---- K2 and K3 are the shared kernels: from what the device wrote
    psum = partial.sum(axis=0)
    if exact:
        want_sum = R.ref_partial_sum(c["XsT"], GT, start, m_pad)[:fa]
        assert np.array_equal(psum, want_sum)
    Wn, Vn, t = R.ref_update(psum, c["W"], c["V"], c["col_lr"], c["col_l2"],
                             None, inv_m, np.float32(lr_scale), mom32,
                             c["intercept_row"])
    assert np.array_equal(WbfT_got, R.bf16_rne(W_got).T), "WbfT != bf16(W)ᵀ"
    assert (W_got[:, ncols:] == 0).all() and (W_got[f + 1:] == 0).all()
    if l1:
        # the clip is live: weights the L2-only step leaves non-zero end
        # at exactly 0, none crosses 0, and the intercept row is not clipped
        body = np.abs(Wn[:f, :ncols]) > 0
        assert ((W_got[:f, :ncols] == 0) & body).any()
        assert (W_got[:f, :ncols] * Wn[:f, :ncols] >= 0).all()
        assert (np.abs(W_got[:f, :ncols]) <= np.abs(Wn[:f, :ncols])).all()
    else:
        # the fp32 bound of test_staged_step for K3
        tol_w = EPS * (8 * t["S"] + 3 * t["M"] + t["W"]) * (1 + 2.0 ** -10)
        if not exact:
            tol_w = tol_w + (8 * EPS * np.abs(partial).sum(axis=0)
                             * float(inv_m)
                             * np.abs(c["col_lr"])[None, :] * lr_scale)
        bad = np.argwhere(np.abs(W_got - Wn) > tol_w)
        assert len(bad) == 0, ("W (row, col)", bad[:8], len(bad))
    dW = W_got - c["W"]
    assert np.abs(dW[:, 0] - dW[:, 2]).max() > 1e-3
    assert np.abs(dW[0] - dW[3]).max() > 1e-3


# ------------------------------------------------------------------ #
# bit-identity with today's kernels
# ------------------------------------------------------------------ #

def _class_case(ncols, ovo, row_w, loss_id):
    """The `tiles` shape with class-target columns only: classes 0..2 (y is
    in 0..2), folds cycling; ``ovo`` gives every column a partner class."""
    s = _SHAPES["tiles"]
    c = R.make_case(17, s["n"], s["f"], s["fa"], ncols, loss_id,
                    dyadic=False, ovo=False, row_w=row_w, momentum=0.9)
    k = np.arange(ncols)
    c["col_class"][:ncols] = k % 3
    c["col_fold"][:ncols] = np.array([0, 1, 2, -2])[k % 4]
    if ovo:
        c["col_class2"][:ncols] = (k % 3 + 1 + (k // 3) % 2) % 3
    return c, s


@pytest.mark.parametrize("loss_id", [0, 1])
@pytest.mark.parametrize("ncols", [130, 256])
@pytest.mark.parametrize("ovo", [False, True], ids=["onehot", "pairmask"])
def test_planes_equal_todays_kernels_bitwise(ovo, ncols, loss_id):
    """A one-hot plane is class targets; targets = (y == a) with the mask
    (y == a) | (y == b) is the one-vs-one column (a, b).  GT, the partial
    sums, W, V and WbfT must agree bit for bit.  Pad columns (ncols = 130)
    are outside the comparison of GT and the partial sums: k_fwd_gt gives a
    pad column the target y, a bit plane gives it 0, and either is
    multiplied by lr = 0.  With ncols = 256 there are none."""
    c, s = _class_case(ncols, ovo, row_w=not ovo, loss_id=loss_id)
    start, m, n = s["start"], s["m"], s["n"]
    ncp, n_pad = c["ncols_pad"], c["n_pad"]
    y = c["y"]
    cls, c2 = c["col_class"][:ncols], c["col_class2"][:ncols]
    T = (y[:, None] == cls[None, :]).astype(np.uint8)
    M = None
    if ovo:
        assert (c2 >= 0).all() and (c2 != cls).all()
        M = (T != 0) | (y[:, None] == c2[None, :])
        assert 0.5 < M.mean() < 0.8
    inv_m = float(R.inv_m_of(c, start, m))
    ir = c["intercept_row"]

    d0 = _device_step_buffers(c, m, 8)
    _ext().sgd_step(*_step_args(d0), start, m, loss_id, 1.0, 0.9, ir, inv_m)
    d1 = _device_step_buffers(c, m, 8)
    # the class vectors are ignored with planes: hand over wrong ones
    d1["col_class"] = torch.full_like(d1["col_class"], 1)
    d1["col_class2"] = torch.full_like(d1["col_class2"], -1)
    _ext().sgd_step_bits(*_step_args(d1), start, m, loss_id, 1.0, 0.9, ir,
                         inv_m, _plane_t(T, n_pad, ncp),
                         _plane_t(M, n_pad, ncp) if ovo else _no_plane())
    torch.cuda.synchronize()
    for d in (d0, d1):
        for k in ("GT_can", "W_can", "WbfT_can", "partial_can", "V_can"):
            assert _canary_intact(d[k]), k
    assert d0["GT"][:ncols].float().abs().max() > 0.1
    assert torch.equal(d0["GT"][:ncols], d1["GT"][:ncols])
    assert torch.equal(d0["partial"][:, :, :ncols],
                       d1["partial"][:, :, :ncols])
    for k in ("W", "V", "WbfT"):
        assert torch.equal(d0[k], d1[k]), k
    assert (d0["W"].cpu().double().numpy() != c["W"]).any()


def test_l1_update_with_a_one_hot_plane_equals_sgd_epoch_l1_bitwise():
    c, s = _class_case(130, False, row_w=True, loss_id=0)
    n, ncols, ncp, n_pad = s["n"], 130, c["ncols_pad"], c["n_pad"]
    T = (c["y"][:, None] == c["col_class"][None, :ncols]).astype(np.uint8)
    bs = 256
    inv_m = torch.tensor([R.inv_m_of(c, st, min(bs, n - st))
                          for st in range(0, n, bs)], dtype=torch.float32)
    col_l1 = np.zeros(ncp)
    col_l1[:ncols:2] = 2.0 ** -6
    outs = []
    for bits in (False, True):
        d = _device_step_buffers(c, bs, 8)
        l1 = (_f32(col_l1), torch.zeros_like(d["W"]),
              torch.zeros_like(d["W"]))
        if bits:
            _ext().sgd_epoch_bits(*_step_args(d), inv_m, bs, 0, 1.0, 0.9,
                                  c["intercept_row"],
                                  _plane_t(T, n_pad, ncp), _no_plane(), *l1)
        else:
            _ext().sgd_epoch_l1(*_step_args(d), inv_m, bs, 0, 1.0, 0.9,
                                c["intercept_row"], *l1)
        torch.cuda.synchronize()
        for k in ("W_can", "V_can", "WbfT_can", "partial_can", "GT_can"):
            assert _canary_intact(d[k]), k
        outs.append((d["W"].clone(), d["V"].clone(), d["WbfT"].clone(),
                     l1[1], l1[2]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert (outs[0][3] != 0).any()             # the L1 credits moved


# ------------------------------------------------------------------ #
# solve level and binding checks
# ------------------------------------------------------------------ #

def _solve_case():
    n, bs, f, fa, ncols = 400, 256, 150, 160, 130
    c = R.make_case(5, n, f, fa, ncols, R.LOSS_LOG, dyadic=False,
                    ovo=False, row_w=True, fmask=True, momentum=0.9)
    T, M = _planes(29, n, ncols, True)
    inv_m = torch.tensor([R.inv_m_of(c, s, min(bs, n - s))
                          for s in range(0, n, bs)], dtype=torch.float32)
    return c, T, M, inv_m, bs


def test_solve_bits_replay_equals_eager_epochs():
    """sgd_solve_bits(epochs=3) replays a captured epoch twice; three
    sgd_epoch_bits(lr_scale=1) calls launch the same kernels eagerly."""
    c, T, M, inv_m, bs = _solve_case()
    ncp, n_pad = c["ncols_pad"], c["n_pad"]
    outs = []
    for solve in (True, False):
        d = _device_step_buffers(c, bs, 8)
        a = _step_args(d)
        tb, mb = _plane_t(T, n_pad, ncp), _plane_t(M, n_pad, ncp)
        if solve:
            _ext().sgd_solve_bits(*a, inv_m, bs, R.LOSS_LOG, 0.9,
                                  c["intercept_row"], 3, tb, mb)
        else:
            for _ in range(3):
                _ext().sgd_epoch_bits(*a, inv_m, bs, R.LOSS_LOG, 1.0, 0.9,
                                      c["intercept_row"], tb, mb)
        torch.cuda.synchronize()
        for k in ("W_can", "V_can", "WbfT_can", "partial_can", "GT_can"):
            assert _canary_intact(d[k]), k
        outs.append((d["W"].clone(), d["V"].clone(), d["WbfT"].clone()))
    for x, y in zip(*outs):
        assert torch.isfinite(x.float()).all()
        assert torch.equal(x, y)
    moved = outs[0][0].cpu().double().numpy() - c["W"]
    assert np.abs(moved[: c["f"] + 1, : c["ncols"]]).max() > 1e-2


@pytest.fixture(scope="module")
def good_bits():
    """Buffers every *_bits entry accepts (one batch of 128 rows)."""
    n, f, fa, ncols = 256, 20, 32, 9
    c = R.make_case(1, n, f, fa, ncols, R.LOSS_LOG, dyadic=False, ovo=False,
                    row_w=True, fmask=True, momentum=0.9)
    d = _device_step_buffers(c, 128, 2)
    T, M = _planes(31, n, ncols, True)
    tb = _plane_t(T, c["n_pad"], c["ncols_pad"])
    mb = _plane_t(M, c["n_pad"], c["ncols_pad"])
    inv_m = torch.tensor([1 / 128.0, 1 / 128.0], dtype=torch.float32)
    for entry in _ENTRIES:
        _call_bits(entry, d, inv_m, c["intercept_row"], tb, mb)
    torch.cuda.synchronize()
    return c, d, inv_m, tb, mb


_ENTRIES = ["sgd_step_bits", "sgd_epoch_bits", "sgd_solve_bits"]


def _call_bits(entry, d, inv_m, ir, tb, mb):
    ext, a = _ext(), _step_args(d)
    if entry == "sgd_step_bits":
        ext.sgd_step_bits(*a, 0, 128, 0, 1.0, 0.9, ir, 1 / 128.0, tb, mb)
    elif entry == "sgd_epoch_bits":
        ext.sgd_epoch_bits(*a, inv_m, 128, 0, 1.0, 0.9, ir, tb, mb)
    else:
        ext.sgd_solve_bits(*a, inv_m, 128, 0, 0.9, ir, 1, tb, mb)


# every bad plane is as large as the good one or larger (or a view into a
# larger allocation): a missing check shows as "did not raise", never as an
# access outside an allocation
_BAD_PLANES = {
    "dtype": lambda t: t.long(),
    "shape": lambda t: torch.zeros(t.shape[0], t.shape[1] + 4,
                                   dtype=torch.int32, device=DEV),
    "rows": lambda t: torch.zeros(t.shape[0] + 128, t.shape[1],
                                  dtype=torch.int32, device=DEV),
    "noncontiguous": lambda t: torch.zeros(
        t.shape[0], 2 * t.shape[1], dtype=torch.int32, device=DEV)[:, ::2],
    "host": lambda t: t.cpu(),
}


@pytest.mark.parametrize("bad", list(_BAD_PLANES))
@pytest.mark.parametrize("which", ["tbits", "mbits"])
@pytest.mark.parametrize("entry", _ENTRIES)
def test_bits_entries_reject_a_bad_plane(good_bits, entry, which, bad):
    c, d, inv_m, tb, mb = good_bits
    make = _BAD_PLANES[bad]
    if which == "tbits":
        tb = make(tb)
    else:
        mb = make(mb)
    assert (bad == "noncontiguous") == (not (tb.is_contiguous()
                                             and mb.is_contiguous()))
    with pytest.raises(RuntimeError, match=which):
        _call_bits(entry, d, inv_m, c["intercept_row"], tb, mb)


def test_bits_entries_reject_softmax_and_half_an_l1_state(good_bits):
    c, d, inv_m, tb, mb = good_bits
    ext, a, ir = _ext(), _step_args(d), c["intercept_row"]
    with pytest.raises(RuntimeError, match="softmax|group_k"):
        ext.sgd_step_bits(*a, 0, 128, 3, 1.0, 0.9, ir, 1 / 128.0, tb, mb)
    col_l1 = torch.zeros(128, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="L1|col_l1"):
        ext.sgd_step_bits(*a, 0, 128, 0, 1.0, 0.9, ir, 1 / 128.0, tb, mb,
                          col_l1)
    torch.cuda.synchronize()
