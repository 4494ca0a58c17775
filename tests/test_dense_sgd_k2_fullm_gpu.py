"""
The whole-fa split-K gradient kernel k_grad_partial_fullm
(ops/csrc/sgd_kernels.hip), launched alone through ``ext.grad_partial``.

One workgroup of the kernel owns every feature row of one column tile and
one slab, and stages both operands through a ring of LDS stages whose
loads stay in flight across the k-loop's barriers.  What can go wrong is
therefore the ring (prologue, steady state and drain at every slab
length), the instantiation for an fa below the tile's 288 rows, which
must stage and multiply only the chunks below fa, and the claim
that a ``partial`` element is the same chain of MFMA accumulations as
under the 128-row and 96-row tiles:

(a) dyadic inputs, every slab against the float64 product, bit for bit,
    with NaN wherever the kernel must not read and canaries wherever it
    must not write;
(b) random inputs, bit for bit against the legacy kernels;
(c) the launcher's routing rule;
(d) graph replay of a solve whose K2 is the new kernel.

The helpers and canaries are those of test_dense_sgd_kernels_gpu.py.
"""

import numpy as np
import pytest
import torch

import _dense_ref as R
import test_dense_sgd_kernels_gpu as K

pytestmark = pytest.mark.gpu

DEV = K.DEV
RING = 3            # K2F_NS of the kernel that ships
NCP = 256           # two column tiles of 128

# (m_pad, splitk) -> k-steps of 32 per slab
_PAIRS = [(128, 8), (128, 4), (128, 2), (384, 4), (384, 3), (640, 4),
          (384, 1), (512, 3)]


def _steps(m_pad, splitk):
    return [(k1 - k0) // 32 for k0, k1 in R.slab_bounds(m_pad, splitk)]


def test_pairs_reach_every_ring_path():
    seen = set()
    for p in _PAIRS:
        seen.update(_steps(*p))
    # empty slab, shorter than / equal to / longer than the ring, deep
    assert {0, 1, 2, 3, 4, 5, 12} <= seen
    assert {RING - 1, RING, RING + 1} <= seen
    assert _steps(512, 3) == [6, 6, 4]               # uneven last slab
    assert _steps(128, 8) == [1, 1, 1, 1, 0, 0, 0, 0]


def _nan_guarded_bf16(values, extra_rows):
    """``values`` as the leading rows of an allocation whose trailing rows
    are NaN: a read past the last row poisons what it feeds."""
    v = torch.tensor(np.asarray(values, np.float64), dtype=torch.float32)
    big = torch.full((v.shape[0] + extra_rows, v.shape[1]), float("nan"),
                     dtype=torch.float32)
    big[: v.shape[0]] = v
    big = big.to(torch.bfloat16).to(DEV)
    view = big.narrow(0, 0, v.shape[0])
    assert view.is_contiguous()
    return view


def _k2_case(seed, fa, m_pad, start, dyadic):
    """XsT [fa_store, n_pad] with rows fa.. zero, GT [NCP, m_pad + 128]
    with NaN past m_pad.  Dyadic: multiples of 1/4 and 1/8 below 2 in
    magnitude, so a product is a multiple of 1/32 below 4 and a sum of up
    to 1024 of them is exact in fp32 in any order."""
    rng = np.random.default_rng(seed)
    fa_store = R.ceil_to(fa, 128)
    n_pad = R.ceil_to(start + m_pad, 128)
    xt = np.zeros((fa_store, n_pad))
    gt = np.full((NCP, m_pad + 128), np.nan)
    if dyadic:
        xt[:fa] = rng.integers(-7, 8, (fa, n_pad)) / 4.0
        gt[:, :m_pad] = rng.integers(-15, 16, (NCP, m_pad)) / 8.0
    else:
        xt[:fa] = R.bf16_rne(rng.standard_normal((fa, n_pad)))
        gt[:, :m_pad] = R.bf16_rne(rng.standard_normal((NCP, m_pad)))
    return xt, gt


def _upload(xt, gt, fa, splitk):
    d = {}
    d["XsT"] = _nan_guarded_bf16(xt, 16)
    g = torch.tensor(gt, dtype=torch.float32).to(torch.bfloat16)
    big = torch.full((NCP + 8, gt.shape[1]), K.CANARY, dtype=torch.bfloat16)
    big[:NCP] = g
    big = big.to(DEV)
    d["GT"], d["GT_can"] = big.narrow(0, 0, NCP), big.narrow(0, NCP, 8)
    d["partial"], d["partial_can"] = K._guarded(
        np.full((splitk, fa, NCP), K.CANARY), torch.float32, 1)
    return d


def _launch(d, start, m, variant):
    K._ext().grad_partial(d["XsT"], d["GT"], d["partial"], start, m,
                          variant)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ #
# (a) exact against float64
# ------------------------------------------------------------------ #

@pytest.mark.parametrize("start", [0, 8])
@pytest.mark.parametrize("m_pad,splitk", _PAIRS)
@pytest.mark.parametrize("fa", [32, 160, 288])
def test_fullm_slabs_exact(fa, m_pad, splitk, start):
    xt, gt = _k2_case(100 + fa + m_pad + splitk + start, fa, m_pad, start,
                      dyadic=True)
    d = _upload(xt, gt, fa, splitk)
    gt_before = d["GT"].clone()
    _launch(d, start, m_pad, 3)
    assert K._canary_intact(d["partial_can"]), "wrote past partial"
    assert K._canary_intact(d["GT_can"])
    assert torch.equal(d["GT"].view(torch.int16),
                       gt_before.view(torch.int16)), "K2 wrote GT"
    partial = K._np(d["partial"])
    assert np.isfinite(partial).all(), "read past k1, m_pad or fa_store"
    win = xt[:fa, start:start + m_pad]
    for zi, (k0, k1) in enumerate(R.slab_bounds(m_pad, splitk)):
        want = win[:, k0:k1] @ gt[:, k0:k1].T          # zeros when empty
        bad = np.argwhere(partial[zi] != want)
        assert len(bad) == 0, ("partial slab", zi, (k0, k1), bad[:8],
                               len(bad))
    # both column tiles and the last feature rows carry a gradient
    psum = np.abs(partial.sum(axis=0))
    assert psum[:, :128].max() > 1 and psum[:, 128:].max() > 1
    assert psum[fa - 16:].max() > 1


# ------------------------------------------------------------------ #
# (b) bitwise against the legacy kernels
# ------------------------------------------------------------------ #

@pytest.mark.parametrize("splitk", [3, 8])
@pytest.mark.parametrize("fa", [160, 288])
def test_fullm_equals_legacy_bitwise(fa, splitk):
    m_pad, start = 384, 8
    xt, gt = _k2_case(7 + fa + splitk, fa, m_pad, start, dyadic=False)
    got = {}
    for variant in (3, 1, 2) if fa == 288 else (3, 1):
        d = _upload(xt, gt, fa, splitk)
        _launch(d, start, m_pad, variant)
        assert K._canary_intact(d["partial_can"]), variant
        got[variant] = d["partial"].clone()
    p3 = got[3]
    assert torch.isfinite(p3).all()
    assert (p3 != K.CANARY).all(), "a row below fa was not written"
    # order matters on these inputs: the float64 product differs
    want = xt[:fa, start:start + m_pad] @ gt[:, :m_pad].T
    assert (K._np(p3).sum(axis=0) != want).any()
    for variant, p in got.items():
        assert torch.equal(p3.view(torch.int32), p.view(torch.int32)), \
            ("variant", variant)


# ------------------------------------------------------------------ #
# (c) routing
# ------------------------------------------------------------------ #

def test_rule_routes_whole_fa_kernel_up_to_288():
    m_pad, start, splitk = 384, 0, 3
    xt, gt = _k2_case(3, 288, m_pad, start, dyadic=False)
    out = []
    for variant in (0, 3):
        d = _upload(xt, gt, 288, splitk)
        _launch(d, start, m_pad, variant)
        out.append(d["partial"].clone())
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


def test_rule_keeps_legacy_tiles_above_288():
    fa, m_pad, start, splitk = 320, 384, 0, 3
    assert not R.ceil_to(fa, 96) < R.ceil_to(fa, 128)   # the 128-row tile
    xt, gt = _k2_case(4, fa, m_pad, start, dyadic=False)
    out = []
    for variant in (0, 1):
        d = _upload(xt, gt, fa, splitk)
        _launch(d, start, m_pad, variant)
        assert K._canary_intact(d["partial_can"])
        out.append(d["partial"].clone())
    assert torch.isfinite(out[0]).all() and (out[0] != K.CANARY).all()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    d = _upload(xt, gt, fa, splitk)
    with pytest.raises(RuntimeError, match="288"):
        K._ext().grad_partial(d["XsT"], d["GT"], d["partial"], start,
                              m_pad, 3)
    torch.cuda.synchronize()
    assert (d["partial"] == K.CANARY).all()            # nothing launched


def test_grad_partial_rejects_bad_arguments():
    xt, gt = _k2_case(5, 160, 128, 0, dyadic=True)
    d = _upload(xt, gt, 160, 2)
    ext = K._ext()
    ok = (d["XsT"], d["GT"], d["partial"])
    with pytest.raises(RuntimeError, match="variant"):
        ext.grad_partial(*ok, 0, 128, 4)
    with pytest.raises(RuntimeError, match="start"):
        ext.grad_partial(*ok, 4, 128, 3)
    with pytest.raises(RuntimeError, match="n_pad"):
        ext.grad_partial(*ok, 8, 128, 3)
    with pytest.raises(RuntimeError, match="GT"):
        ext.grad_partial(d["XsT"], d["GT"].float(), d["partial"], 0, 128, 3)
    with pytest.raises(RuntimeError, match="gt_stride"):
        ext.grad_partial(*ok, 0, 384, 3)
    # fa = 352: 96-row tiles need 384 rows of XsT, fa_store is 384 -> fine;
    # fa = 480: they need 480 <= 512 too.  fa = 224 needs 288 > 256.
    xt2, gt2 = _k2_case(6, 224, 128, 0, dyadic=True)
    d2 = _upload(xt2, gt2, 224, 2)
    with pytest.raises(RuntimeError, match="fa_store"):
        ext.grad_partial(d2["XsT"], d2["GT"], d2["partial"], 0, 128, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ #
# (d) graph replay
# ------------------------------------------------------------------ #

def test_graph_replay_with_whole_fa_kernel():
    """The shape of test_graph_replay_equals_eager_epochs (fa = 160, two
    column tiles): K2 inside the captured epoch is now the whole-fa
    kernel, whose LDS attribute call must have happened before capture."""
    n, bs, f, fa, ncols = 400, 256, 150, 160, 130
    c = R.make_case(5, n, f, fa, ncols, R.LOSS_LOG, dyadic=False,
                    row_w=True, fmask=True, momentum=0.9)
    inv_m = torch.tensor([R.inv_m_of(c, s, min(bs, n - s))
                          for s in range(0, n, bs)], dtype=torch.float32)
    outs = []
    for solve in (True, False):
        d = K._device_step_buffers(c, bs, 8)
        a = K._step_args(d)
        if solve:
            K._ext().sgd_solve(*a, inv_m, bs, R.LOSS_LOG, 0.9,
                               c["intercept_row"], 3)
        else:
            for _ in range(3):
                K._ext().sgd_epoch(*a, inv_m, bs, R.LOSS_LOG, 1.0, 0.9,
                                   c["intercept_row"])
        torch.cuda.synchronize()
        for k in ("W_can", "V_can", "WbfT_can", "partial_can", "GT_can"):
            assert K._canary_intact(d[k]), k
        outs.append((d["W"].clone(), d["V"].clone(), d["WbfT"].clone(),
                     d["partial"].clone(), d["GT"].clone()))
    for x, y in zip(*outs):
        assert torch.isfinite(x.float()).all()
        assert torch.equal(x, y)
    moved = outs[0][0].cpu().double().numpy() - c["W"]
    assert np.abs(moved[: f + 1, :ncols]).max() > 1e-2
