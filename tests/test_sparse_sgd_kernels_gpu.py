"""
The sparse text-scale SGD kernels (ops/csrc/sparse_sgd_kernels.hip), one
kernel at a time against the float64 references of tests/_sparse_ref.py.

One ``ext.sp_sgd_epoch[_l1]`` call with n <= batch_size is one step:
[catch-up ->] K1 (k_sp_fwd) -> K2a (k_sp_colsum) -> K2b (k_sp_bias_scale)
-> K3 (k_sp_update).  Afterwards G shows K1 (and, through the weights the
forward read, the catch-up), ``part`` K2a, Wb / s / hb / U K2b and W / h /
q / uw / ul K3.  Each is compared with its reference fed with what the
previous kernel actually wrote, so a failure names one kernel.

Dyadic cases (hinge and squared loss, adaptive off) are compared bit for
bit: tests/test_sparse_ref.py pins that no fp32 operation of such a step
can round.  Log-loss cases run with adaptive on: a G element may leave
bf16_rne(reference) only where the reference lies within a derived delta
of a bf16 rounding boundary (``_sparse_ref.g_interval``), and the later
kernels carry fp32 chain bounds derived in comments below.

name of a ``_sparse_ref.STEP_CASES`` entry -> what it reaches
  c64-m5               rows not a multiple of rpb = 4; a partial block
  c64-m1-l1-mid        one row
  c128-m31-mid         tile 128, rpb 2; one colsum chunk with a tail
  c192-m33-l1-mid      cp 192 = 3 tiles of 64; second chunk of one row
  c192-m96-mid         cp 192; nch 3; a feature present in every row
  c256-m128-l1         tile 256; nch 4
  c320-m33-l1-mid      second blockIdx.y block and its c >= cp guard
  c320-m96             the same from a fresh state, a feature in every row
  c256-m2100-mid       rows > 2048 blocks: grid-stride second pass; nch 66
  c256-uf2400-l1-mid   slots > 2048 blocks: grid-stride second pass in K3
                       and the catch-up
  c64-m8200-mid        8200 rows at 4 per block: second pass; chunk 64,
                       nch 129
  c64-empty-l1-mid     every row empty: z = Wb, uf == 0, K3 and the
                       catch-up do not launch
  log-*                the same tiles under the log loss with Adagrad
All but the last two kinds hold CSR rows of 0, 1, 3, 4, 5, 7, 8 and 9
entries and CSC slots of 1, 3, 4, 5 and 9 rows (both unroll-by-4 tails).
"""

import numpy as np
import pytest
import torch

import _sparse_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = R.EPS32
SLACK = 1 + 2.0 ** -10   # second-order terms of the first-order bounds
RSQ = 2.0 ** -20         # relative allowance for the Adagrad rsqrt
CANARY = 12345.0         # finite, and no kernel result equals it
STALE = 7.0              # pre-fill of G; rows past m must keep it


def _ext():
    from skdist_amd.ops import require_hip

    return require_hip()


def _f32(a):
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return torch.tensor(a, dtype=torch.float32, device=DEV)


def _int(a, dt):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV)


def _np(t):
    return t.detach().cpu().to(torch.float64).numpy()


def _guarded(values, dtype, extra_rows):
    """``values`` [r, ...] as the leading rows of a larger allocation whose
    trailing ``extra_rows`` rows hold CANARY; narrowing dim 0 of a
    contiguous tensor keeps it contiguous.  Returns (view, canary view)."""
    v = torch.tensor(np.asarray(values, np.float64), dtype=torch.float32)
    assert np.array_equal(v.double().numpy(), np.asarray(values, np.float64))
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


_TABLES = ("W", "h", "q", "uw", "ul")
_VECTORS = ("Wb", "s", "hb", "U")


def _upload(c, st=None, g_rows=None):
    """One case on the device.  Every buffer a kernel writes sits in front
    of canary rows; G holds ``g_rows`` + 3 rows of STALE and ``part`` the
    chunk rows of the largest batch + 3 rows of CANARY."""
    st = R.state_of(c) if st is None else st
    cp = c["cp"]
    d = {"can": {}}
    for k in _TABLES + _VECTORS:
        if st[k] is None:
            d[k] = torch.empty(0, dtype=torch.float32, device=DEV)
        else:
            d[k], d["can"][k] = _guarded(st[k], torch.float32,
                                         2 if k in _TABLES else 64)
    m0 = min(c["batch_size"], c["n"]) if g_rows is None else g_rows
    d["G"], d["can"]["G"] = _guarded(np.full((m0 + 3, cp), STALE),
                                     torch.bfloat16, 2)
    d["part"], d["can"]["part"] = _guarded(
        np.full((R.chunk_rule(m0)[1] + 3, cp), CANARY), torch.float32, 2)
    d["crow"] = _int(c["crow"], torch.int64)
    d["cidx"] = _int(c["cidx"], torch.int32)
    d["cval"] = _f32(c["cval"])
    d["y"] = _f32(c["y"])
    d["fold"] = _int(c["fold"], torch.int32)
    d["row_w"] = (_f32(c["row_w"]) if c["row_w"] is not None
                  else torch.empty(0, dtype=torch.float32, device=DEV))
    for k in ("col_class", "col_fold", "col_class2"):
        d[k] = _int(c[k], torch.int32)
    d["col_lr"], d["col_l2"] = _f32(c["col_lr"]), _f32(c["col_l2"])
    if c["l1"]:
        d["col_l1"] = _f32(c["col_l1"])
    d["ufeat"] = _int(c["ufeat"], torch.int32)
    d["cptr"] = _int(c["cptr"], torch.int64)
    d["ridx"] = _int(c["ridx"], torch.int32)
    d["bval"] = _f32(c["bval"])
    d["ub_ptr"] = torch.tensor(c["ub_ptr"], dtype=torch.int64)
    inv = np.asarray(c["inv_m"], np.float64)
    assert R.is_f32(inv)
    d["inv_m"] = torch.tensor(inv, dtype=torch.float32)
    return d


def _args(d, c):
    return (d["crow"], d["cidx"], d["cval"], d["W"], d["Wb"], d["s"],
            d["h"], d["hb"], d["G"], d["part"], d["y"], d["fold"],
            d["row_w"], d["col_class"], d["col_fold"], d["col_class2"],
            d["col_lr"], d["col_l2"], d["ufeat"], d["cptr"], d["ridx"],
            d["bval"], d["ub_ptr"], d["inv_m"], c["batch_size"],
            c["loss_id"])


def _epoch(d, c):
    if c["l1"]:
        _ext().sp_sgd_epoch_l1(*_args(d, c), c["lr_scale"], d["col_l1"],
                               d["U"], d["q"], d["uw"], d["ul"])
    else:
        _ext().sp_sgd_epoch(*_args(d, c), c["lr_scale"])
    torch.cuda.synchronize()


def _read_state(d):
    return {k: (_np(d[k]) if d[k].numel() else None)
            for k in _TABLES + _VECTORS}


def _canaries(d):
    for k, t in d["can"].items():
        assert _canary_intact(t), ("canary after", k)


def _no_bad(name, got, want, tol=None):
    if tol is None:
        bad = np.argwhere(got != want)
    else:
        bad = np.argwhere(~(np.abs(got - want) <= tol))
    assert len(bad) == 0, (name, bad[:8], len(bad))


def _touch_bound(t, dw, rho, adaptive):
    """fp32 error bounds of one sp_l1_touch whose incoming weight is off
    by at most dw and whose rsqrt by at most rho (relative), every other
    input being exact; eps = 2^-24 per fp32 operation:
      d = U - ul, credit = d r       <= |credit| (2 eps + rho)
      u = uw + credit                <= that + eps |u|            =: du
      t = u +- q                     <= du + eps |t|              =: dt
      pre = w -+ t                   <= dw + dt + eps |pre|       =: dpre
      w' = clamp(pre) (1-Lipschitz)  <= dpre =: dw', and 0 where pre is
                                     past 0 by more than dpre: both clamp
      q' = q + (w' - w)              <= dw' + dw + eps (|w' - w| + |q'|)
    Returns (dw', dq', du)."""
    du = np.zeros_like(t["w"])
    if adaptive:
        credit = np.abs(t["u"] - (t["uw_in"]))
        du = credit * (2 * EPS + rho) + EPS * np.abs(t["u"])
    dt = du + EPS * np.abs(t["t"])
    dpre = dw + dt + EPS * np.abs(t["pre"])
    dpre = dpre * SLACK
    both0 = ((t["w_in"] > 0) & (t["pre"] + dpre <= 0)) | (
        (t["w_in"] < 0) & (t["pre"] - dpre >= 0))
    dwn = np.where(both0, 0.0, dpre)
    dq = dwn + dw + EPS * (np.abs(t["w"] - t["w_in"]) + np.abs(t["q"]))
    return dwn, dq * SLACK, du * SLACK


def _dphi(g, dg, h0):
    """Bound on |phi(x) - phi(g)| for |x - g| <= dg, phi(x) = x rsqrt(h0 +
    x x + 1e-12): dg times phi' at the smallest |x| in reach."""
    xlo = np.maximum(np.abs(g) - dg, 0.0)
    return dg * (h0 + R.H_EPS) / (h0 + R.H_EPS + xlo ** 2) ** 1.5


# ------------------------------------------------------------------ #
# staged single-step tests
# ------------------------------------------------------------------ #

@pytest.mark.parametrize("name", list(R.STEP_CASES))
def test_staged_step(name):
    c = R.step_case(name)
    exact = c["loss_id"] != R.LOSS_LOG
    ad, l1, cp, nc, f = c["adaptive"], c["l1"], c["cp"], c["ncols"], c["f"]
    start, m, ufeat, cptr = R.batch_slices(c, 0)
    assert start == 0 and m == c["n"]
    rows = np.arange(m)
    j = np.asarray(ufeat, np.int64)
    st0 = R.state_of(c)
    inv_m, ls = float(c["inv_m"][0]), c["lr_scale"]
    chunk, nch = R.chunk_rule(m)

    # ---- the step on the device
    d = _upload(c)
    _epoch(d, c)
    got = _read_state(d)
    G = _np(d["G"])
    part = _np(d["part"])
    _canaries(d)

    # ---- catch-up.  Its output is overwritten by K3, so it shows through
    # G: the reference forward reads the caught-up weights.  Dyadic cases
    # use the reference touch (exact).  Otherwise the touch rounds, and
    # the weights the forward really read are taken from k_sp_l1_flush --
    # the same device function over all rows -- run on a copy of the start
    # state, after checking them against the reference touch.
    st_c, tc = R.catchup(c, st0, ufeat)
    if tc is not None and not exact:
        p = _upload(c)
        _ext().sp_l1_flush(p["W"], p["h"], p["U"], p["q"], p["uw"], p["ul"])
        torch.cuda.synchronize()
        _canaries(p)
        proxy = _read_state(p)
        tc.update(w_in=st0["W"][j], uw_in=st0["uw"][j])
        dwc, dqc, duc = _touch_bound(tc, 0.0, RSQ + EPS, True)
        _no_bad("flush W", proxy["W"][j], st_c["W"][j], dwc)
        _no_bad("flush q", proxy["q"][j], st_c["q"][j], dqc)
        _no_bad("flush uw", proxy["uw"][j], st_c["uw"][j], duc)
        _no_bad("flush ul", proxy["ul"][j], st_c["ul"][j])
        for k in ("W", "q", "uw", "ul"):
            st_c[k][j] = proxy[k][j]

    # ---- K1
    fw = R.ref_fwd(c["crow"], c["cidx"], c["cval"], st_c["W"], st_c["Wb"],
                   st_c["s"], c["y"], c["fold"], c["row_w"], c["col_class"],
                   c["col_fold"], c["col_class2"], rows, c["loss_id"])
    train = fw["train"]
    want_g = R.bf16_rne(fw["g"])
    assert (G[m:] == STALE).all(), "K1 wrote past m"
    assert (~train[:, :nc]).any() and (G[:m][~train] == 0).all(), \
        "masked element not 0"
    if exact:
        _no_bad("G (row, col)", G[:m], want_g)
    else:
        lo, hi, near, delta = R.g_interval(c, fw, rows)
        print(f"{name}: near a bf16 boundary: {near.mean():.4%} of G")
        bad = np.argwhere((G[:m] < lo) | (G[:m] > hi))
        assert len(bad) == 0, ("G (row, col)", bad[:8], len(bad))
        # ... and a near-boundary element is at most one bf16 step off.
        # That follows from the interval only while delta is below half a
        # bf16 step; for |g| under about 2^8 delta (a saturated sigmoid:
        # g ~ 1e-8 against delta ~ 1e-6) the interval spans many bf16
        # values and is itself the criterion.
        step1 = R.bf16_step(np.abs(fw["g"]) + delta)
        narrow = near & (delta <= step1 / 2)
        assert (np.abs(G[:m] - want_g) <= step1)[narrow].all()
        if c["midfit"] and m >= 31:
            assert (np.abs(fw["z"]) > 30).any()     # the clamp is reached
    empty = fw["nnz"] == 0
    if empty.any():                      # an empty row gives z = Wb
        assert np.array_equal(fw["z"][empty][0], st_c["Wb"])
    if l1 and c["midfit"] and len(j):
        # the forward without the catch-up would have differed
        fw0 = R.ref_fwd(c["crow"], c["cidx"], c["cval"], st0["W"],
                        st0["Wb"], st0["s"], c["y"], c["fold"], c["row_w"],
                        c["col_class"], c["col_fold"], c["col_class2"],
                        rows, c["loss_id"])
        assert (R.bf16_rne(fw0["g"]) != want_g).any()
    if m > 3:   # transpose detection: g differs across columns and rows
        assert np.abs(fw["g"] - fw["g"][:, :1]).max() > 0.1
        assert np.abs(fw["g"] - fw["g"][:1]).max() > 0.1

    # ---- K2a, from the G the device wrote
    want_part = R.ref_colsum(G, m, chunk)
    assert (part[nch:] == CANARY).all(), "K2a wrote past n_chunks"
    if exact:
        _no_bad("part (chunk, col)", part[:nch], want_part)
    else:
        # at most `chunk` adds per chunk, each rounding a running sum of
        # at most sum |G| over the chunk
        tol = chunk * EPS * R.ref_colsum(np.abs(G), m, chunk)
        _no_bad("part (chunk, col)", part[:nch], want_part, tol)

    # ---- K2b, from the chunks the device wrote
    b = R.ref_bias_scale(part[:nch], st0["Wb"], st0["s"], st0["hb"],
                         c["col_lr"], c["col_l2"], inv_m, ls, c["col_l1"],
                         st0["U"])
    # lr, lr_scale, l2 and s are powers of two in every case: s' is exact
    _no_bad("s", got["s"], b["s"])
    if exact:
        _no_bad("Wb", got["Wb"], b["Wb"])
        if l1:
            _no_bad("U", got["U"], b["U"])
    else:
        # g = (sum of nch chunks) inv_m: at most nch adds, each rounding a
        # running sum of at most sum |part|, then one product
        #   dg   = nch eps sum|part| inv_m + eps |g|
        #   hb'  = hb + g g       <= 2 |g| dg + dg^2 + eps (g^2 + hb')
        #   step = lr phi(g), phi(x) = x rsqrt(hb + x x + 1e-12), computed
        #          from the device's own g: phi' = (hb + 1e-12) /
        #          (hb + x x + 1e-12)^1.5, largest at the smallest |x| in
        #          reach, carries dg; the roundings on the way (x x, the
        #          two adds, the rsqrt at 2^-20, the product; lr g is
        #          exact, lr being a power of two) add (2^-20 + 3 eps)
        #   Wb'  = Wb - step      <= dstep + eps |Wb'|
        #   U'   = U + lr l1 / s' (product and quotient exact)
        #                         <= eps |U'|
        dg = nch * EPS * np.abs(part[:nch]).sum(axis=0) * inv_m \
            + EPS * np.abs(b["g"])
        dhb = 2 * np.abs(b["g"]) * dg + dg * dg \
            + EPS * (b["g"] ** 2 + b["hb"])
        dstep = b["lr"] * _dphi(b["g"], dg, st0["hb"]) \
            + np.abs(b["step"]) * (RSQ + 3 * EPS)
        _no_bad("hb", got["hb"], b["hb"], dhb * SLACK)
        _no_bad("Wb", got["Wb"], b["Wb"],
                (dstep + EPS * np.abs(b["Wb"])) * SLACK)
        if l1:
            _no_bad("U", got["U"], b["U"], EPS * np.abs(b["U"]))

    # ---- K3, from the G, s' and U' the device wrote
    u = R.ref_update(ufeat, cptr, c["ridx"], c["bval"], G[:m], st_c["W"],
                     st_c["h"], got["s"], c["col_lr"], inv_m, ls,
                     got["U"], st_c["q"], st_c["uw"], st_c["ul"])
    rest = np.setdiff1d(np.arange(f), j)
    for k in _TABLES:                 # rows of no batch feature never move
        if got[k] is not None:
            _no_bad(k + " untouched", got[k][rest], st0[k][rest])
    moved = np.abs(u["step"] / got["s"][None, :])
    if exact:
        R.assert_exact_step(c, st_c, fw, G[:m], part[:nch], b, u)
        _no_bad("W (feature, col)", got["W"], u["W"])
        if l1:
            _no_bad("q (feature, col)", got["q"], u["q"])
    elif len(j):
        # a slot of cnt rows: cnt products and cnt + 3 adds at most, each
        # rounding a running sum of at most sum |bval G|
        #   da   = (cnt + 3) eps sum|bval G|;  dg = da inv_m + eps |g|
        #   h'   = h + g g        <= 2 |g| dg + dg^2 + eps (g^2 + h')
        #   step = lr phi(g)      as in K2b
        #   w1   = W - step / s'  (s' a power of two: the quotient is
        #                          exact)  <= dstep / s' + eps |w1|
        # then, with L1, one touch with dw = dw1 (_touch_bound); its
        # r = rsqrt(h' + 1e-12) carries dg at relative |g| dg / (h' +
        # 1e-12), taken at the smallest |g| in reach, plus the roundings
        dg = (u["cnt"][:, None] + 3) * EPS * u["absa"] * inv_m \
            + EPS * np.abs(u["g"])
        hn, h0 = u["h"][j], st_c["h"][j]
        dh = 2 * np.abs(u["g"]) * dg + dg * dg + EPS * (u["g"] ** 2 + hn)
        lr = (c["col_lr"] * ls)[None, :]
        dstep = lr * _dphi(u["g"], dg, h0) \
            + np.abs(u["step"]) * (RSQ + 3 * EPS)
        xlo = np.maximum(np.abs(u["g"]) - dg, 0.0)
        rho = RSQ + 2 * EPS + np.abs(u["g"]) * dg / (h0 + xlo ** 2 + R.H_EPS)
        dw = (dstep / got["s"][None, :] + EPS * np.abs(u["w1"])) * SLACK
        _no_bad("h (slot, col)", got["h"][j], hn, dh * SLACK)
        if l1:
            t = u["touch"]
            # the touch branches on the sign of w1: the bound holds where
            # the device's w1 has the reference's sign
            assert ((u["w1"] == 0) | (np.abs(u["w1"]) > dw)).all()
            t.update(w_in=u["w1"], uw_in=st_c["uw"][j])
            dw, dq, du = _touch_bound(t, dw, rho, True)
            _no_bad("q (slot, col)", got["q"][j], u["q"][j], dq)
            _no_bad("uw (slot, col)", got["uw"][j], u["uw"][j], du)
            _no_bad("ul (slot, col)", got["ul"][j], u["ul"][j])
        _no_bad("W (slot, col)", got["W"][j], u["W"][j], dw)
        ratio = dw.max() / moved.max()
        print(f"{name}: largest W tolerance / largest step = {ratio:.2e}")
        assert ratio < 1e-4    # a few ulps, far below the step itself
    # pad columns hold exactly what they held
    assert (got["W"][:, nc:] == 0).all() and (got["Wb"][nc:] == 0).all()
    assert (got["s"][nc:] == 1).all()
    if l1:
        assert (got["U"][nc:] == 0).all() and (got["q"][:, nc:] == 0).all()
    if len(j) and m > 3:   # the step moved W, differently per column / row
        dW = (got["W"] - st0["W"])[:, :nc]
        assert np.abs(dW - dW[:, :1]).max() > 1e-3
        assert np.abs(dW - dW[:1]).max() > 1e-3


# ------------------------------------------------------------------ #
# two batches in one call: start != 0
# ------------------------------------------------------------------ #

@pytest.mark.parametrize("ncols,loss_id,l1", [(24, 2, False),
                                              (150, 1, True)])
def test_two_batches_match_two_reference_steps(ncols, loss_id, l1):
    """n = 160 in batches of 128: the second step starts at row 128 with
    m = 32, its own 1/m and its own CSC slice.  Dyadic, so the final state
    is compared bit for bit with two composed reference steps; G rows 32
    and up keep the first batch's values."""
    c = R.make_case(21 + ncols, 160, 60, ncols, loss_id, l1=l1, midfit=True,
                    row_w=True, ovo=True, batch_size=128)
    st = R.state_of(c)
    st1, G1 = R.composed_step(c, st, 0)
    st2, G2 = R.composed_step(c, st1, 1)
    assert G2.shape[0] == 32 and (G1[:32] != G2).any()
    d = _upload(c)
    _epoch(d, c)
    _canaries(d)
    got = _read_state(d)
    for k in ("W", "Wb", "s") + (("U", "q") if l1 else ()):
        _no_bad(k, got[k], st2[k])
    G = _np(d["G"])
    _no_bad("G of batch 2", G[:32], G2)
    _no_bad("G of batch 1", G[32:128], G1[32:])
    assert (G[128:] == STALE).all()
    assert (got["W"] != st1["W"]).any() and (st1["W"] != st["W"]).any()


# ------------------------------------------------------------------ #
# whole-table kernels
# ------------------------------------------------------------------ #

def _table_state(f, ncols, adaptive, seed):
    """Dyadic mid-fit state of an [f, cp] table set with pad columns."""
    rng = np.random.default_rng(seed)
    cp = R.pad_cols(ncols)
    z = lambda: np.zeros((f, cp))
    st = dict(W=z(), q=z(), s=np.ones(cp), U=np.zeros(cp), h=None,
              uw=None, ul=None)
    st["W"][:, :ncols] = rng.integers(-8, 9, size=(f, ncols)) / 16.0
    st["q"][:, :ncols] = rng.integers(-2, 3, size=(f, ncols)) / 16.0
    st["s"][:ncols] = rng.choice([0.5, 0.25, 2.0 ** -10], size=ncols)
    st["U"][:ncols] = rng.integers(1, 5, size=ncols) / 16.0
    if adaptive:
        st["h"], st["uw"], st["ul"] = z(), z(), z()
        # h == 0, or h with an exactly representable 1e-12-free rsqrt is
        # not possible: credit is bitwise only where U == ul or h == 0
        st["h"][:, :ncols] = rng.choice([0.0, 0.25, 4.0], size=(f, ncols))
        st["uw"][:, :ncols] = rng.integers(0, 3, size=(f, ncols)) / 16.0
        st["ul"][:, :ncols] = np.where(
            rng.random((f, ncols)) < 0.5, st["U"][None, :ncols],
            st["U"][None, :ncols] / 2)
    return st, cp


def _up(st, keys):
    d, can = {}, {}
    for k in keys:
        if st[k] is None:
            d[k] = torch.empty(0, dtype=torch.float32, device=DEV)
        else:
            d[k], can[k] = _guarded(st[k], torch.float32,
                                    2 if st[k].ndim == 2 else 64)
    return d, can


_TABLE_SHAPES = [(f, ncols, ad) for f in (1, 3) for ncols in (24, 290)
                 for ad in (False, True)]


@pytest.mark.parametrize("f,ncols,adaptive", _TABLE_SHAPES)
def test_renorm_kernels_bits(f, ncols, adaptive):
    st, cp = _table_state(f, ncols, adaptive, 5)
    # products of dyadic values: exact
    d, can = _up(st, ("W", "s"))
    _ext().sp_renorm(d["W"], d["s"])
    torch.cuda.synchronize()
    _no_bad("renorm W", _np(d["W"]), R.ref_renorm(st["W"], st["s"]))
    _no_bad("renorm s", _np(d["s"]), st["s"])
    d1, can1 = _up(st, ("W", "s", "q", "uw", "ul"))
    _ext().sp_renorm_l1(d1["W"], d1["s"], d1["q"], d1["uw"], d1["ul"])
    torch.cuda.synchronize()
    want = R.ref_renorm_l1(st["W"], st["s"], st["q"], st["uw"], st["ul"])
    for k, w in zip(("W", "q", "uw", "ul"), want):
        if w is not None:
            assert R.is_f32(w)
            _no_bad("renorm_l1 " + k, _np(d1[k]), w)
    for t in list(can.values()) + list(can1.values()):
        assert _canary_intact(t)
    assert (_np(d["W"])[:, ncols:] == 0).all()
    assert (_np(d["W"])[:, :ncols] != st["W"][:, :ncols]).any()


@pytest.mark.parametrize("f,ncols,adaptive", _TABLE_SHAPES)
def test_l1_flush_bits(f, ncols, adaptive):
    st, cp = _table_state(f, ncols, adaptive, 6)
    c = dict(l1=True, adaptive=adaptive, f=f)
    want, t = R.catchup(c, st, np.arange(f))
    d, can = _up(st, ("W", "h", "U", "q", "uw", "ul"))
    _ext().sp_l1_flush(d["W"], d["h"], d["U"], d["q"], d["uw"], d["ul"])
    torch.cuda.synchronize()
    for v in can.values():
        assert _canary_intact(v)
    got = {k: _np(d[k]) for k in ("W", "q", "U")}
    _no_bad("U", got["U"], st["U"])
    if not adaptive:
        for k in ("t", "pre", "w", "q"):
            assert R.is_f32(t[k])
        _no_bad("flush W", got["W"], want["W"])
        _no_bad("flush q", got["q"], want["q"])
    else:
        # where no credit accrues (h == 0 or ul == U) u = uw and the
        # touch is exact; elsewhere the rsqrt rounds: _touch_bound
        t.update(w_in=st["W"], uw_in=st["uw"])
        dw, dq, du = _touch_bound(t, 0.0, RSQ + EPS, True)
        flat = (st["h"] == 0) | (st["ul"] == st["U"][None, :])
        assert flat.any() and (~flat).any()
        for k, tol in (("W", dw), ("q", dq), ("uw", du)):
            g = _np(d[k])
            _no_bad("flush " + k, g, want[k], np.where(flat, 0.0, tol))
        _no_bad("flush ul", _np(d["ul"]),
                np.broadcast_to(st["U"][None, :], st["ul"].shape))
        _no_bad("h", _np(d["h"]), st["h"])
    # the clip took some weights exactly to 0 and left others standing
    z = (got["W"][:, :ncols] == 0) & (st["W"][:, :ncols] != 0)
    assert z.any() and (got["W"][:, :ncols] != 0).any()
    assert (got["W"][:, ncols:] == 0).all()


def _forward_case(f, ncols):
    rng = np.random.default_rng(f + ncols)
    st, cp = _table_state(f, ncols, False, 7)
    st["Wb"] = np.zeros(cp)
    st["Wb"][:ncols] = rng.integers(-4, 5, size=ncols) / 8.0
    # rows: empty, one entry, all features, all features again
    sets = [[], [0], list(range(f)), list(range(f))]
    crow = np.cumsum([0] + [len(x) for x in sets]).astype(np.int64)
    cidx = np.asarray(sum(sets, []), np.int32)
    cval = rng.choice([-1.0, -0.5, 0.5, 1.0], size=len(cidx))
    return st, cp, crow, cidx, cval


@pytest.mark.parametrize("f,ncols", [(1, 24), (3, 24), (1, 290), (3, 290)])
@pytest.mark.parametrize("rows", [[3, 0, 2, 3, 1, 0, 0], [2], []],
                         ids=["unordered", "m1", "m0"])
def test_sp_forward_bits(f, ncols, rows):
    st, cp, crow, cidx, cval = _forward_case(f, ncols)
    rows = np.asarray(rows, np.int64)
    fw = R.ref_fwd(crow, cidx, cval, st["W"], st["Wb"], st["s"],
                   np.zeros(4), np.zeros(4, np.int32), None,
                   np.zeros(cp, np.int32), np.zeros(cp, np.int32),
                   np.full(cp, -1, np.int32), rows, 0)
    assert R.is_f32(fw["z"])                      # dyadic: exact
    Z, can = _guarded(np.full((len(rows) + 2, cp), STALE), torch.float32, 2)
    _ext().sp_forward(_int(crow, torch.int64), _int(cidx, torch.int32),
                      _f32(cval), _f32(st["W"]), _f32(st["Wb"]),
                      _f32(st["s"]), _int(rows, torch.int64),
                      Z.narrow(0, 0, len(rows)))
    torch.cuda.synchronize()
    assert _canary_intact(can)
    got = _np(Z)
    _no_bad("Z", got[:len(rows)], fw["z"])
    assert (got[len(rows):] == STALE).all()       # m = 0: Z untouched
    if len(rows) > 1:
        assert np.array_equal(got[1], st["Wb"])   # the empty row
        assert np.array_equal(got[0], got[3])


# ------------------------------------------------------------------ #
# graph replay
# ------------------------------------------------------------------ #

def test_graph_replay_equals_eager_epochs():
    """sp_sgd_solve(epochs=3) replays a captured epoch twice; three
    sp_sgd_epoch(lr_scale=1) calls launch the same kernels eagerly.  No
    kernel uses atomics and every (item, column) has one owning lane, so
    the two agree bit for bit -- at cp = 192 only since the column tile
    divides the block -- and so do two runs of either."""
    c = R.make_case(9, 160, 60, 150, R.LOSS_LOG, dyadic=False,
                    adaptive=True, midfit=True, row_w=True, ovo=True,
                    batch_size=128, lr_scale=1.0)
    assert c["cp"] == 192 and len(c["inv_m"]) == 2
    outs = []
    for solve in (True, False, True, False):
        d = _upload(c)
        if solve:
            _ext().sp_sgd_solve(*_args(d, c), 3)
        else:
            for _ in range(3):
                _ext().sp_sgd_epoch(*_args(d, c), 1.0)
        torch.cuda.synchronize()
        _canaries(d)
        outs.append([d[k].clone() for k in ("W", "Wb", "s", "h", "hb")])
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.isfinite(x).all()
            assert torch.equal(x, y)
    moved = _np(outs[0][0]) - c["W"]
    assert np.abs(moved[:, :150]).max() > 1e-2
