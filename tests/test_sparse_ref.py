"""
The float64 references of tests/_sparse_ref.py, checked on the CPU against
the project's fp32 eager mirror (``_sparse_sgd._sparse_sgd_eager``,
``_sp_l1_touch``, ``_sp_forward_eager``), so the reference the GPU tests
compare the HIP kernels with is itself tested wherever the suite runs;
plus the input-side half of the GPU test's log-loss criterion (the share
of G elements near a bf16 rounding boundary).
"""

import numpy as np
import pytest
import torch

import _sparse_ref as R
from skdist_amd.models._sparse_sgd import (SparseDeviceDataset,
                                           _sp_forward_eager,
                                           _sparse_sgd_eager)


class _Shim:
    pass


def _t(a, dt=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dt)


def _mirror_fit(c):
    """One epoch (+ renorm check + flush) of the eager mirror from the
    case's start state, lr_scale 1.  Returns the final state as float64."""
    ds = _Shim()
    ds.device, ds.n, ds.f = torch.device("cpu"), c["n"], c["f"]
    sh = dict(crow=_t(c["crow"], torch.int64), cidx=_t(c["cidx"],
              torch.int32), cval=_t(c["cval"]), y=_t(c["y"]),
              fold=_t(c["fold"], torch.int32),
              rw=None if c["row_w"] is None else _t(c["row_w"]),
              inv_m=_t(c["inv_m"]))
    col = dict(cls=_t(c["col_class"], torch.int32),
               fold=_t(c["col_fold"], torch.int32),
               cls2=_t(c["col_class2"], torch.int32),
               lr=_t(c["col_lr"]), l2=_t(c["col_l2"]))
    none = torch.empty(0)
    opt = lambda k: none if c[k] is None else _t(c[k])
    W, Wb, s = _t(c["W"]), _t(c["Wb"]), _t(c["s"])
    H, Hb = opt("h"), opt("hb")
    l1 = None
    if c["l1"]:
        l1 = dict(col=_t(c["col_l1"]), U=_t(c["U"]), q=_t(c["q"]),
                  u=opt("uw"), ul=opt("ul"))
    _sparse_sgd_eager(ds, sh, W, Wb, s, H, Hb, col, c["loss_id"], 1,
                      c["batch_size"], 0.0, c["cp"], l1=l1)
    out = dict(W=W, Wb=Wb, s=s, h=H, hb=Hb)
    if l1 is not None:
        out.update(U=l1["U"], q=l1["q"], uw=l1["u"], ul=l1["ul"])
    return {k: v.double().numpy() for k, v in out.items() if v.numel()}


def _reference_fit(c):
    """The same epoch from the composed float64 references.  Also returns
    the magnitudes the fp32 tolerance is built from."""
    st = R.state_of(c)
    nb = len(c["inv_m"])
    mag = np.abs(st["W"]).copy()
    flip = np.zeros_like(mag)
    for bi in range(nb):
        start, m, ufeat, cptr = R.batch_slices(c, bi)
        pre, _ = R.catchup(c, st, ufeat)
        new, G = R.composed_step(c, st, bi)
        # everything a weight passed through in this step: its values
        # before and after, the gradient step in stored units and, under
        # L1, the credit and the booked penalty
        u = R.ref_update(ufeat, cptr, c["ridx"], c["bval"], G, pre["W"],
                         pre["h"], new["s"], c["col_lr"], c["inv_m"][bi],
                         c["lr_scale"], new["U"], pre["q"], pre["uw"],
                         pre["ul"])
        lr_r_s = (c["col_lr"] * c["lr_scale"])[None, :] * u["r"] \
            / new["s"][None, :]
        j = np.asarray(ufeat, np.int64)
        mag[j] += lr_r_s * u["absa"] * c["inv_m"][bi]
        mag += np.abs(new["W"]) + np.abs(pre["W"])
        if c["l1"]:
            mag += np.abs(new["q"]) + np.abs(pre["q"]) + new["U"][None, :]
            if c["adaptive"]:
                mag += np.abs(new["uw"])
        if c["loss_id"] == R.LOSS_LOG:
            # the mirror's fp32 g may round to the other bf16 neighbour
            # where the reference lies within delta of a boundary: each
            # such element moves a slot's gradient by at most one bf16
            # step times |val|, the weight by lr r / s' times that
            rows = start + np.arange(m)
            fw = R.ref_fwd(c["crow"], c["cidx"], c["cval"], pre["W"],
                           pre["Wb"], pre["s"], c["y"], c["fold"],
                           c["row_w"], c["col_class"], c["col_fold"],
                           c["col_class2"], rows, c["loss_id"])
            lo, hi, near, delta = R.g_interval(c, fw, rows)
            one = near * R.bf16_step(np.abs(fw["g"]) + delta)
            X = R.csr_rows_dense(c["crow"], c["cidx"], c["cval"], rows,
                                 c["f"])
            flip[j] += (lr_r_s * (np.abs(X).T @ one)[j]) * c["inv_m"][bi]
        st = new
    if st["s"].min() < 1e-3:                 # the per-epoch renorm check
        if c["l1"]:
            st["W"], st["q"], st["uw"], st["ul"] = R.ref_renorm_l1(
                st["W"], st["s"], st["q"], st["uw"], st["ul"])
            st["U"] = st["U"] * st["s"]
        else:
            st["W"] = R.ref_renorm(st["W"], st["s"])
        mag = mag * st["s"][None, :]
        flip = flip * st["s"][None, :]
        st["s"] = np.ones_like(st["s"])
    if c["l1"]:
        st = R.flush(c, st)
    return st, mag, flip


# (loss, adaptive, l1, row_w, ovo, regress, ncols, n, batch, midfit,
#  renorm).  ncols 150 pads to 192 and 290 to 320.  Log loss stays on one
# batch and off the adaptive-L1 pair, so that the only effect of a bf16
# boundary flip is the one-step term derived in _reference_fit.  For the
# same reason the adaptive-L1 pair (whose catch-up leaves weights that are
# no longer dyadic, so z is not exact) runs with the hinge loss from a
# mid-fit state, where g depends on the sign of 1 - s z alone, and with
# the squared loss only from a fresh state on one batch (z = 0 exactly).
_CASES = [
    (1, False, False, False, False, False, 24, 70, 70, True, False),
    (1, True, True, True, True, False, 150, 100, 64, True, False),
    (2, True, True, False, False, False, 24, 70, 70, False, False),
    (2, False, True, True, True, True, 290, 100, 64, True, False),
    (2, True, False, False, False, True, 150, 70, 70, True, False),
    (1, True, True, True, False, False, 24, 100, 64, True, True),
    (1, False, True, False, True, False, 290, 70, 70, True, True),
    (1, False, False, True, False, False, 150, 100, 64, True, True),
    (0, True, False, True, True, False, 150, 70, 70, True, False),
    (0, False, True, False, False, False, 290, 70, 70, True, False),
    (0, False, False, True, True, False, 24, 70, 70, True, False),
]


@pytest.mark.parametrize(
    "loss,adaptive,l1,row_w,ovo,regress,ncols,n,bs,midfit,renorm", _CASES)
def test_composed_reference_matches_eager_mirror(
        loss, adaptive, l1, row_w, ovo, regress, ncols, n, bs, midfit,
        renorm):
    c = R.make_case(3 + loss + ncols, n, 30, ncols, loss,
                    dyadic=loss != R.LOSS_LOG, adaptive=adaptive, l1=l1,
                    midfit=midfit, row_w=row_w, ovo=ovo, regress=regress,
                    batch_size=bs, lr_scale=1.0)
    if renorm:
        c["s"][:ncols] *= 2.0 ** -9          # below the 1e-3 threshold
    want, mag, flip = _reference_fit(c)
    assert (want["s"] == 1).all() == renorm   # the renorm fired, or not
    got = _mirror_fit(c)

    # fp32 against float64: every fp32 operation of the mirror rounds a
    # value no larger than the magnitudes collected above; a slot sums at
    # most bs products and the chain around it is short, so bs + 32
    # roundings bound it (eps = 2^-24 each)
    tol = (bs + 32) * R.EPS32 * mag + flip
    nc = ncols
    err = np.abs(got["W"] - want["W"])
    bad = np.argwhere(err[:, :nc] > tol[:, :nc])
    assert len(bad) == 0, (bad[:8], err.max(), tol.max())
    moved = np.abs(want["W"] - c["W"])[:, :nc].max()
    assert np.median(tol[:, :nc]) < 1e-3 * moved, (np.median(tol), moved)
    for k in ("Wb", "s", "hb", "U"):
        if k in got:
            scale = np.abs(want[k]) + np.abs(c[k]) + 1.0
            e = np.abs(got[k] - want[k])[:nc]
            lim = (n + 32) * R.EPS32 * scale[:nc]
            if loss == R.LOSS_LOG:
                lim = lim + 2.0 ** -9 * 0.02   # <= 1% of rows flip a step
            assert (e <= lim).all(), (k, e.max())
    for k in ("q", "uw", "ul", "h"):
        if k in got:
            e = np.abs(got[k] - want[k])[:, :nc]
            lim = 4 * tol[:, :nc] + (bs + 32) * R.EPS32 * (
                np.abs(want[k][:, :nc]) + 1.0)
            assert (e <= lim).all(), (k, e.max())
    # pad columns never move
    assert (want["W"][:, nc:] == 0).all() and (want["Wb"][nc:] == 0).all()
    assert (want["s"][nc:] == 1).all()
    if l1:
        assert (want["U"][nc:] == 0).all()
        # exact zeros appear that the start state did not hold
        assert ((want["W"][:, :nc] == 0) & (c["W"][:, :nc] != 0)).any() \
            or not midfit
    # transpose detection: the fit differs across columns and rows
    d = (want["W"] - c["W"])[:, :nc]
    assert np.abs(d - d[:, :1]).max() > 1e-3
    assert np.abs(d - d[:1]).max() > 1e-3


def test_ref_fwd_matches_forward_mirror_on_unordered_rows():
    c = R.make_case(1, 40, 30, 290, R.LOSS_LOG, dyadic=False, midfit=True)
    rows = np.array([7, 0, 39, 7, 8, 0])       # row 0 and 8 are empty
    assert c["crow"][1] == c["crow"][0]
    ds = _Shim()
    ds.device = torch.device("cpu")
    ds.crow, ds.cidx, ds.cval = (_t(c["crow"], torch.int64),
                                 _t(c["cidx"], torch.int32), _t(c["cval"]))
    one = np.ones(c["cp"])
    Z = torch.empty(len(rows), c["cp"])
    _sp_forward_eager(ds, _t(c["W"]), _t(c["Wb"]), _t(rows, torch.int64), Z)
    fw = R.ref_fwd(c["crow"], c["cidx"], c["cval"], c["W"], c["Wb"], one,
                   c["y"], c["fold"], None, c["col_class"], c["col_fold"],
                   c["col_class2"], rows, 0)
    tol = (fw["nnz"][:, None] + 2) * R.EPS32 * (fw["absz"]
                                                + np.abs(c["Wb"])[None, :])
    assert (np.abs(Z.double().numpy() - fw["z"]) <= tol).all()
    assert np.array_equal(fw["z"][1], c["Wb"])  # an empty row gives Wb
    assert np.array_equal(fw["z"][0], fw["z"][3])


def test_chunk_rule_and_colsum():
    assert [R.chunk_rule(m) for m in (1, 31, 32, 33, 96, 2100, 8200)] == [
        (32, 1), (32, 1), (32, 1), (32, 2), (32, 3), (32, 66), (64, 129)]
    assert R.chunk_rule(8192) == (32, 256) and R.chunk_rule(8193)[0] == 64
    G = np.arange(70 * 2, dtype=np.float64).reshape(70, 2)
    p = R.ref_colsum(G, 66, 32)
    assert p.shape == (3, 2)
    assert np.array_equal(p[2], G[64:66].sum(axis=0))
    assert np.array_equal(p.sum(axis=0), G[:66].sum(axis=0))


def test_l1_touch_by_hand():
    # columns: positive clipped part-way, positive taken exactly to 0,
    # positive overshooting (clamped), negative, exact zero
    w = np.array([[1.0, 0.5, 0.25, -1.0, 0.0]])
    U = np.array([0.5, 0.25, 0.5, 0.5, 0.5])
    q = np.array([[-0.25, 0.25, 0.0, 0.25, 0.125]])
    t = R.ref_l1_touch(w, None, U, q, None, None)
    assert t["w"].tolist() == [[0.75, 0.0, 0.0, -0.75, 0.0]]
    assert t["q"].tolist() == [[-0.5, -0.25, -0.25, 0.5, 0.125]]
    # adaptive: credit (U - ul) rsqrt(h); none while h == 0
    h = np.array([[4.0, 0.0, 4.0, 4.0, 4.0]])
    z = np.zeros_like(w)
    ta = R.ref_l1_touch(w, h, U, z, z + 0.125, z + 0.25)
    assert np.allclose(ta["uw"], [[0.25, 0.125, 0.25, 0.25, 0.25]],
                       rtol=1e-12)
    assert np.array_equal(ta["ul"], U[None, :])
    assert np.allclose(ta["w"], [[0.75, 0.375, 0.0, -0.75, 0.0]], rtol=1e-12)


def test_batch_csc_matches_dataset_shuffle():
    import scipy.sparse as sp

    rng = np.random.default_rng(0)
    n, f, bs = 150, 37, 64
    Xd = rng.standard_normal((n, f)).astype(np.float32)
    Xd[np.abs(Xd) < 1.2] = 0
    Xd[5] = 0                                   # an empty row
    y = rng.integers(0, 2, size=n)
    ds = SparseDeviceDataset(sp.csr_matrix(Xd), y, device="cpu")
    assert ds.set_cv_partition([])
    sh = ds.shuffled(3, bs)
    crow, cidx, cval = (sh[k].numpy() for k in ("crow", "cidx", "cval"))
    ufeat, cptr, ridx, bval, ub_ptr = R.batch_csc(crow, cidx, cval, n, bs)
    assert np.array_equal(ufeat, sh["ufeat"].numpy())
    assert np.array_equal(cptr, sh["cptr"].numpy())
    assert np.array_equal(ridx, sh["ridx"].numpy())
    assert np.array_equal(bval, sh["bval"].numpy().astype(np.float64))
    assert np.array_equal(ub_ptr, sh["ub_ptr"].numpy())
    assert len(ub_ptr) == 4 and ub_ptr[-1] == len(ufeat) > f


def test_case_generator_reaches_the_unroll_tails():
    c = R.step_case("c192-m33-l1-mid")
    nnz = set(np.diff(c["crow"]).tolist())
    assert set(R.NNZ_CYCLE) <= nnz
    assert set(R.SLOT_ROWS) <= set(np.diff(c["cptr"]).tolist())
    c = R.step_case("c192-m96-mid")              # every_row
    assert np.diff(c["cptr"])[0] == 96 and c["ufeat"][0] == 0
    c = R.step_case("c256-uf2400-l1-mid")
    assert len(c["ufeat"]) > 2048
    c = R.step_case("c64-empty-l1-mid")
    assert len(c["ufeat"]) == 0 and c["crow"][-1] == 0
    mid = [k for k, v in R.STEP_CASES.items() if v.get("midfit")]
    assert 2 * len(mid) >= len(R.STEP_CASES)


@pytest.mark.parametrize(
    "name", [k for k, v in R.STEP_CASES.items()
             if v["loss_id"] != R.LOSS_LOG])
def test_exact_cases_are_exact_in_fp32(name):
    """The GPU test compares the dyadic cases bit for bit; this pins, from
    the inputs alone, that no fp32 operation of such a step can round."""
    c = R.step_case(name)
    start, m, ufeat, cptr = R.batch_slices(c, 0)
    st, tc = R.catchup(c, R.state_of(c), ufeat)
    if tc is not None:
        for k in ("t", "pre", "w", "q"):
            assert R.is_f32(tc[k]), ("catch-up", k)
    fw = R.ref_fwd(c["crow"], c["cidx"], c["cval"], st["W"], st["Wb"],
                   st["s"], c["y"], c["fold"], c["row_w"], c["col_class"],
                   c["col_fold"], c["col_class2"], np.arange(m),
                   c["loss_id"])
    G = R.bf16_rne(fw["g"])
    part = R.ref_colsum(G, m, R.chunk_rule(m)[0])
    b = R.ref_bias_scale(part, st["Wb"], st["s"], None, c["col_lr"],
                         c["col_l2"], c["inv_m"][0], c["lr_scale"],
                         c["col_l1"], st["U"])
    u = R.ref_update(ufeat, cptr, c["ridx"], c["bval"], G, st["W"], None,
                     b["s"], c["col_lr"], c["inv_m"][0], c["lr_scale"],
                     b["U"], st["q"], None, None)
    R.assert_exact_step(c, st, fw, G, part, b, u)
    # the masks are live, and the step is not a no-op
    nc = c["ncols"]
    assert fw["train"][:, :nc].any() and (~fw["train"][:, :nc]).any()
    if len(ufeat) and m > 1:
        assert (u["W"] != c["W"]).any()


@pytest.mark.parametrize(
    "name", [k for k, v in R.STEP_CASES.items()
             if v["loss_id"] == R.LOSS_LOG])
def test_log_loss_cases_keep_g_off_bf16_boundaries(name):
    """The GPU test lets a G element differ from bf16_rne(reference) only
    where the reference lies within delta of a rounding boundary; this
    pins that such elements are at most 1% of each case's G, from the
    inputs alone."""
    c = R.step_case(name)
    start, m, ufeat, cptr = R.batch_slices(c, 0)
    st, _ = R.catchup(c, R.state_of(c), ufeat)
    rows = np.arange(m)
    fw = R.ref_fwd(c["crow"], c["cidx"], c["cval"], st["W"], st["Wb"],
                   st["s"], c["y"], c["fold"], c["row_w"], c["col_class"],
                   c["col_fold"], c["col_class2"], rows, c["loss_id"])
    lo, hi, near, delta = R.g_interval(c, fw, rows)
    print(f"{name}: near a bf16 boundary: {near.mean():.4%} of G")
    assert near.mean() <= 0.01, near.mean()
