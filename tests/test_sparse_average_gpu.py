"""
Averaged SGD on the sparse-native kernels (k_sp_bias_scale_avg,
k_sp_update_avg, k_sp_avg_finish) against the plain average: the mean of
s_t * W_t and of Wb_t over the averaged steps, no u, no A, no laziness.

Dyadic cases (hinge loss, adaptive off, N a power of two): two
``sp_sgd_epoch_avg`` calls and the finish, bit for bit against float64
``_sparse_ref.composed_step`` steps, after asserting that nothing rounds.
Log-loss cases (Adagrad): one batch per call, so every iterate is read
back and the plain average is taken over the DEVICE's iterates; only the
averaging arithmetic is under test, within the bound derived in
test_sparse_average.py (``PlainAverage``; an fma for u += Aprev d rounds
once where the bound allows twice).
"""

import numpy as np
import pytest
import torch

import _sparse_ref as R
import test_sparse_average as C
import test_sparse_sgd_kernels_gpu as K

pytestmark = pytest.mark.gpu
_AVG = ("u", "A", "Aprev", "Wbsum")

# name -> (make_case arguments, first averaged batch of each epoch).  c64:
# rows no multiple of rpb = 4; c192: three 64-wide tiles, mid-epoch start;
# c320: second blockIdx.y block, a whole epoch with avg_on = 0; uf2400:
# 2400 slots at one per block, K3's grid-stride second pass carries u.
# f = 50 cases hold a feature in one row (the lazy gap) and one in all.
_B = dict(f=50, every_row=True, loss_id=1)
_L = dict(_B, loss_id=0, dyadic=False, adaptive=True)
CASES = {
    "c64": (dict(n=41, ncols=24, batch_size=11, **_B), (0, 0)),
    "c192": (dict(n=96, ncols=150, batch_size=32, row_w=True, **_B), (2, 0)),
    "c320": (dict(n=130, ncols=290, batch_size=40, ovo=True, **_B), (4, 0)),
    "uf2400": (dict(n=900, f=2400, ncols=200, loss_id=1, batch_size=300,
                    nnz_cycle=(8,), layout="blocks"), (2, 0)),
    "log-c64": (dict(n=41, ncols=24, batch_size=11, row_w=True, **_L), (1, 0)),
    "log-c320": (dict(n=130, ncols=290, batch_size=40, **_L), (2, 0)),
}


def _setup(name):
    kw, first = CASES[name]
    c = R.make_case(sum(map(ord, name)), **kw)
    per = np.bincount(c["cidx"], minlength=c["f"])
    assert c["f"] != 50 or (per[0] == c["n"] and (per == 1).any())
    d = K._upload(c)
    for k in _AVG:
        shape = (c["f"], c["cp"]) if k == "u" else (c["cp"],)
        d[k], d["can"][k] = K._guarded(np.zeros(shape), torch.float32,
                                       2 if k == "u" else 64)
    return c, d, first, len(c["inv_m"])


def _epoch(d, c, first_avg, bi=None, **swap):
    """One ``sp_sgd_epoch_avg`` call: the whole epoch, or batch ``bi``
    alone (row pointers, labels, folds and row weights from its first row
    on, its own CSC slice and 1/m).  ``swap`` replaces averaging tensors."""
    t = dict(d, **swap)
    if bi is not None:
        r0, m, _, _ = R.batch_slices(c, bi)
        t.update(crow=d["crow"][r0: r0 + m + 1], y=d["y"][r0:],
                 fold=d["fold"][r0:], row_w=d["row_w"][r0:],
                 ub_ptr=d["ub_ptr"][bi: bi + 2], inv_m=d["inv_m"][bi: bi + 1])
    names = ("crow cidx cval W Wb s h hb G part y fold row_w col_class "
             "col_fold col_class2 col_lr col_l2 ufeat cptr ridx bval ub_ptr "
             "inv_m").split()
    K._ext().sp_sgd_epoch_avg(*(t[k] for k in names), c["batch_size"],
                              c["loss_id"], c["lr_scale"],
                              *(t[k] for k in _AVG), first_avg)
    torch.cuda.synchronize()
    K._canaries(d)


def _finish(d, n_avg):
    K._ext().sp_avg_finish(d["W"], d["u"], d["A"], 1.0 / n_avg)
    torch.cuda.synchronize()
    K._canaries(d)
    return K._np(d["u"])


@pytest.mark.parametrize("name", [k for k in CASES if k[:3] != "log"])
def test_averaged_fit_bits(name):
    c, d, first, nb = _setup(name)
    n, vmax, cp = c["n"], np.abs(c["cval"]).max(), c["cp"]
    st = R.state_of(c)
    acc, u = np.zeros_like(st["W"]), np.zeros_like(st["W"])
    accb, A, n_avg = np.zeros(cp), np.zeros(cp), 0
    for epoch in range(2):
        for bi in range(nb):
            old, (st, G) = st, R.composed_step(c, st, bi)
            # no sum leaves the 2^24 grid whatever its order: at most n
            # terms of at most max |a| max |b| on the grid of a times b
            for a, b in ((c["cval"], old["W"]), (c["cval"], G),
                         (np.ones(1), G)):
                assert not b.any() or n * vmax * np.abs(b).max() / (
                    R.grid_of(a) * R.grid_of(b)) < 2.0 ** 24
            if bi >= first[epoch]:
                u += A[None, :] * (old["W"] - st["W"])
                A, n_avg = A + st["s"], n_avg + 1
                acc += st["s"][None, :] * st["W"]
                accb += st["Wb"]
            for x in (st["W"], st["Wb"], st["s"], old["W"] - st["W"], u, A,
                      acc, accb, A[None, :] * st["W"]):
                assert R.is_f32(x)
                assert np.abs(x).max() / R.grid_of(x) < 2.0 ** 24
    want = acc / n_avg
    assert n_avg & (n_avg - 1) == 0 and R.is_f32(want)
    assert np.abs(want - st["s"][None, :] * st["W"]).max() > 1e-3
    for epoch in range(2):
        _epoch(d, c, first[epoch])
    for k, w in (("W", st["W"]), ("A", A), ("Wbsum", accb), ("u", u)):
        K._no_bad(k, K._np(d[k]), w)
    K._no_bad("average", _finish(d, n_avg), want)
    K._no_bad("W after the finish", K._np(d["W"]), st["W"])


@pytest.mark.parametrize("name", [k for k in CASES if k[:3] == "log"])
def test_averaged_fit_against_the_plain_average(name):
    c, d, first, nb = _setup(name)
    f, nc = c["f"], c["ncols"]
    read = lambda: {k: K._np(d[k]) for k in ("W", "Wb", "s") + _AVG}
    old, pa = read(), C.PlainAverage(np.zeros((f, c["cp"])))
    for epoch in range(2):
        for bi in range(nb):
            on = bi >= first[epoch]
            _epoch(d, c, 0 if on else 1, bi)
            new = read()
            rest = np.setdiff1d(np.arange(f), R.batch_slices(c, bi)[2])
            assert (new["W"] != old["W"]).any()
            for k in ("W", "u"):    # rows of no batch feature: no work
                K._no_bad(k + " untouched", new[k][rest], old[k][rest])
            if not on:
                for k in _AVG:
                    K._no_bad(k + " before the start", new[k], old[k])
            else:
                K._no_bad("Aprev", new["Aprev"], old["A"])
                for k, v in (("A", "s"), ("Wbsum", "Wb")):
                    K._no_bad(k, new[k], old[k] + new[v],
                              K.EPS * np.abs(new[k]))
            pa.step(new["W"], new["Wb"], new["s"], on)
            old = new
    want, tol = pa.finish()
    got = _finish(d, pa.k)
    K._no_bad("average", got, want, tol)
    print(f"{name}: largest tolerance / largest average = "
          f"{tol.max() / np.abs(want).max():.2e}")
    assert tol.max() < 1e-4 * np.abs(want).max()
    assert np.abs(want - old["s"][None, :] * old["W"])[:, :nc].max() > 1e-3
    assert (got[:, nc:] == 0).all()


def test_binding_rejects_bad_averaging_state():
    c, d, _, _ = _setup("c64")
    for k in ("u", "A", "Wbsum"):
        for t in (d[k][:-1], d[k].double(), d[k].cpu()):
            with pytest.raises(RuntimeError):
                _epoch(d, c, 0, **{k: t})
            if k != "Wbsum":
                a = dict(d, **{k: t})
                with pytest.raises(RuntimeError):
                    K._ext().sp_avg_finish(d["W"], a["u"], a["A"], 0.5)
    torch.cuda.synchronize()
    assert not K._np(d["W"]).any() and not K._np(d["u"]).any()
