"""
``average=`` on the sparse-native solver, CPU side: the eager mirror's lazy
average against the plain one (the mean of s_t * W_t and Wb_t over the
averaged steps: no u, no A, no laziness), and the public interface.

``PlainAverage`` takes the iterates and carries the fp32 bound of the lazy
arithmetic (eps = 2^-24 per operation, d_t = W_{t-1} - W_t, k averaged
steps so far, path = sum |Aprev d| >= |u|):
  A += s' rounds once per step: k eps A, into Aprev d_t and the last A W
  d is booked before W - d rounds: |Aprev| eps |W_t|
  u += Aprev d: eps (|Aprev d_t| + path)
  finish: (k eps |A W| + eps (2 |A W| + path)) / N + 2 eps |result|
Adagrad off: dyadic hinge fits in one call against float64
``composed_step`` iterates (no operation of the trajectory rounds).
Adagrad on: log loss, one batch per call, against the mirror's own
iterates read after every step.
"""

import pickle
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _sparse_ref as R
from skdist_amd.models import LogisticRegression
from skdist_amd.models import _sparse_sgd as S

EPS = R.EPS32


class PlainAverage:
    def __init__(self, W):
        self.prev = np.array(W)
        self.acc, self.tol, self.path = (np.zeros_like(W) for _ in range(3))
        self.accb, self.A, self.k = 0.0, 0.0, 0

    def step(self, W, Wb, s, on):
        if on:
            ad = self.A * np.abs(self.prev - W)
            self.path += ad
            self.tol += EPS * (self.k * ad + ad + self.path
                               + self.A * np.abs(W))
            self.k += 1
            self.A = self.A + s[None, :]
            self.acc += s[None, :] * W
            self.accb = self.accb + Wb
        self.prev = np.array(W)

    def renorm(self, s):          # W *= s, s = 1 keeps A W with A /= s
        self.prev, self.A = self.prev * s[None, :], self.A / s[None, :]

    def finish(self):
        aw, want = self.A * np.abs(self.prev), self.acc / self.k
        tol = (self.tol + EPS * ((self.k + 2) * aw + self.path)) / self.k
        return want, (tol + 2 * EPS * np.abs(want)) * (1 + 2.0 ** -10)


def _mirror(c, epochs, first, state=None, bi=None):
    """_sparse_sgd_eager on a ``make_case`` case: the whole fit, or one
    step on batch ``bi`` alone from a carried state (no finish)."""
    t = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    f, cp, nb = c["f"], c["cp"], len(c["inv_m"])
    r0, n = (0, c["n"]) if bi is None else R.batch_slices(c, bi)[:2]
    ds = types.SimpleNamespace(device=torch.device("cpu"), n=n, f=f)
    sh = dict(crow=t(c["crow"][r0: r0 + n + 1], torch.int64),
              cidx=t(c["cidx"], torch.int32), cval=t(c["cval"]),
              y=t(c["y"][r0:]), fold=t(c["fold"][r0:], torch.int32),
              rw=None, inv_m=t(c["inv_m"][bi or 0:]))
    col = {k: t(c["col_" + v], torch.int32) for k, v in
           (("cls", "class"), ("fold", "fold"), ("cls2", "class2"))}
    col.update(lr=t(c["col_lr"]), l2=t(c["col_l2"]))
    if state is None:
        H, Hb = (z(f, cp), z(cp)) if c["adaptive"] else (z(0), z(0))
        avg = dict(u=z(f + 1, cp), A=z(cp), Aprev=z(cp), Wbsum=z(cp))
        state = (z(f + 1, cp), z(cp), torch.ones(cp), H, Hb, avg)
    W, Wb, s, H, Hb, avg = state
    avg.update(first=first, n_avg=0 if bi is not None else
               sum(nb - fb for fb in first))
    S._sparse_sgd_eager(ds, sh, W, Wb, s, H, Hb, col, c["loss_id"], epochs,
                        c["batch_size"], 0.0, cp,
                        avg=avg if first else None)
    return state


def _np(x):
    return x.double().numpy()


# name -> (rows, batch size, epochs, average=, averaged steps).  renorm: a
# halving column reaches 2^-10 < 1e-3 after the 10 steps of two epochs
CASES = {"from-0": (41, 11, 2, True, 8), "mid-epoch": (41, 11, 2, 60, 3),
         "never-starts": (41, 11, 2, 83, 0), "renorm": (50, 10, 3, 25, 13)}


@pytest.mark.parametrize("name", list(CASES))
def test_mirror_against_plain_average(name):
    n, bs, epochs, average, n_avg = CASES[name]
    c = R.make_case(sum(map(ord, name)), n, 40, 24, R.LOSS_HINGE,
                    batch_size=bs, every_row=True, lr_scale=1.0)
    per = np.bincount(c["cidx"], minlength=c["f"])
    assert per[0] == n and (per == 1).any()    # every row / a single row
    first = [S._first_avg_batch(S._average_start(average), e, n, bs)
             for e in range(epochs)]
    st, renorms = R.state_of(c), 0
    pa = PlainAverage(st["W"])
    for epoch in range(epochs):
        for bi in range(len(c["inv_m"])):
            st, _ = R.composed_step(c, st, bi)
            assert all(R.is_f32(st[x]) for x in ("W", "Wb", "s"))
            pa.step(st["W"], st["Wb"], st["s"], bi >= first[epoch])
        if st["s"].min() < 1e-3:      # the driver's renorm, exact here
            pa.renorm(st["s"])
            st["W"], st["s"] = st["W"] * st["s"][None, :], 1 + 0 * st["s"]
            renorms += 1
    assert renorms == (name == "renorm") and pa.k == n_avg
    W, Wb, s, _, _, avg = _mirror(c, epochs, first)
    if n_avg == 0:        # the count is never reached: the last iterate
        assert not avg["u"].any() and not avg["A"].any()
        assert np.array_equal(_np(W[:-1] * s), st["s"][None, :] * st["W"])
        assert np.array_equal(_np(Wb), st["Wb"])
        return
    want, tol = pa.finish()
    assert np.abs(want - st["s"][None, :] * st["W"]).max() > 1e-3
    assert (np.abs(_np(avg["u"][:-1]) - want) <= tol).all()
    # Wbsum: N adds of exact terms
    assert (np.abs(_np(avg["Wbsum"]) - pa.accb) <= n_avg * EPS
            * np.abs(pa.accb)).all()


@pytest.mark.parametrize("first", [(0, 0), (2, 0)], ids=["from-0", "mid"])
def test_mirror_adagrad_against_its_own_iterates(first):
    c = R.make_case(77, 41, 40, 24, R.LOSS_LOG, dyadic=False, adaptive=True,
                    batch_size=11, every_row=True, lr_scale=1.0)
    nb, state = len(c["inv_m"]), None
    pa = PlainAverage(np.zeros((c["f"], c["cp"])))
    for epoch in range(2):
        for bi in range(nb):
            on = bi >= first[epoch]
            state = _mirror(c, 1, [0 if on else 1], state, bi)
            W, Wb, s, H, _, avg = state
            assert H.any() and (on or not avg["u"].any())
            pa.step(_np(W[:-1]), _np(Wb), _np(s), on)
    _mirror(c, 0, first, state)                  # the finish alone
    want, tol = pa.finish()
    assert pa.k == sum(nb - fb for fb in first)
    assert (np.abs(_np(avg["u"][:-1]) - want) <= tol).all()
    assert tol.max() < 1e-4 * np.abs(want).max()
    assert np.abs(want - _np(s)[None, :] * _np(W[:-1])).max() > 1e-3


@pytest.fixture(scope="module")
def text():
    X = sp.random(300, 500, density=0.03, random_state=3, format="csr",
                  dtype=np.float32)
    w = np.random.default_rng(3).standard_normal(500)
    return X, (X @ w > 0).astype(np.int64)


def _lr(**kw):
    return LogisticRegression(epochs=4, batch_size=64, random_state=0, **kw)


def test_estimator(text, monkeypatch):
    from skdist_amd.models._sgd import ColumnSpec

    monkeypatch.setenv("SKDIST_AMD_FORCE_SPARSE", "1")
    X, y = text
    est, last = _lr(average=True).fit(X, y), _lr().fit(X, y)
    ds = S.SparseDeviceDataset(X, y, device="cpu", task="cls")
    ds.set_cv_partition([])
    one = lambda v, dt=np.float32: np.full(1, v, dt)
    spec = ColumnSpec(ds.device, col_fold=one(-2, np.int32),
                      col_class=one(1, np.int32), col_lr=one(est.lr),
                      col_l2=one(est._lam(ds.n)[0]))
    W = S.sparse_sgd_fit(ds, spec, "log", 4, 64, seed=0, average=True)
    assert np.array_equal(est.coef_[0], W[:-1, 0].numpy())
    assert est.intercept_[0] == W[-1, 0].item()
    assert np.abs(est.coef_ - last.coef_).max() > 1e-3
    for off in (False, np.False_, 10 ** 9):    # off, or never reached
        assert np.array_equal(last.coef_, _lr(average=off).fit(X, y).coef_)
    again = pickle.loads(pickle.dumps(est))
    assert again.get_params()["average"] is True
    assert np.array_equal(again.predict(X), est.predict(X))
    del again.__dict__["average"]       # pickled before the parameter
    assert np.array_equal(again.fit(X, y).coef_, last.coef_)
    for dense in (False, True):
        Xd = X.toarray() if dense else X
        if dense:
            monkeypatch.delenv("SKDIST_AMD_FORCE_SPARSE")
        for bad in (0, -3, 1.5, "yes", None):
            with pytest.raises(ValueError, match="average must be"):
                _lr(average=bad).fit(Xd, y)
    with pytest.raises(ValueError, match="sparse-native solver only"):
        _lr(average=True).fit(Xd, y)
    monkeypatch.setenv("SKDIST_AMD_FORCE_SPARSE", "1")
    with pytest.raises(ValueError, match="L1"):
        _lr(average=True, penalty="l1").fit(X, y)
