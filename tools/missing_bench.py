"""Cost of the missing-value mode of the boosted family on the device.

Seeded binary problem, 1,000,000 rows x 64 features by default, 10% of the
cells NaN (the label also depends on whether feature 0 is missing), 50
rounds, max_depth=3.  Two fits, host numpy in, fitted model out:

  nan      ``allow_nan=True`` on the data with its NaN cells
  imputed  the default estimator on the same data, median-imputed (what a
           user had to do before; also runs on a checkout without the
           parameter: compare two commits by alternating processes with
           ``--root``)

One process, one warm-up fit, then ``--repeats`` rounds of the chosen fits
alternating; the device is synchronised before each clock read.

``--split-kernel`` times the split scan alone instead: ``tree_split`` on a
random [8, features, 256, 3] histogram (the frontier of a depth-3 level),
plain and in missing mode, with device events around 200 launches each.
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))),
    help="checkout whose skdist_amd package is measured")
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--features", type=int, default=64)
ap.add_argument("--rounds", type=int, default=50)
ap.add_argument("--max-depth", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--nan-frac", type=float, default=0.10)
ap.add_argument("--mode", default="both", choices=["both", "nan", "imputed"])
ap.add_argument("--split-kernel", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np
import torch

import skdist_amd
from skdist_amd.models import HistGradientBoostingClassifier


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def data():
    rng = np.random.default_rng(0)
    n, f = args.rows, args.features
    X = rng.standard_normal((n, f)).astype(np.float32)
    t = np.sin(X[:, 0]) + 0.5 * X[:, 1] ** 2 + X[:, 2]
    gone = rng.random((n, f)) < args.nan_frac
    y = np.where(gone[:, 0], 1, t > np.median(t)).astype(np.int64)
    X[gone] = np.nan
    return X, y


def fits():
    X, y = data()
    Xi = np.where(np.isnan(X), np.nanmedian(X, axis=0)[None, :], X).astype(
        np.float32)
    print(f"X {X.shape}  NaN cells {np.isnan(X).mean():.3f}  rounds "
          f"{args.rounds}  max_depth {args.max_depth}", flush=True)

    def fit(kind):
        kw = {"allow_nan": True} if kind == "nan" else {}
        m = HistGradientBoostingClassifier(
            n_estimators=args.rounds, max_depth=args.max_depth,
            random_state=0, **kw)
        data_ = X if kind == "nan" else Xi
        _sync()
        t0 = time.perf_counter()
        m.fit(data_, y)
        _sync()
        return time.perf_counter() - t0, m

    kinds = {"both": ["imputed", "nan"], "nan": ["nan"],
             "imputed": ["imputed"]}[args.mode]
    fit(kinds[-1])                      # warm-up
    times = {k: [] for k in kinds}
    models = {}
    for _ in range(args.repeats):
        for k in kinds:
            t, models[k] = fit(k)
            times[k].append(t)
    for k in kinds:
        ts = times[k]
        Xe = X if k == "nan" else Xi
        acc = (models[k].predict(Xe[:50_000]) == y[:50_000]).mean()
        print(f"{k:<8} median {np.median(ts):7.3f}s  "
              f"spread {max(ts) - min(ts):6.3f}s  "
              f"runs {[round(t, 3) for t in ts]}  train acc {acc:.4f}",
              flush=True)
    if len(kinds) == 2:
        print(f"nan / imputed = "
              f"{np.median(times['nan']) / np.median(times['imputed']):.3f}")


def split_kernel():
    from skdist_amd.ops import require_hip

    ext = require_hip()
    dev = "cuda"
    NF, f, nbins, S = 8, args.features, 256, 3
    g = torch.Generator(device="cpu").manual_seed(0)
    w = torch.randint(1, 40, (NF, f, nbins), generator=g).float()
    ybar = torch.randn(NF, f, nbins, generator=g)
    hist = torch.stack([w, w * ybar, w * (ybar ** 2 + 1)], dim=3).to(dev)
    seed = torch.zeros(NF, dtype=torch.int32, device=dev)
    oi = lambda: torch.zeros(NF, dtype=torch.int32, device=dev)
    of = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    out = (oi(), oi(), of(NF), of(NF), of(NF), of(NF, S), of(NF, S))
    base = (hist, seed, f, nbins, S, 0, 2, f, 0, 1.0, *out, -1)
    calls = {"plain": base, "missing": base + (1, oi())}
    for name, call in calls.items():
        for _ in range(20):
            ext.tree_split(*call)
        _sync()
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(200):
            ext.tree_split(*call)
        b.record()
        _sync()
        print(f"tree_split {name:<8} [{NF}, {f}, {nbins}, {S}]: "
              f"{a.elapsed_time(b) / 200 * 1e3:8.1f} us per launch",
              flush=True)


if __name__ == "__main__":
    dev = (torch.cuda.get_device_name(0) if torch.cuda.is_available()
           else "cpu")
    print(f"package: {os.path.dirname(skdist_amd.__file__)}")
    print(f"device: {dev}", flush=True)
    if args.split_kernel:
        split_kernel()
    else:
        fits()
