"""Wall time of a weighted against an unweighted binary boosted fit on
the device, host numpy in, fitted model out.

Seeded imbalanced binary problem (about 8% positives): 200,000 rows x 32
features, 20 rounds, max_depth=3; the weighted fit passes the balanced
class weights as ``sample_weight``.

One process, one warm-up fit, then ``--repeats`` rounds of
(unweighted, weighted) alternating; the device is synchronised before
each clock read.  ``--mode unweighted|weighted`` runs one kind only (for
a kernel trace, or for a checkout without weighted fits: compare the
unweighted time of two commits by alternating processes with ``--root``).
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))),
    help="checkout whose skdist_amd package is measured")
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--features", type=int, default=32)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--max-depth", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--mode", default="both",
                choices=["both", "unweighted", "weighted"])
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np
import torch
from sklearn.metrics import recall_score
from sklearn.utils.class_weight import compute_sample_weight

import skdist_amd
from skdist_amd.models import HistGradientBoostingClassifier


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def main():
    rng = np.random.default_rng(0)
    n, f = args.rows, args.features
    X = rng.standard_normal((n, f)).astype(np.float32)
    y = (2 * X[:, 0] - 2.8 + 0.5 * rng.standard_normal(n) > 0).astype(
        np.int64)
    sw = compute_sample_weight("balanced", y)
    dev = (torch.cuda.get_device_name(0) if torch.cuda.is_available()
           else "cpu")
    print(f"package: {os.path.dirname(skdist_amd.__file__)}")
    print(f"device: {dev}  X {X.shape}  positives {y.mean():.3f}  "
          f"rounds {args.rounds}  max_depth {args.max_depth}", flush=True)

    def fit(weighted):
        m = HistGradientBoostingClassifier(
            n_estimators=args.rounds, max_depth=args.max_depth,
            random_state=0)
        _sync()
        t0 = time.perf_counter()
        m.fit(X, y, sample_weight=sw if weighted else None)
        _sync()
        return time.perf_counter() - t0, m

    kinds = {"both": [False, True], "unweighted": [False],
             "weighted": [True]}[args.mode]
    fit(kinds[-1])                      # warm-up
    times = {k: [] for k in kinds}
    models = {}
    for _ in range(args.repeats):
        for k in kinds:
            t, models[k] = fit(k)
            times[k].append(t)
    for k in kinds:
        ts = times[k]
        rec = recall_score(y[:20000], models[k].predict(X[:20000]))
        print(f"{'weighted' if k else 'unweighted':<10} "
              f"median {np.median(ts):7.3f}s  "
              f"spread {max(ts) - min(ts):6.3f}s  "
              f"runs {[round(t, 3) for t in ts]}  recall {rec:.3f}",
              flush=True)
    if len(kinds) == 2:
        print(f"weighted / unweighted = "
              f"{np.median(times[True]) / np.median(times[False]):.3f}")


if __name__ == "__main__":
    main()
