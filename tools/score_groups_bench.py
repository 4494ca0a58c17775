"""
``batched_scores_by_fold`` of one multiclass search: the fused route
(k_score_groups; k_score_counts for the F1 metrics) against the
``_MetricState`` torch route (forced by patching ``_sgd._use_hip``),
alternating in one process.  Prints one JSON line: per metric and route
[median, min, max] ms of a host timer around the call (it ends in
device-to-host copies), and the largest difference between the two routes'
scores (the torch route rounds z to bf16).

    python tools/score_groups_bench.py [--rows 200000] [--candidates 300]

The F1 figures of docs/BENCHMARKS.md, at the training set of
examples/search/covtype_scale.py and at 1M rows x 500 models:

    ... --metrics f1_weighted --features 54 --classes 7 \
        --rows 464809 --candidates 4        (and --rows 1000000
                                             --candidates 100)
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--candidates", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--metrics", default="accuracy,neg_log_loss")
    a = ap.parse_args()
    a.folds, a.warmup = 5, 2
    if not torch.cuda.is_available():
        sys.exit("score_groups_bench: needs a GPU (no CPU timing)")

    import skdist_amd.models._sgd as S

    rng = np.random.default_rng(0)
    n, f, K, nm = a.rows, a.features, a.classes, a.candidates * a.folds
    X = rng.standard_normal((n, f)).astype(np.float32)
    Wtrue = rng.standard_normal((f, K))
    y = (X @ Wtrue + rng.standard_normal((n, K))).argmax(axis=1)
    ds = S.DeviceDataset(X, y, device="cuda")
    idx = np.arange(n)
    assert ds.set_cv_partition([(np.setdiff1d(idx, idx[k::a.folds]),
                                 idx[k::a.folds]) for k in range(a.folds)])
    # weights of a plausible fit, noisy, at one scale per model
    W = np.zeros((ds.fa, nm * K), dtype=np.float32)
    W[:f] = (np.tile(Wtrue, (1, nm)) + 0.3 * rng.standard_normal(
        (f, nm * K))) * np.repeat(np.logspace(-2, 0, nm), K)
    W = torch.tensor(W, device="cuda")
    mfold = np.arange(nm) % a.folds
    col_class = np.tile(np.arange(K), nm).astype(np.int32)

    routes = {"fused": S._use_hip, "torch": lambda d: False}
    res = {"rows": n, "fa": int(ds.fa), "classes": K, "models": nm,
           "folds": a.folds}
    for metric in a.metrics.split(","):
        t = {r: [] for r in routes}
        score = {}
        for rep in range(a.warmup + a.repeats):
            for r, use in routes.items():   # alternate: drift hits both
                S._use_hip = use
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                score[r] = S.batched_scores_by_fold(
                    ds, W, mfold, col_class, K, metric)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    t[r].append((time.perf_counter() - t0) * 1e3)
        S._use_hip = routes["fused"]
        res[metric] = {
            r + "_ms": [round(float(np.median(v)), 3), round(min(v), 3),
                        round(max(v), 3)] for r, v in t.items()}
        res[metric]["max_abs_diff"] = float(
            np.abs(score["fused"] - score["torch"]).max())
        res[metric]["score_min_max"] = [float(score["fused"].min()),
                                        float(score["fused"].max())]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
