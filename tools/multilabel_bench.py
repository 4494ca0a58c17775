"""
Multilabel one-vs-rest on the batched solver, measured two ways on the
device, at one shape:

    python tools/multilabel_bench.py [--rows 200000] [--features 256]
        [--labels 512] [--per-row 3] [--generic-labels N] [--out FILE]

1. Whole fit: wall time of ``DistOneVsRestClassifier(LogisticRegression,
   sc=Cluster()).fit(X, Y)`` on the batched route (every label a column of
   one solve, targets as bit planes) against the generic route on the same
   data (one task, one dataset upload and one one-column solve per label).
   The generic route is forced by making the estimator's batched hook
   decline; the code that then runs is the generic path unchanged.
   ``--generic-labels N`` fits only the first N labels there (the route is
   linear in the label count) and the line says so.

2. K1 alone: one solve with per-element targets (k_fwd_gt_bits) against one
   with class targets (k_fwd_gt's general path) at the same rows, features
   and column count -- the one-hot plane of a class vector, so both train
   the same models.  Device events around whole solves give microseconds
   per step; under ``rocprofv3 --kernel-trace --stats`` (``--kernels-only``
   skips part 1) the kernel table gives the per-launch times of the two K1
   kernels; K2 and K3 are shared.  ``--only VARIANT`` runs one of
   class_targets / bit_planes / bit_planes_masked, so that a traced process
   holds one K1 variant.

Prints one JSON line per part and appends it to ``--out`` (default
profiles/r13_multilabel.txt, whose last section holds these raw lines under
the hand-written summary; ``--out ""`` only prints).
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _data(rows, features, labels, per_row, seed=0):
    """Tag-like data: label j fires on a row with probability that depends
    on a random linear score, about ``per_row`` labels per row."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, features)).astype(np.float32)
    Wt = rng.standard_normal((features, labels)).astype(np.float32)
    S = X @ Wt
    S += 0.5 * np.sqrt(features) * rng.standard_normal(
        (rows, labels)).astype(np.float32)
    # per-label threshold at the (1 - per_row / labels) quantile
    q = np.quantile(S[: min(rows, 20000)], 1.0 - per_row / labels, axis=0)
    return X, (S > q[None, :]).astype(np.uint8)


def whole_fit(a, X, Y, emit):
    from skdist_amd import Cluster
    from skdist_amd.distribute.multiclass import DistOneVsRestClassifier
    from skdist_amd.models import LogisticRegression
    from skdist_amd.models.linear import FallbackToGeneric

    def make():
        return LogisticRegression(epochs=a.epochs, random_state=0)

    sc = Cluster()
    DistOneVsRestClassifier(make(), sc=sc).fit(X[:4096], Y[:4096, :8])
    torch.cuda.synchronize()
    batched = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        clf = DistOneVsRestClassifier(make(), sc=sc).fit(X, Y)
        torch.cuda.synchronize()
        batched.append(time.perf_counter() - t0)
    acc = float((clf.predict(X[:20000]) == Y[:20000]).mean())

    class Declining(LogisticRegression):
        def batched_multiclass_fit(self, *args, **kw):
            raise FallbackToGeneric("measuring the generic route")

    g = a.generic_labels or Y.shape[1]
    t0 = time.perf_counter()
    gen = DistOneVsRestClassifier(
        Declining(epochs=a.epochs, random_state=0), sc=sc).fit(X, Y[:, :g])
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    agree = float((gen.predict(X[:20000]) == clf.predict(X[:20000])[:, :g])
                  .mean())
    emit({
        "part": "whole_fit", "rows": a.rows, "features": a.features,
        "labels": a.labels, "labels_per_row": round(float(Y.sum(1).mean()), 2),
        "epochs": a.epochs,
        "batched_fit_s": round(float(np.median(batched)), 3),
        "batched_fit_s_min_max": [round(min(batched), 3),
                                  round(max(batched), 3)],
        "generic_labels_fitted": g,
        "generic_fit_s": round(t_gen, 3),
        "generic_s_per_label": round(t_gen / g, 4),
        "generic_fit_s_scaled_to_all_labels": round(
            t_gen / g * Y.shape[1], 2),
        "train_indicator_accuracy": round(acc, 4),
        "generic_vs_batched_indicator_agreement": round(agree, 4),
    })


def k1_steps(a, X, emit):
    from skdist_amd.models._sgd import LOSS_LOG, ColumnSpec, DeviceDataset
    from skdist_amd.ops import hip_sgd_solve

    rng = np.random.default_rng(1)
    L = a.labels
    y = rng.integers(0, L, size=a.rows)
    ds = DeviceDataset(X, y, device="cuda")
    ds.set_cv_partition([])
    onehot = torch.zeros(a.rows, L, dtype=torch.uint8, device=ds.device)
    onehot[torch.arange(a.rows, device=ds.device),
           torch.as_tensor(y, device=ds.device)] = 1
    mask = torch.as_tensor(rng.random((a.rows, L)) < 0.7, device=ds.device)

    def spec(**kw):
        return ColumnSpec(
            ds.device, np.full(L, -2, np.int32), np.arange(L, dtype=np.int32),
            np.full(L, 0.1, np.float32), np.full(L, 1e-4, np.float32), **kw)

    specs = {"class_targets": spec(), "bit_planes": spec(targets=onehot),
             "bit_planes_masked": spec(targets=onehot, train_mask=mask)}
    if a.only:      # one K1 variant per process: a kernel table of its own
        specs = {a.only: specs[a.only]}
    bs = 8192
    steps = a.k1_epochs * ((a.rows + bs - 1) // bs)

    def timed(sp):
        hip_sgd_solve(ds, sp, LOSS_LOG, 2, bs, 0, 0.9, 0.0)     # warm-up
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        # a solve with targets packs its planes before the first step, so
        # the pack (once per solve) is inside the events; the kernel trace
        # is the per-launch comparison
        t0.record()
        hip_sgd_solve(ds, sp, LOSS_LOG, a.k1_epochs, bs, 0, 0.9, 0.0)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / steps

    out = {k: [] for k in specs}
    for _ in range(a.repeats):          # alternate: drift hits all alike
        for k, sp in specs.items():
            out[k].append(timed(sp))
    # one plane's pack on its own (a solve with targets packs one plane, a
    # masked one two, before its first step)
    from skdist_amd.ops import pack_bit_plane

    perm = torch.randperm(a.rows, device=ds.device)
    n_pad, ncp = (a.rows + 127) // 128 * 128, (L + 127) // 128 * 128
    packs = []
    for _ in range(a.repeats + 1):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        pack_bit_plane(onehot, perm, n_pad, ncp)
        t1.record()
        torch.cuda.synchronize()
        packs.append(t0.elapsed_time(t1) * 1e3)
    pack_us = float(np.median(packs[1:]))
    res = {"part": "k1_steps", "rows": a.rows, "fa": int(ds.Xaug.shape[1]),
           "columns": L, "batch": bs, "steps_per_solve": steps}
    for k, v in out.items():
        res[k + "_step_us"] = round(float(np.median(v)), 2)
        res[k + "_step_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    res["pack_one_plane_us"] = round(pack_us, 1)
    res["pack_one_plane_us_per_step"] = round(pack_us / steps, 2)
    if not a.only:
        W0 = hip_sgd_solve(ds, specs["class_targets"], LOSS_LOG, 2, bs, 0,
                           0.9, 0.0)
        W1 = hip_sgd_solve(ds, specs["bit_planes"], LOSS_LOG, 2, bs, 0, 0.9,
                           0.0)
        res["bitwise_equal_W"] = bool(torch.equal(W0, W1))
        res["bit_planes_over_class_targets"] = round(
            res["bit_planes_step_us"] / res["class_targets_step_us"], 4)
    emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--labels", type=int, default=512)
    ap.add_argument("--per-row", type=float, default=3.0)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--k1-epochs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--generic-labels", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--only", default=None,
                    choices=["class_targets", "bit_planes",
                             "bit_planes_masked"],
                    help="time one K1 variant only (for a kernel trace "
                         "per variant); implies nothing about part 1")
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "r13_multilabel.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multilabel_bench: needs a GPU (no CPU timing)")

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    X, Y = _data(a.rows, a.features, a.labels, a.per_row)
    if not a.kernels_only:
        whole_fit(a, X, Y, emit)
    k1_steps(a, X, emit)


if __name__ == "__main__":
    main()
