"""Cost of the L1 / elastic-net update of the batched linear solvers on
the device, against the L2-only solve on the same columns.

Two seeded problems, each solved with ``col_l1`` unset (L2-only kernels)
and set (the ``*_l1`` kernels), the variants alternating for ``--repeats``
rounds after one warm-up solve each; the device is synchronised before
every clock read, and the times are whole solves (host driver included)
divided by the number of mini-batch steps.

  dense   the flagship shape: ``--rows`` x ``--features`` standardized
          bf16 X, ``--candidates`` x (folds + 1 refit) columns,
          momentum 0.9 (k_reduce_update vs k_reduce_update_l1)
  sparse  hashed-text-like CSR: ``--sp-rows`` x 2^20 features,
          ``--nnz`` stored entries per row, ``--sp-cols`` columns, with
          and without Adagrad scaling (the L1 fit adds the catch-up, the
          flush and one to three [f, columns] fp32 tables)

Also prints the peak device memory of each sparse solve, and the bytes of
the L1 tables computed from the shapes.
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--features", type=int, default=256)
ap.add_argument("--candidates", type=int, default=100)
ap.add_argument("--folds", type=int, default=5)
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--batch-size", type=int, default=8192)
ap.add_argument("--sp-rows", type=int, default=200_000)
ap.add_argument("--sp-features", type=int, default=2 ** 20)
ap.add_argument("--nnz", type=int, default=60)
ap.add_argument("--sp-cols", type=int, default=240)
ap.add_argument("--sp-batch-size", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", default="both", choices=["both", "dense", "sparse"])
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import scipy.sparse as sp
import torch

from skdist_amd.models._sgd import ColumnSpec, DeviceDataset, batched_sgd_fit
from skdist_amd.models._sparse_sgd import SparseDeviceDataset
from skdist_amd.ops import require_hip

require_hip()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def folds_of(ds, n, k):
    fold = np.arange(n) % k
    assert ds.set_cv_partition([
        (np.flatnonzero(fold != i), np.flatnonzero(fold == i))
        for i in range(k)])


def specs(ds, ncols, lam, rho):
    assert ncols % (args.folds + 1) == 0
    kw = dict(
        # per candidate: one column per fold, then the refit column
        col_fold=np.tile(np.r_[np.arange(args.folds), -2].astype(np.int32),
                         ncols // (args.folds + 1)),
        col_class=np.ones(ncols, dtype=np.int32),
        col_lr=np.full(ncols, 0.5, dtype=np.float32),
        col_l2=((1 - rho) * lam).astype(np.float32))
    return (ColumnSpec(ds.device, **kw),
            ColumnSpec(ds.device, col_l1=(rho * lam).astype(np.float32),
                       **kw))


def compare(name, ds, spec_l2, spec_l1, steps, **kw):
    runs = {"l2": [], "l1": []}
    out = {}
    for which, spec in (("l2", spec_l2), ("l1", spec_l1)):   # warm-up
        batched_sgd_fit(ds, spec, "log", **kw)
    for _ in range(args.repeats):
        for which, spec in (("l2", spec_l2), ("l1", spec_l1)):
            torch.cuda.reset_peak_memory_stats()
            t, W = timed(lambda: batched_sgd_fit(ds, spec, "log", **kw))
            runs[which].append(t)
            out[which] = (W, torch.cuda.max_memory_allocated())
    for which in ("l2", "l1"):
        ts = np.array(runs[which])
        W, peak = out[which]
        print(f"{name} {which}: solve {ts.min():.3f}-{ts.max():.3f} s "
              f"(median {np.median(ts):.3f}), {steps} steps, "
              f"{1e3 * np.median(ts) / steps:.3f} ms/step, "
              f"zero weights {float((W == 0).float().mean()):.3f}, "
              f"peak device memory {peak / 2 ** 30:.2f} GiB", flush=True)
    r = np.median(runs["l1"]) / np.median(runs["l2"])
    print(f"{name}: l1 / l2 step time = {r:.3f}", flush=True)


if args.only in ("both", "dense"):
    rng = np.random.default_rng(0)
    n, f = args.rows, args.features
    X = rng.standard_normal((n, f), dtype=np.float32)
    w = rng.standard_normal(f) * (rng.random(f) < 0.25)
    y = (X @ w + rng.standard_normal(n) > 0).astype(np.int64)
    ds = DeviceDataset(X, y, device="cuda")
    folds_of(ds, n, args.folds)
    ncols = args.candidates * (args.folds + 1)
    lam = np.repeat(1.0 / (np.logspace(-4, 0, args.candidates) * n),
                    args.folds + 1)
    s2, s1 = specs(ds, ncols, lam, 0.5)
    steps = args.epochs * -(-n // args.batch_size)
    print(f"dense: {n} x {f}, {ncols} columns, {args.epochs} epochs, "
          f"batch {args.batch_size}", flush=True)
    compare("dense", ds, s2, s1, steps, epochs=args.epochs,
            batch_size=args.batch_size, seed=0, momentum=0.9)
    del ds, X

if args.only in ("both", "sparse"):
    rng = np.random.default_rng(1)
    n, f, k = args.sp_rows, args.sp_features, args.nnz
    cols = rng.integers(0, f // 16, size=(n, k)) * 16 \
        + rng.integers(0, 16, size=(n, k))
    X = sp.csr_matrix(
        (np.full(n * k, 1 / np.sqrt(k), dtype=np.float32),
         cols.ravel(), np.arange(0, n * k + 1, k)), shape=(n, f))
    X.sum_duplicates()
    w = np.zeros(f)
    w[rng.integers(0, f, 4096)] = rng.standard_normal(4096)
    y = (np.asarray(X @ w).ravel() > 0).astype(np.int64)
    ds = SparseDeviceDataset(X, y, device="cuda")
    folds_of(ds, n, args.folds)
    ncols = args.sp_cols
    lam = np.repeat(
        1.0 / (np.logspace(-1, 1, ncols // (args.folds + 1)) * n),
        args.folds + 1)
    s2, s1 = specs(ds, ncols, lam, 0.5)
    cp = (ncols + 63) // 64 * 64
    steps = args.epochs * -(-n // args.sp_batch_size)
    print(f"sparse: {n} x {f}, {k} nnz/row, {ncols} columns (padded "
          f"{cp}), {args.epochs} epochs, batch {args.sp_batch_size}; one "
          f"[f, cp] fp32 table = {f * cp * 4 / 2 ** 30:.3f} GiB "
          "(L1 adds 1 with adaptive off, 3 with adaptive on)", flush=True)
    for adaptive in (True, False):
        compare(f"sparse adaptive={adaptive}", ds, s2, s1, steps,
                epochs=args.epochs, batch_size=args.sp_batch_size, seed=0,
                adaptive=adaptive)
