"""Tree serving and binning on scipy-sparse (CSR) input, host CSR in and
numpy out, warm.

Seeded synthetic count data: 200,000 rows, about 64 stored entries per
row (small integer counts), and a 100-tree depth-10 sklearn
RandomForestClassifier fitted on the first 20,000 rows.

  (a) serve    predict_proba of that forest on 200k x 4096 through the
               flattened device forest
  (b) wide     the same forest and rows spread over 2**20 columns
               (column j -> 256*j); skipped, and reported as such, on a
               checkout whose device forest densifies sparse input
  (c) bin      BinnedDataset build for the 200k x 4096 matrix: from CSR
               where the checkout supports it, else from ``toarray()``

One process times one checkout: one warm-up, then ``--repeats`` timed
runs per case.  To compare two commits on one box, alternate processes:

    python tools/sparse_trees_bench.py --repeats 1 --model-cache rf.pkl
    python tools/sparse_trees_bench.py --repeats 1 --model-cache rf.pkl \\
        --root ../parent

and take medians over the rounds (``--model-cache`` fits the forest once
and shares it between the processes).
"""
import argparse
import os
import pickle
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))),
    help="checkout whose skdist_amd package is measured")
ap.add_argument("--rows", type=int, default=200_000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--cases", default="serve,wide,bin")
ap.add_argument("--model-cache", default=None,
                help="pickle of the fitted forest (written if missing)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np
import scipy.sparse as sp
import torch
from sklearn.ensemble import RandomForestClassifier

import skdist_amd
from skdist_amd.models import forest as F

N_FEAT = 4096
NNZ_ROW = 64
SPREAD = 256            # 4096 * 256 = 2**20
FIT_ROWS = 20_000


def _data(n):
    rng = np.random.default_rng(20240611)
    cols = rng.integers(0, N_FEAT, size=(n, NNZ_ROW))
    cols[:, :16] = rng.integers(0, 128, size=(n, 16))   # frequent terms
    vals = rng.integers(1, 6, size=(n, NNZ_ROW)).astype(np.float32)
    rows = np.repeat(np.arange(n), NNZ_ROW)
    X = sp.csr_matrix((vals.ravel(), (rows, cols.ravel())),
                      shape=(n, N_FEAT))
    X.sum_duplicates()
    X.sort_indices()
    head = np.asarray(X[:, :128].sum(axis=1)).ravel()
    lo = np.asarray(X[:, :64].sum(axis=1)).ravel()
    y = (2 * lo > head).astype(np.int64)
    return X, y


def _forest(X, y):
    path = args.model_cache
    if path and os.path.exists(path):
        with open(path, "rb") as fh:
            return pickle.load(fh)
    rf = RandomForestClassifier(
        n_estimators=100, max_depth=10, random_state=0,
        n_jobs=min(16, os.cpu_count() or 1),
    ).fit(X[:FIT_ROWS], y[:FIT_ROWS])
    if path:
        with open(path, "wb") as fh:
            pickle.dump(rf, fh)
    return rf


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _time(fn, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(args.repeats):
        _sync()
        t0 = time.perf_counter()
        out = fn()
        _sync()
        ts.append(time.perf_counter() - t0)
    return ts, out


def _report(name, path, ts):
    print(f"{name:<6} {path:<22} median {np.median(ts):8.3f}s  "
          f"runs {[round(t, 3) for t in ts]}", flush=True)


def main():
    cases = args.cases.split(",")
    csr_native = hasattr(F, "_csr_row_chunks")
    print(f"package: {os.path.dirname(skdist_amd.__file__)}")
    print(f"device: {torch.cuda.get_device_name(0)}  rows: {args.rows}  "
          f"csr-native trees: {csr_native}", flush=True)
    X, y = _data(args.rows)
    print(f"X {X.shape} nnz/row {X.nnz / X.shape[0]:.1f}", flush=True)
    rf = _forest(X, y)
    nodes = sum(e.tree_.node_count for e in rf.estimators_)
    print(f"forest: {len(rf.estimators_)} trees, {nodes} nodes", flush=True)
    path = "csr kernel" if csr_native else "toarray + dense kernel"

    if "serve" in cases:
        flat = F.flat_forest_for(rf, "cuda")
        ts, out = _time(lambda: flat.predict_proba(X))
        _report("serve", path, ts)
        ref = rf.predict_proba(X[:2000])
        print(f"serve  max |device - sklearn| on 2000 rows = "
              f"{np.abs(out[:2000] - ref).max():.3g}", flush=True)
        del flat

    if "wide" in cases:
        if not csr_native:
            print("wide   skipped: this checkout densifies sparse input "
                  f"({args.rows} x 2**20 float32 = "
                  f"{args.rows * 2 ** 20 * 4 / 1e12:.1f} TB)", flush=True)
        else:
            trees = []
            for e in rf.estimators_:
                t = F._sklearn_tree_to_hist_tree(e, "proba")
                t.feature = np.where(
                    t.feature >= 0, t.feature * SPREAD, -1
                ).astype(np.int32)
                t.n_features_in_ = N_FEAT * SPREAD
                trees.append(t)
            flat = F.FlatForest(trees, "cuda")
            Xw = sp.csr_matrix(
                (X.data, X.indices.astype(np.int64) * SPREAD, X.indptr),
                shape=(X.shape[0], N_FEAT * SPREAD))
            ts, outw = _time(lambda: flat.predict_value(Xw))
            _report("wide", path, ts)
            if "serve" in cases:
                print(f"wide   equals the 4096-column result: "
                      f"{np.array_equal(outw, out)}", flush=True)
            del flat, Xw

    if "bin" in cases:
        if csr_native:
            fn = lambda: F.BinnedDataset(X, y, "cuda", is_cls=True)
            how = "csr kernel"
        else:
            fn = lambda: F.BinnedDataset(X.toarray(), y, "cuda",
                                         is_cls=True)
            how = "toarray + dense binning"
        ts, ds = _time(fn)
        _report("bin", how, ts)
        print(f"bin    codes {tuple(ds.codes.shape)} "
              f"sum {int(ds.codes.sum(dtype=torch.int64))}", flush=True)


if __name__ == "__main__":
    main()
