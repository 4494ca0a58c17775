"""
One multinomial (softmax) SGD step against one one-vs-rest (sigmoid) step
at the same shape, on the device: a digits-like case, K = 10 classes and a
few hundred models, the same rows, features and epochs for both.

    python tools/softmax_step_bench.py [--models 300] [--epochs 200]

Prints one JSON line with the per-step times (device events around whole
solves; a solve replays one captured epoch, so launch overhead is the
graph's) and their ratio.  Under ``rocprofv3 --kernel-trace --stats`` the
kernel table shows where the softmax step's time goes (k_fwd_gt_softmax
against k_fwd_gt; K2 and K3 are shared, on 128-padded columns: 3200 for the
softmax layout of 300 models, 3072 for one-vs-rest).
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=300)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1797)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("softmax_step_bench: needs a GPU (no CPU timing)")

    from skdist_amd.models._sgd import (
        LOSS_LOG, LOSS_SOFTMAX, ColumnSpec, DeviceDataset)
    from skdist_amd.ops import hip_sgd_solve

    rng = np.random.default_rng(0)
    K, nm = a.classes, a.models
    X = rng.standard_normal((a.rows, a.features)).astype(np.float32)
    y = rng.integers(0, K, size=a.rows)
    ds = DeviceDataset(X, y, device="cuda")
    ds.fold_id = torch.as_tensor(rng.integers(0, 3, size=a.rows),
                                 dtype=torch.int32, device=ds.device)
    mfold = np.array([0, 1, 2, -2])[np.arange(nm) % 4]

    def spec(group_k):
        return ColumnSpec(
            ds.device, np.repeat(mfold, K).astype(np.int32),
            np.tile(np.arange(K, dtype=np.int32), nm),
            np.full(nm * K, 0.1, np.float32),
            np.full(nm * K, 1e-3, np.float32), group_k=group_k)

    steps = a.epochs * ((a.rows + 8191) // 8192)

    def timed(loss, sp):
        hip_sgd_solve(ds, sp, loss, 3, 8192, 0, 0.9, 0.0)   # warm-up
        torch.cuda.synchronize()
        out = []
        for _ in range(a.repeats):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            hip_sgd_solve(ds, sp, loss, a.epochs, 8192, 0, 0.9, 0.0)
            t1.record()
            torch.cuda.synchronize()
            out.append(t0.elapsed_time(t1) * 1e3 / steps)
        return out

    # alternate the two so that drift hits both alike
    ovr, smx = [], []
    sp_o, sp_s = spec(None), spec(K)
    for _ in range(2):
        ovr += timed(LOSS_LOG, sp_o)
        smx += timed(LOSS_SOFTMAX, sp_s)
    res = {
        "rows": a.rows, "fa": int(ds.Xaug.shape[1]), "classes": K,
        "models": nm, "steps_per_solve": steps,
        "ovr_step_us": round(float(np.median(ovr)), 2),
        "ovr_step_us_min_max": [round(min(ovr), 2), round(max(ovr), 2)],
        "softmax_step_us": round(float(np.median(smx)), 2),
        "softmax_step_us_min_max": [round(min(smx), 2), round(max(smx), 2)],
    }
    res["softmax_over_ovr"] = round(
        res["softmax_step_us"] / res["ovr_step_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
