"""K2 of the dense SGD step alone, at the flagship's shape, for timing under
a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -- \
        python tools/sgd_k2_bench.py --fa 288 --variant 3

ncols_pad 3072, m 8192, splitk 8, random bf16 operands; 8 warm-up launches
of ``ext.grad_partial`` and then ``--launches`` more.  The script times
nothing itself: read the kernel's rows of the trace.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

NCOLS_PAD, M, SPLITK, WARMUP = 3072, 8192, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fa", type=int, default=288)
    ap.add_argument("--variant", type=int, default=0,
                    help="0 the launcher's rule, 1 128-row tile, "
                         "2 96-row tile, 3 whole-fa kernel")
    ap.add_argument("--launches", type=int, default=32)
    a = ap.parse_args()

    from skdist_amd.ops import require_hip

    ext = require_hip()
    g = torch.Generator(device="cuda").manual_seed(0)
    fa_store = (a.fa + 127) // 128 * 128
    XsT = torch.zeros(fa_store, M, dtype=torch.bfloat16, device="cuda")
    XsT[: a.fa] = torch.randn(a.fa, M, device="cuda", generator=g)
    GT = torch.randn(NCOLS_PAD, M, device="cuda", generator=g) \
        .to(torch.bfloat16)
    partial = torch.empty(SPLITK, a.fa, NCOLS_PAD, dtype=torch.float32,
                          device="cuda")
    for _ in range(WARMUP + a.launches):
        ext.grad_partial(XsT, GT, partial, 0, M, a.variant)
    torch.cuda.synchronize()
    print(f"fa {a.fa} variant {a.variant}: {a.launches} launches after "
          f"{WARMUP} warm-up, checksum {float(partial.float().sum()):.6e}")


if __name__ == "__main__":
    main()
