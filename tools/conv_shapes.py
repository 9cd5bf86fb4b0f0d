#!/usr/bin/env python3
"""Time of one loss_grad of the convolutional spectral kernel (k_conv) across shapes (GPU box).

    python tools/conv_shapes.py > profiles/conv_shapes.txt

Per shape (T, D, W, N, Rn, Rs, C), seeded randn inputs: 3 warm-up calls, then 3 windows of REPS
calls between device events (the median window is reported, with the spread).  Reported:
  * ms per ConvPlan.loss_grad (prep + kernel columns + k_conv + slab sum);
  * useful fp32 TFLOP/s, counting 2 T' D W K for the forward product and the same again for the
    recompute and for the dK product (3 products; padding columns are not counted), and its
    share of the 157.3 TFLOP/s vector peak;
  * the bytes of X the kernel requests from global memory (from the shapes: every tile stages its
    TT + W - 1 rows of every D chunk, twice for all chunks but the last when D is chunked) against
    the T * D * 4 ideal.  This is a count from the tile geometry, not a counter reading;
  * where the existing route can express the data term (N >= 2, inside the spectral envelope):
    ms per SpectralPlan.loss_grad on util.windowed_view of the same series with the same ranks, in
    the same process, and the ratio.
"""
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd.util import windowed_view  # noqa: E402

dev = "cuda:0"
PEAK = 157.3e12
SHAPES = [
    (65790, 128, 255, 4, 8, 8, 2),   # the conv analogue of configs 5 and 6
    (100000, 512, 33, 2, 4, 4, 2),
    (1008, 64, 9, 3, 16, 4, 4),      # the test sweep's largest three (T = T' + W - 1)
    (332, 130, 33, 4, 3, 5, 3),
    (216, 300, 17, 7, 8, 8, 2),
]


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    out.sort()
    return out[1], out[0], out[2]


def main():
    shapes = SHAPES
    if len(sys.argv) > 1:
        shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]]
    for T, D, W, N, Rn, Rs, C in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(T, D, device=dev, generator=g)
        y = torch.randn(T, N, device=dev, generator=g)
        Tp, R, K = T - W + 1, Rn + Rs, Rn + Rs * C
        plan = _engine.ConvPlan(W, D, N, Rn, Rs, C, T, [False] * 3, None, dev)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        arena = plan.pack([rn(W, Rn) / W ** 0.5, rn(W, Rs, C) / W ** 0.5], [rn(D, R) / D ** 0.5, rn(N, R)], rn(N))
        target = y[W // 2: T - W // 2].contiguous()
        grad = torch.zeros(plan.num_grads, device=dev)
        reps = 20 if Tp * D * W * K < 1e10 else 3
        ms, lo, hi = timed(lambda: plan.loss_grad(X, target, None, float(Tp * N), arena, None, grad), reps)
        flops = 3 * 2.0 * Tp * D * W * K
        tt = int(re.search(r"TT=(\d+)", plan.describe).group(1))
        dc = int(re.search(r"DC=(\d+)", plan.describe).group(1))
        ntiles = -(-Tp // tt)
        nch = -(-D // dc)
        staged_cols = D if nch == 1 else 2 * D - min(dc, D - (nch - 1) * dc)
        xbytes = 4.0 * staged_cols * sum(min(tt + W - 1, T - i * tt) for i in range(ntiles))
        path = plan.describe.split(" path=")[1].split()[0]
        print(f"(T, D, W, N, Rn, Rs, C) = ({T}, {D}, {W}, {N}, {Rn}, {Rs}, {C}): {path} DC={dc}", flush=True)
        print(f"    conv loss_grad {ms:9.4f} ms (min {lo:.4f}, max {hi:.4f}; {reps} calls per window)  "
              f"{flops / (ms * 1e-3) / 1e12:7.3f} useful TFLOP/s = {flops / (ms * 1e-3) / PEAK * 100:5.2f} % of the "
              f"fp32 vector peak;  X requested {xbytes / 1e6:.1f} MB = {xbytes / (T * D * 4.0):.2f} x ideal",
              flush=True)
        if N >= 2:
            try:
                Xw, yw = windowed_view(X, y, (-(W // 2), W // 2 + 1))
                sp = _engine.SpectralPlan(W, D, N, Rn, Rs, C, Xw.shape[0], [False] * 3, None, dev)
                sar = sp.pack([rn(W, Rn, 1), rn(D, Rn, 1), rn(N, Rn, 1)], [rn(W, Rs, C), rn(D, Rs, 1), rn(N, Rs, 1)],
                              rn(N))
                w = torch.ones(R, device=dev)
                sg = torch.zeros(sp.num_grads, device=dev)
                yw = yw.contiguous()
                sms, slo, shi = timed(lambda: sp.loss_grad(Xw, yw, None, float(Tp * N), sar, w, sg), reps)
                spath = sp.describe.split(" path=")[1].split()[0]
                print(f"    windowed spectral loss_grad ({spath}) {sms:9.4f} ms (min {slo:.4f}, max {shi:.4f});  "
                      f"conv / windowed = {ms / sms:.2f}", flush=True)
                sp.destroy()
            except Exception as e:  # an envelope error is a result too
                print(f"    windowed spectral route: {type(e).__name__}: {e}", flush=True)
        plan.destroy()
        del X, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
