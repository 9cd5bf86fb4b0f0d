#!/usr/bin/env python3
"""Time of one loss_grad of the convolutional Fourier plan with the spectrum penalty off and on, and
of the spectrum stage alone (GPU box).

    python tools/fourier_shapes.py > profiles/fourier_shapes.txt

Per shape (T, D, W, N, Rn, Rs, C), seeded randn inputs, a smoothing kernel of S = 101 taps, n_fft = T:
3 warm-up calls, then 3 windows of REPS calls between device events (the median window is reported,
with the spread).  Off is prep + k_conv_kp + k_conv + k_conv_finish (the conv plan's pass); on adds
k_conv<0> (y_hat), the forward DFT, the spectrum terms and the adjoint DFT before k_conv.  The spectrum
stage alone is tr_conv_spectrum_penalty on a series of T' rows: both DFT passes and the small kernels
between them.  Each DFT pass does 4 T' F N useful flops (F = n_fft / 2 + 1 bins, one fmaf per cos and
per sin term); the useful rate printed is 8 T' F N over the stage's time, the small kernels included.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_regression_amd import _engine  # noqa: E402

dev = "cuda:0"
S_TAPS = 101
SHAPES = [
    (65790, 128, 255, 4, 8, 8, 2),  # the conv analogue of configs 5 and 6
    (20000, 16, 33, 2, 4, 4, 2),
    (1008, 64, 9, 3, 16, 4, 4),
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
    x = np.arange(-(S_TAPS // 2), S_TAPS // 2 + 1)
    sig = (S_TAPS - 1) / 7
    taps = (1 / (np.sqrt(2 * np.pi) * sig) * np.exp(-np.power(x / sig, 2) / 2)).astype(np.float32)
    for T, D, W, N, Rn, Rs, C in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(T, D, device=dev, generator=g)
        y = torch.randn(T, N, device=dev, generator=g)
        Tp, R, K, F = T - W + 1, Rn + Rs, Rn + Rs * C, T // 2 + 1
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        Kn, Ks, Bd, Bo, bias = rn(W, Rn) / W ** 0.5, rn(W, Rs, C) / W ** 0.5, rn(D, R) / D ** 0.5, rn(N, R), rn(N)
        plan = _engine.ConvFourierPlan(W, D, N, Rn, Rs, C, T, [False] * 3, None, dev)
        arena = plan.pack([Kn, Ks], [Bd, Bo], bias)
        target = y[W // 2: T - W // 2].contiguous()
        grad = torch.zeros(plan.num_grads, device=dev)
        reps = 20 if Tp * D * W * K < 1e10 else 3
        norm = float(Tp * N)
        run = lambda: plan.loss_grad(X, target, None, norm, arena, None, grad)  # noqa: E731
        off1 = timed(run, reps)
        plan.set_spectrum_penalty(0.05, taps, T, target)
        path = plan.describe.split(" path=")[1].split()[0]
        on = timed(run, reps)
        series = torch.randn(Tp, N, device=dev, generator=g)
        stage = timed(lambda: plan.conv_spectrum_penalty(series), reps)
        plan.set_spectrum_penalty(0.0, None, 0, None)
        off2 = timed(run, reps)
        flops = 8.0 * Tp * F * N
        print(f"(T, D, W, N, Rn, Rs, C) = ({T}, {D}, {W}, {N}, {Rn}, {Rs}, {C}): {path}, K = {K}, n_fft = {T}, "
              f"bins = {F}, taps = {S_TAPS}; {reps} calls per window", flush=True)
        print(f"    penalty off loss_grad  {off1[0]:9.4f} ms (min {off1[1]:.4f}, max {off1[2]:.4f})", flush=True)
        print(f"    penalty on  loss_grad  {on[0]:9.4f} ms (min {on[1]:.4f}, max {on[2]:.4f})   on / off = "
              f"{on[0] / off1[0]:.4f}", flush=True)
        print(f"    spectrum stage alone   {stage[0]:9.4f} ms (min {stage[1]:.4f}, max {stage[2]:.4f})   two DFT passes "
              f"of {flops / 2e9:.2f} GFLOP each: {flops / stage[0] / 1e9:.2f} TFLOP/s useful", flush=True)
        print(f"    penalty off again      {off2[0]:9.4f} ms (min {off2[1]:.4f}, max {off2[2]:.4f})   off / off = "
              f"{off2[0] / off1[0]:.4f}", flush=True)
        plan.destroy()
        del X, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
