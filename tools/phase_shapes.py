#!/usr/bin/env python3
"""Time of one loss_grad of the phase-constrained plan beside a ConvPlan with C = 2 (GPU box).

    python tools/phase_shapes.py > profiles/phase_shapes.txt

Per shape (T, D, W, N, Rn, Rs), seeded randn inputs, both plans in the same process on the same
series: 3 warm-up calls, then 3 windows of REPS calls between device events (the median window is
reported, with the spread).  The phase plan's pass is prep + k_phase_kp + k_conv + k_phase_finish,
the conv plan's prep + k_conv_kp + k_conv + k_conv_finish; k_conv does the same work in both (the
same K = Rn + 2 Rs kernel columns), so the difference is the two small kernels: O(W^2 Rs) fmaf
against O(T' D W K) of the pass.  The conv plan's Ks holds [k, H k] of the phase plan's k, so both
passes see the same values.  A last line per plan gives the plans' own per-kernel event times.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd.phase_constrained_spectral_convolutional_tensor_regression import \
    quadrature_matrix  # noqa: E402

dev = "cuda:0"
SHAPES = [
    (65790, 128, 255, 4, 8, 8),  # the conv analogue of configs 5 and 6
    (1008, 64, 9, 3, 16, 4),
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
    for T, D, W, N, Rn, Rs in shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(T, D, device=dev, generator=g)
        y = torch.randn(T, N, device=dev, generator=g)
        Tp, R, K = T - W + 1, Rn + Rs, Rn + 2 * Rs
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
        Kn, Ks, Bd, Bo, bias = rn(W, Rn) / W ** 0.5, rn(W, Rs) / W ** 0.5, rn(D, R) / D ** 0.5, rn(N, R), rn(N)
        Hk = (quadrature_matrix(W).to(dev) @ Ks.double()).float()
        phase = _engine.ConvPhasePlan(W, D, N, Rn, Rs, T, [False] * 3, None, dev)
        conv = _engine.ConvPlan(W, D, N, Rn, Rs, 2, T, [False] * 3, None, dev)
        a_phase = phase.pack([Kn, Ks], [Bd, Bo], bias)
        a_conv = conv.pack([Kn, torch.stack([Ks, Hk], dim=-1).contiguous()], [Bd, Bo], bias)
        target = y[W // 2: T - W // 2].contiguous()
        g_phase = torch.zeros(phase.num_grads, device=dev)
        g_conv = torch.zeros(conv.num_grads, device=dev)
        reps = 20 if Tp * D * W * K < 1e10 else 3
        norm = float(Tp * N)
        # interleaved: conv, phase, conv, so that a drift of the clocks shows as a conv / conv spread
        c1 = timed(lambda: conv.loss_grad(X, target, None, norm, a_conv, None, g_conv), reps)
        p1 = timed(lambda: phase.loss_grad(X, target, None, norm, a_phase, None, g_phase), reps)
        c2 = timed(lambda: conv.loss_grad(X, target, None, norm, a_conv, None, g_conv), reps)
        l_phase, l_conv = float(g_phase[phase.num_params]), float(g_conv[conv.num_params])
        dl = abs(l_phase - l_conv) / abs(l_conv)
        path = phase.describe.split(" path=")[1].split()[0]
        print(f"(T, D, W, N, Rn, Rs) = ({T}, {D}, {W}, {N}, {Rn}, {Rs}): {path}, K = {K}; {reps} calls per window; "
              f"data loss phase vs conv {dl:.1e} relative", flush=True)
        print(f"    conv C=2 loss_grad   {c1[0]:9.4f} ms (min {c1[1]:.4f}, max {c1[2]:.4f})", flush=True)
        print(f"    phase    loss_grad   {p1[0]:9.4f} ms (min {p1[1]:.4f}, max {p1[2]:.4f})   phase / conv = "
              f"{p1[0] / c1[0]:.4f}", flush=True)
        print(f"    conv C=2 again       {c2[0]:9.4f} ms (min {c2[1]:.4f}, max {c2[2]:.4f})   conv / conv = "
              f"{c2[0] / c1[0]:.4f}", flush=True)
        # where the difference sits: the plans' own per-kernel events (prep = softplus + kernel columns,
        # stream_fused = k_conv, reduce = the finish kernel), 20 bracketed calls each
        for tag, plan, fn in (("conv C=2", conv, lambda: conv.loss_grad(X, target, None, norm, a_conv, None, g_conv)),
                              ("phase   ", phase,
                               lambda: phase.loss_grad(X, target, None, norm, a_phase, None, g_phase))):
            plan.set_timing(True)
            for _ in range(20):
                fn()
            t = plan.read_timing()
            plan.set_timing(False)
            kinds = [k for k in ("prep", "stream_fused", "reduce") if t[k][1]]
            print(f"    {tag} per kernel, us: " + "  ".join(f"{k} {1e3 * t[k][0] / t[k][1]:.1f}" for k in kinds),
                  flush=True)
        phase.destroy()
        conv.destroy()
        del X, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
