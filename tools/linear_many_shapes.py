#!/usr/bin/env python
"""Time the shared-X linear sweep (fit_Adam_many) against the loop of single fits it replaces.

Per shape and group size M: ms per iteration of the batch (end to end, and the kernels alone from
run_linear_many's trace), ms per iteration of M sequential fit_Adam calls on the same X (the route
without the sweep), and X bytes per second counting ONE read of X per iteration.  Device events,
a warm-up of every shape, the batch and the loop alternating in one process, the median of
`--windows` windows and their spread (max - min) reported.

  python tools/linear_many_shapes.py [--out profiles/linear_many_shapes.txt] [--iters 20] [--windows 3]
                                     [--small]   (two small shapes: a dry run of the tool itself)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd import standard_tensor_regression as S  # noqa: E402

DEV = "cuda:0"
# (name, (N, I, J), rank, group sizes)
SHAPES = [("notebook", (2000, 500, 500), 10, (1, 2, 4, 8, 16, 30)),
          ("config2", (65536, 256, 128), 8, (4, 8, 16))]
SMALL = [("small-a", (256, 64, 32), 4, (1, 4, 16, 17)), ("small-b", (2000, 32, 32), 8, (4, 16))]


def models_for(shape, rank, M, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(M):
        B0 = [(torch.randn(d, rank, generator=g) * 0.05).to(DEV) for d in shape[1:]]
        out.append(S.CP_linear_regression(shape, rank=rank, device=DEV, Bcp_init=B0))
    return out


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def measure(X, y, shape, rank, M, iters, windows):
    lams = [10.0 ** (-6 + 0.25 * j) for j in range(M)]  # a lambda grid, as the notebook sweeps
    ak = {"lr": 1e-3}
    kernel_ms = []
    real = _engine.run_linear_many

    def traced(dev, Xd, members, **kw):
        trace = []
        res = real(dev, Xd, members, trace=trace, **kw)
        kernel_ms.append(sum(ms for _, ms in trace))
        return res

    def batch():
        ms = models_for(shape, rank, M, 1)
        _engine.run_linear_many = traced
        try:
            S.fit_Adam_many(ms, X, y, lambda_L2=lams, max_iter=iters, tol=0.0, Adam_kwargs=ak, min_batch=1)
        finally:
            _engine.run_linear_many = real

    def loop():
        for m, lam in zip(models_for(shape, rank, M, 1), lams):
            m.fit_Adam(X, y, lambda_L2=lam, max_iter=iters, tol=0.0, Adam_kwargs=ak)

    batch()
    loop()  # warm-up of both routes at this shape and M
    tb, tl, tk = [], [], []
    for _ in range(windows):  # alternating
        kernel_ms.clear()
        tb.append(timed(batch) / iters)
        tk.append(sum(kernel_ms) / iters)
        tl.append(timed(loop) / iters)
    med = statistics.median
    return (med(tb), max(tb) - min(tb)), (med(tk), max(tk) - min(tk)), (med(tl), max(tl) - min(tl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "linear_many_shapes.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    lines = [f"# tools/linear_many_shapes.py --iters {a.iters} --windows {a.windows}: {torch.cuda.get_device_name(0)}",
             "# ms per iteration: median of the windows (spread = max - min); batch = fit_Adam_many(min_batch=1) end",
             "# to end, kernels = its tr_linear_many_fit calls alone, loop = M sequential fit_Adam calls on the same X.",
             "# X TB/s counts ONE read of X per iteration (the batch reads it twice, the loop M times).",
             "# The gradient pass is the MFMA form and the two passes are full passes (last row chunk first): the",
             "# VALU gradient form and the row-block variant are not built, so there is nothing to compare them with.",
             f"{'shape':<22}{'rank':>5}{'M':>4}{'groups':>7}{'batch ms':>11}{'(spread)':>10}{'kernels ms':>12}"
             f"{'(spread)':>10}{'loop ms':>10}{'(spread)':>10}{'loop/batch':>11}{'X TB/s':>8}"]
    for name, shape, rank, Ms in (SMALL if a.small else SHAPES):
        g = torch.Generator(device=DEV).manual_seed(0)
        X = torch.randn(*shape, device=DEV, generator=g)
        y = torch.randn(shape[0], device=DEV, generator=g)
        xbytes = X.numel() * 4
        for M in Ms:
            (b, bs), (k, ks), (l, ls) = measure(X, y, shape, rank, M, a.iters, a.windows)
            lines.append(f"{name + ' ' + 'x'.join(map(str, shape)):<22}{rank:>5}{M:>4}{-(-M // 16):>7}{b:>11.3f}"
                         f"{bs:>10.3f}{k:>12.3f}{ks:>10.3f}{l:>10.3f}{ls:>10.3f}{l / b:>11.2f}"
                         f"{xbytes / (b * 1e-3) / 1e12:>8.2f}")
            print(lines[-1], flush=True)
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
