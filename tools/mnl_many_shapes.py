#!/usr/bin/env python
"""Time the shared-X multinomial sweep (multinomial_tensor_regression.fit_Adam_many) against the loop
of single fits it replaces.

Per shape, class count and group size M: ms per iteration of the group (end to end, and the kernels
alone from run_mnl_many's trace), ms per iteration of M sequential fit_Adam calls on the same X (the
route without the sweep), and X bytes per second counting ONE read of X per iteration.  Device events,
a warm-up of every shape and M, the group and the loop alternating in one process, the median of
`--windows` windows and their spread (max - min) reported.

  python tools/mnl_many_shapes.py [--out profiles/mnl_many_shapes.txt] [--iters 20] [--windows 3]
                                  [--small]          (small shapes: a dry run of the tool itself)
                                  [--only NAME --m M] (one row, e.g. under a counter run)
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd import multinomial_tensor_regression as Mn  # noqa: E402

DEV = "cuda:0"
# (name, (N, I, J), classes, rank, group sizes)
# the notebook's sweep, bench.py's config 3 and C = 16; the config 3 shape again at C = 5 and C = 16, so
# that every class count is measured both where the single fit takes two passes over X (the notebook's
# 1 MB rows) and where it takes one at stream speed (config 3's 32 KB rows)
SHAPES = [("notebook", (2000, 500, 500), 5, 4, (1, 2, 3, 6, 12)),
          ("config3", (65536, 128, 64), 10, 8, (2, 3, 6)),
          ("notebook-c16", (2000, 500, 500), 16, 4, (4,)),
          ("config3-c5", (65536, 128, 64), 5, 8, (1, 2, 3, 6, 12)),
          ("config3-c16", (65536, 128, 64), 16, 8, (2, 4))]
SMALL = [("small-a", (256, 64, 32), 5, 4, (1, 12)), ("small-b", (2000, 32, 32), 10, 8, (2, 6)),
         ("small-c", (300, 16, 16), 16, 4, (4,))]


def models_for(X, y, C, rank, M, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(M):
        B0 = [(torch.randn(d, rank, generator=g) * 0.05).to(DEV) for d in list(X.shape[1:]) + [C]]
        out.append(Mn.CP_logistic_regression(X, y, rank=rank, device=DEV, Bcp_init=B0))
    return out


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def measure(X, y, C, rank, M, iters, windows):
    lams = [10.0 ** (-6 + 0.25 * j) for j in range(M)]  # a grid of one hyperparameter, as the notebook sweeps
    ak = {"lr": 1e-3}
    cw = np.ones(C, np.float32)
    kernel_ms = []
    real = _engine.run_mnl_many

    def traced(dev, Xd, members, **kw):
        trace = []
        res = real(dev, Xd, members, trace=trace, **kw)
        kernel_ms.append(sum(ms for _, ms in trace))
        return res

    def group():
        ms = models_for(X, y, C, rank, M, 1)
        _engine.run_mnl_many = traced
        try:
            rep = {}
            Mn.fit_Adam_many(ms, lambda_L2=lams, max_iter=iters, tol=0.0, weights=cw, Adam_kwargs=ak, min_batch=1,
                             report=rep)
            assert rep["batched"] == list(range(M)) and rep["groups"] == 1, rep
        finally:
            _engine.run_mnl_many = real

    def loop():
        for m, lam in zip(models_for(X, y, C, rank, M, 1), lams):
            m.fit_Adam(lambda_L2=lam, max_iter=iters, tol=0.0, weights=cw, Adam_kwargs=ak)

    group()
    loop()  # warm-up of both routes at this shape and M
    tb, tl, tk = [], [], []
    for _ in range(windows):  # alternating
        kernel_ms.clear()
        tb.append(timed(group) / iters)
        tk.append(sum(kernel_ms) / iters)
        tl.append(timed(loop) / iters)
    med = statistics.median
    return (med(tb), max(tb) - min(tb)), (med(tk), max(tk) - min(tk)), (med(tl), max(tl) - min(tl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mnl_many_shapes.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--m", type=int, default=None)
    a = ap.parse_args()
    lines = [f"# tools/mnl_many_shapes.py --iters {a.iters} --windows {a.windows}: {torch.cuda.get_device_name(0)}",
             "# ms per iteration: median of the windows (spread = max - min); group = fit_Adam_many(min_batch=1) end",
             "# to end, kernels = its tr_mnl_many_fit calls alone, loop = M sequential fit_Adam calls on the same X",
             "# (the route without the sweep).  X TB/s counts ONE read of X per iteration (the group reads it twice,",
             "# the loop M times).  cols = M * C columns of the 64 a group holds.",
             f"{'shape':<28}{'C':>4}{'rank':>5}{'M':>4}{'cols':>5}{'group ms':>11}{'(spread)':>10}{'kernels ms':>12}"
             f"{'(spread)':>10}{'loop ms':>10}{'(spread)':>10}{'loop/group':>11}{'X TB/s':>8}"]
    for name, shape, C, rank, Ms in (SMALL if a.small else SHAPES):
        if a.only is not None and name != a.only:
            continue
        g = torch.Generator(device=DEV).manual_seed(0)
        X = torch.randn(*shape, device=DEV, generator=g)
        y = torch.randint(0, C, (shape[0],), device=DEV, generator=g)
        y[:C] = torch.arange(C, device=DEV)
        xbytes = X.numel() * 4
        for M in Ms:
            if a.m is not None and M != a.m:
                continue
            (b, bs), (k, ks), (l, ls) = measure(X, y, C, rank, M, a.iters, a.windows)
            lines.append(f"{name + ' ' + 'x'.join(map(str, shape)):<28}{C:>4}{rank:>5}{M:>4}{M * C:>5}{b:>11.3f}"
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
