#!/usr/bin/env python
"""Time scoring the linear sweep (score_many) against the loop it replaces: predict per model, with the
metrics formed on the host from the downloaded y_hat.

Per shape and group size M: ms per call of score_many(min_batch=1) end to end (wall clock around the
call, which ends in its one host sync), ms of its tr_linear_many_score calls alone (device events, from
run_linear_score's trace), ms of the loop of M predict calls plus host metrics on the same X, and X
bytes per second counting ONE read of X over the kernels' time.  A warm-up of every shape and M, the
group and the loop alternating in one process, `--reps` calls per window, the median of `--windows`
windows and their spread (max - min) reported.

  python tools/linear_score_shapes.py [--out profiles/linear_score_shapes.txt] [--reps 50] [--windows 3]
                                      [--small]   (two small shapes: a dry run of the tool itself)
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd import standard_tensor_regression as S  # noqa: E402

DEV = "cuda:0"
# (name, (N, I, J), rank, group sizes)
SHAPES = [("notebook", (2000, 500, 500), 10, (1, 2, 4, 16)),
          ("config2", (65536, 256, 128), 8, (1, 2, 4, 16))]
SMALL = [("small-a", (256, 64, 32), 4, (1, 4, 16, 17)), ("small-b", (2000, 32, 32), 8, (2, 16))]


def models_for(shape, rank, M, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(M):
        B0 = [(torch.randn(d, rank, generator=g) * 0.05).to(DEV) for d in shape[1:]]
        out.append(S.CP_linear_regression(shape, rank=rank, device=DEV, Bcp_init=B0))
    return out


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def measure(X, y, y_host, shape, rank, M, reps, windows):
    models = models_for(shape, rank, M, 1)
    kernel_ms = []
    real = _engine.run_linear_score

    def traced(dev, Xd, members, want, trace=None):
        trace = []
        res = real(dev, Xd, members, want, trace)
        kernel_ms.append(sum(ms for ms, _ in trace))
        return res

    def group():
        _engine.run_linear_score = traced
        try:
            S.score_many(models, X, y, min_batch=1)
        finally:
            _engine.run_linear_score = real

    def loop():
        for m in models:
            S._host_metrics(m.predict(X), y_host)

    group()
    loop()  # warm-up of both routes at this shape and M
    tg, tk, tl = [], [], []
    for _ in range(windows):  # alternating
        kernel_ms.clear()
        tg.append(wall_ms(group, reps))
        tk.append(sum(kernel_ms) / reps)
        tl.append(wall_ms(loop, reps))
    med = statistics.median
    return (med(tg), max(tg) - min(tg)), (med(tk), max(tk) - min(tk)), (med(tl), max(tl) - min(tl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "linear_score_shapes.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    lines = [f"# tools/linear_score_shapes.py --reps {a.reps} --windows {a.windows}: {torch.cuda.get_device_name(0)}",
             "# ms per call: median of the windows (spread = max - min); group = score_many(min_batch=1) end to end",
             "# (wall clock, its host sync included), kernels = its tr_linear_many_score calls alone (device events),",
             "# loop = M predict calls plus the float64 host metrics on the same X (wall clock).",
             "# X TB/s: ONE read of X over the kernels' ms (the loop reads X M times).",
             f"{'shape':<22}{'rank':>5}{'M':>4}{'groups':>7}{'group ms':>11}{'(spread)':>10}{'kernels ms':>12}"
             f"{'(spread)':>10}{'loop ms':>10}{'(spread)':>10}{'loop/group':>11}{'X TB/s':>8}"]
    for name, shape, rank, Ms in (SMALL if a.small else SHAPES):
        g = torch.Generator(device=DEV).manual_seed(0)
        X = torch.randn(*shape, device=DEV, generator=g)
        y = torch.randn(shape[0], device=DEV, generator=g)
        y_host = y.cpu().numpy()
        xbytes = X.numel() * 4
        for M in Ms:
            (b, bs), (k, ks), (l, ls) = measure(X, y, y_host, shape, rank, M, a.reps, a.windows)
            lines.append(f"{name + ' ' + 'x'.join(map(str, shape)):<22}{rank:>5}{M:>4}{-(-M // 16):>7}{b:>11.3f}"
                         f"{bs:>10.3f}{k:>12.3f}{ks:>10.3f}{l:>10.3f}{ls:>10.3f}{l / b:>11.2f}"
                         f"{xbytes / (k * 1e-3) / 1e12:>8.2f}")
            print(lines[-1], flush=True)
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
