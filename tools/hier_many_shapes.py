#!/usr/bin/env python3
"""Fits per second of fit_Adam_many (one launch, a workgroup per model) against a loop of fit_Adam
calls (GPU box).

    python tools/hier_many_shapes.py > profiles/hier_many_shapes.txt

Per shape (N, I0, I1), classes C, rank R and batch size M: M freshly built models, each with its own
seeded randn X (mean-subtracted along axis 1), labels and start, all factors non-negative, the
notebook's hyperparameters (lambda 0.005, lr 0.05, AMSGrad), tol = 0 so that every fit runs all its
ITERS iterations.  After one warm-up of 64 iterations per way, in ONE process and alternating:
batch, loop, batch (and a second loop where M <= 16).  Both ways are timed as wall time between two
device synchronisations around the whole call(s), models already built (their X on the device), so
both include packing the factors, the host synchronisations and the write-back.  Reported:
  * ms per iteration of the whole batch (wall time / ITERS) and fits per second, both ways;
  * the share of the batch's wall time in which the GPU is idle: 1 - (sum over launches of the ms
    between device events around the table upload + kernel) / wall time, for the whole call and for
    the chunk loop alone (there it is the host's table build and the stop array's round trip);
  * the slowest and fastest launch of 64 iterations (a per-launch trace: a clock that ramps, or a
    second wave of workgroups, shows here);
  * for M = 1, the single resident fit_Adam beside the batch entry (the loop IS that fit).
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H  # noqa: E402

dev = "cuda:0"
ITERS = 2048
HYPER = dict(lambda_L2=0.005, tol=0.0, patience=100)
ADAM = {"lr": 0.05, "amsgrad": True}
SHAPES = [("the notebook's shape", (227, 8, 12), 4, 6), ("a tiny problem", (64, 4, 4), 2, 1)]
BATCHES = [1, 2, 16, 256, 512]


def make_data(shape, C, R, M):
    out = []
    for j in range(M):
        rng = np.random.default_rng(j)
        X = rng.standard_normal(shape).astype(np.float32)
        X = torch.tensor(X - X.mean(axis=1, keepdims=True), device=dev)
        y = rng.integers(0, C, size=shape[0])
        y[:C] = np.arange(C)
        g = torch.Generator().manual_seed(j)
        B0 = [torch.rand(k, R, generator=g).to(dev) for k in shape[1:] + (C,)]
        out.append((X, torch.tensor(y, device=dev), B0))
    return out


def build(data, R):
    return [H.CP_logistic_regression(X, y, rank=R, non_negative=True,
                                     Bcp_init=[b.clone().requires_grad_(True) for b in B0], device=dev)
            for X, y, B0 in data]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_many(data, R, iters, trace=None):
    models = build(data, R)
    orig = _engine.run_resident_many
    if trace is not None:
        _engine.run_resident_many = lambda d, mbs: orig(d, mbs, trace=trace)
    try:
        report = {}
        ms = timed(lambda: H.fit_Adam_many(models, max_iter=iters, Adam_kwargs=dict(ADAM), report=report, **HYPER))
    finally:
        _engine.run_resident_many = orig
    assert report["batched"] == list(range(len(models))) and all(len(m.loss_running) == iters for m in models)
    return ms, models


def run_loop(data, R, iters):
    models = build(data, R)

    def go():
        for m in models:
            m.fit_Adam(max_iter=iters, Adam_kwargs=dict(ADAM), **HYPER)
    ms = timed(go)
    assert all("fit=resident" in m._plan.describe and len(m.loss_running) == iters for m in models)
    return ms, models


def main():
    os.environ.pop("TR_MNL_RESIDENT", None)
    for label, shape, C, R in SHAPES:
        print(f"{label}: X {shape}, C {C}, R {R}, {ITERS} iterations per fit", flush=True)
        data = make_data(shape, C, R, max(BATCHES))
        run_many(data[:2], R, 64)  # warm-up: code objects, pinned memory, the foreach copy
        run_loop(data[:2], R, 64)
        for M in BATCHES:
            d = data[:M]
            many, loop, idle = [], [], []
            order = ["many", "loop", "many"] + (["loop"] if M <= 16 else [])
            for way in order:
                if way == "many":
                    trace = []
                    ms, mm = run_many(d, R, ITERS, trace=trace)
                    busy = sum(t[1] for t in trace)
                    loop_wall = sum(t[2] for t in trace)
                    full = [t[1] for t in trace if t[0] == 64]
                    many.append(ms)
                    idle.append((1.0 - busy / ms, 1.0 - busy / loop_wall, min(full), max(full), full[0], full[-1]))
                else:
                    ms, ml = run_loop(d, R, ITERS)
                    loop.append(ms)
            same = all(np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy())
                       for x, y in zip(mm, ml) for a, b in zip(x.Bcp, y.Bcp))
            bm, bl = min(many), min(loop)
            print(f"    M {M:4d}  batch {bm / ITERS:8.4f} ms / iteration ({', '.join(f'{x:.1f}' for x in many)} ms), "
                  f"{1e3 * M / bm:9.1f} fits/s;  loop {bl / ITERS:8.4f} ms / iteration "
                  f"({', '.join(f'{x:.1f}' for x in loop)} ms), {1e3 * M / bl:9.1f} fits/s;  "
                  f"batch / loop = {bl / bm:6.2f}x;  factors bitwise equal: {same}", flush=True)
            for k, (i_all, i_loop, lo, hi, first, last) in enumerate(idle):
                print(f"            batch run {k}: GPU idle {100 * i_all:5.1f}% of the call, {100 * i_loop:5.1f}% of the "
                      f"chunk loop;  a 64-iteration launch {lo:.3f} .. {hi:.3f} ms (first {first:.3f}, last "
                      f"{last:.3f})", flush=True)
            if M == 1:
                spread = (max(loop) - min(loop)) / min(loop)
                print(f"            M = 1: the single resident fit {bl / ITERS:.4f} ms / iteration (its two runs differ "
                      f"by {100 * spread:.1f}%), the batch entry {bm / ITERS:.4f}: {100 * (bm / bl - 1):+.1f}%",
                      flush=True)


if __name__ == "__main__":
    main()
