#!/usr/bin/env python3
"""ms per iteration of the hierarchical multinomial module's fit_Adam on its two routes (GPU box).

    python tools/hier_shapes.py > profiles/hier_shapes.txt

Per shape (N, I0, I1), classes C, rank R, seeded randn X (mean-subtracted along axis 1), all factors
non-negative, the notebook's hyperparameters (lambda 0.005, lr 0.05, AMSGrad), tol = 0 so that every
fit runs all its iterations: one warm-up fit of 64 iterations per route, then whole fit_Adam calls of
ITERS iterations from the same start, in ONE process and in the order resident, streamed, resident
(the resident route before and after).  The streamed route is selected with TR_MNL_RESIDENT=0 and is
the code path a fit took before the resident kernel existed: the multinomial plan's passes plus the
grouped update step, per iteration.  Reported per fit:
  * ms per iteration between two device events recorded around the fit_Adam call;
  * ms per iteration of wall time between two device synchronisations around the same call.
Both include the call's fixed cost (packing the factors, one host synchronisation per 64 iterations,
the write-back), spread over ITERS iterations.  One sample past the LDS envelope only the streamed
route exists, and the module is asserted to take it.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensor_regression_amd import _lib  # noqa: E402
from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H  # noqa: E402

dev = "cuda:0"
ITERS = 2048
HYPER = dict(lambda_L2=0.005, tol=0.0, patience=100)
ADAM = {"lr": 0.05, "amsgrad": True}


def shapes():
    nmax = int(_lib.load().tr_mnl_resident_max_rows(8, 12, 4, 6))
    return [("the notebook's shape", (227, 8, 12), 4, 6),
            ("a tiny problem", (64, 4, 4), 2, 1),
            ("just inside the LDS envelope", (nmax, 8, 12), 4, 6),
            ("one sample past the envelope", (nmax + 1, 8, 12), 4, 6)]


def one_fit(X, y, B0, rank, route, iters):
    if route == "streamed":
        os.environ["TR_MNL_RESIDENT"] = "0"
    else:
        os.environ.pop("TR_MNL_RESIDENT", None)
    Bcp = [b.clone().requires_grad_(True) for b in B0]
    m = H.CP_logistic_regression(X, y, rank=rank, non_negative=True, Bcp_init=Bcp, device=dev)
    m.fit_Adam(max_iter=64, Adam_kwargs=dict(ADAM), **HYPER)  # warm-up: plan, code objects, caches
    with torch.no_grad():
        for A, b in zip(m.Bcp, B0):
            A.copy_(b)
    m.loss_running = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    m.fit_Adam(max_iter=iters, Adam_kwargs=dict(ADAM), **HYPER)
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    took = "resident" if "fit=resident" in m._plan.describe else "streamed"
    assert len(m.loss_running) == iters
    return a.elapsed_time(b) / iters, wall / iters, took, m._plan.describe, m.loss_running[-1]


def main():
    for label, shape, C, R in shapes():
        rng = np.random.default_rng(0)
        X = rng.standard_normal(shape).astype(np.float32)
        X = torch.tensor(X - X.mean(axis=1, keepdims=True), device=dev)
        y = rng.integers(0, C, size=shape[0])
        y[:C] = np.arange(C)
        y = torch.tensor(y, device=dev)
        torch.manual_seed(0)
        B0 = [torch.rand(k, R, device=dev) for k in shape[1:] + (C,)]
        print(f"{label}: X {shape}, C {C}, R {R}, {ITERS} iterations per fit", flush=True)
        res = {}
        for k, route in enumerate(["resident", "streamed", "resident"]):
            ev, wall, took, desc, last = one_fit(X, y, B0, R, route, ITERS)
            if took != route:
                if k == 0:
                    print("    resident route: not taken (outside the envelope)", flush=True)
                continue
            res.setdefault(route, []).append(ev)
            print(f"    {route:8s} {ev:8.4f} ms / iteration by device events, {wall:8.4f} by wall time;  "
                  f"last loss {last:.6f}  [{desc}]", flush=True)
        if "resident" in res:
            r = min(res["resident"])
            print(f"    streamed / resident = {res['streamed'][0] / r:.2f}", flush=True)


if __name__ == "__main__":
    main()
