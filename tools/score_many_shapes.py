#!/usr/bin/env python
"""Times the scoring of a hyperparameter sweep on the GPU: the loop a notebook runs today (per entry
`predict`, `confusion_matrix` and the accuracy on the host) against `score_many` and `predict_many`
on the same entries, in one process, alternating the routes.  Writes profiles/score_many_shapes.txt.

  python tools/score_many_shapes.py [--models 256] [--repeats 7] [--out profiles/score_many_shapes.txt]

Workloads: the notebook shape ((227, 8, 12), 4 classes, rank 6), `--models` models x 4 data sets each
(held-out half, training half and two shuffled copies); the same for ONE entry; and entries of 65536
rows (the streamed regime).  Per route: the median over `--repeats` windows of the wall time of the
whole call (it ends in a device synchronise) and, for the batch routes, of the time between device
events around the launches; launches and bytes downloaded are counted from the shapes.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensor_regression_amd import _engine  # noqa: E402
from tensor_regression_amd import multinomial_tensor_regression as M  # noqa: E402

DEV = "cuda:0"


def build(n_models, n_rows, dims=(8, 12), C=4, R=6, n_sets=4, seed=0):
    """`n_models` models with `n_sets` device-resident data sets each: entries (model, X, y)."""
    rng = np.random.default_rng(seed)
    models, Xs, ys = [], [], []
    for j in range(n_models):
        X = rng.standard_normal((n_rows,) + dims).astype(np.float32)
        y = rng.integers(0, C, size=n_rows)
        y[:C] = np.arange(C)
        Bcp = [torch.tensor((rng.random((k, R)) - 0.5).astype(np.float32), device=DEV) for k in dims + (C,)]
        m = M.CP_logistic_regression(X, y, rank=R, Bcp_init=Bcp, device=DEV)
        for s in range(n_sets):
            models.append(m)
            if s == 0:
                Xs.append(None)
                ys.append(None)
            else:  # a held-out draw and shuffled copies: other data of the same shape, on the device
                Xs.append(torch.tensor(rng.permutation(X.reshape(n_rows, -1), axis=1).reshape(X.shape), device=DEV))
                ys.append(torch.tensor(rng.permutation(y), device=DEV))
    return models, Xs, ys


def present_route(models, Xs, ys):
    """What a grid does today: predict, confusion_matrix and the accuracy, one entry at a time."""
    out = []
    for m, X, y in zip(models, Xs, ys):
        prob, pred = m.predict(X=X)
        yh = (m.y if y is None else y).cpu().numpy()
        cm = M.confusion_matrix(pred, yh)
        out.append(np.trace(cm) / np.sum(cm))
    return out


def timed(fn, repeats):
    torch.cuda.synchronize()
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(walls), min(walls), max(walls)


def device_ms(want, models, Xs, ys, repeats):
    """Median ms between device events around tr_mnl_score_many's launches, and the bytes downloaded."""
    entries = M._score_entries("tool", models, Xs, ys if want == "score" else None, None, None, want == "score")
    members = M._score_members(entries, 0, want == "score")
    ms, down = [], 0
    for _ in range(repeats):
        trace = []
        _engine.run_score_many(0, members, want, trace=trace)
        ms.append(trace[0][0])
        down = trace[0][1]
    return statistics.median(ms), down


def compare(title, models, Xs, ys, repeats, lines):
    n = len(models)
    rows = int(models[0].X.shape[0])
    C = int(models[0].Bcp[-1].shape[0])
    routes = {"present": lambda: present_route(models, Xs, ys),
              "score_many": lambda: M.score_many(models, X=Xs, y_true=ys),
              "predict_many": lambda: M.predict_many(models, X=Xs)}
    for fn in routes.values():  # warm-up: code objects, plans, the foreach kernels
        fn()
        fn()
    res = {k: [] for k in routes}
    for _ in range(repeats):  # alternate the routes, one window each per round
        for k, fn in routes.items():
            res[k].append(timed(fn, 1)[0])
    acc_now = present_route(models, Xs, ys)
    acc_new = [np.trace(s["cm"]) / np.sum(s["cm"]) for s in M.score_many(models, X=Xs, y_true=ys)]
    agree = sum(abs(a - b) < 1e-12 for a, b in zip(acc_now, acc_new))
    dev_s, down_s = device_ms("score", models, Xs, ys, repeats)
    dev_p, down_p = device_ms("predict", models, Xs, ys, repeats)
    lines.append(f"## {title}: {n} entries of {rows} rows")
    lines.append(f"{'route':14s} {'wall ms (median, min, max)':32s} {'us/entry':>10s} {'device ms':>10s} "
                 f"{'launches':>9s} {'bytes down':>12s}")
    med = {k: statistics.median(v) for k, v in res.items()}
    info = {"present": ("-", f">= {n}", n * rows * C * 4), "score_many": (f"{dev_s:.3f}", "3", down_s),
            "predict_many": (f"{dev_p:.3f}", "1", down_p)}
    for k, v in res.items():
        lines.append(f"{k:14s} {med[k]:10.3f} {min(v):10.3f} {max(v):10.3f}  {med[k] * 1e3 / n:10.2f} "
                     f"{info[k][0]:>10s} {info[k][1]:>9s} {info[k][2]:12d}")
    lines.append(f"present / score_many = {med['present'] / med['score_many']:.1f}x, "
                 f"present / predict_many = {med['present'] / med['predict_many']:.1f}x; "
                 f"accuracies agree on {agree}/{n} entries")
    lines.append("")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_many_shapes.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_many_shapes.py measures on the GPU; no HIP device found")
    lines = ["# Scoring a sweep: per-entry predict + host metrics against score_many / predict_many",
             f"# device: {torch.cuda.get_device_name(0)}; median of {a.repeats} alternating windows after warm-up;",
             "# wall = host clock around the whole call, ending in a device synchronise; device = events around",
             "# the table upload and the launches of tr_mnl_score_many; the present route's launch count is a",
             "# lower bound (one forward launch per entry; packing and the download add more)", ""]
    sweep = compare("the notebook sweep", *build(a.models, 227), a.repeats, lines)
    compare("one entry", *build(1, 227, n_sets=1), a.repeats, lines)
    big = compare("streamed regime", *build(2, 65536, n_sets=2), a.repeats, lines)
    x_bytes = 4 * 65536 * 96 * 4
    lines.append(f"# streamed regime: X read once is {x_bytes / 1e6:.1f} MB over the 4 entries")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return sweep, big


if __name__ == "__main__":
    main()
