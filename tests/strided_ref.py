"""Strided and windowed X for the fp32 kernel families: layouts, runners, comparisons (no kernels here).

tr_plan_set_x_stride lets every fp32 kernel read X in place through a row stride: sample n sits at
X + n * stride and its P floats are contiguous.  The contract the tests built on this module hold the
kernels to: A RESULT DEPENDS ONLY ON THE P FLOATS OF EACH ROW.  A layout therefore places the rows in
a 1-D float32 `base` in which every float that belongs to no row is a NaN canary: the gaps between
rows, at least P floats before the first row and at least P floats after the last.  A kernel may load
a canary as long as the value is selected away; one that multiplies it by a zero coefficient turns its
result into NaN, and one that reads a row at the wrong place reads other data.

Layouts (row stride; where row 0 starts):
  pad4  P + 4                               16-B aligned   gaps; the vector paths stay on when P % 4 == 0
  pad5  P + 5                               16-B aligned   gaps; odd stride: rows start only 4-B aligned
  ovl4  largest multiple of 4 in [4, P/2]   16-B aligned   overlapping rows, aligned
  ovl3  P - 3 (P >= 4)                      16-B aligned   overlapping rows, odd
  win   prod(F[1:]) (len(F) >= 2)           16-B aligned   util.windowed_view's rows, one time step apart
  off1  P + 5                               16 B + 4 B     misaligned pointer (the scalar paths must take it)
  one   P + 5, N = 1                        16-B aligned   a stride is passed but irrelevant
Overlapping layouts cannot hold an arbitrary X: the series is drawn and X derived from it.
"""
import math
import types

import numpy as np
import torch

LAYOUTS = ("pad4", "pad5", "ovl4", "ovl3", "win", "off1", "one")
OVERLAPPING = ("ovl4", "ovl3", "win")


def volume(F):
    return int(math.prod(int(d) for d in F))


def row_stride(layout, F):
    """The layout's row stride in floats, or None where the layout does not exist for rows of shape F."""
    F = tuple(int(d) for d in F)
    P = volume(F)
    if layout == "pad4":
        return P + 4
    if layout in ("pad5", "off1", "one"):
        return P + 5
    if layout == "ovl4":
        s = (P // 2) // 4 * 4
        return s if s >= 4 else None
    if layout == "ovl3":
        return P - 3 if P >= 4 else None
    if layout == "win":
        return volume(F[1:]) if len(F) >= 2 else None
    raise ValueError(f"unknown layout {layout!r}")


def applies(layout, N, F):
    if row_stride(layout, F) is None:
        return False
    return True if layout == "one" else int(N) >= 2


def _draw(n, gen):
    return torch.randn(n, generator=gen)


def build(layout, N, F, seed=0, draw=None, X=None):
    """-> namespace(layout, base, offset, stride, shape, strides, X, P, N) on the CPU.

    torch.as_strided(base, shape, strides, offset) equals X exactly; every float of base outside the
    rows is NaN.  draw(n, generator) -> n float32 values (default: standard normal) fills the rows, or,
    for an overlapping layout, the series they are cut from.  X (N, *F), if given, is placed as it is;
    an overlapping layout refuses it.  `one` ignores N and holds one row."""
    F = tuple(int(d) for d in F)
    P = volume(F)
    stride = row_stride(layout, F)
    if stride is None:
        raise ValueError(f"layout {layout} does not exist for rows of shape {F}")
    N = 1 if layout == "one" else int(N)
    draw = draw or _draw
    gen = torch.Generator().manual_seed(int(seed))
    offset = (P + 3) // 4 * 4 + (1 if layout == "off1" else 0)  # >= P canaries first; 16-B phase 0 (off1: 4 B)
    span = (N - 1) * stride + P
    total = offset + span + P
    total = (total + 3) // 4 * 4
    base = torch.full((total,), float("nan"), dtype=torch.float32)
    inner = [1] * len(F)
    for d in range(len(F) - 2, -1, -1):
        inner[d] = inner[d + 1] * F[d + 1]
    strides = (stride, *inner)
    if layout in OVERLAPPING:
        if X is not None:
            raise ValueError(f"an overlapping layout ({layout}) derives X from its series")
        base[offset:offset + span] = draw(span, gen).to(torch.float32)
        X = torch.as_strided(base, (N, *F), strides, offset).clone(memory_format=torch.contiguous_format)
    else:
        if X is None:
            X = draw(N * P, gen).to(torch.float32).reshape(N, *F)
        X = X.to(torch.float32).reshape(N, *F).clone(memory_format=torch.contiguous_format)
        for n in range(N):
            base[offset + n * stride:offset + n * stride + P] = X[n].reshape(-1)
    return types.SimpleNamespace(layout=layout, base=base, offset=offset, stride=stride, shape=(N, *F),
                                 strides=strides, X=X, P=P, N=N)


def view_of(lay, base=None):
    """The layout's view of `base` (default: its own CPU base; pass a device copy of it for a device view)."""
    return torch.as_strided(lay.base if base is None else base, lay.shape, lay.strides, lay.offset)


def row_mask(lay):
    """bool [len(base)]: True where a float belongs to at least one row."""
    m = np.zeros(lay.base.numel(), dtype=bool)
    for n in range(lay.N):
        m[lay.offset + n * lay.stride:lay.offset + n * lay.stride + lay.P] = True
    return m


def guard_bands(lay):
    """(floats before the first row, floats after the last row)."""
    return lay.offset, lay.base.numel() - (lay.offset + (lay.N - 1) * lay.stride + lay.P)


# ---- comparisons -------------------------------------------------------------------------------------
def _np(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def same_bits(a, b):
    """Same shape, dtype and bytes (a NaN equals a NaN of the same bits; +0 differs from -0)."""
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def has_nan(a):
    return bool(np.isnan(_np(a)).any())


_STRATEGY_KEYS = ("path", "T", "CH", "grid", "W", "pk", "S", "clusters", "units", "waves", "wg/cu", "nbuf", "lds",
                  "form", "rowblocks", "rk", "jt", "xform", "slsp", "xpieces", "vec", "KT", "recovered", "fit")


def strategy_words(describe):
    """Everything in a plan description that names a kernel choice, as a tuple of its words in order:
    path=, T=, CH=, grid=, W=, pk=, S=, clusters=, the `duo ...` clause (units waves wg/cu nbuf lds form),
    rowblocks=, rk=, jt=, xform=, and for the spectral plans the path, KT=, S=, slsp=, xpieces= and vec=.
    Shape, sizes of the workspace and the device's CU count are left out."""
    out = []
    for tok in describe.split():
        key = tok.split("=", 1)[0]
        if tok == "duo" or ("=" in tok and key in _STRATEGY_KEYS):
            out.append(tok)
    return tuple(out)


def word(describe, key):
    """The value of `key=` in a description, or None."""
    for tok in describe.split():
        if tok.startswith(key + "="):
            return tok[len(key) + 1:]
    return None


# ---- a numpy row reader, and the mistakes a strided kernel can make ----------------------------------
READER_BUGS = ("p_plus_1", "stride_P", "next_row_quad", "align_down")


def emulate_reader(base, offset, stride, N, P, bug=None):
    """A row reader as the kernels are: out[n] = sum_j c[j] * x[n, j] in float64 over the row's floats, read
    from `base` (1-D) at offset + n * stride.  bug:
      p_plus_1       reads P + 1 floats (a reduction that runs one float too far; the extra weighs 1)
      stride_P       reads the rows at stride P instead of `stride`
      next_row_quad  reads whole quads and relies on a zero coefficient for the floats past P
      align_down     rounds the row start down to 16 bytes
    Reads past the end of `base` return 0, as a range-checked buffer load does."""
    base = np.asarray(base, dtype=np.float32)
    c = (np.arange(P, dtype=np.float64) % 7 + 1.0) / 4.0
    out = np.zeros(N, dtype=np.float64)
    if bug == "stride_P":
        stride = P
    n_read = P + 1 if bug == "p_plus_1" else (P + 3) // 4 * 4 if bug == "next_row_quad" else P
    coef = np.zeros(n_read, dtype=np.float64)
    coef[:P] = c
    if bug == "p_plus_1":
        coef[P] = 1.0
    for n in range(N):
        at = offset + n * stride
        if bug == "align_down":
            at = at // 4 * 4
        x = np.zeros(n_read, dtype=np.float64)
        have = max(0, min(n_read, base.size - at))
        x[:have] = base[at:at + have]
        with np.errstate(invalid="ignore"):
            out[n] = float(np.sum(coef * x))
    return out


def bug_can_show(bug, lay):
    """Whether the mistake changes what the reader reads on this layout (against the contiguous copy)."""
    if bug == "p_plus_1":
        return True
    if bug == "stride_P":
        return lay.N >= 2
    if bug == "next_row_quad":  # past every row's P floats or, in an overlapping layout, past the last row's
        return lay.P % 4 != 0   # lies a canary; finite floats times zero leave no trace
    if bug == "align_down":
        return any((lay.offset + n * lay.stride) % 4 != 0 for n in range(lay.N))
    raise ValueError(bug)


# ---- rows more than 2 GiB apart ----------------------------------------------------------------------
FAR_STRIDE = (1 << 29) + 4  # floats: 2 GiB + 16 B between rows
FAR_OFFSET = 1 << 29        # floats: row 0 starts 2 GiB into the allocation


def far_aliases(n, offset=FAR_OFFSET, stride=FAR_STRIDE):
    """Float indices (into the allocation) where row n would be read if its byte offset from row 0,
    4 * n * stride, were truncated to 32 bits: (as signed, as unsigned)."""
    b = 4 * n * stride
    u = b & 0xFFFFFFFF
    s = u - (1 << 32) if u >= (1 << 31) else u
    assert s % 4 == 0 and u % 4 == 0
    return offset + s // 4, offset + u // 4


def far_total(P, N=3, offset=FAR_OFFSET, stride=FAR_STRIDE):
    """Floats of the allocation: the rows, and P floats past the last."""
    return offset + (N - 1) * stride + 2 * P


def far_canary_ranges(P, N=3, offset=FAR_OFFSET, stride=FAR_STRIDE):
    """[(start, stop)] float ranges to fill with NaN: P floats on either side of every row, and P floats
    at each truncation alias of rows 1.. that lies outside every row.  (An alias inside another row
    reads that row's data, which the comparison with the contiguous copy catches.)"""
    rows = [(offset + n * stride, offset + n * stride + P) for n in range(N)]
    out = []
    for a, b in rows:
        out += [(a - P, a), (b, b + P)]
    for n in range(1, N):
        for at in set(far_aliases(n, offset, stride)):
            if (at, at + P) in rows:
                continue  # not truncated: the row itself
            lo, hi = at, at + P
            pieces = [(lo, hi)]
            for a, b in rows:  # cut the rows out of the alias range
                nxt = []
                for p, q in pieces:
                    if q <= a or p >= b:
                        nxt.append((p, q))
                    else:
                        if p < a:
                            nxt.append((p, a))
                        if q > b:
                            nxt.append((b, q))
                pieces = nxt
            out += pieces
    return [(a, b) for a, b in out if b > a]


# ---- runners: one call sequence per family, every raw buffer returned ---------------------------------
def run_linear(plan, X, y, Bcp, bias, weights, lam, calls=1):
    """pack, loss_grad (x calls: consecutive calls walk the rows in opposite directions), finalize_grad,
    forward.  -> dict(grad=[arena with the data-loss and status slots, per call], gtot, loss, fwd, describe)."""
    dev = X.device
    arena = plan.pack(Bcp, bias)
    grads = []
    for _ in range(calls):
        grad = torch.zeros(plan.num_grads, device=dev)
        plan.loss_grad(X, y, None, float(X.shape[0]), arena, weights, grad)
        grads.append(grad)
    gtot = torch.zeros(plan.num_params, device=dev)
    loss = torch.zeros(1, device=dev)
    plan.finalize_grad(arena, grads[-1], lam, gtot, loss)
    fwd = plan.forward(X, arena, weights)
    torch.cuda.synchronize(dev)
    return dict(grad=grads, gtot=gtot, loss=loss, fwd=fwd, describe=plan.describe)


def run_multinomial(plan, X, y, class_w, Bcp, weights, lam, calls=1):
    """As run_linear for the multinomial plan (class_w on the device; the normaliser is sum_n class_w[y_n])."""
    dev = X.device
    arena = plan.pack(Bcp)
    norm = float(class_w.double()[y].sum().item())
    grads = []
    for _ in range(calls):
        grad = torch.zeros(plan.num_grads, device=dev)
        plan.loss_grad(X, y, class_w, norm, arena, weights, grad)
        grads.append(grad)
    gtot = torch.zeros(plan.num_params, device=dev)
    loss = torch.zeros(1, device=dev)
    plan.finalize_grad(arena, grads[-1], lam, gtot, loss)
    fwd = plan.forward(X, arena, weights)
    torch.cuda.synchronize(dev)
    return dict(grad=grads, gtot=gtot, loss=loss, fwd=fwd, describe=plan.describe)


def run_spectral(plan, X, y, Bcp_n, Bcp_c, bias, weights, lam, calls=1):
    """As run_linear for the spectral plan; also the fit model's y_hat and the latents (rank_normal > 0)."""
    dev = X.device
    arena = plan.pack(Bcp_n, Bcp_c, bias)
    grads = []
    yhat = torch.empty_like(y)
    for _ in range(calls):
        grad = torch.zeros(plan.num_grads, device=dev)
        plan.loss_grad(X, y, None, float(y.numel()), arena, weights, grad, yhat=yhat)
        grads.append(grad)
    gtot = torch.zeros(plan.num_params, device=dev)
    loss = torch.zeros(1, device=dev)
    plan.finalize_grad(arena, grads[-1], lam, gtot, loss)
    fwd = plan.forward(X, arena, weights)
    out = dict(grad=grads, gtot=gtot, loss=loss, yhat=yhat, fwd=fwd)
    if plan.rank_normal:
        out["lat"] = plan.latents(X, arena)
    torch.cuda.synchronize(dev)
    out["describe"] = plan.describe
    return out


def run_resident(model, **fit_kwargs):
    """fit_Adam of a hierarchical multinomial model.  -> dict(loss=[history], factors=[...], describe,
    x_stride=the row stride of the X the kernel was handed)."""
    model.fit_Adam(**fit_kwargs)
    _, Xd, _ = model._device_data()
    return dict(loss=np.asarray(model.loss_running, dtype=np.float64),
                factors=[A.detach().cpu().clone() for A in model.Bcp], describe=model._plan.describe,
                x_stride=int(Xd.stride(0)))


def buffers(res):
    """The comparable tensors of a runner's result, by name (lists flattened)."""
    out = {}
    for k, v in res.items():
        if k in ("describe", "x_stride"):
            continue
        if isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                out[f"{k}[{i}]"] = t
        else:
            out[k] = v
    return out
