"""Host-side checks of the shared-X multinomial sweep (multinomial_tensor_regression.fit_Adam_many and
the tr_mnl_many_* entries), no GPU:

  * the header, the library and _lib.py agree on the new symbols and on tr_mnl_many_member's layout; the
    ABI version is still 9
  * the C entries' argument checks answer without a device and name the offending member: NULL buffers,
    n_iters out of range, n_classes 1 or 17, rank 0 or 33, cw_norm <= 0, amsgrad without its buffer,
    65 columns in total, a short table, a short workspace
  * tests/cpp/mnl_many_check.cpp, the geometry, the column packing and the table builder under
    AddressSanitizer and UBSan, built with the host compiler and run as a child process; nothing is
    preloaded
  * the routing of fit_Adam_many with the engine call stubbed: grouping by X identity, group filling by
    columns (13 models of C = 5 give 12 + 1), min_batch, TR_MNL_MANY=0, a hierarchical instance, a P
    that is no multiple of 4 and a HostStream alone, per-model lists of the wrong length
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensor_regression_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "tensor_regression_hip.h")
SRC = os.path.join(ROOT, "tests", "cpp", "mnl_many_check.cpp")
TR_E_ARG, TR_E_UNSUPPORTED = -1, -2
SYMBOLS = ("tr_mnl_many_envelope", "tr_mnl_many_workspace_bytes", "tr_mnl_many_member_table_bytes",
           "tr_mnl_many_loss_grad", "tr_mnl_many_step", "tr_mnl_many_fit")


def _M():
    from tensor_regression_amd import multinomial_tensor_regression as M
    return M


# ---- symbols and the struct's layout --------------------------------------------------------------

C_TYPES = {"const float*": (ctypes.c_void_p, 8), "float*": (ctypes.c_void_p, 8), "double*": (ctypes.c_void_p, 8),
           "int32_t*": (ctypes.c_void_p, 8), "const int64_t*": (ctypes.c_void_p, 8), "int64_t": (ctypes.c_int64, 8),
           "int32_t": (ctypes.c_int32, 4), "float": (ctypes.c_float, 4), "double": (ctypes.c_double, 8)}


def header_struct_fields(struct):
    """[(name, ctype, count)] of `struct`, parsed from the header."""
    txt = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"((?:const )?\w+\s*\*?)\s*(.*)", decl)
        ctype, names = m.group(1).replace(" *", "*").strip(), m.group(2)
        for nm in (n.strip() for n in names.split(",")):
            star = nm.startswith("*")
            nm = nm.lstrip("*")
            arr = re.match(r"(\w+)\[(\d+)\]", nm)
            out.append((arr.group(1) if arr else nm, ctype + ("*" if star else ""), int(arr.group(2)) if arr else 1))
    return out


def test_new_symbols_and_struct_layout_agree_with_the_header():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    txt = open(HEADER).read()
    for s in SYMBOLS:
        assert re.search(r"^\s*(?:int|int64_t)\s+" + s + r"\s*\(", txt, flags=re.M), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.SIGNATURES["tr_mnl_many_member_table_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["tr_mnl_many_workspace_bytes"][0] is ctypes.c_int64
    for s, at in (("tr_mnl_many_loss_grad", 6), ("tr_mnl_many_fit", 6), ("tr_mnl_many_step", 3)):
        assert _lib.SIGNATURES[s][1][at]._type_ is _lib.MnlManyMember
    assert lib.tr_abi_version() == _lib.TR_ABI_VERSION == 9
    assert ctypes.sizeof(_lib.LinearMember) == 184  # the linear sweep's struct is as it was
    fields = header_struct_fields("tr_mnl_many_member")
    assert [f[0] for f in fields] == [f[0] for f in _lib.MnlManyMember._fields_]
    off = 0
    for (name, ctype, count), (pname, ptype) in zip(fields, _lib.MnlManyMember._fields_):
        base, size = C_TYPES[ctype]
        want = base * count if count > 1 else base
        assert ctypes.sizeof(ptype) == ctypes.sizeof(want) == size * count, name
        if count == 1:
            assert ptype is base, name
        else:
            assert ptype._type_ is base and ptype._length_ == count, name
        off = -(-off // size) * size  # the C compiler's natural alignment
        assert getattr(_lib.MnlManyMember, name).offset == off, (name, off)
        off += size * count
    assert ctypes.sizeof(_lib.MnlManyMember) == -(-off // 8) * 8 == 208
    assert np.dtype(_lib.MnlManyMember).itemsize == 208
    # the Adam, history and stop fields carry tr_linear_member's names (tr_member_table.h serves both)
    shared = {"exp_avg", "exp_avg_sq", "max_exp_avg_sq", "grad", "loss_hist", "stop_flag", "amsgrad", "n_iters", "lr",
              "beta1", "beta2", "eps", "weight_decay", "step", "hist_base", "iter", "patience", "tol", "lambda_l2"}
    assert shared <= {f[0] for f in fields} and shared <= {f[0] for f in _lib.LinearMember._fields_}


def test_envelope_edges():
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    env = lib.tr_mnl_many_envelope
    assert env(8, 12, 0, 5, 32) == 1 and env(8, 12, 0, 5, 33) == 0 and env(8, 12, 0, 5, 0) == 0
    assert env(8, 12, 0, 2, 4) == 1 and env(8, 12, 0, 1, 4) == 0 and env(8, 12, 0, 16, 4) == 1 and env(8, 12, 0, 17, 4) == 0
    assert env(3, 3, 0, 5, 2) == 0 and env(3, 4, 0, 5, 2) == 1 and env(6, 5, 0, 3, 2) == 0   # P % 4
    assert env(8, 12, 98, 5, 2) == 0 and env(8, 12, 100, 5, 2) == 1                         # stride % 4
    assert env(9, 12, 12, 4, 2) == 1                                                        # a windowed view
    assert env(8, 12, -4, 5, 2) == 0 and env(0, 12, 0, 5, 2) == 0
    assert _engine.mnl_many_envelope(500, 500, 250000, 5, 4) and not _engine.mnl_many_envelope(5, 5, 25, 5, 4)
    ws = lib.tr_mnl_many_workspace_bytes
    assert ws(2000, 500, 500) > 2 * 64 * 250000 * 4
    assert ws(10, 3, 3) == 0 and ws(0, 8, 12) == 0 and ws(3, 8, 4) % 256 == 0 and ws(3, 8, 4) > 0


# ---- the C entries ----------------------------------------------------------------------------------

def _members(n, n_iters=1, n_classes=5):
    """Well-formed members over host memory (the checks never dereference a buffer)."""
    from tensor_regression_amd import _lib
    arr = (_lib.MnlManyMember * n)()
    keep = []
    for j, r in enumerate(arr):
        buf = (ctypes.c_double * 8)()
        keep.append(buf)
        p = ctypes.addressof(buf)
        for f in ("params", "weights", "y", "class_weights", "exp_avg", "exp_avg_sq", "grad", "loss_hist", "stop_flag"):
            setattr(r, f, p)
        r.n_classes, r.rank, r.cw_norm = n_classes, (1, 3, 8, 32)[j % 4], 10.0
        r.softplus_beta, r.softplus_threshold, r.lambda_l2 = 50.0, 1.0, 0.01
        r.n_iters, r.step = n_iters, 1
        r.lr, r.beta1, r.beta2, r.eps = 0.01, 0.9, 0.999, 1e-8
        r.patience = 10
    return arr, keep


def test_c_entries_check_every_member_without_a_device():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    M = 3
    nbytes = int(lib.tr_mnl_many_member_table_bytes(M))
    per = int(lib.tr_mnl_many_member_table_bytes(4)) - nbytes  # one row; the column map follows the rows
    assert per > 0 and nbytes > M * per and lib.tr_mnl_many_member_table_bytes(-1) == 0
    assert int(lib.tr_mnl_many_member_table_bytes(6)) - nbytes == 3 * per
    big = int(lib.tr_mnl_many_member_table_bytes(33))
    host = (ctypes.c_char * big)()
    devb = (ctypes.c_char * big)()  # never touched: every call below fails its checks first
    wsb = int(lib.tr_mnl_many_workspace_bytes(10, 8, 12))
    X = (ctypes.c_char * 4096)()
    xp = (ctypes.addressof(X) + 255) // 256 * 256  # aligned stand-ins for X and the workspace

    def fit(arr, n=M, I0=8, I1=12, stride=0, th=host, td=devb, nb=big, x=xp, ws=xp, wb=wsb, rows=10):
        rc = lib.tr_mnl_many_fit(0, x, rows, stride, I0, I1, arr, n, ws, wb, th, td, nb, None)
        return rc, (lib.tr_last_error() or b"").decode()

    def grad(arr, n=M):
        rc = lib.tr_mnl_many_loss_grad(0, xp, 10, 0, 8, 12, arr, n, xp, wsb, host, devb, big, None)
        return rc, (lib.tr_last_error() or b"").decode()

    def step(arr, n=M):
        rc = lib.tr_mnl_many_step(0, 8, 12, arr, n, host, devb, big, None)
        return rc, (lib.tr_last_error() or b"").decode()

    for at, code, fields in [
        (1, TR_E_ARG, dict(n_iters=65)), (0, TR_E_ARG, dict(n_iters=-1)), (2, TR_E_ARG, dict(params=None)),
        (1, TR_E_ARG, dict(stop_flag=None)), (0, TR_E_ARG, dict(loss_hist=None)), (2, TR_E_ARG, dict(amsgrad=1)),
        (1, TR_E_ARG, dict(y=None)), (0, TR_E_ARG, dict(class_weights=None)), (2, TR_E_ARG, dict(weights=None)),
        (0, TR_E_ARG, dict(step=0)), (2, TR_E_ARG, dict(lr=-0.5)), (1, TR_E_ARG, dict(lr=float("nan"))),
        (0, TR_E_ARG, dict(hist_base=-1)), (2, TR_E_ARG, dict(grad=None)), (1, TR_E_ARG, dict(cw_norm=0.0)),
        (2, TR_E_ARG, dict(cw_norm=-1.0)), (0, TR_E_ARG, dict(cw_norm=float("nan"))),
        (0, TR_E_UNSUPPORTED, dict(rank=33)), (1, TR_E_UNSUPPORTED, dict(rank=0)),
        (2, TR_E_UNSUPPORTED, dict(n_classes=1)), (1, TR_E_UNSUPPORTED, dict(n_classes=17)),
    ]:
        arr, keep = _members(M)
        for k, v in fields.items():
            setattr(arr[at], k, v)
        rc, msg = fit(arr)
        assert rc == code, (at, fields, rc, msg)
        assert msg.startswith(f"member {at}:"), (fields, msg)
    # the first bad member is named; the step entry takes n_iters 0 or 1 only; an evaluation needs no Adam buffers
    arr, keep = _members(M)
    arr[2].n_iters, arr[1].step = 99, 0
    assert fit(arr)[1].startswith("member 1:")
    arr, keep = _members(M, n_iters=2)
    rc, msg = step(arr)
    assert rc == TR_E_ARG and msg.startswith("member 0:")
    arr, keep = _members(M)
    arr[1].n_classes = 17
    assert grad(arr) == (TR_E_UNSUPPORTED, "member 1: n_classes outside 2..16") and step(arr)[0] == TR_E_UNSUPPORTED
    # 64 columns pass the checks, 65 do not; 33 members neither
    arr13, keep13 = _members(13, n_classes=5)
    for entry in (fit, grad, step):
        rc, msg = entry(arr13, n=13)
        assert rc == TR_E_ARG and "64 columns" in msg, (rc, msg)
    arr4, keep4 = _members(5, n_iters=0, n_classes=16)
    assert step(arr4, n=4)[0] == 0 and fit(arr4, n=4)[0] == 0  # exactly 64 columns, nothing to step: success
    assert step(arr4, n=5)[0] == TR_E_ARG
    arr33, keep33 = _members(33, n_classes=2)
    rc, msg = fit(arr33, n=33)
    assert rc == TR_E_ARG and "32" in msg
    # the call's own arguments
    arr, keep = _members(M)
    assert fit(arr, n=-1)[0] == TR_E_ARG and fit(None)[0] == TR_E_ARG
    assert fit(arr, th=None)[0] == TR_E_ARG and fit(arr, td=None)[0] == TR_E_ARG
    rc, msg = fit(arr, nb=nbytes - 1)
    assert rc == TR_E_ARG and "tr_mnl_many_member_table_bytes" in msg
    assert fit(arr, x=None)[0] == TR_E_ARG and fit(arr, ws=None)[0] == TR_E_ARG
    rc, msg = fit(arr, wb=wsb - 1)
    assert rc == TR_E_ARG and "tr_mnl_many_workspace_bytes" in msg
    assert fit(arr, rows=0)[0] == TR_E_ARG
    assert fit(arr, I0=3, I1=3)[0] == TR_E_UNSUPPORTED and fit(arr, stride=98)[0] == TR_E_UNSUPPORTED
    assert fit(arr, x=xp + 4)[0] == TR_E_UNSUPPORTED  # X not 16-byte aligned
    # nothing to do: no members, or every member at n_iters = 0 — success without a device
    assert fit(arr, n=0)[0] == 0 and grad(arr, n=0)[0] == 0 and step(arr, n=0)[0] == 0
    arr0, keep0 = _members(M, n_iters=0)
    assert fit(arr0)[0] == 0 and step(arr0)[0] == 0
    if not torch.cuda.is_available():
        rc, msg = fit(arr)  # well-formed: the failure is the missing device, reported as a HIP error
        assert rc > 0 and msg


# ---- the geometry, the packing and the table builder under sanitizers -------------------------------

def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_member_tables_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) on this machine")
    exe = str(tmp_path / "mnl_many_check")
    # the sanitizer runtimes are linked into the program itself (clang's default; asked of g++)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "mnl many ok" and run.stderr == ""


# ---- the routing of fit_Adam_many, the engine stubbed ------------------------------------------------

def host_model(X, C=5, R=2, seed=0, cls=None):
    M = _M()
    g = torch.Generator().manual_seed(seed)
    N = X.shape[0] if isinstance(X, torch.Tensor) else len(X)
    y = torch.arange(N) % C
    B0 = [torch.randn(d, R, generator=g) for d in list(X.shape[1:]) + [C]]
    return (cls or M.CP_logistic_regression)(X, y, rank=R, device="cpu", Bcp_init=B0)


@pytest.fixture
def stubbed(monkeypatch):
    """The device side replaced: _device_data hands back the host tensors, the class weights stay on the
    host, the engine call records its groups, a model's own fit_Adam records its call."""
    from tensor_regression_amd import _engine
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    M = _M()
    log = types_ns(groups=[], alone=[])

    def device_data(self):
        return 0, self.X, self.y

    def class_weights(self, weights, dev, yd):
        C = int(self.Bcp[-1].shape[0])
        cw = torch.ones(C) if weights is None else torch.as_tensor(weights, dtype=torch.float32)
        return cw, float(cw.double()[yd].sum())

    def run(dev, X, members, **kw):
        log.groups.append((X, [int(mb.n_classes) for mb in members], [mb.lambda_L2 for mb in members]))
        return [0] * len(members), 2 * max(int(mb.max_iter) for mb in members)

    def own_fit(self, **kw):
        log.alone.append((self, kw))
        return True
    monkeypatch.setattr(M.CP_logistic_regression, "_device_data", device_data)
    monkeypatch.setattr(M.CP_logistic_regression, "_class_weights", class_weights)
    monkeypatch.setattr(M.CP_logistic_regression, "fit_Adam", own_fit)
    monkeypatch.setattr(H.CP_logistic_regression, "fit_Adam", own_fit)
    monkeypatch.setattr(_engine, "run_mnl_many", run)
    return log


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


AK = {"lr": 0.01}


def test_exported():
    assert "fit_Adam_many" in _M().__all__


def test_grouping_by_x_identity_and_columns(stubbed):
    M = _M()
    Xa, Xb = torch.zeros(10, 8, 12), torch.zeros(10, 8, 12)
    ms = [host_model(Xa, seed=j) for j in range(13)] + [host_model(Xb, C=3, seed=20 + j) for j in range(2)]
    lams = [0.001 * j for j in range(15)]
    rep = {}
    out = M.fit_Adam_many(ms, lambda_L2=lams, max_iter=7, Adam_kwargs=AK, min_batch=1, report=rep)
    assert out == [False] * 15
    # 13 models of 5 classes on one X: 12 fill 60 of the 64 columns, the 13th opens a group; Xb is its own
    assert [(g[0] is Xa, g[1]) for g in stubbed.groups] == [(True, [5] * 12), (True, [5]), (False, [3, 3])]
    assert stubbed.groups[0][2] == lams[:12] and stubbed.groups[2][2] == lams[13:]
    assert rep == {"batched": list(range(15)), "alone": [], "groups": 3, "x_passes": 3 * 14}
    # the same storage seen through another tensor object groups; a view at another offset or stride does not
    stubbed.groups.clear()
    big = torch.zeros(21, 8, 12)
    ms = [host_model(big[:10], seed=1), host_model(big[:10], seed=2), host_model(big[1:11], seed=3),
          host_model(big[:20:2], seed=4)]
    M.fit_Adam_many(ms, Adam_kwargs=AK, min_batch=1, report=rep)
    assert [g[1] for g in stubbed.groups] == [[5, 5], [5], [5]] and rep["groups"] == 3
    # mixed class counts fill by columns: 16 + 16 + 16 + 10 = 58, the next 10 do not fit
    stubbed.groups.clear()
    ms = [host_model(Xa, C=c, seed=j) for j, c in enumerate([16, 16, 16, 10, 10, 2])]
    M.fit_Adam_many(ms, Adam_kwargs=AK, min_batch=1)
    assert [g[1] for g in stubbed.groups] == [[16, 16, 16, 10], [10, 2]]


def test_min_batch_and_the_switch(stubbed, monkeypatch):
    M = _M()
    Xa = torch.zeros(10, 8, 12)
    ms = [host_model(Xa, seed=j) for j in range(13)]
    rep = {}
    M.fit_Adam_many(ms, max_iter=[3] * 12 + [9], Adam_kwargs=AK, min_batch=2, report=rep)
    assert rep == {"batched": list(range(12)), "alone": [12], "groups": 1, "x_passes": 6}
    assert [(a[0] is ms[12], a[1]["max_iter"], a[1]["weights"]) for a in stubbed.alone] == [(True, 9, None)]
    # the default comes from the measured table, by the group's largest class count
    stubbed.alone.clear()
    monkeypatch.setattr(M, "MNL_MANY_MIN_BATCH", {5: 3, 10: 6, 16: None})
    assert M.mnl_many_min_batch(2) == 3 and M.mnl_many_min_batch(5) == 3 and M.mnl_many_min_batch(6) == 6
    assert M.mnl_many_min_batch(11) is None and M.mnl_many_min_batch(16) is None
    M.fit_Adam_many(ms[:3], Adam_kwargs=AK, report=rep)
    assert rep["batched"] == [0, 1, 2]
    M.fit_Adam_many(ms[:2], Adam_kwargs=AK, report=rep)
    assert rep["batched"] == [] and rep["alone"] == [0, 1]
    m16 = [host_model(Xa, C=16, seed=j) for j in range(4)]
    M.fit_Adam_many(m16, Adam_kwargs=AK, report=rep)
    assert rep["alone"] == [0, 1, 2, 3]  # a class count that never won stays with the loop by default
    M.fit_Adam_many(m16, Adam_kwargs=AK, min_batch=4, report=rep)
    assert rep["batched"] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="min_batch"):
        M.fit_Adam_many(ms, Adam_kwargs=AK, min_batch=0)
    # the switch: nothing is asked of any device
    from tensor_regression_amd import _engine

    def boom(*a, **k):
        raise AssertionError("the grouped route was taken")
    monkeypatch.setattr(_engine, "run_mnl_many", boom)
    monkeypatch.setattr(M.CP_logistic_regression, "_device_data", boom)
    monkeypatch.setenv("TR_MNL_MANY", "0")
    M.fit_Adam_many(ms, Adam_kwargs=AK, min_batch=1, report=rep)
    assert rep == {"batched": [], "alone": list(range(13)), "groups": 0, "x_passes": 0}


def test_outside_the_envelope_goes_alone(stubbed):
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    from tensor_regression_amd.util import HostStream
    from golden_util import load
    M = _M()
    Xa = torch.zeros(10, 8, 12)
    d = load("mnl_nonneg_weighted_amsgrad")
    assert tuple(d["X"].shape) == (160, 6, 5)  # P = 30 is no multiple of 4
    odd = M.CP_logistic_regression(d["X"], d["y"], rank=d["meta"]["rank"], device="cpu",
                                   Bcp_init=[torch.tensor(a) for a in d["Bcp0_list"]])
    hier = host_model(Xa, seed=5, cls=H.CP_logistic_regression)
    four_d = host_model(torch.zeros(10, 4, 2, 3), seed=6)
    r33 = host_model(Xa, R=33, seed=7)
    f64 = host_model(Xa, seed=8)
    f64.X = f64.X.double()
    hs = M.CP_logistic_regression.__new__(M.CP_logistic_regression)
    hs.__dict__.update(host_model(Xa, seed=9).__dict__)
    hs.X = HostStream.__new__(HostStream)
    inside = [host_model(Xa, seed=j) for j in range(2)]
    ms = [inside[0], odd, hier, four_d, r33, f64, hs, inside[1]]
    rep = {}
    M.fit_Adam_many(ms, Adam_kwargs=AK, min_batch=1, report=rep)
    assert rep == {"batched": [0, 7], "alone": [1, 2, 3, 4, 5, 6], "groups": 1, "x_passes": 2000}
    assert [a[0] for a in stubbed.alone] == ms[1:7]
    assert "weights" not in stubbed.alone[1][1]  # the hierarchical fit_Adam takes no class weights
    assert stubbed.alone[0][1]["weights"] is None and stubbed.alone[0][1]["verbose"] is False


def test_argument_errors(stubbed):
    M = _M()
    Xa = torch.zeros(10, 8, 12)
    a, b = host_model(Xa, seed=1), host_model(Xa, seed=2)
    assert M.fit_Adam_many([], Adam_kwargs=AK) == []
    for kw in (dict(lambda_L2=[0.1, 0.2, 0.3]), dict(max_iter=[1]), dict(tol=[0.0] * 3), dict(patience=[]),
               dict(weights=[None, None, None]), dict(weights=[np.ones(5)])):
        with pytest.raises(ValueError, match="one value per model"):
            M.fit_Adam_many([a, b], **{"Adam_kwargs": AK, **kw})
    with pytest.raises(ValueError, match="one value per model"):
        M.fit_Adam_many([a, b], Adam_kwargs=[AK])
    with pytest.raises(ValueError, match="twice"):
        M.fit_Adam_many([a, b, a], Adam_kwargs=AK)
    with pytest.raises(NotImplementedError):
        M.fit_Adam_many([a, b], Adam_kwargs=AK, verbose=2)
    with pytest.raises(TypeError):
        M.fit_Adam_many([a, b])  # Adam_kwargs=None, as fit_Adam
    with pytest.raises(TypeError, match="CP_logistic_regression"):
        M.fit_Adam_many([a, object()], Adam_kwargs=AK)
    assert stubbed.groups == [] and stubbed.alone == []
    # one class-weight vector for all models, as a list of numbers or an array; a list of vectors per model
    M.fit_Adam_many([a, b], weights=[1.0, 2.0, 1.0, 1.0, 1.0], Adam_kwargs=AK, min_batch=1)
    M.fit_Adam_many([a, b], weights=np.ones(5), Adam_kwargs=AK, min_batch=1)
    M.fit_Adam_many([a, b], weights=[np.ones(5), None], Adam_kwargs=AK, min_batch=1)
    assert len(stubbed.groups) == 3
