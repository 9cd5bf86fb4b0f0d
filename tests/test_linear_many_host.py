"""Host-side checks of the shared-X linear sweep (standard_tensor_regression.fit_Adam_many and the
tr_linear_many_* entries), no GPU:

  * the Python surface: scalars and lists broadcast, every argument error raised before any device
    work, [] for no models, verbose=2, a model of another class, feature dims that differ from X
  * tr_linear_many_envelope on its edges, and a 4-D X refused by Python's routing
  * the C entries' argument checks answer without a device and name the offending member; 17 members
    are refused, 0 accepted
  * the header, the library and _lib.py agree on the new symbols and on tr_linear_member's layout
  * tests/cpp/linear_many_check.cpp, the geometry and the table builder under AddressSanitizer and
    UBSan, built with the host compiler and run as a child process; nothing is preloaded
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
SRC = os.path.join(ROOT, "tests", "cpp", "linear_many_check.cpp")
TR_E_ARG, TR_E_UNSUPPORTED = -1, -2


def _S():
    from tensor_regression_amd import standard_tensor_regression as S
    return S


def host_model(dims=(8, 12), R=2, seed=0, N=10):
    torch.manual_seed(seed)
    return _S().CP_linear_regression((N,) + tuple(dims), rank=R, device="cpu")


@pytest.fixture
def no_device_work(monkeypatch):
    """Any step towards the device fails the test: the errors below must come first."""
    from tensor_regression_amd import _engine

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("compute_device", "run_linear_many", "_pack_arena", "as_device_rows", "linear_many_envelope"):
        monkeypatch.setattr(_engine, name, boom)
    monkeypatch.setattr(_S(), "as_device_f32", boom)
    monkeypatch.setattr(_S().CP_linear_regression, "fit_Adam", boom)


# ---- the Python surface ----------------------------------------------------------------------------

def test_exported():
    import tensor_regression_amd as T
    assert "fit_Adam_many" in _S().__all__ and T.fit_Adam_many is _S().fit_Adam_many


def test_per_member_broadcast():
    S = _S()
    assert S._per_member("lambda_L2", 0.01, 3) == [0.01] * 3
    assert S._per_member("max_iter", [1, 2, 3], 3) == [1, 2, 3]
    assert S._per_member("tol", (0.0, 1e-5), 2) == [0.0, 1e-5]
    ak = {"lr": 0.1}
    assert S._per_member("Adam_kwargs", ak, 2) == [ak, ak]
    assert S._per_member("Adam_kwargs", [ak, None], 2) == [ak, None]
    for name, value, M in (("lambda_L2", [0.1, 0.2], 3), ("Adam_kwargs", [ak], 2), ("patience", [], 1)):
        with pytest.raises(ValueError, match="one value per model"):
            S._per_member(name, value, M)
    y = torch.zeros(5)
    assert S._targets(y, 3) == ([y, y, y], True)
    ys, shared = S._targets([y, y + 1], 2)
    assert not shared and len(ys) == 2
    assert S._targets([0.0, 1.0, 2.0], 2)[1]  # a plain list of numbers is one target
    with pytest.raises(ValueError, match="one target per model"):
        S._targets([y, y], 3)


def test_empty_list_returns_empty(no_device_work):
    report = {"stale": 1}
    assert _S().fit_Adam_many([], None, None, Adam_kwargs={"lr": 0.1}, report=report) == []
    assert report == {"batched": [], "alone": [], "groups": 0, "x_passes": 0}
    assert _S().fit_Adam_many([], torch.zeros(4, 8, 12), torch.zeros(4)) == []


def test_argument_errors_come_before_any_device_work(no_device_work):
    S = _S()
    a, b = host_model(seed=1), host_model(seed=2)
    X, y = torch.zeros(10, 8, 12), torch.zeros(10)
    ak = {"lr": 0.01}
    with pytest.raises(ValueError, match="one value per model"):
        S.fit_Adam_many([a, b], X, y, lambda_L2=[0.1, 0.2, 0.3], Adam_kwargs=ak)
    with pytest.raises(ValueError, match="one value per model"):
        S.fit_Adam_many([a, b], X, y, Adam_kwargs=[ak])
    with pytest.raises(ValueError, match="one target per model"):
        S.fit_Adam_many([a, b], X, [y, y, y], Adam_kwargs=ak)
    with pytest.raises(ValueError, match="twice"):
        S.fit_Adam_many([a, b, a], X, y, Adam_kwargs=ak)
    with pytest.raises(NotImplementedError):
        S.fit_Adam_many([a, b], X, y, Adam_kwargs=ak, verbose=2)
    with pytest.raises(TypeError):
        S.fit_Adam_many([a, b], X, y)  # Adam_kwargs=None, as fit_Adam
    with pytest.raises(TypeError):
        S.fit_Adam_many([a, b], X, y, Adam_kwargs=[ak, None])
    with pytest.raises(TypeError):
        S.fit_Adam_many([a, b], X, y, Adam_kwargs=[ak, {"lr": 0.1, "nesterov": True}])
    with pytest.raises(ValueError):
        S.fit_Adam_many([a, b], X, y, Adam_kwargs=[ak, {"lr": -1.0}])
    with pytest.raises(TypeError, match="CP_linear_regression"):
        S.fit_Adam_many([a, object()], X, y, Adam_kwargs=ak)
    from tensor_regression_amd.spectral_tensor_regression import CP_linear_regression as Spectral
    other = Spectral((10, 8, 12), (10, 2), rank_normal=1, rank_spectral=1, n_complex_dim=1, device="cpu")
    with pytest.raises(TypeError, match="CP_linear_regression"):
        S.fit_Adam_many([a, other], X, y, Adam_kwargs=ak)
    with pytest.raises(ValueError, match="model 1: Incorrect shapes"):  # feature dims that differ from X
        S.fit_Adam_many([a, host_model(dims=(8, 4))], X, y, Adam_kwargs=ak)
    with pytest.raises(ValueError, match="model 0: Incorrect shapes"):
        S.fit_Adam_many([a, b], torch.zeros(10, 8, 12, 2), y, Adam_kwargs=ak)
    with pytest.raises(ValueError, match="len\\(y\\) == X.shape\\[0\\]"):
        S.fit_Adam_many([a, b], X, torch.zeros(9), Adam_kwargs=ak)
    with pytest.raises(ValueError, match="y\\[1\\] must be 1-D"):
        S.fit_Adam_many([a, b], X, [y, torch.zeros(10, 1)], Adam_kwargs=ak)
    with pytest.raises(ValueError, match="min_batch"):
        S.fit_Adam_many([a, b], X, y, Adam_kwargs=ak, min_batch=0)
    with pytest.raises(TypeError, match="torch tensor"):
        S.fit_Adam_many([a, b], np.zeros((10, 8, 12), np.float32), y, Adam_kwargs=ak)
    assert a.loss_running == [] and b.loss_running == [] and a._plan is None


def test_routing_without_a_device(monkeypatch):
    """What goes alone is decided on the host: a 4-D X, a float64 X, TR_LINEAR_MANY=0 and a group
    below min_batch reach the models' own fit_Adam and nothing else."""
    S = _S()
    from tensor_regression_amd import _engine
    calls = []

    def fake_fit(self, X, y, **kw):
        calls.append((self, kw["max_iter"]))
        return True

    def boom(*a, **k):
        raise AssertionError("the grouped route was taken")
    monkeypatch.setattr(S.CP_linear_regression, "fit_Adam", fake_fit)
    monkeypatch.setattr(_engine, "run_linear_many", boom)
    ak = {"lr": 0.01}
    # 4-D X: never grouped, whatever the envelope says of its leading dims
    torch.manual_seed(0)
    m4 = [S.CP_linear_regression((6, 4, 2, 4), rank=2, device="cpu") for _ in range(2)]
    rep = {}
    assert S.fit_Adam_many(m4, torch.zeros(6, 4, 2, 4), torch.zeros(6), max_iter=[3, 4], Adam_kwargs=ak, min_batch=1,
                           report=rep) == [True, True]
    assert rep == {"batched": [], "alone": [0, 1], "groups": 0, "x_passes": 0}
    assert calls == [(m4[0], 3), (m4[1], 4)]
    # float64
    m64 = [S.CP_linear_regression((6, 8, 12), rank=2, device="cpu", dtype=torch.float64)]
    S.fit_Adam_many(m64, torch.zeros(6, 8, 12, dtype=torch.float64), torch.zeros(6), Adam_kwargs=ak, min_batch=1,
                    report=rep)
    assert rep["alone"] == [0] and rep["groups"] == 0
    # the switch: no device is asked for anything
    monkeypatch.setattr(_engine, "compute_device", boom)
    monkeypatch.setenv("TR_LINEAR_MANY", "0")
    ms = [host_model(seed=3), host_model(seed=4)]
    S.fit_Adam_many(ms, torch.zeros(10, 8, 12), torch.zeros(10), Adam_kwargs=ak, min_batch=1, report=rep)
    assert rep == {"batched": [], "alone": [0, 1], "groups": 0, "x_passes": 0}
    assert S.LINEAR_MANY_MIN_BATCH >= 1


# ---- the envelope ----------------------------------------------------------------------------------

def test_envelope_edges():
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    env = lib.tr_linear_many_envelope
    assert env(8, 12, 0, 32) == 1 and env(8, 12, 0, 33) == 0 and env(8, 12, 0, 0) == 0  # rank 32 against 33
    assert env(3, 3, 0, 2) == 0 and env(3, 4, 0, 2) == 1          # P % 4
    assert env(8, 12, 98, 2) == 0 and env(8, 12, 100, 2) == 1     # stride % 4
    assert env(9, 12, 12, 2) == 1                                 # stride < P: a windowed view
    assert env(8, 12, -4, 2) == 0 and env(0, 12, 0, 2) == 0
    assert _engine.linear_many_envelope(256, 128, 256 * 128, 8) and not _engine.linear_many_envelope(5, 5, 25, 8)
    ws = lib.tr_linear_many_workspace_bytes
    assert ws(2000, 500, 500, 16) > 2 * 16 * 250000 * 4 and ws(2000, 500, 500, 16) == ws(2000, 500, 500, 1)
    assert ws(10, 3, 3, 2) == 0 and ws(0, 8, 12, 2) == 0 and ws(10, 8, 12, 17) == 0
    assert ws(3, 8, 4, 1) % 256 == 0


# ---- the C entries ----------------------------------------------------------------------------------

def _members(n, n_iters=1):
    """Well-formed members over host memory (the checks never dereference a buffer)."""
    from tensor_regression_amd import _lib
    arr = (_lib.LinearMember * n)()
    keep = []
    for j, r in enumerate(arr):
        buf = (ctypes.c_double * 8)()
        keep.append(buf)
        p = ctypes.addressof(buf)
        for f in ("params", "weights", "y", "exp_avg", "exp_avg_sq", "grad", "loss_hist", "stop_flag"):
            setattr(r, f, p)
        r.rank = (1, 3, 8, 32)[j % 4]
        r.softplus_beta, r.softplus_threshold, r.lambda_l2 = 50.0, 1.0, 0.01
        r.n_iters, r.step = n_iters, 1
        r.lr, r.beta1, r.beta2, r.eps = 0.01, 0.9, 0.999, 1e-8
        r.patience = 10
    return arr, keep


def test_c_entries_check_every_member_without_a_device():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    M = 3
    nbytes = int(lib.tr_linear_member_table_bytes(M))
    assert nbytes > 0 and nbytes % M == 0 and lib.tr_linear_member_table_bytes(0) == 0
    assert lib.tr_linear_member_table_bytes(6) == 2 * nbytes
    big = int(lib.tr_linear_member_table_bytes(17))
    host = (ctypes.c_char * big)()
    devb = (ctypes.c_char * big)()  # never touched: every call below fails its checks first
    wsb = int(lib.tr_linear_many_workspace_bytes(10, 8, 12, M))
    X = (ctypes.c_char * 4096)()
    xp = (ctypes.addressof(X) + 255) // 256 * 256  # aligned stand-ins for X and the workspace

    def fit(arr, n=M, I0=8, I1=12, stride=0, th=host, td=devb, nb=big, x=xp, ws=xp, wb=wsb, rows=10):
        rc = lib.tr_linear_many_fit(0, x, rows, stride, I0, I1, arr, n, ws, wb, th, td, nb, None)
        return rc, (lib.tr_last_error() or b"").decode()

    def grad(arr, n=M):
        rc = lib.tr_linear_many_loss_grad(0, xp, 10, 0, 8, 12, arr, n, xp, wsb, host, devb, big, None)
        return rc, (lib.tr_last_error() or b"").decode()

    def step(arr, n=M):
        rc = lib.tr_linear_many_step(0, 8, 12, arr, n, host, devb, big, None)
        return rc, (lib.tr_last_error() or b"").decode()

    for at, code, fields in [
        (1, TR_E_ARG, dict(n_iters=65)), (0, TR_E_ARG, dict(n_iters=-1)), (2, TR_E_ARG, dict(params=None)),
        (1, TR_E_ARG, dict(stop_flag=None)), (0, TR_E_ARG, dict(loss_hist=None)), (2, TR_E_ARG, dict(amsgrad=1)),
        (1, TR_E_ARG, dict(y=None)), (0, TR_E_ARG, dict(step=0)), (2, TR_E_ARG, dict(lr=-0.5)),
        (1, TR_E_ARG, dict(lr=float("nan"))), (0, TR_E_ARG, dict(hist_base=-1)), (2, TR_E_ARG, dict(grad=None)),
        (0, TR_E_UNSUPPORTED, dict(rank=33)), (1, TR_E_UNSUPPORTED, dict(rank=0)),
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
    arr[1].rank = 33
    assert grad(arr) == (TR_E_UNSUPPORTED, "member 1: rank outside 1..32") and step(arr)[0] == TR_E_UNSUPPORTED
    # the call's own arguments
    arr, keep = _members(M)
    assert fit(arr, n=-1)[0] == TR_E_ARG and fit(None)[0] == TR_E_ARG
    arr17, keep17 = _members(17)
    rc, msg = fit(arr17, n=17)
    assert rc == TR_E_ARG and "16" in msg
    assert grad(arr17, n=17)[0] == TR_E_ARG and step(arr17, n=17)[0] == TR_E_ARG
    assert fit(arr, th=None)[0] == TR_E_ARG and fit(arr, td=None)[0] == TR_E_ARG
    rc, msg = fit(arr, nb=nbytes - 1)
    assert rc == TR_E_ARG and "tr_linear_member_table_bytes" in msg
    assert fit(arr, x=None)[0] == TR_E_ARG and fit(arr, ws=None)[0] == TR_E_ARG
    rc, msg = fit(arr, wb=wsb - 1)
    assert rc == TR_E_ARG and "tr_linear_many_workspace_bytes" in msg
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


# ---- symbols and the struct's layout --------------------------------------------------------------

C_TYPES = {"const float*": (ctypes.c_void_p, 8), "float*": (ctypes.c_void_p, 8), "double*": (ctypes.c_void_p, 8),
           "int32_t*": (ctypes.c_void_p, 8), "int64_t": (ctypes.c_int64, 8), "int32_t": (ctypes.c_int32, 4),
           "float": (ctypes.c_float, 4), "double": (ctypes.c_double, 8)}


def header_struct_fields():
    """[(name, ctype, count)] of tr_linear_member, parsed from the header."""
    txt = open(HEADER).read()
    body = re.search(r"typedef struct tr_linear_member \{(.*?)\} tr_linear_member;", txt, flags=re.S).group(1)
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
    for s in ("tr_linear_many_envelope", "tr_linear_many_workspace_bytes", "tr_linear_member_table_bytes",
              "tr_linear_many_loss_grad", "tr_linear_many_step", "tr_linear_many_fit"):
        assert re.search(r"^\s*(?:int|int64_t)\s+" + s + r"\s*\(", txt, flags=re.M), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.SIGNATURES["tr_linear_member_table_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["tr_linear_many_workspace_bytes"][0] is ctypes.c_int64
    for s, at in (("tr_linear_many_loss_grad", 6), ("tr_linear_many_fit", 6), ("tr_linear_many_step", 3)):
        assert _lib.SIGNATURES[s][1][at]._type_ is _lib.LinearMember
    assert lib.tr_abi_version() == _lib.TR_ABI_VERSION == 9
    fields = header_struct_fields()
    assert [f[0] for f in fields] == [f[0] for f in _lib.LinearMember._fields_]
    off = 0
    for (name, ctype, count), (pname, ptype) in zip(fields, _lib.LinearMember._fields_):
        base, size = C_TYPES[ctype]
        want = base * count if count > 1 else base
        assert ctypes.sizeof(ptype) == ctypes.sizeof(want) == size * count, name
        if count == 1:
            assert ptype is base, name
        else:
            assert ptype._type_ is base and ptype._length_ == count, name
        off = -(-off // size) * size  # the C compiler's natural alignment
        assert getattr(_lib.LinearMember, name).offset == off, (name, off)
        off += size * count
    assert ctypes.sizeof(_lib.LinearMember) == -(-off // 8) * 8 == 184
    assert np.dtype(_lib.LinearMember).itemsize == 184


# ---- the geometry and the table builder under sanitizers --------------------------------------------

def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_member_tables_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) on this machine")
    exe = str(tmp_path / "linear_many_check")
    # the sanitizer runtimes are linked into the program itself (clang's default; asked of g++)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "linear many ok" and run.stderr == ""
