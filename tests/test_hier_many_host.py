"""Host-side checks of the resident sweep (fit_Adam_many / tr_fit_adam_resident_many), no GPU:

  * the Python surface: scalars and lists broadcast, every argument error raised before any device
    work, [] for no models
  * the C entry's argument checks answer without a device and name the offending member
  * the header, the library and _lib.py agree on the new symbols and on tr_resident_member's layout
  * tests/cpp/resident_many_check.cpp, the host table builder under AddressSanitizer and UBSan, built
    with the host compiler and run as a child process; nothing is preloaded
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
SRC = os.path.join(ROOT, "tests", "cpp", "resident_many_check.cpp")
TR_E_ARG, TR_E_UNSUPPORTED = -1, -2


def _H():
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    return H


def host_model(N=12, dims=(3, 4), C=3, R=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N,) + tuple(dims)).astype(np.float32)
    y = np.arange(N) % C
    return _H().CP_logistic_regression(X, y, rank=R, device="cpu")


@pytest.fixture
def no_device_work(monkeypatch):
    """Any step towards the device fails the test: the errors below must come first."""
    from tensor_regression_amd import _engine

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("compute_device", "run_resident_many", "_pack_arena", "resident_max_rows"):
        monkeypatch.setattr(_engine, name, boom)
    monkeypatch.setattr(_H().CP_logistic_regression, "_device_data", boom)
    monkeypatch.setattr(_H().CP_logistic_regression, "fit_Adam", boom)


# ---- the Python surface ----------------------------------------------------------------------------

def test_per_member_broadcast():
    H = _H()
    assert H._per_member("lambda_L2", 0.01, 3) == [0.01] * 3
    assert H._per_member("max_iter", [1, 2, 3], 3) == [1, 2, 3]
    assert H._per_member("tol", (0.0, 1e-5), 2) == [0.0, 1e-5]
    ak = {"lr": 0.1}
    assert H._per_member("Adam_kwargs", ak, 2) == [ak, ak]
    assert H._per_member("Adam_kwargs", [ak, None], 2) == [ak, None]
    # group_lr is itself a sequence: one schedule for all, or a list of one per model
    one = [0.1, [(0, 0.1), (3, 0.2)], 0.3]
    assert H._per_member("group_lr", None, 2) == [None, None]
    assert H._per_member("group_lr", one, 2) == [one, one]
    assert H._per_member("group_lr", one, 3) == [one] * 3
    assert H._per_member("group_lr", [0.1, 0.2, 0.3], 3) == [[0.1, 0.2, 0.3]] * 3
    assert H._per_member("group_lr", [None, one, None], 3) == [None, one, None]
    assert H._per_member("group_lr", [one, [0.1, 0.2, 0.3], one], 3) == [one, [0.1, 0.2, 0.3], one]
    assert H._per_member("group_lr", [one, None], 2) == [one, None]
    for name, value, M in (("lambda_L2", [0.1, 0.2], 3), ("Adam_kwargs", [ak], 2), ("group_lr", [None, None], 3),
                           ("group_lr", [one, one], 3), ("patience", [], 1)):
        with pytest.raises(ValueError):
            H._per_member(name, value, M)


def test_empty_list_returns_empty(no_device_work):
    report = {"stale": 1}
    assert _H().fit_Adam_many([], Adam_kwargs={"lr": 0.1}, report=report) == []
    assert report == {"batched": [], "alone": [], "launches": 0}
    assert _H().fit_Adam_many([]) == []


def test_argument_errors_come_before_any_device_work(no_device_work):
    H = _H()
    a, b = host_model(seed=1), host_model(seed=2)
    ak = {"lr": 0.01}
    with pytest.raises(ValueError, match="one value per model"):
        H.fit_Adam_many([a, b], lambda_L2=[0.1, 0.2, 0.3], Adam_kwargs=ak)
    with pytest.raises(ValueError, match="one value per model"):
        H.fit_Adam_many([a, b], Adam_kwargs=[ak])
    with pytest.raises(ValueError, match="twice"):
        H.fit_Adam_many([a, b, a], Adam_kwargs=ak)
    with pytest.raises(NotImplementedError):
        H.fit_Adam_many([a, b], Adam_kwargs=ak, verbose=2)
    with pytest.raises(TypeError):
        H.fit_Adam_many([a, b])  # Adam_kwargs=None, as fit_Adam
    with pytest.raises(TypeError):
        H.fit_Adam_many([a, b], Adam_kwargs=[ak, None])
    with pytest.raises(KeyError):
        H.fit_Adam_many([a, b], Adam_kwargs=[ak, {"amsgrad": True}])
    with pytest.raises(TypeError):
        H.fit_Adam_many([a, b], Adam_kwargs=[ak, {"lr": 0.1, "nesterov": True}])
    with pytest.raises(ValueError, match="exactly 3"):
        H.fit_Adam_many([a, b], Adam_kwargs=ak, group_lr=[None, [0.1, 0.2]])
    with pytest.raises(ValueError, match="start at iteration 0"):
        H.fit_Adam_many([a, b], Adam_kwargs=ak, group_lr=[0.1, [(1, 0.1)], 0.1])
    with pytest.raises(ValueError, match="strictly increase"):
        H.fit_Adam_many([a, b], Adam_kwargs=ak, group_lr=[[0.1, [(0, 0.1), (0, 0.2)], 0.1], None])
    with pytest.raises(ValueError):
        H.fit_Adam_many([a, b], Adam_kwargs=[ak, {"lr": -1.0}])
    with pytest.raises(TypeError):
        H.fit_Adam_many([a, object()], Adam_kwargs=ak)
    assert a.loss_running == [] and b.loss_running == []


def test_models_on_different_devices(monkeypatch):
    H = _H()
    from tensor_regression_amd import _engine
    a, b = host_model(seed=1), host_model(seed=2)
    a.device, b.device = "cuda:0", "cuda:1"  # (X on the host: the model's device decides)

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(_engine, "run_resident_many", boom)
    monkeypatch.setattr(H.CP_logistic_regression, "_device_data", boom)
    monkeypatch.setattr(H.CP_logistic_regression, "fit_Adam", boom)
    with pytest.raises(ValueError, match="different devices"):
        H.fit_Adam_many([a, b], Adam_kwargs={"lr": 0.01})


# ---- the C entry ----------------------------------------------------------------------------------

def _members(lib, shapes, n_iters=4):
    """Well-formed members over host memory (the checks never dereference a buffer); returns the
    ctypes array and the objects that keep the memory alive."""
    from tensor_regression_amd import _lib
    arr = (_lib.ResidentMember * len(shapes))()
    keep = []
    for r, (N, I0, I1, C, R) in zip(arr, shapes):
        buf = (ctypes.c_double * 8)()
        keep.append(buf)
        p = ctypes.addressof(buf)
        for f in ("X", "target", "params", "weights", "exp_avg", "exp_avg_sq", "loss_hist", "stop_flag"):
            setattr(r, f, p)
        r.n_rows, r.I0, r.I1, r.n_classes, r.rank = N, I0, I1, C, R
        r.softplus_beta, r.softplus_threshold, r.lambda_l2 = 50.0, 1.0, 0.01
        r.n_iters, r.step = n_iters, 1
        r.lr[0] = r.lr[1] = r.lr[2] = 0.01
        r.beta1, r.beta2, r.eps = 0.9, 0.999, 1e-8
        r.patience = 10
    return arr, keep


def test_c_entry_checks_every_member_without_a_device():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    nmax = int(lib.tr_mnl_resident_max_rows(8, 12, 4, 6))
    assert nmax >= 227
    shapes = [(1, 2, 3, 2, 1), (40, 8, 12, 4, 6), (nmax, 8, 12, 4, 6)]
    nbytes = int(lib.tr_resident_member_table_bytes(len(shapes)))
    assert nbytes > 0 and nbytes % len(shapes) == 0 and lib.tr_resident_member_table_bytes(0) == 0
    assert lib.tr_resident_member_table_bytes(6) == 2 * nbytes
    host = (ctypes.c_char * nbytes)()
    devb = (ctypes.c_char * nbytes)()  # never touched: every call below fails its checks first

    def call(arr, n=len(shapes), th=host, td=devb, nb=nbytes):
        rc = lib.tr_fit_adam_resident_many(0, arr, n, th, td, nb, None)
        return rc, (lib.tr_last_error() or b"").decode()

    def spoiled(at, **fields):
        arr, keep = _members(lib, shapes)
        for k, v in fields.items():
            if k == "lr1":
                arr[at].lr[1] = v
            else:
                setattr(arr[at], k, v)
        return arr, keep

    for at, code, fields in [
        (1, TR_E_ARG, dict(n_iters=65)), (0, TR_E_ARG, dict(n_iters=-1)), (2, TR_E_ARG, dict(X=None)),
        (1, TR_E_ARG, dict(stop_flag=None)), (0, TR_E_ARG, dict(loss_hist=None)), (2, TR_E_ARG, dict(amsgrad=1)),
        (1, TR_E_ARG, dict(n_rows=0)), (0, TR_E_ARG, dict(step=0)), (2, TR_E_ARG, dict(lr1=-0.5)),
        (1, TR_E_ARG, dict(lr1=float("nan"))), (0, TR_E_ARG, dict(hist_base=-1)),
        (2, TR_E_UNSUPPORTED, dict(n_rows=nmax + 1)),  # one row past the envelope
        (0, TR_E_UNSUPPORTED, dict(n_classes=17)), (1, TR_E_UNSUPPORTED, dict(rank=17)),
    ]:
        arr, keep = spoiled(at, **fields)
        rc, msg = call(arr)
        assert rc == code, (at, fields, rc, msg)
        assert msg.startswith(f"member {at}:"), (fields, msg)
    # a bad member behind good ones is found although the first members are fine; the first bad one is named
    arr, keep = spoiled(2, n_iters=99)
    arr[1].step = 0
    assert call(arr)[1].startswith("member 1:")
    # the call's own arguments
    arr, keep = _members(lib, shapes)
    assert call(arr, n=-1)[0] == TR_E_ARG
    assert call(None)[0] == TR_E_ARG
    assert call(arr, th=None)[0] == TR_E_ARG and call(arr, td=None)[0] == TR_E_ARG
    rc, msg = call(arr, nb=nbytes - 1)
    assert rc == TR_E_ARG and "tr_resident_member_table_bytes" in msg
    # nothing to do: no members, or every member at n_iters = 0 — success without a device
    assert call(arr, n=0)[0] == 0
    arr0, keep0 = _members(lib, shapes, n_iters=0)
    assert call(arr0)[0] == 0
    if not torch.cuda.is_available():
        rc, msg = call(arr)  # well-formed: the failure is the missing device, reported as a HIP error
        assert rc > 0 and msg


# ---- symbols and the struct's layout --------------------------------------------------------------

C_TYPES = {"const float*": (ctypes.c_void_p, 8), "const void*": (ctypes.c_void_p, 8), "float*": (ctypes.c_void_p, 8),
           "double*": (ctypes.c_void_p, 8), "int32_t*": (ctypes.c_void_p, 8), "int64_t": (ctypes.c_int64, 8),
           "int32_t": (ctypes.c_int32, 4), "float": (ctypes.c_float, 4), "double": (ctypes.c_double, 8)}


def header_struct_fields():
    """[(name, ctype, count)] of tr_resident_member, parsed from the header."""
    txt = open(HEADER).read()
    body = re.search(r"typedef struct tr_resident_member \{(.*?)\} tr_resident_member;", txt, flags=re.S).group(1)
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
    for s in ("tr_fit_adam_resident_many", "tr_resident_member_table_bytes"):
        assert re.search(r"^\s*(?:int|int64_t)\s+" + s + r"\s*\(", txt, flags=re.M), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.SIGNATURES["tr_resident_member_table_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["tr_fit_adam_resident_many"][1][1]._type_ is _lib.ResidentMember
    assert lib.tr_abi_version() == _lib.TR_ABI_VERSION == 9
    assert re.search(r"#define TR_ABI_VERSION 9\b", txt)
    fields = header_struct_fields()
    assert [f[0] for f in fields] == [f[0] for f in _lib.ResidentMember._fields_]
    off = 0
    for (name, ctype, count), (pname, ptype) in zip(fields, _lib.ResidentMember._fields_):
        base, size = C_TYPES[ctype]
        want = base * count if count > 1 else base
        assert ctypes.sizeof(ptype) == ctypes.sizeof(want) == size * count, name
        if count == 1:
            assert ptype is base, name
        else:
            assert ptype._type_ is base and ptype._length_ == count, name
        off = -(-off // size) * size  # the C compiler's natural alignment
        assert getattr(_lib.ResidentMember, name).offset == off, (name, off)
        off += size * count
    assert ctypes.sizeof(_lib.ResidentMember) == -(-off // 8) * 8 == 240
    assert np.dtype(_lib.ResidentMember).itemsize == 240


# ---- the table builder under sanitizers -----------------------------------------------------------

def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_member_tables_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) on this machine")
    exe = str(tmp_path / "resident_many_check")
    # the sanitizer runtimes are linked into the program itself (clang's default; asked of g++)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "resident many ok" and run.stderr == ""
