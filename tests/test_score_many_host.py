"""Host-side checks of the scoring sweep (predict_many / score_many / tr_mnl_score_many), no GPU:

  * the header, the library and _lib.py agree on the new symbols and on tr_score_member's layout; the
    ABI version stays 9
  * tr_mnl_score_envelope contains the resident fit's envelope and ends where it says
  * the C entry's argument checks answer without a device and name the offending member
  * the Python surface: every argument error raised before any device work, [] for no entries
  * tests/cpp/score_many_check.cpp, the geometry and the table builder under AddressSanitizer and UBSan,
    built with the host compiler and run as a child process; nothing is preloaded
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
SRC = os.path.join(ROOT, "tests", "cpp", "score_many_check.cpp")
TR_E_ARG, TR_E_UNSUPPORTED = -1, -2
NEW_SYMBOLS = ("tr_mnl_score_envelope", "tr_score_member_table_bytes", "tr_mnl_score_many")


def _M():
    from tensor_regression_amd import multinomial_tensor_regression as M
    return M


def _H():
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    return H


def host_model(mod=None, N=12, dims=(3, 4), C=3, R=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N,) + tuple(dims)).astype(np.float32)
    y = np.arange(N) % C
    return (mod or _M()).CP_logistic_regression(X, y, rank=R, device="cpu")


@pytest.fixture
def no_device_work(monkeypatch):
    """Any step towards the device fails the test: the errors below must come first."""
    from tensor_regression_amd import _engine

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("compute_device", "run_score_many", "upload_packed", "_pack_arena", "score_envelope",
                 "as_device_rows"):
        monkeypatch.setattr(_engine, name, boom)
    for mod in (_M(), _H()):
        monkeypatch.setattr(mod.CP_logistic_regression, "_device_data", boom)
        monkeypatch.setattr(mod.CP_logistic_regression, "predict", boom)


# ---- symbols and the struct's layout --------------------------------------------------------------

C_TYPES = {"const float*": (ctypes.c_void_p, 8), "const void*": (ctypes.c_void_p, 8), "float*": (ctypes.c_void_p, 8),
           "double*": (ctypes.c_void_p, 8), "int32_t*": (ctypes.c_void_p, 8), "int64_t*": (ctypes.c_void_p, 8),
           "int64_t": (ctypes.c_int64, 8), "int32_t": (ctypes.c_int32, 4), "float": (ctypes.c_float, 4),
           "double": (ctypes.c_double, 8)}


def header_struct_fields(name):
    """[(name, ctype, count)] of a struct of the header, parsed from its text."""
    txt = open(HEADER).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", txt, flags=re.S).group(1)
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


def test_new_symbols_are_in_the_header_the_library_and_signatures():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    txt = open(HEADER).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"^\s*(?:int|int64_t)\s+" + s + r"\s*\(", txt, flags=re.M), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.SIGNATURES["tr_score_member_table_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["tr_mnl_score_envelope"][0] is ctypes.c_int
    assert _lib.SIGNATURES["tr_mnl_score_many"][1][1]._type_ is _lib.ScoreMember
    assert lib.tr_abi_version() == _lib.TR_ABI_VERSION == 9
    assert re.search(r"#define TR_ABI_VERSION 9\b", txt)
    block = int(re.search(r"#define TR_SCORE_ROW_BLOCK (\d+)\b", txt).group(1))
    from tensor_regression_amd import _engine
    assert _engine.SCORE_ROW_BLOCK == _lib.TR_SCORE_ROW_BLOCK == block


def test_score_member_layout_agrees_with_the_header():
    from tensor_regression_amd import _lib
    fields = header_struct_fields("tr_score_member")
    assert [f[0] for f in fields] == [f[0] for f in _lib.ScoreMember._fields_]
    for want in ("X", "target", "params", "weights", "class_weights", "prob", "pred", "counts", "loss", "n_rows",
                 "x_row_stride", "I0", "I1", "n_classes", "rank", "nonneg", "softplus_beta", "softplus_threshold"):
        assert want in [f[0] for f in fields], want
    off = 0
    for (name, ctype, count), (pname, ptype) in zip(fields, _lib.ScoreMember._fields_):
        base, size = C_TYPES[ctype]
        want = base * count if count > 1 else base
        assert ctypes.sizeof(ptype) == ctypes.sizeof(want) == size * count, name
        if count == 1:
            assert ptype is base, name
        else:
            assert ptype._type_ is base and ptype._length_ == count, name
        off = -(-off // size) * size  # the C compiler's natural alignment
        assert getattr(_lib.ScoreMember, name).offset == off, (name, off)
        off += size * count
    assert ctypes.sizeof(_lib.ScoreMember) == -(-off // 8) * 8
    # the resident sweep's struct is as it was
    assert ctypes.sizeof(_lib.ResidentMember) == 240


# ---- the envelope ---------------------------------------------------------------------------------

def _largest_i1(fn, I0, C, R):
    """The largest I1 for which fn(I0, I1, C, R) holds (0: none), by bisection."""
    if not fn(I0, 1, C, R):
        return 0
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fn(I0, mid, C, R) else (lo, mid - 1)
    return lo


def test_envelope_contains_the_resident_envelope():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    res = lambda I0, I1, C, R: lib.tr_mnl_resident_max_rows(I0, I1, C, R) >= 1
    env = lambda I0, I1, C, R: lib.tr_mnl_score_envelope(I0, I1, C, R) == 1
    n_res = 0
    for I0 in (1, 2, 3, 8, 33, 64, 257):
        for I1 in (1, 2, 5, 12, 40, 100, 513):
            for C in (1, 2, 4, 16):
                for R in (1, 6, 16):
                    if res(I0, I1, C, R):
                        n_res += 1
                        assert env(I0, I1, C, R), (I0, I1, C, R)
    assert n_res > 100
    assert res(8, 12, 16, 16) and env(8, 12, 16, 16)
    for I0, C, R in ((1, 16, 16), (1, 16, 1), (8, 4, 6), (7, 1, 1), (64, 16, 16)):
        top = _largest_i1(res, I0, C, R)  # the largest P C the resident route admits along this line
        assert top >= 1 and env(I0, top, C, R) and env(I0, top + 1, C, R), (I0, C, R, top)
        assert _largest_i1(env, I0, C, R) > top


def test_envelope_ends_where_it_says():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    env = lambda I0, I1, C, R: lib.tr_mnl_score_envelope(I0, I1, C, R) == 1
    assert env(8, 12, 4, 6) and env(1, 1, 1, 1) and env(8, 12, 16, 16)
    assert not env(8, 12, 17, 6) and not env(8, 12, 4, 17)
    assert not env(8, 12, 0, 6) and not env(8, 12, 4, 0) and not env(0, 12, 4, 6) and not env(8, -1, 4, 6)
    assert not env(1024, 1024, 4, 6)                    # P C = 4 Mi words
    top = _largest_i1(env, 2, 16, 1)
    assert top >= 1 and not env(2, top + 1, 16, 1)
    words = 2 * top * 16                                # the dense P x C image alone
    assert 160 * 1024 - 8192 < 4 * words <= 160 * 1024  # it fills the CU's LDS to within the fixed pieces


# ---- the C entry ----------------------------------------------------------------------------------

def _members(shapes):
    """Well-formed members over host memory (the checks never dereference a buffer); returns the
    ctypes array and the objects that keep the memory alive."""
    from tensor_regression_amd import _lib
    arr = (_lib.ScoreMember * len(shapes))()
    keep = []
    for r, (N, I0, I1, C, R) in zip(arr, shapes):
        buf = (ctypes.c_double * 8)()
        keep.append(buf)
        p = ctypes.addressof(buf)
        for f in ("X", "target", "params", "weights", "class_weights", "prob", "pred", "counts", "loss",
                  "loss_parts"):
            setattr(r, f, p)
        r.n_rows, r.I0, r.I1, r.n_classes, r.rank = N, I0, I1, C, R
        r.softplus_beta, r.softplus_threshold = 50.0, 1.0
    return arr, keep


def test_c_entry_checks_every_member_without_a_device():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    shapes = [(1, 2, 3, 2, 1), (227, 8, 12, 4, 6), (100000, 8, 12, 16, 16)]
    nbytes = int(lib.tr_score_member_table_bytes(len(shapes)))
    assert nbytes > 0 and nbytes % len(shapes) == 0 and lib.tr_score_member_table_bytes(0) == 0
    assert lib.tr_score_member_table_bytes(6) == 2 * nbytes
    host = (ctypes.c_char * nbytes)()
    devb = (ctypes.c_char * nbytes)()  # never touched: every call below fails its checks first

    def call(arr, n=len(shapes), th=host, td=devb, nb=nbytes):
        rc = lib.tr_mnl_score_many(0, arr, n, th, td, nb, None)
        return rc, (lib.tr_last_error() or b"").decode()

    def spoiled(at, **fields):
        arr, keep = _members(shapes)
        for k, v in fields.items():
            setattr(arr[at], k, v)
        return arr, keep

    for at, code, fields in [
        (1, TR_E_ARG, dict(X=None)), (0, TR_E_ARG, dict(params=None)), (2, TR_E_ARG, dict(weights=None)),
        (1, TR_E_ARG, dict(n_rows=0)), (0, TR_E_ARG, dict(n_rows=-3)), (2, TR_E_ARG, dict(x_row_stride=-1)),
        (1, TR_E_ARG, dict(target=None, loss=None)),    # counts without target
        (0, TR_E_ARG, dict(target=None, counts=None)),  # loss without target
        (2, TR_E_ARG, dict(loss_parts=None)),
        (0, TR_E_UNSUPPORTED, dict(n_classes=17)), (1, TR_E_UNSUPPORTED, dict(rank=17)),
        (2, TR_E_UNSUPPORTED, dict(I0=1024, I1=1024)), (1, TR_E_UNSUPPORTED, dict(n_classes=0)),
    ]:
        arr, keep = spoiled(at, **fields)
        rc, msg = call(arr)
        assert rc == code, (at, fields, rc, msg)
        assert msg.startswith(f"member {at}:"), (fields, msg)
    # a bad member behind good ones is found; the first bad one is named
    arr, keep = spoiled(2, rank=99)
    arr[1].n_rows = 0
    assert call(arr)[1].startswith("member 1:")
    # the call's own arguments
    arr, keep = _members(shapes)
    assert call(arr, n=-1)[0] == TR_E_ARG
    assert call(None)[0] == TR_E_ARG
    assert call(arr, th=None)[0] == TR_E_ARG and call(arr, td=None)[0] == TR_E_ARG
    rc, msg = call(arr, nb=nbytes - 1)
    assert rc == TR_E_ARG and "tr_score_member_table_bytes" in msg
    assert call(arr, n=0)[0] == 0  # nothing to do: success without a device
    if not torch.cuda.is_available():
        rc, msg = call(arr)  # well-formed: the failure is the missing device, reported as a HIP error
        assert rc > 0 and msg


# ---- the Python surface ---------------------------------------------------------------------------

def test_empty_list_returns_empty(no_device_work):
    for mod in (_M(), _H()):
        report = {"stale": 1}
        assert mod.score_many([], report=report) == []
        assert report == {"batched": [], "alone": [], "launches": 0}
        assert mod.predict_many([]) == [] and mod.score_many([]) == []
        assert "score_many" in mod.__all__ and "predict_many" in mod.__all__
    assert _H().score_many is _M().score_many and _H().predict_many is _M().predict_many


def test_argument_errors_come_before_any_device_work(no_device_work):
    M = _M()
    a, b = host_model(seed=1), host_model(_H(), seed=2)  # the two modules' models may be mixed
    X = np.zeros((5, 3, 4), dtype=np.float32)
    y = np.array([0, 1, 2, 0, 1])
    for fn in (M.score_many, M.predict_many):
        with pytest.raises(ValueError, match="one entry per model"):
            fn([a, b], X=[X])
        with pytest.raises(ValueError, match="one entry per model"):
            fn([a, b], X=[X, None, X])
        with pytest.raises(ValueError, match="must be None or a list"):
            fn([a, b], X=X)
        with pytest.raises(ValueError, match="Incorrect shapes for inner product along 2 common modes"):
            fn([a, b], X=[None, np.zeros((5, 4, 3), dtype=np.float32)])
        with pytest.raises(ValueError, match="Incorrect shapes for inner product along 2 common modes"):
            fn([a, a], X=[None, np.zeros((5, 3, 4, 2), dtype=np.float32)])
        with pytest.raises(TypeError):
            fn([a, object()])
    with pytest.raises(ValueError, match="one entry per model"):
        M.score_many([a, b], X=[X, X], y_true=[y])
    with pytest.raises(ValueError, match="one entry per model"):
        M.predict_many([a, b], Bcp=[None])
    with pytest.raises(ValueError, match="5 samples and 4 labels"):
        M.score_many([a, b], X=[X, None], y_true=[y[:4], None])
    with pytest.raises(IndexError, match="Target 3 is out of bounds"):
        M.score_many([a, b], X=[None, X], y_true=[None, np.array([0, 1, 3, 0, 1])])
    with pytest.raises(IndexError, match="Target -1 is out of bounds"):
        M.score_many([a, b], X=[X, None], y_true=[torch.tensor([0, -1, 2, 0, 1]), None])
    with pytest.raises(RuntimeError, match="weight tensor should be defined either for all 3 classes"):
        M.score_many([a, b], weights=np.ones(4))
    with pytest.raises(RuntimeError, match="weight tensor should be defined either for all 3 classes"):
        M.score_many([a, b], weights=[np.ones(3), [1.0, 2.0]])
    with pytest.raises(ValueError, match="one entry per model"):
        M.score_many([a, b], weights=[np.ones(3)])
    # a factor list of another shape: the shape error, and the caller's list is left alone
    Bcp = [np.zeros((3, 2), dtype=np.float32), np.zeros((5, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32)]
    keep = list(Bcp)
    with pytest.raises(ValueError, match="Incorrect shapes"):
        M.predict_many([a, b], Bcp=[None, Bcp])
    assert all(x is y_ for x, y_ in zip(Bcp, keep))


def test_models_on_different_devices(monkeypatch):
    M = _M()
    from tensor_regression_amd import _engine
    a, b = host_model(seed=1), host_model(seed=2)
    a.device, b.device = "cuda:0", "cuda:1"  # (X on the host: the model's device decides)

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("run_score_many", "upload_packed", "_pack_arena"):
        monkeypatch.setattr(_engine, name, boom)
    monkeypatch.setattr(M.CP_logistic_regression, "predict", boom)
    for fn in (M.score_many, M.predict_many):
        with pytest.raises(ValueError, match="different devices"):
            fn([a, b])


def test_host_metrics_of_an_entry_scored_alone():
    """The fallback's host arithmetic against its definition: the CrossEntropyLoss of the softmax output."""
    M = _M()
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((9, 4))
    S = (np.exp(Z) / np.exp(Z).sum(1, keepdims=True)).astype(np.float32)
    y = np.arange(9) % 4
    pred = S.argmax(1)
    cw = np.array([0.5, 1.0, 2.0, 1.5])
    lsum, wsum, counts = M._host_score(S, pred, y, cw, 4)
    want = torch.nn.CrossEntropyLoss(weight=torch.tensor(cw))(torch.tensor(S, dtype=torch.float64), torch.tensor(y))
    assert abs(lsum / wsum - float(want)) <= 1e-12 * abs(float(want))
    assert counts.sum() == 9 and all(counts[p, t] >= 1 for p, t in zip(pred, y))
    assert np.array_equal(counts / counts.sum(0)[None, :], M.confusion_matrix(pred, y))


# ---- the geometry and the table builder under sanitizers ------------------------------------------

def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_score_tables_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) on this machine")
    exe = str(tmp_path / "score_many_check")
    # the sanitizer runtimes are linked into the program itself (clang's default; asked of g++)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "score many ok" and run.stderr == ""
