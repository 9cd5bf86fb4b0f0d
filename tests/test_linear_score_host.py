"""Host-side checks of scoring the linear sweep (standard_tensor_regression.predict_many / score_many and
the tr_linear_score_* / tr_linear_many_score entries), no GPU:

  * the header, the library and _lib.py agree on the new symbols and on tr_linear_score_member's layout;
    tr_linear_member keeps its 184 bytes
  * tr_linear_score_envelope and _workspace_bytes against a Python restatement of the geometry
  * [] for no models, every argument error raised before any device work
  * with the route off or no device X every entry goes alone, and the host metrics equal a float64
    numpy computation; N = 1 gives nan without a warning
  * the C entry checks the shape and every member without a device and names the offending member
  * tests/cpp/linear_score_check.cpp, the geometry, the carve and the table builder under
    AddressSanitizer and UBSan, built with the host compiler and run as a child process; nothing is
    preloaded
"""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

from test_linear_many_host import C_TYPES, CSRC, HEADER, ROOT, TR_E_ARG, TR_E_UNSUPPORTED, _host_compiler, host_model

SRC = os.path.join(ROOT, "tests", "cpp", "linear_score_check.cpp")
C_TYPES = dict(C_TYPES, **{"const double*": (ctypes.c_void_p, 8)})


def _S():
    from tensor_regression_amd import standard_tensor_regression as S
    return S


@pytest.fixture
def no_device_work(monkeypatch):
    """Any step towards the device fails the test: the errors below must come first."""
    from tensor_regression_amd import _engine, _fit

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("compute_device", "run_linear_score", "_pack_arena", "as_device_rows", "linear_score_envelope"):
        monkeypatch.setattr(_engine, name, boom)
    monkeypatch.setattr(_S(), "as_device_f32", boom)
    monkeypatch.setattr(_fit, "coerce_predict_inputs", boom)
    monkeypatch.setattr(_S().CP_linear_regression, "predict", boom)


# ---- symbols and the struct's layout ----------------------------------------------------------------

def header_struct_fields(name):
    txt = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"((?:const )?\w+\s*\*?)\s*(.*)", decl)
        ctype, names = m.group(1).replace(" *", "*").strip(), m.group(2)
        for nm in (n.strip() for n in names.split(",")):
            arr = re.match(r"(\w+)\[(\d+)\]", nm)
            out.append((arr.group(1) if arr else nm, ctype, int(arr.group(2)) if arr else 1))
    return out


def test_symbols_and_struct_layout_agree_with_the_header():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    txt = open(HEADER).read()
    for s in ("tr_linear_score_envelope", "tr_linear_score_workspace_bytes", "tr_linear_score_table_bytes",
              "tr_linear_many_score"):
        assert re.search(r"^\s*(?:int|int64_t)\s+" + s + r"\s*\(", txt, flags=re.M), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert _lib.SIGNATURES["tr_linear_score_table_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["tr_linear_score_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["tr_linear_many_score"][1][6]._type_ is _lib.LinearScoreMember
    assert lib.tr_abi_version() == _lib.TR_ABI_VERSION
    fields = header_struct_fields("tr_linear_score_member")
    assert [f[0] for f in fields] == [f[0] for f in _lib.LinearScoreMember._fields_]
    assert [f[0] for f in fields] == ["params", "weights", "y", "yhat", "sums", "rank", "nonneg", "softplus_beta",
                                      "softplus_threshold"]
    off = 0
    for (name, ctype, count), (pname, ptype) in zip(fields, _lib.LinearScoreMember._fields_):
        base, size = C_TYPES[ctype]
        want = base * count if count > 1 else base
        assert ctypes.sizeof(ptype) == ctypes.sizeof(want) == size * count, name
        if count == 1:
            assert ptype is base, name
        else:
            assert ptype._type_ is base and ptype._length_ == count, name
        off = -(-off // size) * size
        assert getattr(_lib.LinearScoreMember, name).offset == off, (name, off)
        off += size * count
    assert dict(fields_count(fields))["nonneg"] == 3
    assert ctypes.sizeof(_lib.LinearScoreMember) == -(-off // 8) * 8 == 64
    assert np.dtype(_lib.LinearScoreMember).itemsize == 64
    assert ctypes.sizeof(_lib.LinearMember) == 184  # the sweep's own struct is as it was


def fields_count(fields):
    return [(name, count) for name, _, count in fields]


# ---- the envelope and the workspace against a restatement ------------------------------------------

def py_envelope(dims, xld, rank):
    if len(dims) not in (2, 3) or any(d < 1 or d > 2**20 for d in dims):
        return False
    P = int(np.prod([int(d) for d in dims], dtype=object))
    return P <= 2**30 and P % 4 == 0 and xld >= 0 and xld % 4 == 0 and 1 <= rank <= 32


def py_forward_split(N, P):
    """linear_many_geom's forward split (tr_linear_many.h), restated."""
    nrw = -(-N // 128)
    ns = max(1, min(-(-1024 // nrw), -(-P // 1024)))
    slice_ = -(-(-(-P // ns)) // 512) * 512
    return nrw, slice_, -(-P // slice_)


def py_workspace_bytes(N, dims):
    if N < 1 or N > 2**30 or not py_envelope(dims, 0, 1):
        return 0
    P, isum = int(np.prod(dims)), sum(dims)
    _, _, ns = py_forward_split(N, P)
    nepi = -(-N // 256)
    npad = nepi * 256
    r256 = lambda b: -(-b // 256) * 256
    pieces = [16 * P * 4, 16 * isum * 32 * 4]
    if len(dims) == 2:
        pieces.append(16 * isum * 32 * 4)  # k_lm_prep's dphi
    pieces += [ns * npad * 16 * 4, nepi * 16 * 5 * 8]
    return sum(r256(b) for b in pieces)


def _dims(d):
    return (ctypes.c_int64 * len(d))(*d)


def test_envelope_and_workspace_agree_with_a_restatement():
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    for dims in [(8, 12), (3, 3), (3, 4), (9, 12), (0, 12), (2**20, 2**20), (500, 500), (4, 3, 8), (3, 3, 3),
                 (8, 4, 8), (2**20, 2**10, 4), (8,), (2, 2, 2, 2)]:
        for xld in (0, 12, 98, 100, -4):
            for rank in (0, 1, 32, 33):
                assert lib.tr_linear_score_envelope(len(dims), _dims(dims), xld, rank) == int(py_envelope(dims, xld, rank)), \
                    (dims, xld, rank)
    assert _engine.linear_score_envelope((4, 3, 8), 96, 8) and not _engine.linear_score_envelope((2, 3), 6, 8)
    assert lib.tr_linear_score_envelope(2, None, 0, 1) == 0
    ws = lib.tr_linear_score_workspace_bytes
    for N in (1, 3, 37, 130, 257, 2000, 70000):
        for dims in [(8, 4), (8, 12), (33, 36), (256, 128), (500, 500), (4, 3, 8), (8, 4, 8), (3, 3)]:
            assert ws(N, len(dims), _dims(dims), 16) == py_workspace_bytes(N, list(dims)), (N, dims)
    d = _dims((500, 500))
    assert ws(2000, 2, d, 1) == ws(2000, 2, d, 16) and ws(2000, 2, d, 17) == 0 and ws(0, 2, d, 1) == 0
    # no gradient slabs: a small fraction of the fit's workspace at the notebook's shape
    assert 0 < ws(2000, 2, d, 16) * 4 < lib.tr_linear_many_workspace_bytes(2000, 500, 500, 16)
    # the forward split is the fit's: the restated split reproduces the fit's Z piece too
    nb = int(lib.tr_linear_score_table_bytes(3))
    assert nb > 0 and nb % 3 == 0 and lib.tr_linear_score_table_bytes(0) == 0 and lib.tr_linear_score_table_bytes(-2) == 0
    assert nb // 3 > lib.tr_linear_member_table_bytes(1)


# ---- the Python surface -----------------------------------------------------------------------------

def test_exported_and_empty(no_device_work):
    S = _S()
    assert "predict_many" in S.__all__ and "score_many" in S.__all__
    for call in (lambda r: S.predict_many([], None, report=r), lambda r: S.score_many([], None, None, report=r)):
        report = {"stale": 1}
        assert call(report) == []
        assert report == {"batched": [], "alone": [], "groups": 0, "x_passes": 0}
    assert S.score_many([], torch.zeros(4, 8, 12), torch.zeros(4)) == []
    assert S.LINEAR_SCORE_MIN_BATCH >= 1


def test_argument_errors_come_before_any_device_work(no_device_work):
    S = _S()
    a, b = host_model(seed=1), host_model(seed=2)
    X, y = torch.zeros(10, 8, 12), torch.zeros(10)
    with pytest.raises(TypeError, match="CP_linear_regression"):
        S.score_many([a, object()], X, y)
    with pytest.raises(TypeError, match="CP_linear_regression"):
        S.predict_many([a, object()], X)
    from tensor_regression_amd.spectral_tensor_regression import CP_linear_regression as Spectral
    other = Spectral((10, 8, 12), (10, 2), rank_normal=1, rank_spectral=1, n_complex_dim=1, device="cpu")
    with pytest.raises(TypeError, match="CP_linear_regression"):
        S.score_many([a, other], X, y)
    with pytest.raises(ValueError, match="model 1: Incorrect shapes"):
        S.score_many([a, host_model(dims=(8, 4))], X, y)
    with pytest.raises(ValueError, match="model 0: Incorrect shapes"):
        S.predict_many([a, b], torch.zeros(10, 8, 12, 2))
    with pytest.raises(ValueError, match="model 1: Incorrect shapes"):  # the override's dims count, not the model's
        S.predict_many([a, b], X, Bcp=[None, [np.zeros((8, 2), np.float32), np.zeros((4, 2), np.float32)]])
    with pytest.raises(ValueError, match="one value per model"):
        S.predict_many([a, b], X, Bcp=[None])
    with pytest.raises(ValueError, match="len\\(y\\) == X.shape\\[0\\]"):
        S.score_many([a, b], X, torch.zeros(9))
    with pytest.raises(ValueError, match="y\\[1\\] must be 1-D"):
        S.score_many([a, b], X, [y, torch.zeros(10, 1)])
    with pytest.raises(ValueError, match="one target per model"):
        S.score_many([a, b], X, [y, y, y])
    with pytest.raises(ValueError, match="min_batch"):
        S.score_many([a, b], X, y, min_batch=0)
    with pytest.raises(ValueError, match="min_batch"):
        S.predict_many([a, b], X, min_batch=0)
    c = host_model(seed=3)
    c.weights = torch.ones(3)
    with pytest.raises(ValueError, match="model 1: weights holds 3 values, the rank is 2"):
        S.score_many([a, c], X, y)
    bf = host_model(seed=4)
    bf.dtype = torch.bfloat16
    with pytest.raises(NotImplementedError):
        S.score_many([a, bf], X, y)
    # the same object twice is allowed: nothing is refused for it (it reaches the routing, here alone)


def test_routing_without_a_device_and_host_metrics(monkeypatch):
    """TR_LINEAR_MANY=0, a numpy X, a float64 X and a group below min_batch reach the models' own predict and
    nothing else; the metrics are float64 numpy's."""
    S = _S()
    from tensor_regression_amd import _engine
    rng = np.random.default_rng(5)
    N = 12
    fake = {}

    def fake_predict(self, X, Bcp=None, device=None, plot_pref=False):
        fake.setdefault("calls", []).append((self, Bcp))
        return fake[id(self)]

    def boom(*a, **k):
        raise AssertionError("the grouped route was taken")
    monkeypatch.setattr(S.CP_linear_regression, "predict", fake_predict)
    monkeypatch.setattr(_engine, "run_linear_score", boom)
    ms = [host_model(seed=3, N=N), host_model(seed=4, N=N)]
    for m in ms:
        fake[id(m)] = rng.standard_normal(N).astype(np.float32)
    y = rng.standard_normal(N) + 3.0
    ys = [y, rng.standard_normal(N).astype(np.float32)]

    def expect(yh, yt):
        yh, yt = yh.astype(np.float64), np.asarray(yt, dtype=np.float64)
        return {"loss": np.mean((yh - yt) ** 2), "var_ratio": np.var(yh, ddof=1) / np.var(yt, ddof=1),
                "r2": 1.0 - np.sum((yh - yt) ** 2) / np.sum((yt - yt.mean()) ** 2)}

    def check(res, targets):
        for m, r, yt in zip(ms, res, targets):
            want = expect(fake[id(m)], yt)
            assert set(r) == {"loss", "var_ratio", "r2"}
            for k in want:
                assert abs(r[k] - want[k]) <= 1e-13 * abs(want[k]), (k, r[k], want[k])

    rep = {}
    monkeypatch.setattr(_engine, "compute_device", boom)
    # a numpy X and a float64 X are never grouped
    check(S.score_many(ms, np.zeros((N, 8, 12), np.float32), y, report=rep, min_batch=1), [y, y])
    assert rep == {"batched": [], "alone": [0, 1], "groups": 0, "x_passes": 0}
    check(S.score_many(ms, torch.zeros(N, 8, 12, dtype=torch.float64), ys, report=rep, min_batch=1), ys)
    assert rep["alone"] == [0, 1] and rep["groups"] == 0
    # the switch
    monkeypatch.setenv("TR_LINEAR_MANY", "0")
    check(S.score_many(ms, torch.zeros(N, 8, 12), torch.as_tensor(y), report=rep, min_batch=1), [y, y])
    assert rep == {"batched": [], "alone": [0, 1], "groups": 0, "x_passes": 0}
    fake["calls"] = []
    override = [np.zeros((8, 2), np.float32), np.zeros((12, 2), np.float32)]
    out = S.predict_many([ms[0], ms[1], ms[0]], torch.zeros(N, 8, 12), Bcp=[None, override, None], report=rep)
    assert rep["alone"] == [0, 1, 2] and len(out) == 3
    assert out[0] is fake[id(ms[0])] and out[2] is out[0] and out[1] is fake[id(ms[1])]
    assert [c[1] for c in fake["calls"]] == [None, override, None] and fake["calls"][1][1] is override
    monkeypatch.delenv("TR_LINEAR_MANY")
    # a group below min_batch goes alone (the envelope is asked, the grouped call is not made)
    monkeypatch.setattr(_engine, "compute_device", lambda X, d: 0)
    monkeypatch.setattr(_engine, "as_device_rows", lambda X, dev, dt: X)
    check(S.score_many(ms, torch.zeros(N, 8, 12), y, report=rep, min_batch=3), [y, y])
    assert rep == {"batched": [], "alone": [0, 1], "groups": 0, "x_passes": 0}


def test_one_row_gives_nan_without_a_warning(monkeypatch):
    S = _S()
    monkeypatch.setattr(S.CP_linear_regression, "predict", lambda self, X, Bcp=None: np.array([1.5], np.float32))
    monkeypatch.setenv("TR_LINEAR_MANY", "0")
    m = host_model(N=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = S.score_many([m], torch.zeros(1, 8, 12), torch.tensor([2.0]))[0]
        s = S._metrics_from_sums([0.25, -0.5, 0.25, 0.0, 0.0], 1)
    assert r["loss"] == 0.25 and np.isnan(r["var_ratio"]) and r["r2"] == -np.inf
    assert s["loss"] == 0.25 and np.isnan(s["var_ratio"]) and s["r2"] == -np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r0 = S._host_metrics(np.array([2.0]), np.array([2.0]))
        s0 = S._metrics_from_sums([0.0, 0.0, 0.0, 0.0, 0.0], 1)
    assert all(np.isnan(r0[k]) and np.isnan(s0[k]) for k in ("var_ratio", "r2")) and r0["loss"] == s0["loss"] == 0.0


def test_metrics_from_sums_match_the_direct_formulas():
    S = _S()
    rng = np.random.default_rng(11)
    y = rng.standard_normal(1000) + 1e4
    yh = y + 0.3 * rng.standard_normal(1000)
    k = y[0]
    e = yh - y
    sums = [np.sum(e * e), np.sum(yh - k), np.sum((yh - k) ** 2), np.sum(y - k), np.sum((y - k) ** 2)]
    a, b = S._metrics_from_sums(sums, 1000), S._host_metrics(yh, y)
    for key in a:
        assert abs(a[key] - b[key]) <= 1e-12 * abs(b[key]), (key, a[key], b[key])


# ---- the C entry ------------------------------------------------------------------------------------

def _members(n):
    """Well-formed members over host memory (the checks never dereference a buffer)."""
    from tensor_regression_amd import _lib
    arr = (_lib.LinearScoreMember * n)()
    keep = []
    for j, r in enumerate(arr):
        buf = (ctypes.c_double * 8)()
        keep.append(buf)
        p = ctypes.addressof(buf)
        for f in ("params", "weights", "y", "yhat", "sums"):
            setattr(r, f, p)
        r.rank = (1, 3, 8, 32)[j % 4]
        r.softplus_beta, r.softplus_threshold = 50.0, 1.0
    return arr, keep


def test_c_entry_checks_every_member_without_a_device():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    M = 3
    nbytes = int(lib.tr_linear_score_table_bytes(M))
    big = int(lib.tr_linear_score_table_bytes(17))
    host = (ctypes.c_char * big)()
    devb = (ctypes.c_char * big)()  # never touched: every call below fails its checks first
    d2 = _dims((8, 12))
    wsb = int(lib.tr_linear_score_workspace_bytes(10, 2, d2, M))
    X = (ctypes.c_char * 4096)()
    xp = (ctypes.addressof(X) + 255) // 256 * 256  # aligned stand-ins for X and the workspace

    def score(arr, n=M, nm=2, dims=d2, stride=0, th=host, td=devb, nb=big, x=xp, ws=xp, wb=wsb, rows=10):
        rc = lib.tr_linear_many_score(0, x, rows, stride, nm, dims, arr, n, ws, wb, th, td, nb, None)
        return rc, (lib.tr_last_error() or b"").decode()

    for at, code, fields in [
        (2, TR_E_ARG, dict(params=None)), (0, TR_E_ARG, dict(weights=None)), (1, TR_E_ARG, dict(sums=None)),
        (2, TR_E_ARG, dict(y=None, yhat=None)), (0, TR_E_UNSUPPORTED, dict(rank=33)),
        (1, TR_E_UNSUPPORTED, dict(rank=0)),
    ]:
        arr, keep = _members(M)
        for k, v in fields.items():
            setattr(arr[at], k, v)
        rc, msg = score(arr)
        assert rc == code, (at, fields, rc, msg)
        assert msg.startswith(f"member {at}:"), (fields, msg)
    arr, keep = _members(M)
    arr[2].rank, arr[1].weights = 99, None
    assert score(arr)[1].startswith("member 1:")  # the first bad member is named
    arr, keep = _members(M)
    arr[0].sums = None
    arr[0].y = None  # predict only needs no sums
    arr[1].yhat = None  # score only needs no yhat
    if not torch.cuda.is_available():
        rc, msg = score(arr)  # well-formed: the failure is the missing device, reported as a HIP error
        assert rc > 0 and msg
    # the call's own arguments
    arr, keep = _members(M)
    assert score(arr, n=-1)[0] == TR_E_ARG and score(None)[0] == TR_E_ARG
    arr17, keep17 = _members(17)
    rc, msg = score(arr17, n=17)
    assert rc == TR_E_ARG and "16" in msg
    assert score(arr, th=None)[0] == TR_E_ARG and score(arr, td=None)[0] == TR_E_ARG
    rc, msg = score(arr, nb=nbytes - 1)
    assert rc == TR_E_ARG and "tr_linear_score_table_bytes" in msg
    assert score(arr, x=None)[0] == TR_E_ARG and score(arr, ws=None)[0] == TR_E_ARG and score(arr, dims=None)[0] == TR_E_ARG
    rc, msg = score(arr, wb=wsb - 1)
    assert rc == TR_E_ARG and "tr_linear_score_workspace_bytes" in msg
    assert score(arr, rows=0)[0] == TR_E_ARG
    assert score(arr, dims=_dims((3, 3)))[0] == TR_E_UNSUPPORTED and score(arr, stride=98)[0] == TR_E_UNSUPPORTED
    assert score(arr, nm=1)[0] == TR_E_UNSUPPORTED and score(arr, nm=4, dims=_dims((2, 2, 2, 2)))[0] == TR_E_UNSUPPORTED
    assert score(arr, nm=3, dims=_dims((3, 3, 3)))[0] == TR_E_UNSUPPORTED
    assert score(arr, x=xp + 4)[0] == TR_E_UNSUPPORTED  # X not 16-byte aligned
    assert score(arr, n=0)[0] == 0  # nothing to do: success without a device


# ---- the geometry, the carve and the table builder under sanitizers ----------------------------------

def test_score_tables_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) on this machine")
    exe = str(tmp_path / "linear_score_check")
    # the sanitizer runtimes are linked into the program itself (clang's default; asked of g++)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "linear score ok" and run.stderr == ""
