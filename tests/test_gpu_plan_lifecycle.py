"""Plan lifecycle through the C ABI: one create / describe / destroy cycle per creator on the smallest
shapes, and the timing records' path through tr_plan_read_timing and tr_plan_destroy.  The plan owns
its workspace and its timing events; nothing here provokes an error."""
import ctypes
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

_DIMS = (ctypes.c_int64 * 2)(4, 3)
_NN = (ctypes.c_int32 * 3)(0, 0, 0)
_CONV = (7, 4, 2, 1, 1)  # n_w, n_d, n_out, rank_normal, rank_spectral (the conv test files' smallest plan)

# creator -> (call, the description's last field)
CREATORS = {
    "linear": (lambda lib, h: lib.tr_plan_create(h, 0, 0, 2, _DIMS, 1, 2, 8, _NN, 50.0, 1.0), r" pk=\d+$"),
    "multinomial": (lambda lib, h: lib.tr_plan_create(h, 0, 1, 2, _DIMS, 3, 2, 8, _NN, 50.0, 1.0),
                    r" workspace=\d+\.\dMiB$"),
    "spectral": (lambda lib, h: lib.tr_plan_create_spectral(h, 0, 8, 5, 1, 2, 2, 2, 4, _NN, 50.0, 1.0),
                 r" xpieces=\d$"),
    "conv": (lambda lib, h: lib.tr_plan_create_conv(h, 0, *_CONV, 2, 600, _NN, 50.0, 1.0), r" workspace=\d+\.\dMiB$"),
    "conv_phase": (lambda lib, h: lib.tr_plan_create_conv_phase(h, 0, *_CONV, 600, _NN, 50.0, 1.0),
                   r" workspace=\d+\.\dMiB$"),
    "conv_fourier": (lambda lib, h: lib.tr_plan_create_conv_fourier(h, 0, *_CONV, 2, 600, _NN, 50.0, 1.0),
                     r" workspace=\d+\.\dMiB$"),
    "f64": (lambda lib, h: lib.tr_plan_create_f64(h, 0, 2, _DIMS, 2, 8, _NN, 50.0, 1.0), r" workspace=\d+\.\dMiB$"),
}


@pytest.mark.parametrize("name", list(CREATORS))
def test_create_describe_destroy(name):
    from tensor_regression_amd import _lib
    lib = _lib.load()
    create, last_field = CREATORS[name]
    h = ctypes.c_void_p()
    with torch.cuda.device(0):
        rc = create(lib, ctypes.byref(h))
    assert rc == 0, lib.tr_last_error()
    assert h.value
    ws = lib.tr_plan_workspace_bytes(h)
    desc = lib.tr_plan_describe(h).decode()
    print(name, ws, desc)
    assert ws > 0 and ws % 256 == 0
    assert desc.startswith("model=") and " path=" in desc
    assert re.search(last_field, desc), desc
    assert lib.tr_plan_num_params(h) > 0 and lib.tr_plan_num_grads(h) == lib.tr_plan_num_params(h) + 2
    assert lib.tr_plan_destroy(h) == 0


def test_timing_records_are_consumed_once_and_destroy_takes_pending_ones():
    """All kinds timed on the tiny linear plan: the first read reports the launches of one tr_loss_grad,
    the second read nothing (every record was consumed, its events back in the pool), and a plan destroyed
    with records still pending releases them."""
    from tensor_regression_amd import _lib
    lib = _lib.load()
    n = len(_lib.KERNEL_KINDS)
    h = ctypes.c_void_p()
    with torch.cuda.device(0):
        assert CREATORS["linear"][0](lib, ctypes.byref(h)) == 0, lib.tr_last_error()
    g = torch.Generator().manual_seed(0)
    X = torch.randn(8, 12, generator=g).to(DEV)
    y = torch.randn(8, generator=g).to(DEV)
    params = (torch.randn(lib.tr_plan_num_params(h), generator=g) * 0.3).to(DEV)
    weights = torch.ones(2, device=DEV)
    grad = torch.zeros(lib.tr_plan_num_grads(h), device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def loss_grad():
        return lib.tr_loss_grad(h, _lib.ptr(X), 8, _lib.ptr(y), None, 8.0, _lib.ptr(params), _lib.ptr(weights),
                                _lib.ptr(grad), None, None, st)

    def read():
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        assert lib.tr_plan_read_timing(h, ms, cnt) == 0, lib.tr_last_error()
        return list(ms), list(cnt)

    assert lib.tr_plan_set_timing(h, -1) == 0
    assert loss_grad() == 0, lib.tr_last_error()
    ms, cnt = read()
    assert sum(cnt) >= 1 and all(c >= 0 for c in cnt)
    assert all(m >= 0.0 for m in ms) and all(m == 0.0 for m, c in zip(ms, cnt) if c == 0)
    assert torch.isfinite(grad).all()
    ms2, cnt2 = read()
    assert cnt2 == [0] * n and ms2 == [0.0] * n
    assert loss_grad() == 0, lib.tr_last_error()  # records pending at destroy
    assert lib.tr_plan_destroy(h) == 0
    torch.cuda.synchronize()
