"""Device-scaled vanilla models and in-place skip bins, the part that needs no GPU: the binding has the three methods,
the library exports the three symbols, and every entry point refuses a NULL context with CPECAN_EINVAL and a message
before it touches a device (no context can exist without a GPU, so this is all a machine without one can see of
them; the tables themselves are checked in test_vanilla_scaled_models_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from cpecan_load import binding, em

cp = binding()

SYMBOLS = {
    "cpecan_hip_modelsv_create_scaled": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p],
    "cpecan_hip_modelsv_download": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)],
    "cpecan_hip_modelsv_set_skip_probs": [C.c_void_p, C.c_void_p],
}


def test_context_has_the_three_methods():
    for name in ("modelsv_create_scaled", "modelsv_set_skip_probs", "modelsv_download"):
        assert callable(getattr(cp.Context, name, None)), name
    assert hasattr(em(), "PersistentVanillaEStep")


def test_library_exports_the_three_symbols_with_the_bindings_argtypes():
    raw = C.CDLL(cp.LIB_PATH)
    for name, argtypes in SYMBOLS.items():
        assert name in cp.EXPORTS, name
        assert hasattr(raw, name), name
        assert list(getattr(cp.lib(), name).argtypes) == argtypes, name


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_null_context_is_refused_before_any_device_is_touched(name):
    L = cp.lib()
    assert L.cpecan_hip_device_count(None) == cp.EINVAL  # leaves a message of its own behind
    other = L.cpecan_hip_last_error().decode()
    match = np.ones(cp.MODEL_TABLE_LEN)
    skip = np.full(60, 0.2)
    desc = cp.VanillaModelDesc()
    desc.m_to_y_not_x, desc.e_to_e = 0.17, 0.55
    desc.match_probs, desc.skip_probs, desc.gap_y_probs = match.ctypes.data, skip.ctypes.data, match.ctypes.data
    scalings = np.array([[1.0, 0.0, 1.0, 1.0, 1.0]])
    ids = np.zeros(1, np.int32)
    n = C.c_int64(-1)
    out = np.zeros(8)
    rc = {
        "cpecan_hip_modelsv_create_scaled":
            lambda: L.cpecan_hip_modelsv_create_scaled(None, C.byref(desc), _ptr(scalings), 1, 1, _ptr(ids)),
        "cpecan_hip_modelsv_download": lambda: L.cpecan_hip_modelsv_download(None, 0, _ptr(out), out.size, C.byref(n)),
        "cpecan_hip_modelsv_set_skip_probs": lambda: L.cpecan_hip_modelsv_set_skip_probs(None, _ptr(skip)),
    }[name]()
    assert rc == cp.EINVAL
    msg = L.cpecan_hip_last_error().decode()
    assert msg.strip() != "" and msg != other
    assert ids[0] == 0 and n.value == -1 and not out.any()
