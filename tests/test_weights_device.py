"""The device weight path's host-visible surface (no GPU needed): the three
entry points of include/mzgo.h are exported and refuse null engines, and the
Python switches exist with their defaults.  What the kernels pack is compared
with the host packers byte for byte in tests/test_gpu_weights_device.py."""
import ctypes

import pytest

SYMBOLS = ("mzgo_set_weights_device", "mzgo_weights_copy", "mzgo_weights_export")


def test_library_exports_the_symbols():
    from mzgo import _lib
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), f"{name} is not exported by libmzgo.so"


def test_null_engines_are_refused():
    from mzgo import _lib
    lib = _lib.lib
    n = ctypes.c_int64(-1)
    calls = {
        "mzgo_set_weights_device": lambda: lib.mzgo_set_weights_device(None, None, None, None, None, 0, None),
        "mzgo_weights_copy": lambda: lib.mzgo_weights_copy(None, None, None),
        "mzgo_weights_export": lambda: lib.mzgo_weights_export(None, None, 0, ctypes.byref(n), None),
    }
    for name, call in calls.items():
        assert call() == _lib.MZGO_EINVAL, name
        msg = lib.mzgo_last_error()
        assert name.encode() in msg and b"null" in msg, (name, msg)


def test_device_weights_defaults_to_off():
    import mzgo
    from mzgo.trainer import TrainConfig
    assert mzgo.MuZeroNet.device_weights is False
    assert mzgo.MuZeroNet(32, 26).device_weights is False
    assert mzgo.ResMuZeroNet(64, 26, 1).device_weights is False
    assert TrainConfig().device_weights is False


def test_trainer_needs_a_cuda_net():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    net = mzgo.MuZeroNet(32, 26)
    with pytest.raises(ValueError, match="device_weights"):
        MuZeroTrainer(net, TrainConfig(device_weights=True), mode="batched")
    assert net.device_weights is False
