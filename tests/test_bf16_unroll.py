"""The bf16 mode of the fused unroll on the CPU: the kernels' rounding
(``mzgo_bf16_round_host``, compiled from the function the kernels call) against
torch's ``t.bfloat16().float()`` bit for bit, and every refusal of the mode --
at the C layer and unroll entry points, in ``mzgo.unroll`` and in
``TrainConfig`` -- before any device work.
"""
import ctypes

import numpy as np
import pytest
import torch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _torch_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _edge_values():
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)
    one = 0x3F800000
    ties = [one + 0x8000, one + 0x18000]                    # 1 + 2^-8 (down to even), 1 + 3 2^-8 (up to even)
    vals = []
    for t in ties:
        vals += [t, t - 1, t + 1, t | 0x80000000, (t - 1) | 0x80000000, (t + 1) | 0x80000000]
    vals += [0x00000000, 0x80000000]                        # +-0
    vals += [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x80000001, 0x807FFFFF]   # subnormals
    vals += [0x7F7FFFFF, 0xFF7FFFFF]                        # the largest finite: -> +-inf
    vals += [0x7F7F7FFF, 0x7F7F8000]                        # around the last tie below inf
    vals += [0x7F800000, 0xFF800000]                        # +-inf
    vals += [0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0x7F80FFFF]   # NaNs, quiet and signalling
    return f(vals)


def test_round_host_is_torch_bfloat16_rounding():
    import mzgo
    x = _edge_values()
    got, want = mzgo.bf16_round_host(x), _torch_round(x)
    nan = np.isnan(want)
    assert nan.sum() == 5 and (np.isnan(got) == nan).all()              # NaN stays NaN
    assert (_bits(got)[~nan] == _bits(want)[~nan]).all(), (x[~nan], got[~nan], want[~nan])
    assert np.isinf(got[x == np.float32(3.4028235e38)]).all()           # overflow goes to inf
    assert mzgo.bf16_round_host(np.float32([1 + 2.0 ** -8]))[0] == 1.0  # tie to even: down
    assert mzgo.bf16_round_host(np.float32([1 + 3 * 2.0 ** -8]))[0] == np.float32(1 + 2.0 ** -6)   # tie to even: up
    assert np.signbit(mzgo.bf16_round_host(np.float32([-0.0]))[0])
    # 10^5 random bit patterns
    r = np.random.default_rng(5)
    x = r.integers(0, 1 << 32, size=100_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    got, want = mzgo.bf16_round_host(x), _torch_round(x)
    nan = np.isnan(x)
    assert 100 < nan.sum() < 2000 and (np.isnan(got) == nan).all() and (np.isnan(want) == nan).all()
    assert (_bits(got)[~nan] == _bits(want)[~nan]).all()
    assert (_bits(got) & 0xFFFF == 0).all()                             # a bfloat16 value
    assert mzgo.bf16_round_host(np.zeros((0,), np.float32)).shape == (0,)
    assert mzgo.bf16_round_host(np.ones((2, 3), np.float32)).shape == (2, 3)


def _err():
    from mzgo import _lib
    return _lib.lib.mzgo_last_error().decode()


def test_layer_entry_points_refuse_before_any_device_work():
    from mzgo import _lib
    lib = _lib.lib
    buf = np.zeros(16, np.float32)                          # never dereferenced: every call here is refused
    p = _lib.ptr(buf)
    out = ctypes.c_int64()
    for cin, cout, text in ((48, 32, "Cin must be a multiple of 32 in bf16 mode, got 48"),
                            (32, 48, "Cout must be a multiple of 32 in bf16 mode, got 48"),
                            (0, 32, "Cin must be a multiple of 32 in bf16 mode, got 0")):
        rc = lib.mzgo_conv3x3_relu_forward_bf16(p, None, None, p, p, 1, cin, cout, 5, p, None)
        assert rc == _lib.MZGO_EINVAL and text in _err() and "mzgo_conv3x3_relu_forward_bf16" in _err()
        rc = lib.mzgo_conv3x3_backward_bf16_workspace(1, cin, cout, ctypes.byref(out))
        assert rc == _lib.MZGO_EINVAL and text in _err()
        rc = lib.mzgo_conv3x3_backward_bf16(p, p, p, None, None, p, 1, cin, cout, 5, p, p, p, p, 1 << 30, None)
        assert rc == _lib.MZGO_EINVAL and text in _err() and "mzgo_conv3x3_backward_bf16" in _err()
    for n in (1, 20):
        rc = lib.mzgo_conv3x3_relu_forward_bf16(p, None, None, p, p, 1, 32, 32, n, p, None)
        assert rc == _lib.MZGO_EINVAL and f"N {n} out of range (2..19)" in _err()
        rc = lib.mzgo_conv3x3_backward_bf16(p, p, p, None, None, p, 1, 32, 32, n, p, p, p, p, 1 << 30, None)
        assert rc == _lib.MZGO_EINVAL and f"N {n} out of range (2..19)" in _err()
    rc = lib.mzgo_conv3x3_relu_forward_bf16(p, None, None, p, p, 0, 32, 32, 5, p, None)
    assert rc == _lib.MZGO_EINVAL and "B must be >= 1, got 0" in _err()
    rc = lib.mzgo_conv3x3_relu_forward_bf16(None, None, None, p, p, 1, 32, 32, 5, p, None)
    assert rc == _lib.MZGO_EINVAL and "null argument" in _err()
    rc = lib.mzgo_conv3x3_relu_forward_bf16(p, None, p, p, p, 1, 32, 32, 5, p, None)      # emb without action
    assert rc == _lib.MZGO_EINVAL and "null argument" in _err()
    # the workspace: the float32 call's partials, rounded up to 256, and 36 Cin Cout bytes of packed weights
    f32 = ctypes.c_int64()
    for B, cin, cout in ((1, 32, 32), (17, 32, 64), (9, 160, 96)):
        assert lib.mzgo_conv3x3_backward_bf16_workspace(B, cin, cout, ctypes.byref(out)) == 0
        assert lib.mzgo_conv3x3_backward_workspace(B, cin, cout, ctypes.byref(f32)) == 0
        assert out.value == (f32.value + 255) // 256 * 256 + 36 * cin * cout
    assert lib.mzgo_conv3x3_backward_bf16_workspace(1, 32, 32, ctypes.byref(out)) == 0
    rc = lib.mzgo_conv3x3_backward_bf16(p, p, p, None, None, p, 1, 32, 32, 5, p, p, p, p, out.value - 1, None)
    assert rc == _lib.MZGO_EINVAL and "workspace too small" in _err()


def _unroll_calls(C, precision, emb_rows=26):
    """(rc, message) of the three _p entry points at (B, K, N) = (2, 1, 5) with dummy buffers."""
    import mzgo
    from mzgo import _lib
    from mzgo.unroll import _Table
    lib = _lib.lib
    # (a refusal on the dimensions or the precision comes before the table is read)
    sd = {k: v.numpy() for k, v in mzgo.deterministic_state_dict(16, 26, 0).items()}
    arrays = list(sd.values())
    t = _Table(list(sd), [a.shape for a in arrays])
    buf = np.zeros(16, np.float32)
    p = _lib.ptr(buf)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    res = []
    rc = lib.mzgo_unroll_workspace_p(2, 1, C, 5, emb_rows, precision, ctypes.byref(a), ctypes.byref(b))
    res.append((rc, _err()))
    rc = lib.mzgo_unroll_forward_p(t.keys, t.pointers(arrays), t.shapes, t.ndims, t.n, p, p, 2, 1, C, 5, emb_rows, p,
                                   1 << 30, p, p, p, precision, None)
    res.append((rc, _err()))
    grads = [buf for _ in t.keys]
    rc = lib.mzgo_unroll_backward_p(t.keys, t.pointers(arrays), t.shapes, t.ndims, t.pointers(grads), t.n, p, 1 << 30,
                                    p, p, p, 2, 1, C, 5, emb_rows, p, 1 << 30, precision, None)
    res.append((rc, _err()))
    return res


def test_unroll_entry_points_refuse_before_any_device_work():
    from mzgo import _lib
    for rc, msg in _unroll_calls(48, 1):
        assert rc == _lib.MZGO_EINVAL and "C must be a multiple of 32 in bf16 mode, got 48" in msg, msg
    for rc, msg in _unroll_calls(16, 1):
        assert rc == _lib.MZGO_EINVAL and "C must be a multiple of 32 in bf16 mode, got 16" in msg, msg
    for bad in (2, -1, 7):
        for rc, msg in _unroll_calls(32, bad):
            assert rc == _lib.MZGO_EINVAL and f"unknown precision {bad}" in msg, msg
    # the dimension checks of the float32 calls hold in both modes
    for prec in (0, 1):
        for rc, msg in _unroll_calls(24, prec):
            assert rc == _lib.MZGO_EINVAL and "C must be a multiple of 16, got 24" in msg, msg


def test_workspace_p_is_workspace_at_f32_and_grows_by_the_packed_weights_at_bf16():
    from mzgo import _lib
    from mzgo.unroll import _sizes, workspace_bytes
    lib = _lib.lib
    for B, K, C, N, rows in ((2, 1, 16, 5, 26), (2, 0, 32, 5, 26), (128, 10, 128, 6, 37), (9, 4, 64, 6, 37),
                             (4, 5, 1024, 6, 37), (3, 2, 96, 19, 362)):
        s0, w0, s1, w1 = (ctypes.c_int64() for _ in range(4))
        assert lib.mzgo_unroll_workspace(B, K, C, N, rows, ctypes.byref(s0), ctypes.byref(w0)) == 0
        assert lib.mzgo_unroll_workspace_p(B, K, C, N, rows, 0, ctypes.byref(s1), ctypes.byref(w1)) == 0
        assert (s0.value, w0.value) == (s1.value, w1.value)
        assert workspace_bytes(B, K, C, N, rows) == (s0.value, w0.value) == workspace_bytes(B, K, C, N, rows, "fp32")
        if C % 32 == 0:
            assert lib.mzgo_unroll_workspace_p(B, K, C, N, rows, 1, ctypes.byref(s1), ctypes.byref(w1)) == 0
            assert s1.value == s0.value + (36 * C * C + 255) // 256 * 256 and w1.value == w0.value
            assert workspace_bytes(B, K, C, N, rows, "bf16") == (s1.value, w1.value)
            assert (B, K, C, N, rows, "bf16") in _sizes and (B, K, C, N, rows, "fp32") in _sizes
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        workspace_bytes(2, 1, 32, 5, 26, "fp16")


def test_python_refusals():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    obs = torch.zeros(2, 6, 5, 5)
    acts = torch.zeros(2, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16', got 'fp16'"):
        mzgo.unroll(mzgo.MuZeroNet(32, 26), obs, acts, precision="fp16")
    with pytest.raises(ValueError, match="latent_dim to be a multiple of 32, got 48"):
        mzgo.unroll(mzgo.MuZeroNet(48, 26), obs, acts, precision="bf16")
    with pytest.raises(TypeError, match="ResMuZeroNet"):
        mzgo.unroll(mzgo.ResMuZeroNet(64, 26, 1), obs, acts, precision="bf16")
    with pytest.raises(ValueError, match="runs on the GPU"):          # (the mode itself is accepted)
        mzgo.unroll(mzgo.MuZeroNet(32, 26), obs, acts, precision="bf16")

    assert TrainConfig().unroll_precision == "fp32"
    net = mzgo.MuZeroNet(32, 26)
    with pytest.raises(ValueError, match="unroll_precision='bf16' needs fused_unroll=True"):
        MuZeroTrainer(net, TrainConfig(unroll_precision="bf16"), mode="batched")
    with pytest.raises(ValueError, match="unroll_precision='bf16' needs mode='batched'"):
        MuZeroTrainer(net, TrainConfig(unroll_precision="bf16"), mode="reference")
    with pytest.raises(ValueError, match="unroll_precision='bf16' needs mode='batched'"):
        MuZeroTrainer(net, TrainConfig(unroll_precision="bf16", fused_unroll=True), mode="reference")
    with pytest.raises(ValueError, match="unroll_precision must be 'fp32' or 'bf16', not 'fp16'"):
        MuZeroTrainer(net, TrainConfig(unroll_precision="fp16"), mode="batched")
    with pytest.raises(ValueError, match="latent_dim to be a multiple of 32, got 48"):
        MuZeroTrainer(mzgo.MuZeroNet(48, 26), TrainConfig(unroll_precision="bf16", fused_unroll=True), mode="batched")
    with pytest.raises(ValueError, match="MuZeroNet.* only, not ResMuZeroNet"):
        MuZeroTrainer(mzgo.ResMuZeroNet(64, 26, 1), TrainConfig(unroll_precision="bf16", fused_unroll=True),
                      mode="batched")
    with pytest.raises(ValueError, match="needs the net on the GPU"):  # (a CPU net: fused_unroll's own refusal)
        MuZeroTrainer(net, TrainConfig(unroll_precision="bf16", fused_unroll=True), mode="batched")
    # the default leaves every other path as it was
    MuZeroTrainer(net, TrainConfig(), mode="reference")
    MuZeroTrainer(mzgo.MuZeroNet(48, 26), TrainConfig(), mode="batched")
