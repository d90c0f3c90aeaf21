"""The weight blob's host twin (no GPU needed): ``mzgo.pack_weights_host``
(mzgo_weights_pack_host, csrc/mzgo_weights.hip) walks the pack plan of
csrc/mzgo_weights.hpp serially through the element rules that k_pack_weights
runs per thread.  Its blobs are held to tests/golden/weight_blobs.json -- the
bytes ``Engine.export_weights()`` gave before the host and the device shared
one text (scripts/record_weight_blobs.py) -- on the six kernel sets and two
state dicts each, and its refusals are mzgo_set_weights_device's."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_blobs.json")
with open(GOLDEN) as _f:
    CASES = json.load(_f)["cases"]
KERNEL_SETS = [(5, 96), (6, 64), (6, 96), (6, 128), (9, 96), (19, 96)]


def state_dict(name, C, A):
    from oracle.weights import deterministic_state_dict, scaled_state_dict
    return {"deterministic_3": lambda: deterministic_state_dict(C, A, 3),
            "scaled_7": lambda: scaled_state_dict(C, A, 7)}[name]()


def test_the_goldens_cover_every_kernel_set_twice():
    assert sorted((c["board_size"], c["latent_dim"], c["state_dict"]) for c in CASES) == sorted(
        (N, C, name) for N, C in KERNEL_SETS for name in ("deterministic_3", "scaled_7"))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['board_size']}-{c['latent_dim']}-{c['state_dict']}")
def test_blob_is_the_recorded_one(case):
    import mzgo
    N, C = case["board_size"], case["latent_dim"]
    blob = mzgo.pack_weights_host(state_dict(case["state_dict"], C, N * N + 1), N)
    assert blob.dtype == np.float32 and blob.ndim == 1
    assert blob.size == case["n_floats"] and blob.size % 64 == 0
    assert hashlib.sha256(blob.tobytes()).hexdigest() == case["sha256"]


def test_embedding_rows_past_the_actions_stay_out():
    import mzgo
    N, C = 6, 64
    A = N * N + 1
    sd = state_dict("deterministic_3", C, A)
    want = mzgo.pack_weights_host(sd, N)
    wide = dict(sd)
    wide["dynamics.action_embedding.weight"] = np.concatenate(
        [sd["dynamics.action_embedding.weight"], np.ones((54 - A, C), np.float32)])
    assert np.array_equal(mzgo.pack_weights_host(wide, N).view(np.uint32), want.view(np.uint32))


def test_refusals():
    import mzgo
    N, C = 5, 96
    A = N * N + 1
    sd = state_dict("deterministic_3", C, A)
    key = "dynamics.reward_conv.bias"
    with pytest.raises(mzgo.MzgoError, match=rf"mzgo error -1: missing weight '{key}'"):
        mzgo.pack_weights_host({k: v for k, v in sd.items() if k != key}, N)
    with pytest.raises(mzgo.MzgoError, match=rf"mzgo error -1: duplicate key '{key}'"):
        mzgo.pack_weights_host(list(sd.items()) + [(key, sd[key])], N)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: unexpected key 'nonsense'"):
        mzgo.pack_weights_host({**sd, "nonsense": sd[key]}, N)
    bad = dict(sd)
    bad["dynamics.conv.weight"] = np.zeros((C, C + 1, 3, 3), np.float32)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: 'dynamics.conv.weight': dim 1 is 97, expected 96"):
        mzgo.pack_weights_host(bad, N)
    bad["dynamics.conv.weight"] = np.zeros((C, C * 9), np.float32)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: 'dynamics.conv.weight': expected 4 dims, got 2"):
        mzgo.pack_weights_host(bad, N)
    # a (board_size, latent_dim) without a kernel set: 7x7, and 5x5 at C = 64
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: mzgo_weights_pack_host: no kernels built for board_size 7"):
        mzgo.pack_weights_host(state_dict("deterministic_3", C, 50), 7)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: mzgo_weights_pack_host: no kernels built for board_size 5"):
        mzgo.pack_weights_host(state_dict("deterministic_3", 64, A), N)


def test_size_query_and_cap():
    from mzgo import _lib
    from mzgo.engine import _weight_table
    lib = _lib.lib
    N, C = 5, 96
    sd = state_dict("deterministic_3", C, N * N + 1)
    keys, data, shapes, ndims, n, keep = _weight_table(sd.items(), N * N + 1)
    total = ctypes.c_int64(-1)
    assert lib.mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, n, None, 0, ctypes.byref(total)) == 0
    want = next(c["n_floats"] for c in CASES if (c["board_size"], c["latent_dim"]) == (N, C))
    assert total.value == want
    # one float short: refused, and nothing written
    blob = np.full(want, 7.0, np.float32)
    rc = lib.mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, n, _lib.ptr(blob), want - 1, ctypes.byref(total))
    assert rc == _lib.MZGO_EINVAL
    assert f"cap {want - 1} < {want} floats".encode() in lib.mzgo_last_error()
    assert np.all(blob == 7.0)
    assert lib.mzgo_weights_pack_host(N, C, None, data, shapes, ndims, n, None, 0, ctypes.byref(total)) == _lib.MZGO_EINVAL
    assert b"mzgo_weights_pack_host" in lib.mzgo_last_error() and b"null" in lib.mzgo_last_error()
    assert lib.mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, n, None, 0, None) == _lib.MZGO_EINVAL
