"""Trained weights to the engines on the device (csrc/mzgo_weights.hip:
k_pack_weights; mzgo_set_weights_device, mzgo_weights_copy,
mzgo_weights_export; ``Engine.set_parameters_device`` / ``copy_weights_from``,
``MuZeroNet.device_weights``, ``TrainConfig.device_weights``,
``SelfPlay.refresh``).

The device pack must give the host packers' blob: every comparison here is
byte for byte (``view(np.uint32)``), no tolerance.  Engines are 1 game x 1
simulation (``compat="fixed"``) so that 19x19 allocates little.  Both paths
run one text (csrc/mzgo_weights.hpp), so each is also held to the blobs
recorded before they did (tests/golden/weight_blobs.json,
scripts/record_weight_blobs.py).
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KERNEL_SETS = [(5, 96), (6, 64), (6, 96), (6, 128), (9, 96), (19, 96)]


def _engine(N, C, S=1, **kw):
    from mzgo.engine import Engine, EngineConfig
    return Engine(EngineConfig(board_size=N, latent_dim=C, num_games=1, num_simulations=S, compat="fixed", **kw))


def _deterministic(C, A, seed):
    from oracle.weights import deterministic_state_dict
    return {k: torch.from_numpy(v) for k, v in deterministic_state_dict(C, A, seed).items()}


def _scaled_randn(C, A, seed):
    """A seeded CPU randn state_dict, each tensor scaled elementwise by
    10**U(-8, 3), a few entries -0.0: variety in the f64 -> f32 rounding."""
    from oracle.weights import param_specs
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, shape, _ in param_specs(C, A):
        t = torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 11.0 - 8.0)
        flat = t.reshape(-1)
        if flat.numel() >= 16:
            flat[torch.randint(flat.numel(), (max(1, flat.numel() // 50),), generator=g)] = -0.0
        out[key] = t.contiguous()
    return out


def _cuda(sd):
    return {k: v.cuda() for k, v in sd.items()}


def _same_bits(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} of {got.size} floats differ, first at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"


# ---- 1. blob identity on every built kernel set ---------------------------
@pytest.mark.parametrize("N,C", KERNEL_SETS)
def test_blob_is_the_host_packers(N, C):
    A = N * N + 1
    host, dev = _engine(N, C), _engine(N, C)
    cases = [_deterministic(C, A, 3), _scaled_randn(C, A, 7)]
    if (N, C) == (6, 64):
        import mzgo
        net = mzgo.MuZeroNet(C, int(1.5 * N * N), board_size=N).cuda()   # play.py:193's embedding rows
        with torch.no_grad():
            for i, p in enumerate(net.parameters()):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)))
        assert net.state_dict()["dynamics.action_embedding.weight"].shape == (54, C)
        cases.append(net.state_dict())
    for sd in cases:
        host.set_state_dict(sd)
        dev.set_parameters_device(_cuda(sd))
        want, got = host.export_weights(), dev.export_weights()
        assert len(got) == len(want) and len(want) % 64 == 0
        _same_bits(got, want)
    host.close()
    dev.close()


@pytest.mark.parametrize("N,C", KERNEL_SETS)
def test_each_path_gives_the_recorded_blob(N, C):
    from oracle.weights import deterministic_state_dict, scaled_state_dict
    A = N * N + 1
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_blobs.json")) as f:
        golden = {c["state_dict"]: c for c in json.load(f)["cases"] if (c["board_size"], c["latent_dim"]) == (N, C)}
    assert sorted(golden) == ["deterministic_3", "scaled_7"]
    host, dev = _engine(N, C), _engine(N, C)
    for name, sd in (("deterministic_3", deterministic_state_dict(C, A, 3)), ("scaled_7", scaled_state_dict(C, A, 7))):
        sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        host.set_state_dict(sd)
        dev.set_parameters_device(_cuda(sd))
        for path, e in (("set_state_dict", host), ("set_parameters_device", dev)):
            blob = e.export_weights()
            assert blob.size == golden[name]["n_floats"], (path, name)
            assert hashlib.sha256(blob.tobytes()).hexdigest() == golden[name]["sha256"], (path, name)
    host.close()
    dev.close()


# ---- 2. copy ---------------------------------------------------------------
def test_copy_between_engines():
    import mzgo
    N, C = 9, 96
    sd = _scaled_randn(C, N * N + 1, 11)
    b, c, d = _engine(N, C), _engine(N, C), _engine(N, C)
    b.set_parameters_device(_cuda(sd))
    want = b.export_weights()
    c.copy_weights_from(b)
    _same_bits(c.export_weights(), want)
    # a source whose host tensors are still pending is packed first
    h = _engine(N, C)
    h.set_state_dict(sd)
    d.copy_weights_from(h)
    _same_bits(d.export_weights(), want)
    other = _engine(6, 64)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: mzgo_weights_copy: engines differ"):
        other.copy_weights_from(b)
    wide = _engine(6, 96)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: mzgo_weights_copy: engines differ"):
        other.copy_weights_from(wide)
    empty = _engine(N, C)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -3"):
        c.copy_weights_from(empty)                                      # nothing to copy yet
    _same_bits(c.export_weights(), want)


# ---- 3. argument errors ------------------------------------------------------
def test_argument_errors():
    import mzgo
    N, C = 5, 96
    A = N * N + 1
    sd = _cuda(_deterministic(C, A, 0))
    e = _engine(N, C)
    key = "dynamics.reward_conv.bias"
    with pytest.raises(mzgo.MzgoError, match=rf"mzgo error -1: missing weight '{key}'"):
        e.set_parameters_device({k: v for k, v in sd.items() if k != key})
    with pytest.raises(mzgo.MzgoError, match=rf"mzgo error -1: duplicate key '{key}'"):
        e.set_parameters_device(list(sd.items()) + [(key, sd[key])])
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: unexpected key 'nonsense'"):
        e.set_parameters_device({**sd, "nonsense": sd[key]})
    bad = dict(sd)
    bad["dynamics.conv.weight"] = torch.zeros(C, C + 1, 3, 3, device="cuda")
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: 'dynamics.conv.weight': dim 1 is 97, expected 96"):
        e.set_parameters_device(bad)
    with pytest.raises(ValueError, match="not a CUDA tensor"):
        e.set_parameters_device({k: v.cpu() for k, v in sd.items()})
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -3"):
        e.export_weights()                                              # none of them loaded anything
    tower = _engine(5, 64, tower=1, res_blocks=1)
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: mzgo_set_weights_device: tower engines"):
        tower.set_parameters_device(_cuda(_deterministic(64, A, 0)))
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -1: mzgo_weights_copy: tower engines"):
        tower.copy_weights_from(e)
    net = mzgo.ResMuZeroNet(64, A, 1).cuda()
    net.device_weights = True
    with pytest.raises(ValueError, match="tower"):
        net.engine()


# ---- 4. state machine --------------------------------------------------------
def test_host_load_after_a_device_load():
    import mzgo
    from mzgo._lib import lib, ptr
    N, C = 5, 96
    A = N * N + 1
    first, second = _deterministic(C, A, 1), _deterministic(C, A, 2)
    obs = (torch.rand(2, 6, N, N, generator=torch.Generator().manual_seed(0)) > 0.5).float()
    e, host = _engine(N, C), _engine(N, C)
    e.set_parameters_device(_cuda(first))
    assert lib.mzgo_weights_ready(e.handle) == 1
    e.initial_inference(obs)
    bias = np.ascontiguousarray(second["dynamics.conv.bias"].numpy())
    shape = (ctypes.c_int64 * 1)(C)
    assert lib.mzgo_set_weights(e.handle, b"dynamics.conv.bias", ptr(bias), shape, 1) == 0
    assert lib.mzgo_weights_ready(e.handle) == 0
    with pytest.raises(mzgo.MzgoError, match=r"mzgo error -3: missing weight"):
        e.initial_inference(obs)
    e.set_state_dict(second)
    host.set_state_dict(second)
    assert torch.equal(e.initial_inference(obs)[0], host.initial_inference(obs)[0])
    _same_bits(e.export_weights(), host.export_weights())


# ---- 5. behaviour ------------------------------------------------------------
def test_inference_and_search_are_the_host_paths():
    N, C = 5, 96
    A = N * N + 1
    sd = _deterministic(C, A, 0)
    a, b = _engine(N, C, 25), _engine(N, C, 25)
    a.set_state_dict(sd)
    b.set_parameters_device(_cuda(sd))
    obs = (torch.rand(4, 6, N, N, generator=torch.Generator().manual_seed(1)) > 0.5).float()
    act = torch.tensor([0, 7, 12, A - 1])
    ia, ib = a.initial_inference(obs), b.initial_inference(obs)
    for x, y in zip(ia, ib):
        assert torch.equal(x, y)
    for x, y in zip(a.recurrent_inference(ia[0], act), b.recurrent_inference(ib[0], act)):
        assert torch.equal(x, y)
    va, ra = a.search(obs[:1])
    vb, rb = b.search(obs[:1])
    assert va.sum().item() == 25 and torch.equal(va, vb) and torch.equal(ra, rb)


def test_reanalyser_follows_the_net(monkeypatch):
    import mzgo
    from mzgo.engine import Engine
    N, C = 5, 96
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, 4))
    net.device_weights = True
    monkeypatch.setattr(Engine, "set_state_dict", lambda self, sd: pytest.fail("host reload with device_weights"))
    ra = mzgo.Reanalyser(net, 4, slots=2)
    first = ra.engine.export_weights()                                  # packed from the parameters
    _same_bits(net.engine().export_weights(), first)
    with torch.no_grad():
        net.dynamics.conv.bias.add_(0.25)
    want = net.engine().export_weights()
    assert not np.array_equal(want, first)
    ra.refresh()                                                        # a copy from the net's (1,1) engine
    _same_bits(ra.engine.export_weights(), want)
    monkeypatch.undo()
    host = _engine(N, C)
    host.set_state_dict(net.state_dict())
    _same_bits(host.export_weights(), want)


# ---- 6. the trainer loop -------------------------------------------------------
def test_trainer_loop_with_device_weights(monkeypatch):
    import mzgo
    from mzgo.engine import Engine
    from mzgo.trainer import MainSelfPlay, MuZeroTrainer, TrainConfig
    N, C, B, K = 5, 96, 4, 3
    A = N * N + 1
    calls = {"pack": 0, "copy": 0}
    pack, copy = Engine.set_parameters_device, Engine.copy_weights_from

    def counted_pack(self, tensors):
        calls["pack"] += 1
        return pack(self, tensors)

    def counted_copy(self, other):
        calls["copy"] += 1
        return copy(self, other)

    monkeypatch.setattr(Engine, "set_parameters_device", counted_pack)
    monkeypatch.setattr(Engine, "copy_weights_from", counted_copy)
    # Two runs of the HOST path alone differ in the last bits of the 1x1 head
    # convs' weight gradients from the first step on (MIOpen's default backward
    # adds in an order that changes from run to run); its deterministic
    # algorithms make the loop repeatable, so that the two paths can be
    # compared bit for bit at all.
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)

    runs = []
    for on in (False, True):
        torch.manual_seed(0)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 4))
        msp = MainSelfPlay(net, 4, 8, seed=3)
        rp = mzgo.DeviceReplay(N, 8, msp.max_moves, "cuda")
        msp.play_into(rp)
        tr = MuZeroTrainer(net, TrainConfig(unroll_steps=K, device_sampling=True, fused_loss=True,
                                            device_weights=on), mode="batched", hip_forward=True, sample_seed=5)
        assert net.device_weights is on
        stats = []
        for _ in range(3):
            assert tr.train(rp, B) is not None
            stats.append(dict(tr.read_stats()))
        runs.append((net, msp, stats))
    (net_off, _, stats_off), (net_on, msp, stats_on) = runs
    # the (1,1) engine, at each step's first inference: new in step 1, when the
    # self-play engine still holds the current weights, stale after each step
    assert calls == {"pack": 2, "copy": 1}
    assert stats_on == stats_off
    for (k, p), q in zip(net_on.state_dict().items(), net_off.state_dict().values()):
        assert torch.equal(p, q), k

    fresh = _engine(N, C)
    fresh.set_state_dict(net_on.state_dict())
    want = fresh.export_weights()
    calls.update(pack=0, copy=0)
    _same_bits(net_on.engine().export_weights(), want)
    assert calls == {"pack": 1, "copy": 0}
    sp_engine = msp.sp.engine
    assert sp_engine._weights_key != net_on._version()        # still the weights it played with
    assert msp.refresh() is sp_engine
    assert calls == {"pack": 1, "copy": 1}                    # the second engine's refresh was a copy
    _same_bits(sp_engine.export_weights(), want)
    # and the host path's engines of the other net hold the same weights
    _same_bits(net_off.engine().export_weights(), want)
