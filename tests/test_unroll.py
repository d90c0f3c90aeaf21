"""The fused unroll's heads on the CPU (csrc/mzgo_unroll.hpp through
``mzgo_unroll_heads_host``) against torch's autograd on ``_prediction`` and the
reward head of ``recurrent_inference_torch``, evaluated in float32 and again in
float64 on the same float32 inputs; the C entry points' refusals; the
trainer's ``fused_unroll`` switch.

Bar (tests/test_loss.py's for the loss twin): the twin's error against the
float64 result is at most 4x torch-float32's own error against it plus
1e-6 * max(1, |ref|.max()), for the three outputs, the thirteen head-parameter
gradients and the latents' gradient.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SHAPES = [(5, 32, 3, 3), (6, 128, 4, 9), (19, 96, 2, 1), (5, 16, 1, 2)]     # (N, C, S = K + 1, B)
DEAD_UNIT = 5           # the reward-hidden unit whose pre-activation is exactly 0
ZERO_PLANE = (0, 0, 1)  # (step, sample, channel) of the latent plane of zeros


@functools.lru_cache(maxsize=None)
def make_case(N, C, S, B):
    """Head parameters (``deterministic_state_dict``'s, with hidden unit
    DEAD_UNIT's weight and bias 0, so its pre-activation is exactly 0 in any
    precision), ReLU'd normal latents with one plane of zeros, and random
    output gradients; float32 numpy."""
    import mzgo
    from mzgo.unroll import HEAD_KEYS
    A = N * N + 1
    sd = mzgo.deterministic_state_dict(C, A, 7 + N)
    params = {k: sd[k].numpy().copy() for k in HEAD_KEYS}
    params["dynamics.fc_reward_hidden.weight"][DEAD_UNIT] = 0.0
    params["dynamics.fc_reward_hidden.bias"][DEAD_UNIT] = 0.0
    r = np.random.default_rng(100 * N + C + 7 * S + B)
    lat = np.maximum(r.normal(size=(S, B, C, N, N)), 0.0).astype(np.float32)
    lat[ZERO_PLANE] = 0.0
    g = dict(g_logits=r.normal(size=(S, B, A)), g_value=r.normal(size=(S, B)),
             g_reward=r.normal(size=(S - 1, B)) if S > 1 else None)
    g = {k: None if v is None else v.astype(np.float32) for k, v in g.items()}
    for v in list(params.values()) + [lat] + [x for x in g.values() if x is not None]:
        v.setflags(write=False)
    return params, lat, g


def torch_heads(case, dtype):
    """The heads by torch in ``dtype``: outputs, head-parameter gradients and
    the latents' gradient of sum(output * g) over the three outputs, as float64
    numpy."""
    import mzgo
    from mzgo.trainer import _prediction
    params, lat, g = case
    S, B, C, N, _ = lat.shape
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A)
    sd = mzgo.deterministic_state_dict(C, A, 0)
    sd.update({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    net.load_state_dict(sd)
    net = net.to(dtype)
    x = torch.tensor(lat, dtype=dtype).view(S * B, C, N, N).requires_grad_()
    value, logits = _prediction(net, x)
    t = lambda a: torch.tensor(a, dtype=dtype)
    loss = (logits.view(S, B, A) * t(g["g_logits"])).sum() + (value.view(S, B) * t(g["g_value"])).sum()
    reward = None
    if S > 1:
        d = net.dynamics                                  # recurrent_inference_torch's reward head
        reward = d.fc_reward_output(F.relu(d.fc_reward_hidden(d.reward_conv(x[B:]).mean(dim=[2, 3]))))
        loss = loss + (reward.view(S - 1, B) * t(g["g_reward"])).sum()
    loss.backward()
    np64 = lambda a: a.detach().double().numpy()
    named = dict(net.named_parameters())
    grads = {k: np64(named[k].grad) for k in params if named[k].grad is not None}
    return dict(logits=np64(logits).reshape(S, B, A), value=np64(value).reshape(S, B),
                reward=None if reward is None else np64(reward).reshape(S - 1, B), grads=grads,
                g_latent=np64(x.grad).reshape(lat.shape))


def check_bar(name, got, ref32, ref64):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref64.shape, name
    err, own = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
    bound = 4 * own + 1e-6 * max(1.0, np.abs(ref64).max())
    print(f"{name}: max |ref| {np.abs(ref64).max():.4g}  err vs f64 {err:.3g}  torch f32 vs f64 {own:.3g}  "
          f"bound {bound:.3g}")
    assert err <= bound, name


@pytest.mark.parametrize("N,C,S,B", SHAPES)
def test_heads_host_twin_matches_torch_autograd(N, C, S, B):
    import mzgo
    case = make_case(N, C, S, B)
    params, lat, g = case
    logits, value, reward, grads, g_latent = mzgo.unroll_heads_host(params, lat, g["g_logits"], g["g_value"],
                                                                    g["g_reward"])
    ref32, ref64 = torch_heads(case, torch.float32), torch_heads(case, torch.float64)
    check_bar("logits", logits, ref32["logits"], ref64["logits"])
    check_bar("value", value, ref32["value"], ref64["value"])
    if S > 1:
        check_bar("reward", reward, ref32["reward"], ref64["reward"])
    else:
        assert reward is None and ref64["reward"] is None
    assert set(grads) == set(ref64["grads"])              # K = 0: no reward-head gradient, as autograd
    assert len(grads) == (13 if S > 1 else 7)
    for k in grads:
        check_bar(k, grads[k], ref32["grads"][k], ref64["grads"][k])
    check_bar("g_latent", g_latent, ref32["g_latent"], ref64["g_latent"])
    # the pass logit sits in column A - 1 and takes that column's gradient
    assert (logits[..., -1] == params["prediction.pass_logit"][0]).all()
    if S > 1:
        # the unit that is exactly 0 before the ReLU passes nothing back, as autograd's relu
        for k in ("dynamics.fc_reward_hidden.weight", "dynamics.fc_reward_hidden.bias"):
            assert grads[k].reshape(-1)[DEAD_UNIT] == 0.0 and ref64["grads"][k].reshape(-1)[DEAD_UNIT] == 0.0
        assert grads["dynamics.fc_reward_output.weight"].reshape(-1)[DEAD_UNIT] == 0.0
        assert np.count_nonzero(grads["dynamics.fc_reward_hidden.bias"]) > 0


def test_case_holds_the_edge_cases():
    params, lat, g = make_case(6, 128, 4, 9)
    assert params["dynamics.fc_reward_hidden.weight"][DEAD_UNIT] == 0 == params["dynamics.fc_reward_hidden.bias"][DEAD_UNIT]
    assert (lat[ZERO_PLANE] == 0).all() and (lat[0, 0, 0] > 0).any()
    assert make_case(5, 16, 1, 2)[2]["g_reward"] is None


# ---------------------------------------------------------------------------
# MZGO_EINVAL through the ctypes wrappers: every refusal comes before any device work
# ---------------------------------------------------------------------------
def _table(C, emb_rows, drop=None, reshape=None, extra=None):
    import mzgo
    from mzgo.unroll import _Table
    sd = {k: v.numpy() for k, v in mzgo.deterministic_state_dict(C, emb_rows, 0).items()}
    if drop:
        del sd[drop]
    if reshape:
        sd[reshape] = np.zeros(sd[reshape].shape + (1,), np.float32)
    names = list(sd)
    arrays = list(sd.values())
    if extra:
        names.append(extra)
        arrays.append(np.zeros(1, np.float32))
    return _Table(names, [a.shape for a in arrays]), arrays


def _forward(B=2, K=1, C=16, N=5, emb_rows=26, saved_bytes=None, table=None, **null):
    from mzgo import _lib
    from mzgo.unroll import workspace_bytes
    t, arrays = table or _table(16, 26)            # (a refusal on the dimensions comes before the table is read)
    buf = np.zeros(16, np.float32)                        # never dereferenced: every call here is refused
    p = lambda name: None if null.get(name) else _lib.ptr(buf)
    if saved_bytes is None:
        saved_bytes = workspace_bytes(2, 1, 16, 5, 26)[0]
    rc = _lib.lib.mzgo_unroll_forward(t.keys, t.pointers(arrays), t.shapes, t.ndims, t.n, p("obs0"), p("acts"), B, K, C,
                                      N, emb_rows, p("saved"), saved_bytes, p("logits"), p("value"), p("reward"), None)
    return rc, _lib.lib.mzgo_last_error().decode()


def _backward(B=2, K=1, C=16, N=5, emb_rows=26, saved_bytes=None, work_bytes=None, table=None, no_grads=(), **null):
    from mzgo import _lib
    from mzgo.unroll import workspace_bytes
    t, arrays = table or _table(16, 26)            # (a refusal on the dimensions comes before the table is read)
    buf = np.zeros(16, np.float32)
    p = lambda name: None if null.get(name) else _lib.ptr(buf)
    sb, wb = workspace_bytes(2, 1, 16, 5, 26)
    grads = [None if k.decode() in no_grads else buf for k in t.keys]
    rc = _lib.lib.mzgo_unroll_backward(t.keys, t.pointers(arrays), t.shapes, t.ndims,
                                       None if null.get("grads") else t.pointers(grads), t.n, p("saved"),
                                       sb if saved_bytes is None else saved_bytes, p("g_logits"), p("g_value"),
                                       p("g_reward"), B, K, C, N, emb_rows, p("work"),
                                       wb if work_bytes is None else work_bytes, None)
    return rc, _lib.lib.mzgo_last_error().decode()


DIM_REFUSALS = [(dict(B=0), "B must be >= 1"), (dict(K=-1), "K must be >= 0"), (dict(C=24), "multiple of 16"),
                (dict(C=0), "multiple of 16"), (dict(N=1), "N 1 out of range (2..19)"),
                (dict(N=20), "N 20 out of range (2..19)"), (dict(emb_rows=25), "emb_rows 25 < N*N + 1 = 26"),
                # the convs and the chain put the batch in the launch grid's z dimension
                (dict(B=65536), "B = 65536 exceeds the launch grid's z limit of 65535"),
                (dict(B=1 << 20, K=0), "B = 1048576 exceeds the launch grid's z limit of 65535")]


def test_workspace_sizes_and_refusals():
    from mzgo import _lib
    from mzgo.unroll import workspace_bytes
    saved, work = workspace_bytes(2, 1, 16, 5, 26)
    # at least the latents (saved) and their gradients (work)
    assert saved >= 4 * (2 * 2 * 16 * 25 + 2 * 2 * 64 * 25 + 2 * 6 * 25) and work >= 4 * 2 * 2 * 16 * 25
    assert workspace_bytes(2, 3, 16, 5, 26)[0] > saved and workspace_bytes(2, 0, 16, 5, 26)[0] < saved
    # main.py's sizes: the single K B pass keeps its weight partials within 32 MiB
    assert workspace_bytes(128, 10, 128, 6, 37)[1] < 4 * 11 * 128 * 128 * 36 + (48 << 20)
    out = ctypes.c_int64()
    for over, text in DIM_REFUSALS:
        a = dict(B=2, K=1, C=16, N=5, emb_rows=26)
        a.update(over)
        rc = _lib.lib.mzgo_unroll_workspace(a["B"], a["K"], a["C"], a["N"], a["emb_rows"], ctypes.byref(out),
                                            ctypes.byref(out))
        msg = _lib.lib.mzgo_last_error().decode()
        assert rc == _lib.MZGO_EINVAL and text in msg and "mzgo_unroll_workspace" in msg, (over, msg)
    # a wide C: one chunk of all K B boards already passes the 32 MiB (C = 1024: 37.7 MB), and is what is taken
    big = workspace_bytes(4, 5, 1024, 6, 37)[1]            # (K B = 20 boards: 8, 16, then all of them)
    assert 1024 * 1024 * 9 * 4 <= big - 4 * 6 * 4 * 1024 * 36 < 1024 * 1024 * 9 * 4 + (8 << 20)
    assert workspace_bytes(128, 10, 960, 6, 37)[1] < 4 * 11 * 128 * 960 * 36 + (80 << 20)   # 33.2 MB: one chunk fits
    rc = _lib.lib.mzgo_unroll_workspace(1 << 30, 1, 16, 5, 26, ctypes.byref(out), ctypes.byref(out))
    assert rc == _lib.MZGO_EINVAL and b"exceeds 2^31 - 1" in _lib.lib.mzgo_last_error()
    rc = _lib.lib.mzgo_unroll_workspace(2, 1, 16, 5, 26, None, ctypes.byref(out))
    assert rc == _lib.MZGO_EINVAL and b"null saved_bytes" in _lib.lib.mzgo_last_error()


def test_forward_refusals():
    from mzgo import _lib
    cases = DIM_REFUSALS + [
        (dict(obs0=True), "null obs0"), (dict(saved=True), "null saved"), (dict(logits=True), "null logits"),
        (dict(value=True), "null value"), (dict(acts=True), "null acts"), (dict(reward=True), "null reward"),
        (dict(saved_bytes=64), "saved too small: 64 <"),
        (dict(table=_table(16, 26, drop="dynamics.conv.bias")), "missing weight 'dynamics.conv.bias'"),
        (dict(table=_table(16, 26, reshape="prediction.pass_logit")), "'prediction.pass_logit': expected 1 dims, got 2"),
        (dict(table=_table(32, 26)), "dim 0 is 32, expected 16"),
        (dict(table=_table(16, 26), emb_rows=37), "'dynamics.action_embedding.weight': dim 0 is 26, expected 37"),
        (dict(table=_table(16, 26, extra="dynamics.conv.extra")), "unexpected key 'dynamics.conv.extra'"),
        (dict(table=_table(16, 26, extra="prediction.pass_logit")), "duplicate key 'prediction.pass_logit'"),
    ]
    for over, text in cases:
        rc, msg = _forward(**over)
        assert rc == _lib.MZGO_EINVAL and text in msg and "mzgo_unroll_forward" in msg, (over, msg)


def test_backward_refusals():
    from mzgo import _lib
    cases = DIM_REFUSALS + [
        (dict(saved=True), "null saved"), (dict(g_logits=True), "null g_logits"), (dict(g_value=True), "null g_value"),
        (dict(g_reward=True), "null g_reward"), (dict(work=True), "null work"), (dict(grads=True), "null grads"),
        (dict(saved_bytes=64), "saved too small: 64 <"), (dict(work_bytes=128), "work too small: 128 <"),
        (dict(no_grads=("representation.conv2.weight",)), "null gradient for 'representation.conv2.weight'"),
        (dict(no_grads=("dynamics.conv.weight",)), "null gradient for 'dynamics.conv.weight'"),
        (dict(K=0, no_grads=("dynamics.conv.weight", "prediction.value_fc.bias")),
         "null gradient for 'prediction.value_fc.bias'"),           # K = 0: only the dynamics' may be null
        (dict(table=_table(16, 26, drop="prediction.policy_conv.weight")),
         "missing weight 'prediction.policy_conv.weight'"),
    ]
    for over, text in cases:
        rc, msg = _backward(**over)
        assert rc == _lib.MZGO_EINVAL and text in msg and "mzgo_unroll_backward" in msg, (over, msg)


def test_batch_above_the_grid_limit_is_refused_before_any_launch():
    """k_conv_fwd and k_conv_bwd_input (the unroll's chain too) launch a grid with z =
    B: 65536 boards are MZGO_EINVAL from the unroll and from the three layer
    entry points, 65535 pass that check (and fail a later one here)."""
    from mzgo import _lib
    lib, EINVAL = _lib.lib, _lib.MZGO_EINVAL
    buf = np.zeros(16, np.float32)                        # never dereferenced: every call here is refused
    p = _lib.ptr(buf)
    limit = "exceeds the launch grid's z limit of 65535"
    rc = lib.mzgo_conv3x3_relu_forward(p, None, None, p, p, 65536, 6, 64, 5, p, None)
    assert rc == EINVAL and b"mzgo_conv3x3_relu_forward: B = 65536 " + limit.encode() in lib.mzgo_last_error()
    rc = lib.mzgo_conv3x3_relu_forward(p, p, p, p, p, 1 << 30, 16, 16, 2, p, None)
    assert rc == EINVAL and limit.encode() in lib.mzgo_last_error()
    rc = lib.mzgo_conv3x3_backward(p, p, p, None, None, p, 65536, 6, 64, 5, None, p, p, p, 1 << 40, None)
    assert rc == EINVAL and b"mzgo_conv3x3_backward: B = 65536 " + limit.encode() in lib.mzgo_last_error()
    rc = lib.mzgo_dyn_conv_backward(p, p, p, p, p, p, 65536, 16, 5, p, p, p, p, 1 << 40, None)
    assert rc == EINVAL and b"mzgo_dyn_conv_backward: B = 65536 " + limit.encode() in lib.mzgo_last_error()
    # one board fewer is not refused for its batch: the next check is the workspace's size
    rc = lib.mzgo_conv3x3_backward(p, p, p, None, None, p, 65535, 6, 64, 5, None, p, p, p, 64, None)
    assert rc == EINVAL and b"workspace too small: 64 <" in lib.mzgo_last_error()
    rc = lib.mzgo_dyn_conv_backward(p, p, p, p, p, p, 65535, 16, 5, p, p, p, p, 64, None)
    assert rc == EINVAL and b"workspace too small: 64 <" in lib.mzgo_last_error()
    rc, msg = _forward(B=65535, saved_bytes=64)
    assert rc == EINVAL and "saved too small: 64 <" in msg
    rc, msg = _backward(B=65535, work_bytes=128, saved_bytes=1 << 40)
    assert rc == EINVAL and "work too small: 128 <" in msg


def test_heads_host_refusals():
    import mzgo
    from mzgo import _lib
    params, lat, g = make_case(5, 16, 1, 2)
    with pytest.raises(mzgo.MzgoError, match="unexpected key 'dynamics.conv.bias'"):
        mzgo.unroll_heads_host({**params, "dynamics.conv.bias": np.zeros(16, np.float32)}, lat, g["g_logits"],
                               g["g_value"], None)
    with pytest.raises(mzgo.MzgoError, match="missing weight 'prediction.pass_logit'"):
        mzgo.unroll_heads_host({k: v for k, v in params.items() if k != "prediction.pass_logit"}, lat, g["g_logits"],
                               g["g_value"], None)
    with pytest.raises(mzgo.MzgoError, match="C must be a multiple of 16"):
        mzgo.unroll_heads_host(params, np.zeros((1, 2, 8, 5, 5), np.float32), g["g_logits"], g["g_value"], None)
    rc = _lib.lib.mzgo_unroll_heads_host(None, None, None, None, None, 0, None, 0, 1, 16, 5, None, None, None, None,
                                         None, None, None)
    assert rc == _lib.MZGO_EINVAL and b"S must be >= 1" in _lib.lib.mzgo_last_error()
    rc = _lib.lib.mzgo_unroll_heads_host(None, None, None, None, None, 0, None, 1, 1, 16, 5, None, None, None, None,
                                         None, None, None)
    assert rc == _lib.MZGO_EINVAL and b"null latents" in _lib.lib.mzgo_last_error()


# ---------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------
def test_unroll_refuses_what_it_cannot_run():
    import mzgo
    obs = torch.zeros(2, 6, 5, 5)
    acts = torch.zeros(2, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="runs on the GPU"):
        mzgo.unroll(mzgo.MuZeroNet(32, 26), obs, acts)
    with pytest.raises(TypeError, match="ResMuZeroNet"):
        mzgo.unroll(mzgo.ResMuZeroNet(64, 26, 1), obs, acts)
    with pytest.raises(TypeError, match="needs a MuZeroNet"):
        mzgo.unroll(torch.nn.Linear(1, 1), obs, acts)


def test_fused_unroll_switch_and_its_refusals():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    assert TrainConfig().fused_unroll is False
    net = mzgo.MuZeroNet(32, 26)
    with pytest.raises(ValueError, match="fused_unroll needs mode='batched'"):
        MuZeroTrainer(net, TrainConfig(fused_unroll=True), mode="reference")
    with pytest.raises(ValueError, match="two different HIP paths"):
        MuZeroTrainer(net, TrainConfig(fused_unroll=True), mode="batched", hip_forward=True)
    with pytest.raises(ValueError, match="multiple of 16"):
        MuZeroTrainer(mzgo.MuZeroNet(24, 26), TrainConfig(fused_unroll=True), mode="batched")
    with pytest.raises(ValueError, match="needs the net on the GPU"):
        MuZeroTrainer(net, TrainConfig(fused_unroll=True, fused_loss=True), mode="batched")
    with pytest.raises(ValueError, match="MuZeroNet.* only, not ResMuZeroNet"):
        MuZeroTrainer(mzgo.ResMuZeroNet(64, 26, 1), TrainConfig(fused_unroll=True), mode="batched")
    # the other paths are untouched by the switch's existence
    MuZeroTrainer(net, TrainConfig(), mode="reference")
    MuZeroTrainer(mzgo.MuZeroNet(24, 26), TrainConfig(), mode="batched")
