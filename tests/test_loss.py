"""The unroll loss's formulas on the CPU (csrc/mzgo_loss.hpp through
``mzgo_unroll_loss_host``) against torch's autograd on ``_unroll_step``'s own
expressions, evaluated in float32 and again in float64.

Bars (tests/test_gpu_trainer.py's HIP-against-torch ones): total loss
rel 1e-5; per-sample losses and every gradient rtol 1e-3, atol 1e-5 *
max(1, |ref|.max()); and the kernel's error against the float64 reference at
most 4x torch-float32's own error against it plus that atol (test_gpu_net's
4x).  ``make_inputs`` / ``torch_reference`` / ``check_against_reference`` are
shared with tests/test_gpu_loss.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SHAPES = [(1, 0, 26), (3, 1, 26), (5, 10, 82), (2, 3, 362), (128, 10, 37)]
WEIGHTS = dict(value_loss_weight=0.25, policy_loss_weight=1.0, reward_loss_weight=2.0)


@functools.lru_cache(maxsize=None)
def make_inputs(B, K, A):
    """float32 numpy inputs in ``mzgo.unroll_loss``'s layouts.  Policy target
    rows cycle one-hot / half the entries 0 / the float32(1/A) past-the-end row
    / dense; logits row (0, 0) is scaled by 30 (as is every 7th row); value
    (0, 0) is exactly 0.0, value (K, B-1) is negative where that is another
    entry; reward targets are drawn from {-1, 0, 1}."""
    r = np.random.default_rng(1000 * B + 10 * K + A)
    logits = r.normal(size=(K + 1, B, A)) * 2.0
    flat = logits.reshape(-1, A)
    flat[::7] *= 30.0
    value = r.normal(size=(K + 1, B)) * 3.0
    value[K, B - 1] = -abs(value[K, B - 1]) - 0.5
    value[0, 0] = 0.0
    reward = r.normal(size=(K, B))
    t_pol = np.zeros((B, K + 1, A))
    for i, row in enumerate(t_pol.reshape(-1, A)):
        kind = i % 4
        if kind == 0:
            row[r.integers(A)] = 1.0
        elif kind == 1:
            p = r.random(A) + 0.05
            p[r.permutation(A)[:A // 2]] = 0.0
            row[:] = p / p.sum()
        elif kind == 2:
            row[:] = np.float32(1.0 / A)
        else:
            p = r.random(A) + 0.01
            row[:] = p / p.sum()
    t_val = r.normal(size=(B, K + 1)) * 2.0
    t_rew = r.integers(-1, 2, size=(B, K)).astype(np.float64)
    out = dict(logits=logits, value=value, reward=reward, t_pol=t_pol, t_val=t_val, t_rew=t_rew)
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def torch_reference(inp, dtype, device, transform, wts=None):
    """``MuZeroTrainer._unroll_step``'s loss expressions on ``inp`` in
    ``dtype``, differentiated by autograd: the loss is ``per.sum()``, or
    ``(per * wts).sum()`` with sample weights."""
    from mzgo.trainer import reward_value_transform
    t = {k: torch.as_tensor(np.array(v), dtype=dtype, device=device) for k, v in inp.items()}
    logits, value, reward = (t[k].requires_grad_() for k in ("logits", "value", "reward"))
    t_pol, t_val, t_rew = t["t_pol"], t["t_val"], t["t_rew"]
    K = logits.shape[0] - 1
    w_v, w_p, w_r = (WEIGHTS[k] for k in ("value_loss_weight", "policy_loss_weight", "reward_loss_weight"))
    kl = lambda lg, tp: F.kl_div(F.log_softmax(lg, dim=1), tp, reduction="none").sum(dim=1)
    if transform:
        vloss = lambda v, tv: F.mse_loss(reward_value_transform(v), reward_value_transform(tv), reduction="none")
    else:
        vloss = lambda v, tv: F.mse_loss(v, tv, reduction="none")
    v_l = w_v * vloss(value[0], t_val[:, 0])
    p_l = w_p * kl(logits[0], t_pol[:, 0])
    per = v_l + p_l
    tot_v, tot_p, tot_r = v_l.sum().item(), p_l.sum().item(), 0.0
    for k in range(1, K + 1):
        r_l = w_r * F.mse_loss(reward[k - 1], t_rew[:, k - 1], reduction="none")
        v_l = w_v * vloss(value[k], t_val[:, k])
        p_l = w_p * kl(logits[k], t_pol[:, k])
        per = per + r_l + v_l + p_l
        tot_r += r_l.sum().item()
        tot_v += v_l.sum().item()
        tot_p += p_l.sum().item()
    loss = per.sum() if wts is None else (per * torch.as_tensor(wts, dtype=dtype, device=device)).sum()
    loss.backward()
    np64 = lambda x: x.detach().double().cpu().numpy()
    return dict(per=np64(per), totals=np.array([np64(per).sum() if wts is not None else loss.item(), tot_v, tot_p,
                                                tot_r]),
                g_logits=np64(logits.grad), g_value=np64(value.grad),
                g_reward=np64(reward.grad) if K > 0 else None)


def check_close(got, ref, names=("per", "g_logits", "g_value", "g_reward")):
    """Total loss rel 1e-5; per-sample losses and gradients rtol 1e-3, atol
    1e-5 * max(1, |ref|.max())."""
    assert got["totals"][0] == pytest.approx(ref["totals"][0], rel=1e-5)
    for name in names:
        if ref[name] is None:
            assert got[name] is None
            continue
        np.testing.assert_allclose(np.asarray(got[name], dtype=np.float64), ref[name], rtol=1e-3,
                                   atol=1e-5 * max(1.0, np.abs(ref[name]).max()), err_msg=name)


def check_against_reference(got, ref32, ref64):
    """``got``: dict per / totals / g_logits / g_value / g_reward (numpy) from
    the kernel or its host twin; the module docstring's bars."""
    check_close(got, ref32)
    for i, name in ((1, "value"), (2, "policy"), (3, "reward")):
        print(name, got["totals"][i], ref32["totals"][i], ref64["totals"][i])
        # the parts are f64 sums of f32 terms whose errors scale with the rows' largest addends
        assert got["totals"][i] == pytest.approx(ref64["totals"][i], rel=1e-5,
                                                 abs=1e-5 * max(1.0, abs(ref64["totals"][0]))), name
    assert got["totals"][0] == pytest.approx(got["totals"][1:].sum(), rel=1e-5)
    err = abs(got["totals"][0] - ref64["totals"][0])
    own = abs(ref32["totals"][0] - ref64["totals"][0])
    print("total", got["totals"][0], ref32["totals"][0], ref64["totals"][0], err, own)
    assert err <= 4 * own + 1e-5 * max(1.0, abs(ref64["totals"][0]))
    for name in ("per", "g_logits", "g_value", "g_reward"):
        if ref32[name] is None:
            assert got[name] is None
            continue
        g = np.asarray(got[name], dtype=np.float64)
        atol = 1e-5 * max(1.0, np.abs(ref32[name]).max())
        err, own = np.abs(g - ref64[name]).max(), np.abs(ref32[name] - ref64[name]).max()
        print(name, "max |ref|", np.abs(ref32[name]).max(), "err vs f64", err, "torch f32 vs f64", own)
        np.testing.assert_allclose(g, ref32[name], rtol=1e-3, atol=atol, err_msg=name)
        assert err <= 4 * own + atol, name


@pytest.mark.parametrize("transform", [True, False])
@pytest.mark.parametrize("B,K,A", SHAPES)
def test_host_twin_matches_torch_autograd(B, K, A, transform):
    import mzgo
    inp = make_inputs(B, K, A)
    per, totals, g_logits, g_value, g_reward = mzgo.unroll_loss_host(
        inp["logits"], inp["value"], inp["reward"] if K else None, inp["t_pol"], inp["t_val"],
        inp["t_rew"] if K else None, value_transform=transform, **WEIGHTS)
    got = dict(per=per, totals=totals, g_logits=g_logits, g_value=g_value, g_reward=g_reward)
    check_against_reference(got, torch_reference(inp, torch.float32, "cpu", transform),
                            torch_reference(inp, torch.float64, "cpu", transform))


def test_inputs_hold_the_edge_cases():
    A = 82
    inp = make_inputs(5, 10, A)
    rows = inp["t_pol"].reshape(-1, A)
    assert any((row == 1).sum() == 1 and (row == 0).sum() == A - 1 for row in rows)
    assert any((row == 0).sum() == A // 2 for row in rows)
    assert any((row == np.float32(1.0 / A)).all() for row in rows)
    assert np.abs(inp["logits"][0, 0]).max() > 30
    assert inp["value"][0, 0] == 0.0 and inp["value"][10, 4] < 0
    assert set(np.unique(inp["t_rew"])) == {-1.0, 0.0, 1.0}


def test_value_gradient_at_zero_is_autograds():
    """h'(0) = 0.001: torch's sign(0) = 0 removes the square-root branch."""
    import mzgo
    A = 26
    z = np.zeros((1, 1), np.float32)
    t_pol = np.full((1, 1, A), np.float32(1.0 / A))
    out = mzgo.unroll_loss_host(np.zeros((1, 1, A), np.float32), z, None, t_pol, z + 3.0, None,
                                value_loss_weight=1.0, policy_loss_weight=1.0, reward_loss_weight=1.0,
                                value_transform=True)
    v = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    from mzgo.trainer import reward_value_transform
    h3 = reward_value_transform(torch.tensor([3.0], dtype=torch.float64))
    ((reward_value_transform(v) - h3) ** 2).sum().backward()
    assert v.grad.item() == pytest.approx(2 * (0 - h3.item()) * 0.001, rel=1e-12)
    assert out[3][0, 0] == pytest.approx(v.grad.item(), rel=1e-6)
    # the uniform row against uniform logits: KL = A t log(t A) ~ 0, gradient p T - t with T = A float32(1/A)
    T = float(t_pol.astype(np.float64).sum())
    np.testing.assert_allclose(out[2][0, 0], np.full(A, T / A - np.float32(1.0 / A)), atol=1e-7)


def _host_call(**over):
    from mzgo import _lib
    B, K, A = over.pop("B", 2), over.pop("K", 1), over.pop("A", 26)
    f = lambda *s: np.zeros(s, np.float32)
    a = dict(logits=f(K + 1, B, A), value=f(K + 1, B), reward=f(max(K, 1), B), t_pol=f(B, K + 1, A),
             t_val=f(B, K + 1), t_rew=f(B, max(K, 1)), per_sample=f(B), totals=np.zeros(4), g_logits=f(K + 1, B, A),
             g_value=f(K + 1, B), g_reward=f(max(K, 1), B))
    a.update(over)
    p = lambda k: _lib.ptr(a[k])
    rc = _lib.lib.mzgo_unroll_loss_host(p("logits"), p("value"), p("reward"), p("t_pol"), p("t_val"), p("t_rew"),
                                        over.get("B_arg", B), over.get("K_arg", K), over.get("A_arg", A), 1.0, 1.0,
                                        1.0, 1, p("per_sample"), p("totals"), p("g_logits"), p("g_value"),
                                        p("g_reward"))
    return rc, _lib.lib.mzgo_last_error().decode()


def test_einval_refusals():
    from mzgo import _lib
    assert _host_call()[0] == _lib.MZGO_OK
    for over, text in ((dict(B_arg=0), "B must be >= 1"), (dict(K_arg=-1), "K must be >= 0"),
                       (dict(A_arg=1), "A 1 out of range"), (dict(A_arg=363), "A 363 out of range"),
                       (dict(logits=None), "null logits"), (dict(t_val=None), "null t_val"),
                       (dict(totals=None), "null totals"), (dict(g_value=None), "null g_value"),
                       (dict(reward=None), "null reward"), (dict(g_reward=None), "null g_reward")):
        rc, msg = _host_call(**over)
        assert rc == _lib.MZGO_EINVAL and text in msg and "mzgo_unroll_loss_host" in msg, (over, msg)
    # K = 0 has no reward tensors
    assert _host_call(K=0, reward=None, t_rew=None, g_reward=None)[0] == _lib.MZGO_OK
    # the device entry checks its arguments before any device work
    lib = _lib.lib
    none6 = [None] * 6
    rc = lib.mzgo_unroll_loss(*none6, 0, 1, 26, 1.0, 1.0, 1.0, 1, None, None, None, None, None, None)
    assert rc == _lib.MZGO_EINVAL and b"mzgo_unroll_loss: B must be >= 1" in lib.mzgo_last_error()
    rc = lib.mzgo_unroll_loss(*none6, 1, -2, 26, 1.0, 1.0, 1.0, 1, None, None, None, None, None, None)
    assert rc == _lib.MZGO_EINVAL and b"K must be >= 0" in lib.mzgo_last_error()
    rc = lib.mzgo_unroll_loss(*none6, 1, 1, 400, 1.0, 1.0, 1.0, 1, None, None, None, None, None, None)
    assert rc == _lib.MZGO_EINVAL and b"A 400 out of range (2..362)" in lib.mzgo_last_error()
    rc = lib.mzgo_unroll_loss(*none6, 1, 1, 26, 1.0, 1.0, 1.0, 1, None, None, None, None, None, None)
    assert rc == _lib.MZGO_EINVAL and b"mzgo_unroll_loss: null logits" in lib.mzgo_last_error()


def test_unroll_loss_refuses_cpu_tensors():
    import mzgo
    inp = {k: torch.from_numpy(np.array(v)) for k, v in make_inputs(3, 1, 26).items()}
    with pytest.raises(ValueError, match="runs on the GPU"):
        mzgo.unroll_loss(inp["logits"], inp["value"], inp["reward"], inp["t_pol"], inp["t_val"], inp["t_rew"],
                         value_transform=True, **WEIGHTS)


def test_fused_loss_refuses_reference_mode():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    net = mzgo.MuZeroNet(32, 26)
    with pytest.raises(ValueError, match="fused_loss"):
        MuZeroTrainer(net, TrainConfig(fused_loss=True), mode="reference")
    assert TrainConfig().fused_loss is False and TrainConfig().sample_priorities is False
    MuZeroTrainer(net, TrainConfig(fused_loss=True), mode="batched")


def test_sample_priorities_on_a_host_buffer():
    """Batched step on the CPU (torch loss): with ``sample_priorities`` game
    indices[b] gets its own loss, unsampled games keep theirs; unset, every
    sampled game gets the batch mean."""
    import mzgo
    from mzgo.trainer import MuZeroTrainer, PrioritizedReplayBuffer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    N, C = 5, 32
    A = N * N + 1
    trajs = synthetic_trajectories(N, 5, seed=3)
    for flag in (True, False):
        net = mzgo.MuZeroNet(C, A)
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 1))
        buf = PrioritizedReplayBuffer(10)
        for t in trajs:
            buf.add(t)
        seen = {}
        sample = buf.sample
        buf.sample = lambda n: seen.setdefault("s", sample(n))
        np.random.seed(4)
        tr = MuZeroTrainer(net, TrainConfig(unroll_steps=3, sample_priorities=flag), mode="batched",
                           start_index=lambda T: T // 2)
        avg = tr.train(buf, 3)
        idx = list(seen["s"][1])
        rest = [i for i in range(5) if i not in idx]
        assert all(buf.priorities[i] == 1.0 for i in rest)
        if flag:
            per = tr.last_per_sample
            assert per.shape == (3,) and per.dtype == np.float32 and len(set(per.tolist())) == 3
            assert [buf.priorities[i] for i in idx] == [float(p) for p in per]
            assert float(per.astype(np.float64).mean()) == pytest.approx(avg, rel=1e-5)
        else:
            assert tr.last_per_sample is None
            assert [buf.priorities[i] for i in idx] == [avg] * 3
    # a zero loss still leaves a positive weight for np.random.choice
    tr.config.sample_priorities = True
    tr.last_per_sample = np.array([0.0, 2.5], np.float32)
    assert tr._priorities(1.0, 2) == [float(np.finfo(np.float32).tiny), 2.5]
