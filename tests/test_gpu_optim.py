"""The device optimizer on the GPU (csrc/mzgo_optim.hip through
``mzgo.DeviceAdam`` and ``TrainConfig.device_optimizer``).

* The three launches against the host twin (``mzgo.adam_step_host``): the same
  bits for parameters, moments, step counts and the step record, at the CPU
  test's shape set, at parameters and gradients that are views one float into
  their allocation (the single-float path), and at 200 and 1030 small tensors
  (more than one launch's by-value block of addresses).
* 25 steps and a checkpoint exchange against torch's own clip_grad_norm_ +
  Adam + StepLR: the float64 run is the reference, and DeviceAdam's distance
  from it is at most 4x the float32 torch run's in the same test (two float32
  legs round differently along 25 steps), never asked tighter than
  2^-22 |p|max (tests/test_optim.py's one-step bar).
* The trainer's step with the switch on and off, the engines' weights after
  it, and a NaN gradient.
"""
import numpy as np
import pytest
import torch

from test_optim import CH, make_state, shape_set

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, max_grad_norm=1.0, lr_step_size=3, lr_gamma=0.5)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _views(arrays, offset):
    """CUDA copies of ``arrays``, each a contiguous view ``offset`` floats into an allocation of its own."""
    out = []
    for a in arrays:
        buf = torch.zeros(a.size + offset, device="cuda")
        t = buf[offset:offset + a.size].view(a.shape)
        t.copy_(torch.from_numpy(np.array(a)))
        assert t.is_contiguous() and t.data_ptr() % 16 == (buf.data_ptr() + 4 * offset) % 16
        out.append(t)
    return out


def _device_step(state, p_off, g_off, none=(), sched=7, **kw):
    """One DeviceAdam step from ``state`` (make_state's) loaded through
    load_state_dict: numpy (p, m, v, steps, sched, skipped, record)."""
    import mzgo
    p, g, m, v, steps = state
    P = _views(p, p_off)
    for i, (t, x) in enumerate(zip(P, _views(g, g_off))):
        t.grad = None if i in none else x
    opt = mzgo.DeviceAdam(P, **kw)
    h = opt.hyper
    opt.load_state_dict({
        "state": {i: dict(step=torch.tensor(float(steps[i])), exp_avg=torch.from_numpy(np.array(m[i])),
                          exp_avg_sq=torch.from_numpy(np.array(v[i]))) for i in range(len(p))},
        "param_groups": [dict(lr=h.lr0, initial_lr=h.lr0, betas=(h.beta1, h.beta2), eps=h.eps,
                              weight_decay=h.weight_decay, decoupled_weight_decay=bool(h.decoupled),
                              params=list(range(len(p))))],
        "schedule": {"count": sched}})
    versions = [t._version for t in P]
    opt.step()
    assert all(t._version > k for t, k in zip(P, versions))
    rec = opt.record
    assert rec.is_cuda and rec.dtype == torch.float64 and rec.shape == (4,)
    st, sc, sk = opt.counts()
    return ([t.cpu().numpy() for t in P], [t.cpu().numpy() for t in opt.exp_avg],
            [t.cpu().numpy() for t in opt.exp_avg_sq], st, sc, sk, rec.cpu().numpy())


def _assert_same(got, want):
    for j, name in enumerate(("p", "m", "v")):
        for i, (a, b) in enumerate(zip(got[j], want[j])):
            assert _bits(a) == _bits(b), f"{name}[{i}] (shape {a.shape}): {np.abs(a - b).max()}"
    assert got[3].tolist() == want[3].tolist() and got[4] == want[4] and got[5] == want[5]
    assert _bits(got[6]) == _bits(want[6]), (got[6], want[6])


CASES = {
    # name: (shapes, p offset, g offset, tensors without gradient, extra hyper)
    "shape_set": (None, 0, 0, (), dict(weight_decay=0.05)),
    "param_views": (None, 1, 0, (), {}),
    "grad_views": (None, 0, 3, (2, 5), dict(weight_decay=0.05, decoupled_weight_decay=True)),
    "200_tensors": (tuple((i % 7 + 1,) for i in range(199)) + ((CH + 5,),), 0, 0, (0, 95, 96, 198), {}),
    "1030_tensors": (tuple((i % 5 + 1,) for i in range(1030)), 0, 0, (1029,), {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_gives_the_host_twins_bits(case):
    import mzgo
    shapes, p_off, g_off, none, extra = CASES[case]
    state = make_state(21, shapes or shape_set(), 3)
    kw = dict(HYPER, **extra)
    p, g, m, v, steps = state
    want = mzgo.adam_step_host(p, [None if i in none else x for i, x in enumerate(g)], m, v, steps, sched=7, **kw)
    assert want[6][3] == 1.0 and want[6][1] < 1.0 and want[6][2] == 1e-2 * 0.25
    got = _device_step(state, p_off, g_off, none, **kw)
    _assert_same(got, want)
    again = _device_step(state, p_off, g_off, none, **kw)
    _assert_same(again, got)


def test_device_refuses_a_non_finite_gradient_like_the_twin():
    import mzgo
    p, g, m, v, steps = state = make_state(22, shape_set(), 3)
    gb = [x.copy() for x in g]
    gb[10].reshape(-1)[CH + 3] = float("inf")
    want = mzgo.adam_step_host(p, gb, m, v, steps, sched=7, **HYPER)
    got = _device_step((p, gb, m, v, steps), 0, 0, **HYPER)
    assert want[5] == 1 and want[6][3] == 0.0
    _assert_same(got, want)
    for a, b in zip(got[0] + got[1] + got[2], p + m + v):
        assert _bits(a) == _bits(b)


# -- against torch's own optimizer -------------------------------------------------
def _net_params(dtype=torch.float32):
    import mzgo
    sd = mzgo.deterministic_state_dict(16, 5, 3)
    net = mzgo.MuZeroNet(16, 5)
    net.load_state_dict(sd)
    return [p.detach().to("cuda", dtype).clone().requires_grad_() for p in net.parameters()]


def _grads(step, params):
    """Fixed pseudo-random gradients of step ``step``, the same for every leg
    (float32 values; scales from 1e-2 to 10 across the tensors)."""
    gen = torch.Generator().manual_seed(1000 + step)
    return [(torch.randn(p.shape, generator=gen) * 10.0 ** (i % 4 - 2)).to("cuda") for i, p in enumerate(params)]


def _torch_steps(P, first, last, opt=None):
    """Steps first..last-1 of the parent's tail: clip_grad_norm_ + Adam.step + StepLR.step."""
    opt = opt or torch.optim.Adam(P, lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
    for s in range(first, last):
        for p, g in zip(P, _grads(s, P)):
            p.grad = g.to(p.dtype)
        torch.nn.utils.clip_grad_norm_(P, max_norm=1.0)
        opt.step()
        sched.step()
    return opt


def _device_steps(P, first, last, opt=None):
    import mzgo
    opt = opt or mzgo.DeviceAdam(P, lr=1e-2, lr_step_size=10, lr_gamma=0.5, max_grad_norm=1.0)
    for s in range(first, last):
        opt.zero_grad()
        for p, g in zip(P, _grads(s, P)):
            p.grad = g
        opt.step()
    return opt


def distances(P_dev, P_f32, P_f64):
    """Per tensor (DeviceAdam's, torch float32's) largest distance from the float64 leg, and |p|max."""
    out = []
    for a, b, r in zip(P_dev, P_f32, P_f64):
        out.append((float((a.detach().double() - r.detach()).abs().max()),
                    float((b.detach().double() - r.detach()).abs().max()), float(r.detach().abs().max())))
    return out


def assert_within_torchs_own_error(pairs, what):
    bad = [(i, d, t, m) for i, (d, t, m) in enumerate(pairs) if d > max(4.0 * t, 2.0 ** -22 * m)]
    assert not bad, (f"{what}: (tensor, DeviceAdam - f64, torch f32 - f64, |p|max) over the bar {bad}; "
                     f"all pairs {[(f'{d:.3e}', f'{t:.3e}') for d, t, _ in pairs]}")


def run_25_steps():
    P_dev, P_f32, P_f64 = _net_params(), _net_params(), _net_params(torch.float64)
    opt = _device_steps(P_dev, 0, 25)
    _torch_steps(P_f32, 0, 25)
    _torch_steps(P_f64, 0, 25)
    return opt, distances(P_dev, P_f32, P_f64)


def test_25_steps_against_the_parent_path():
    opt, pairs = run_25_steps()
    print([(f"{d:.3e}", f"{t:.3e}") for d, t, _ in pairs])
    steps, sched, skipped = opt.counts()
    assert (steps == 25).all() and sched == 25 and skipped == 0
    assert opt.lr == 1e-2 * 0.25 and opt.record[2].item() == 1e-2 * 0.25      # the 25th step's rate, the 26th's
    assert opt.record[3].item() == 1.0 and 0.0 < opt.record[1].item() < 1.0
    assert_within_torchs_own_error(pairs, "25 steps")


def test_checkpoint_exchange_both_ways():
    import mzgo
    P_f32, P_f64 = _net_params(), _net_params(torch.float64)
    _torch_steps(P_f32, 0, 5)
    _torch_steps(P_f64, 0, 5)
    # torch -> DeviceAdam
    P = _net_params()
    sd = _torch_steps(P, 0, 3).state_dict()
    opt = mzgo.DeviceAdam(P, lr=1e-2, lr_step_size=10, lr_gamma=0.5, max_grad_norm=1.0)
    opt.load_state_dict(sd)
    assert (opt.counts()[0] == 3).all()
    _device_steps(P, 3, 5, opt)
    assert_within_torchs_own_error(distances(P, P_f32, P_f64), "torch -> DeviceAdam")
    # DeviceAdam -> torch
    P = _net_params()
    sd = _device_steps(P, 0, 3).state_dict()
    assert sd["schedule"] == {"count": 3, "skipped": 0} and sorted(sd["state"]) == list(range(len(P)))
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values())
    adam = torch.optim.Adam(P, lr=1e-2)
    adam.load_state_dict(sd)
    _torch_steps(P, 3, 5, adam)
    assert_within_torchs_own_error(distances(P, P_f32, P_f64), "DeviceAdam -> torch")


# -- the trainer -------------------------------------------------------------------
N_, C_, B_, K_ = 6, 64, 8, 3


def _trainer_step(device_optimizer, device_weights=False):
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    A = N_ * N_ + 1
    rp = mzgo.DeviceReplay(N_, B_, int(1.5 * N_ * N_), "cuda")
    for t in synthetic_trajectories(N_, B_, seed=9):
        rp.add(t)
    net = mzgo.MuZeroNet(C_, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C_, A, 6))
    cfg = TrainConfig(learning_rate=1e-3, unroll_steps=K_, fused_loss=True, fused_unroll=True, device_sampling=True,
                      device_weights=device_weights, device_optimizer=device_optimizer)
    tr = MuZeroTrainer(net, cfg, mode="batched", sample_seed=5)
    grads = []
    tail = tr._optimizer_step

    def snap():                          # the gradients as backward() left them (clip_grad_norm_ scales them in place)
        grads.extend(p.grad.detach().clone() for p in net.parameters())
        return tail()

    tr._optimizer_step = snap
    assert tr.train(rp, B_) is not None
    return net, tr, grads, dict(tr.read_stats())


def test_trainer_step_equals_the_torch_tail():
    import mzgo
    net_on, tr_on, g_on, last_on = _trainer_step(True)
    net_off, tr_off, g_off, last_off = _trainer_step(False)
    assert isinstance(tr_on.optimizer, mzgo.DeviceAdam) and tr_on.scheduler is None
    assert isinstance(tr_off.optimizer, torch.optim.Adam)
    for (k, _), a, b in zip(net_on.named_parameters(), g_on, g_off):
        assert torch.equal(a, b), f"gradient of {k}"
    lr = 1e-3
    for (k, p), q in zip(net_on.named_parameters(), net_off.parameters()):
        bar = 2.0 ** -23 * q.detach().abs() + 2.0 ** -19 * lr
        worst = ((p.detach() - q.detach()).abs() / bar).max().item()
        assert worst <= 1.0, f"{k}: |p_on - p_off| is {worst} of the bar"
    for k in ("training_loss", "value_loss", "policy_loss", "reward_loss"):
        assert last_on[k] == pytest.approx(last_off[k], rel=1e-5), k
    assert last_on["lr"] == last_off["lr"] == lr
    assert tr_on.skipped_steps() == 0
    # p.grad keeps the unclipped gradient with the switch on; clip_grad_norm_ scaled it with the switch off
    coef = tr_on.optimizer.record[1].item()
    assert 0.0 < coef < 1.0
    assert torch.equal(next(net_on.parameters()).grad, g_on[0])
    assert not torch.equal(next(net_off.parameters()).grad, g_off[0])


def _blob_of(net):
    from mzgo.engine import Engine, EngineConfig
    fresh = Engine(EngineConfig(board_size=net.board_size, latent_dim=net.latent_dim, num_games=1, num_simulations=1,
                                compat="fixed"))
    fresh.set_state_dict(net.state_dict())
    return fresh.export_weights()


def test_trainer_step_reaches_the_engines_with_device_weights():
    net, tr, _, _ = _trainer_step(True, device_weights=True)
    before = _blob_of_state(net, 6)
    want = _blob_of(net)
    assert _bits(want) != _bits(before)                              # (the step moved the weights)
    assert _bits(net.engine().export_weights()) == _bits(want)       # stale without step()'s version mark


def _blob_of_state(net, seed):
    import mzgo
    A = net.board_size ** 2 + 1
    old = mzgo.MuZeroNet(net.latent_dim, A).cuda()
    old.load_state_dict(mzgo.deterministic_state_dict(net.latent_dim, A, seed))
    return _blob_of(old)


def test_trainer_refuses_a_nan_gradient_on_the_device():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    A = N_ * N_ + 1
    net = mzgo.MuZeroNet(C_, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C_, A, 6))
    tr = MuZeroTrainer(net, TrainConfig(device_optimizer=True, device_weights=True), mode="batched")
    blob = net.engine().export_weights()
    before = [p.detach().clone() for p in net.parameters()]
    gen = torch.Generator().manual_seed(4)
    tr.optimizer.zero_grad()
    for p in net.parameters():                                       # backward()'s part
        p.grad = torch.randn(p.shape, generator=gen).cuda()
    net.dynamics.conv.weight.grad.view(-1)[12345] = float("nan")
    tr.optimizer.step()
    for (k, p), q in zip(net.named_parameters(), before):
        assert torch.equal(p.detach(), q), k
    assert tr.skipped_steps() == 1
    assert tr.optimizer.record[3].item() == 0.0
    assert (tr.optimizer.counts()[0] == 0).all()
    assert _bits(net.engine().export_weights()) == _bits(blob)
    # the next finite step is taken
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=gen).cuda()
    tr.optimizer.step()
    assert tr.skipped_steps() == 1 and (tr.optimizer.counts()[0] == 1).all()
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert _bits(net.engine().export_weights()) == _bits(_blob_of(net)) != _bits(blob)
