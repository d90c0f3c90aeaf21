"""The device optimizer's formulas on the CPU (csrc/mzgo_optim.hpp through
``mzgo_optim_step_host`` / ``mzgo.adam_step_host``) against torch's own
``clip_grad_norm_`` + ``torch.optim.Adam`` (``AdamW``) + ``StepLR`` run in
float64 from the same float32 state.

Bars, elementwise, with lr the step's rate and |g|max the largest gradient
entry of the tensor:

    |p' - ref| <= 2^-22 |ref| + 2^-22 lr
    |m' - ref| <= 2^-22 max(|ref|, |g|max)
    |v' - ref| <= 2^-22 max(|ref|, |g|max^2)

Each output is rounded to float32 once (2^-24); the clip coefficient is rounded
to float32 once, which enters m once (2^-24), v twice (2^-23) and p through
m / sqrt(v) (at most 2^-23); the sum is below 2^-22, and the update's magnitude
is of the order of lr.  The norm is a float64 sum in another order than
torch's: relative 2^-40.  The learning rate against StepLR's sequence:
relative 2^-50.

``shape_set`` / ``make_state`` / ``torch_step`` / ``assert_step_close`` are
shared with tests/test_gpu_optim.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mzgo
from mzgo._lib import MZGO_EINVAL, MzgoError, OptimHyper, lib

CH = mzgo.optim_chunk()
NUMELS = [1, 3, 4, 5, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH + 7]
EPS22 = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def shape_set():
    """The numels at which the kernels take another path (a lone element, around
    a thread's four, around a wave's and a workgroup's share, around one chunk,
    more than two chunks with a ragged tail) and the 22 shapes of the smallest
    reference net, MuZeroNet(16, 5) at N = 2."""
    net = mzgo.MuZeroNet(16, 5)
    return tuple((n,) for n in NUMELS) + tuple(tuple(p.shape) for p in net.parameters())


@functools.lru_cache(maxsize=None)
def make_state(seed, shapes, steps_before, gscale=1.0):
    """float32 (params, grads, exp_avg, exp_avg_sq) and the step counts: the
    moments are zero before the first step and of the gradients' scale later."""
    r = np.random.default_rng(seed)
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    p = [f32(r.normal(size=s)) for s in shapes]
    g = [f32(r.normal(size=s) * gscale) for s in shapes]
    if steps_before:
        m = [f32(r.normal(size=s) * 0.3 * gscale) for s in shapes]
        v = [f32((r.random(size=s) + 0.01) * gscale * gscale) for s in shapes]
    else:
        m = [np.zeros(s, np.float32) for s in shapes]
        v = [np.zeros(s, np.float32) for s in shapes]
    for a in p + g + m + v:
        a.setflags(write=False)
    return p, g, m, v, np.full(len(shapes), steps_before, np.int64)


def torch_step(p, g, m, v, steps, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
               max_grad_norm=None, dtype=torch.float64):
    """clip_grad_norm_ + Adam / AdamW from the given state with torch's own
    code in ``dtype``: (params, exp_avg, exp_avg_sq, step counts, norm)."""
    P = [torch.tensor(x, dtype=dtype, requires_grad=True) for x in p]
    for t, x in zip(P, g):
        if x is not None:
            t.grad = torch.tensor(x, dtype=dtype)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(P, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    for t, a, b, k in zip(P, m, v, steps):
        opt.state[t] = dict(step=torch.tensor(float(k)), exp_avg=torch.tensor(a, dtype=dtype),
                            exp_avg_sq=torch.tensor(b, dtype=dtype))
    norm = torch.nn.utils.clip_grad_norm_(P, float("inf") if max_grad_norm is None else max_grad_norm)
    opt.step()
    st = [opt.state[t] for t in P]
    return ([t.detach().numpy() for t in P], [s["exp_avg"].numpy() for s in st], [s["exp_avg_sq"].numpy() for s in st],
            np.array([int(s["step"]) for s in st]), float(norm))


def step_errors(got, ref, g, lr):
    """Per tensor, the largest (error / bar) of p, m and v against ``ref``."""
    out = []
    for i in range(len(ref[0])):
        gm = 0.0 if g[i] is None or g[i].size == 0 else float(np.abs(g[i]).max())
        rp, rm, rv = (np.asarray(ref[j][i], dtype=np.float64) for j in range(3))
        ep = np.abs(got[0][i] - rp) / (EPS22 * np.abs(rp) + EPS22 * lr)
        em = np.abs(got[1][i] - rm) / (EPS22 * np.maximum(np.abs(rm), gm) + 1e-300)
        ev = np.abs(got[2][i] - rv) / (EPS22 * np.maximum(np.abs(rv), gm * gm) + 1e-300)
        out.append(tuple(float(e.max()) if e.size else 0.0 for e in (ep, em, ev)))
    return out


def assert_step_close(got, ref, g, lr, what=""):
    errs = step_errors(got, ref, g, lr)
    bad = [(i, e) for i, e in enumerate(errs) if max(e) > 1.0]
    assert not bad, f"{what}: (tensor, (p, m, v) error / bar) {bad}"


DECAYS = {"none": dict(weight_decay=0.0), "classic": dict(weight_decay=0.05),
          "decoupled": dict(weight_decay=0.05, decoupled=True)}


@functools.lru_cache(maxsize=None)
def one_step(steps_before, clip, decay, gscale):
    p, g, m, v, steps = make_state(7, shape_set(), steps_before, gscale)
    kw = DECAYS[decay]
    got = mzgo.adam_step_host(p, g, m, v, steps, lr=1e-2, max_grad_norm=clip, weight_decay=kw["weight_decay"],
                              decoupled_weight_decay=kw.get("decoupled", False))
    ref = torch_step(p, g, m, v, steps, lr=1e-2, max_grad_norm=clip, **kw)
    return g, got, ref


@pytest.mark.parametrize("gscale", [1.0, 1e-7, 1e3])
@pytest.mark.parametrize("decay", list(DECAYS))
@pytest.mark.parametrize("clip", [None, 1.0, 1e9])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_one_step_against_float64(step, clip, decay, gscale):
    g, got, ref = one_step(step - 1, clip, decay, gscale)
    gp, gm, gv, steps, sched, skipped, record = got
    norm, coef, lr, applied = record
    assert applied == 1.0 and skipped == 0 and sched == 1 and lr == 1e-2
    assert abs(norm - ref[4]) <= 2.0 ** -40 * ref[4], (norm, ref[4])
    if clip is None or clip == 1e9 or gscale == 1e-7:
        assert coef == 1.0
    else:
        assert 0.0 < coef < 1.0 and coef == float(np.float32(clip / (norm + 1e-6)))
    assert (steps == step).all() and (ref[3] == step).all()
    for a in gp + gm + gv:
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert_step_close(got, ref, g, lr, f"step {step} clip {clip} {decay} gscale {gscale}")


def test_eps_matters_at_small_gradients():
    """At gradients of 1e-7 the denominator sqrt(v) is of eps's order: a twin
    that dropped eps would miss the float64 reference by far more than the bar."""
    g, got, ref = one_step(0, None, "none", 1e-7)
    p = make_state(7, shape_set(), 0, 1e-7)[0]
    moved = max(float(np.abs(a - b).max()) for a, b in zip(got[0], p))
    assert 0.5e-2 < moved < 0.99e-2          # lr * g / (|g| + eps) with |g| ~ 1e-7, eps 1e-8: below lr = 1e-2


def test_step_lr_sequence():
    p, g, m, v, steps = make_state(3, ((5,), (CH + 1,)), 0)
    P = [torch.zeros(1, requires_grad=True)]
    opt = torch.optim.Adam(P, lr=3e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
    count = 0
    for call in range(8):
        want = opt.param_groups[0]["lr"]
        p, m, v, steps, count, skipped, record = mzgo.adam_step_host(p, g, m, v, steps, sched=count, lr=3e-3,
                                                                    lr_step_size=3, lr_gamma=0.5)
        assert count == call + 1 and skipped == 0
        assert abs(record[2] - want) <= 2.0 ** -50 * want, (call, record[2], want)
        opt.step()
        sched.step()
    assert record[2] == 3e-3 * 0.25


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_gradient_is_refused(bad):
    shapes = shape_set()
    p, g, m, v, steps = make_state(11, shapes, 4)
    kw = dict(lr=1e-2, max_grad_norm=1.0, lr_step_size=1000, lr_gamma=0.9)
    gb = [x.copy() for x in g]
    gb[10].reshape(-1)[CH + 3] = bad                   # one element of one tensor, in its second chunk
    p1, m1, v1, s1, sched, skipped, record = mzgo.adam_step_host(p, gb, m, v, steps, **kw)
    for a, b in zip(p1 + m1 + v1, p + m + v):
        assert a.tobytes() == b.tobytes()
    assert (s1 == steps).all() and skipped == 1 and sched == 1
    assert record[3] == 0.0 and not np.isfinite(record[0])
    after = mzgo.adam_step_host(p1, g, m1, v1, s1, sched=sched, skipped=skipped, **kw)
    fresh = mzgo.adam_step_host(p, g, m, v, steps, sched=1, skipped=0, **kw)
    for a, b in zip(after[0] + after[1] + after[2], fresh[0] + fresh[1] + fresh[2]):
        assert a.tobytes() == b.tobytes()
    assert (after[3] == steps + 1).all() and after[4] == 2 and after[5] == 1
    assert after[6].tobytes() == fresh[6].tobytes() and after[6][3] == 1.0


def test_missing_gradients():
    shapes = ((CH + 1,), (7,), (256,), (3, 5), (2 * CH,))
    p, g, m, v, steps = make_state(5, shapes, 2)
    g = [None if i in (1, 3) else x for i, x in enumerate(g)]
    got = mzgo.adam_step_host(p, g, m, v, steps, lr=1e-2, max_grad_norm=1.0)
    ref = torch_step(p, g, m, v, steps, lr=1e-2, max_grad_norm=1.0)
    for i in (1, 3):
        for a, b in ((got[0][i], p[i]), (got[1][i], m[i]), (got[2][i], v[i])):
            assert a.tobytes() == b.tobytes()
    assert got[3].tolist() == [3, 2, 3, 2, 3] and ref[3].tolist() == [3, 2, 3, 2, 3]
    own = np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in g if x is not None))
    assert abs(got[6][0] - own) <= 2.0 ** -40 * own and abs(got[6][0] - ref[4]) <= 2.0 ** -40 * ref[4]
    assert_step_close(got, ref, g, 1e-2, "missing gradients")


def test_two_calls_give_the_same_bits():
    p, g, m, v, steps = make_state(7, shape_set(), 1)
    a = mzgo.adam_step_host(p, g, m, v, steps, lr=1e-2, max_grad_norm=1.0)
    b = mzgo.adam_step_host(p, g, m, v, steps, lr=1e-2, max_grad_norm=1.0)
    for x, y in zip(a[0] + a[1] + a[2] + [a[6]], b[0] + b[1] + b[2] + [b[6]]):
        assert x.tobytes() == y.tobytes()


# -- refusals -------------------------------------------------------------------
def _last_error():
    return lib.mzgo_last_error().decode()


def test_create_refusals():
    out = ctypes.c_void_p()
    numels = (ctypes.c_int64 * 2)(4, -1)
    assert lib.mzgo_optim_create(0, numels, 0, ctypes.byref(out)) == MZGO_EINVAL
    assert "n must be >= 1, got 0" in _last_error()
    assert lib.mzgo_optim_create(-3, numels, 0, ctypes.byref(out)) == MZGO_EINVAL
    assert "n must be >= 1, got -3" in _last_error()
    assert lib.mzgo_optim_create(2, numels, 0, ctypes.byref(out)) == MZGO_EINVAL
    assert "numels[1] must be >= 0, got -1" in _last_error()
    assert lib.mzgo_optim_create(2, None, 0, ctypes.byref(out)) == MZGO_EINVAL
    assert "null numels" in _last_error()
    assert lib.mzgo_optim_create(2, numels, 0, None) == MZGO_EINVAL
    assert "null out" in _last_error()
    assert not out.value


def _host_call(n=1, numels=(4,), null=None, **hyper):
    h = dict(lr0=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, max_norm=1.0, step_size=10,
             gamma=0.5)
    h.update(hyper)
    arrays = [np.zeros(4, np.float32) for _ in range(4)]
    tables = {k: (ctypes.c_void_p * 1)(a.ctypes.data) for k, a in zip(("params", "grads", "exp_avg", "exp_avg_sq"),
                                                                      arrays)}
    steps = np.zeros(1, np.int64)
    sched, skipped = ctypes.c_int64(), ctypes.c_int64()
    record = np.zeros(4)
    args = dict(numels=(ctypes.c_int64 * len(numels))(*numels), **tables, hyper=ctypes.byref(OptimHyper(**h)),
                steps=steps.ctypes.data_as(ctypes.c_void_p), sched=ctypes.byref(sched), skipped=ctypes.byref(skipped),
                record=record.ctypes.data_as(ctypes.c_void_p))
    if null:
        args[null] = None
    return lib.mzgo_optim_step_host(n, *(args[k] for k in ("numels", "params", "grads", "exp_avg", "exp_avg_sq",
                                                           "hyper", "steps", "sched", "skipped", "record")))


@pytest.mark.parametrize("kw, text", [
    (dict(n=0), "n must be >= 1, got 0"),
    (dict(numels=(-4,)), "numels[0] must be >= 0, got -4"),
    (dict(null="numels"), "null numels"),
    (dict(null="params"), "null params table"),
    (dict(null="grads"), "null grads table"),
    (dict(null="exp_avg"), "null exp_avg table"),
    (dict(null="exp_avg_sq"), "null exp_avg_sq table"),
    (dict(null="hyper"), "null hyper"),
    (dict(null="steps"), "null steps"),
    (dict(null="record"), "null record"),
    (dict(beta1=1.0), "beta1 must be in [0, 1), got 1"),
    (dict(beta1=-0.1), "beta1 must be in [0, 1), got -0.1"),
    (dict(beta2=1.5), "beta2 must be in [0, 1), got 1.5"),
    (dict(beta2=float("nan")), "beta2 must be in [0, 1)"),
    (dict(eps=0.0), "eps must be finite and > 0, got 0"),
    (dict(eps=-1e-8), "eps must be finite and > 0"),
    (dict(step_size=0), "step_size must be >= 1, got 0"),
    (dict(lr0=-1.0), "lr0 must be finite and >= 0"),
    (dict(weight_decay=-1.0), "weight_decay must be finite and >= 0"),
    (dict(max_norm=float("nan")), "max_norm is NaN"),
    (dict(gamma=float("inf")), "gamma must be finite and >= 0"),
])
def test_step_host_refusals(kw, text):
    assert _host_call(**kw) == MZGO_EINVAL
    assert "mzgo_optim_step_host" in _last_error() and text in _last_error()


def test_step_host_accepts_the_valid_call():
    assert _host_call() == 0


def test_null_tensor_and_python_refusals():
    p = [np.zeros(4, np.float32)]
    with pytest.raises(MzgoError, match=r"beta1 must be in \[0, 1\)"):
        mzgo.adam_step_host(p, p, p, p, [0], betas=(1.0, 0.999))
    with pytest.raises(MzgoError, match="eps must be finite and > 0"):
        mzgo.adam_step_host(p, p, p, p, [0], eps=0.0)
    with pytest.raises(MzgoError, match="step_size must be >= 1"):
        mzgo.adam_step_host(p, p, p, p, [0], lr_step_size=0)
    with pytest.raises(MzgoError, match="n must be >= 1"):
        mzgo.adam_step_host([], [], [], [], [])
    with pytest.raises(ValueError, match="float32 CUDA tensors"):
        mzgo.DeviceAdam([torch.zeros(3)])
    with pytest.raises(ValueError, match="empty parameter list"):
        mzgo.DeviceAdam([])


def test_trainer_switch_refusals():
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    net = mzgo.MuZeroNet(16, 26)
    with pytest.raises(ValueError, match="device_optimizer needs mode='batched'"):
        MuZeroTrainer(net, TrainConfig(device_optimizer=True), mode="reference")
    with pytest.raises(ValueError, match="device_optimizer needs the net on the GPU"):
        MuZeroTrainer(net, TrainConfig(device_optimizer=True), mode="batched")
    tr = MuZeroTrainer(net, TrainConfig(), mode="batched")
    assert isinstance(tr.optimizer, torch.optim.Adam) and tr.scheduler is not None
    with pytest.raises(ValueError, match="skipped_steps belongs to device_optimizer"):
        tr.skipped_steps()
