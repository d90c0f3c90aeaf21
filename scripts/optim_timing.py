"""The optimizer tail of the batched trainer step with
``TrainConfig.device_optimizer`` off and on (``mzgo.DeviceAdam``:
clip_grad_norm_, Adam and StepLR as one HIP call of three launches), at main.py's
sizes: 6x6, C = 128, batch 128 x unroll 10.  The baselines run in this same
process; the legs alternate.

EXPECTATION, written before the first run (DESIGN §4 "The optimizer tail as one
call"): the parent's tail -- ``clip_grad_norm_`` (foreach norm, stack, norm,
the coefficient's three ops, foreach mul), foreach ``Adam.step`` and
``StepLR.step`` over the 22 tensors -- is some two dozen small launches and
measured 0.239 ms ("Adam + clip_grad_norm_ alone").  DeviceAdam is
three launches at about 5 us each of enqueueing (the 5.3 us per eager launch of
profiles/loss_timing.json) plus the ctypes call and 44 ``data_ptr`` reads on the
host; the kernels move 7 x 1.1 MB.  So: the tail 0.24 -> about 0.03 ms by
events, and the whole step, which is GPU-bound since fused_unroll (5.42 ms
wall, 4.65 ms of it kernels), 5.42 -> about 5.2 ms.  What could undo it: the
step's GPU time is the floor, and of the tail's 0.24 ms only the part that is
GPU time (two dozen short kernels with their gaps) comes off it; the host part
was already hidden behind the unroll's kernels.

Figures, each best / median / spread (max - min) over REPS alternating windows
of STEPS after a warm-up of every leg:

* tail_{torch,torch_fused,device}_wall_ms / _event_ms   the optimizer part
      alone from fixed gradients: the parent's clip_grad_norm_ + foreach Adam +
      StepLR; torch's Adam(fused=True) + clip_grad_norm_ + StepLR (for
      information); DeviceAdam.  Wall time ends in a synchronise; the events
      bracket the same window.
* step_off_ms / step_on_ms   the whole ``train`` step from a ``DeviceReplay``
      with device_sampling + deferred_stats + fused_loss + device_weights +
      fused_unroll, without and with device_optimizer; wall and events.

Before timing, 25 steps of DeviceAdam and of the parent's float32 tail are
compared with the same tail in float64 (tests/test_gpu_optim.py's legs): the
per-tensor pairs of distances go into the output.

Usage (GPU box): python scripts/optim_timing.py [out.json] -> one JSON line
(also written to out.json when given).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

EXPECTATION = {
    "parent_tail_ms": 0.239,
    "parent_tail_launches": "some two dozen (foreach clip, foreach Adam)",
    "device_tail_launches": 3,
    "eager_launch_us": 5.3,
    "tail_ms": "0.24 -> about 0.03 by events",
    "whole_step_ms": "5.42 -> about 5.2",
    "risk": "the step is GPU-bound: only the tail's GPU time comes off it, its host time was already hidden",
}


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def main():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    from test_gpu_optim import run_25_steps
    steps, reps = (int(os.environ.get(k, d)) for k, d in (("STEPS", 10), ("REPS", 7)))
    N, C, B, K = 6, 128, 128, 10
    A = N * N + 1

    _, pairs = run_25_steps()
    accuracy = [{"device_minus_f64": d, "torch_f32_minus_f64": t, "p_absmax": m} for d, t, m in pairs]

    # -- the tail alone, from fixed gradients -------------------------------------
    def params():
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        return list(net.parameters())

    tails = {}
    for name in ("torch", "torch_fused", "device"):
        P = params()
        grads = [torch.randn(p.shape, generator=torch.Generator().manual_seed(i)).cuda() for i, p in enumerate(P)]
        if name == "device":
            opt = mzgo.DeviceAdam(P, lr=1e-4, max_grad_norm=1.0, lr_step_size=1000, lr_gamma=0.9)

            def tail(P=P, grads=grads, opt=opt):
                for p, g in zip(P, grads):
                    p.grad = g
                opt.step()
        else:
            opt = torch.optim.Adam(P, lr=1e-4, fused=(name == "torch_fused"))
            sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1000, gamma=0.9)

            def tail(P=P, grads=grads, opt=opt, sched=sched):
                for p, g in zip(P, grads):                  # (clip_grad_norm_ scales them in place: after the
                    p.grad = g                              # first passes the norm is 1 and the coefficient 1)
                torch.nn.utils.clip_grad_norm_(P, max_norm=1.0)
                opt.step()
                sched.step()
        tails[name] = tail

    # -- the whole step --------------------------------------------------------------
    trajs = synthetic_trajectories(N, B, seed=11)
    legs = ("off", "on")
    trainers, stores = {}, {}
    for name in legs:
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for tr in trajs:
            rp.add(tr)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=True, fused_unroll=True, device_optimizer=(name == "on"))
        trainers[name], stores[name] = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3), rp

    for tail in tails.values():
        for _ in range(5):
            tail()
    for name in legs:
        for _ in range(3):
            trainers[name].train(stores[name], B)
    torch.cuda.synchronize()

    t = {f"tail_{n}_{k}_ms": [] for n in tails for k in ("wall", "event")}
    t.update({f"step_{n}_{k}ms": [] for n in legs for k in ("", "event_")})
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def window(fn):
        e0, e1 = ev()
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, e0.elapsed_time(e1) / steps

    for _ in range(reps):
        for name, tail in tails.items():
            wall, event = window(tail)
            t[f"tail_{name}_wall_ms"].append(wall)
            t[f"tail_{name}_event_ms"].append(event)
        for name in legs:
            wall, event = window(lambda: trainers[name].train(stores[name], B))
            t[f"step_{name}_ms"].append(wall)
            t[f"step_{name}_event_ms"].append(event)
    skipped = trainers["on"].skipped_steps()
    out = {"what": "the optimizer tail alone (the parent's clip_grad_norm_ + foreach Adam + StepLR; torch's fused "
                   "Adam, for information; mzgo.DeviceAdam) and the whole batched trainer step with "
                   "TrainConfig.device_optimizer off and on, ms per step over windows of STEPS; best / median / "
                   "spread (max - min) over REPS alternating windows, by wall clock and by events",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps, "reps": reps},
           "expectation_before_first_run": EXPECTATION, "skipped_steps_on": skipped,
           "accuracy_25_steps_per_tensor": accuracy}
    out.update({k: _summary(v) for k, v in t.items()})
    med = lambda k: out[k]["median"]
    out["tail_device_over_torch_event"] = med("tail_device_event_ms") / med("tail_torch_event_ms")
    out["step_on_over_off"] = med("step_on_ms") / med("step_off_ms")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
