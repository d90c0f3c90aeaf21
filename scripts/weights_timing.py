"""An engine's weight refresh after an optimizer step: through the host
(``Engine.set_state_dict``: 22 device-to-host copies, the host packers, one
blocking upload) against on the device (``Engine.set_parameters_device``: one
pack launch; ``Engine.copy_weights_from``: one device-to-device copy for a
net's further engines), at (6x6, C=128), (9x9, C=96) and (19x19, C=96), and
the whole batched trainer step at main.py's sizes with
``TrainConfig.device_weights`` off and on.

The paths alternate in one process; every figure is per refresh (or per step)
over a window of INNER refreshes (STEPS steps), reported as best / median /
spread (max - min) over REPS windows, after a warm-up of every path:

* host_wall_ms            -- (a) ``set_state_dict`` and the pack + upload it
                             leaves to the engine's next use, wall time,
                             synchronised (the copies block anyway);
                             host_copies_wall_ms is ``set_state_dict`` alone
                             (scripts/replay_timing.py's engine_weight_reload_ms);
* device_event_ms         -- (b) ``set_parameters_device`` by HIP events
                             around the window's launches on the stream;
* device_call_wall_ms     -- (b) the host's time inside the call (it returns
                             before the launch has run);
* device_gpu_ms           -- (b) the pack launch's own time: the window
                             enqueued behind a long matmul, so that the events
                             see the launches back to back without the host;
* copy_event_ms / copy_call_wall_ms -- (c) ``copy_weights_from`` likewise;
* step_off_ms / step_on_ms -- (d) 6x6 / C=128 / batch 128 x unroll 10 from a
                             ``DeviceReplay`` with device_sampling +
                             deferred_stats + fused_loss, wall time over STEPS
                             steps ending in a synchronise.

Before timing a shape the two paths' blobs are compared bit for bit.

Usage (GPU box): python scripts/weights_timing.py [out.json] -> one JSON line
(also written to out.json when given).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _summary(xs):
    return {"best": min(xs), "median": statistics.median(xs), "spread": max(xs) - min(xs), "all": xs}


def refresh_timing(N, C, inner, reps):
    import mzgo
    from mzgo.engine import Engine, EngineConfig
    A = N * N + 1
    net = mzgo.MuZeroNet(C, A).cuda()
    net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
    mk = lambda: Engine(EngineConfig(board_size=N, latent_dim=C, num_games=1, num_simulations=1, compat="fixed"))
    host, dev, cpy = mk(), mk(), mk()
    sd = net.state_dict()

    def run_host():
        for _ in range(inner):
            host.set_state_dict(sd)
            # the host packers and the upload run at the engine's next use: a
            # copy onto itself is that use and nothing more (mzgo_weights_copy
            # packs its source's pending tensors first)
            host.copy_weights_from(host)

    def run_dev():
        for _ in range(inner):
            dev.set_parameters_device(sd)

    def run_copy():
        for _ in range(inner):
            cpy.copy_weights_from(dev)

    for f in (run_host, run_dev, run_copy):                   # warm-up: code objects, the blobs' allocation
        f()
    torch.cuda.synchronize()
    a, b, c = host.export_weights(), dev.export_weights(), cpy.export_weights()
    same = bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)) and
                np.array_equal(a.view(np.uint32), c.view(np.uint32)))
    t = {k: [] for k in ("host_wall_ms", "host_copies_wall_ms", "device_event_ms", "device_call_wall_ms", "device_gpu_ms", "copy_event_ms",
                         "copy_call_wall_ms")}
    big = torch.randn(8192, 8192, device="cuda")
    big_out = torch.empty_like(big)
    torch.mm(big, big, out=big_out)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_host()
        torch.cuda.synchronize()
        t["host_wall_ms"].append((time.perf_counter() - t0) / inner * 1e3)
        t0 = time.perf_counter()
        for _ in range(inner):
            host.set_state_dict(sd)
        torch.cuda.synchronize()
        t["host_copies_wall_ms"].append((time.perf_counter() - t0) / inner * 1e3)
        for f, ev, wall in ((run_dev, "device_event_ms", "device_call_wall_ms"),
                            (run_copy, "copy_event_ms", "copy_call_wall_ms")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            t[wall].append((t1 - t0) / inner * 1e3)
            t[ev].append(e0.elapsed_time(e1) / inner)
        # the pack launch alone: the window is enqueued while a long matmul
        # holds the stream, so the events see the kernels back to back
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.mm(big, big, out=big_out)
        e0.record()
        run_dev()
        e1.record()
        torch.cuda.synchronize()
        t["device_gpu_ms"].append(e0.elapsed_time(e1) / inner)
    out = {"board_size": N, "latent_dim": C, "blob_floats": int(a.size), "blobs_bit_identical": same}
    out.update({k: _summary(v) for k, v in t.items()})
    out["host_over_device_event"] = out["host_wall_ms"]["median"] / out["device_event_ms"]["median"]
    for e in (host, dev, cpy):
        e.close()
    return out


def step_timing(steps, reps):
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    from oracle.make_golden import synthetic_trajectories
    N, C, B, K = 6, 128, 128, 10
    A = N * N + 1
    trajs = synthetic_trajectories(N, B, seed=11)
    trainers, stores = {}, {}
    for name in ("off", "on"):
        rp = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
        for tr in trajs:
            rp.add(tr)
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        cfg = TrainConfig(unroll_steps=K, device_sampling=True, deferred_stats=True, fused_loss=True,
                          device_weights=(name == "on"))
        trainers[name], stores[name] = MuZeroTrainer(net, cfg, mode="batched", sample_seed=3), rp
    losses = {}
    for name, tr in trainers.items():                         # warm-up (MIOpen picks its kernels here)
        for _ in range(3):
            tr.train(stores[name], B)
        losses[name] = tr.read_stats()["training_loss"]
    torch.cuda.synchronize()
    times = {"off": [], "on": []}
    for _ in range(reps):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train(stores[name], B)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    return {"config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps},
            "step_off_ms": _summary(times["off"]), "step_on_ms": _summary(times["on"]),
            "loss_after_warmup": losses}


def main():
    inner, steps, reps = (int(os.environ.get(k, d)) for k, d in (("INNER", 20), ("STEPS", 10), ("REPS", 7)))
    out = {"what": "engine weight refresh through the host (set_state_dict) vs on the device "
                   "(set_parameters_device, copy_weights_from), ms per refresh over windows of INNER refreshes, "
                   "and the batched trainer step with device_weights off / on, ms per step over windows of STEPS "
                   "steps; best / median / spread (max - min) over REPS alternating windows",
           "inner": inner, "reps": reps,
           "refresh": [refresh_timing(N, C, inner, reps) for N, C in ((6, 128), (9, 96), (19, 96))],
           "step": step_timing(steps, reps)}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
