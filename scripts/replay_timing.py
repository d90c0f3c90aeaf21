"""The batched trainer step (mzgo.trainer mode="batched") from a host
trajectory buffer against the same step from a ``mzgo.DeviceReplay``, at
main.py's configuration -- 6x6 board, latent_dim 128, batch 128 trajectories x
unroll 10.  Same games, same start indices, same initial weights; the two
paths alternate in one process, best of REPS.

* step_host_ms / step_device_ms -- the whole step (targets + bootstrap
  inference + forward unroll + backward + Adam), wall time over STEPS steps;
* targets_host_ms -- target assembly alone on the host path
  (``host_targets``: the Python loops, the bootstrap inference, the uploads),
  by perf_counter around synchronised calls;
* targets_device_ms -- ``device_targets`` (k_replay_batch + the bootstrap
  inference over all B (K+1) rows + k_replay_finish) by HIP events on the
  stream, and targets_device_wall_ms by perf_counter as for the host;
* engine_weight_reload_ms -- ``Engine.set_state_dict`` from the module, which
  every step of either path pays before its bootstrap inference (the weights
  changed) and which the target timings above leave out (they do not change).

Usage (GPU box): python scripts/replay_timing.py [out.json] -> one JSON line
(also written to out.json when given).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


class _Buf:
    def __init__(self, trajs):
        self.trajs = trajs

    def sample(self, n):
        return self.trajs[:n], None


def main():
    import mzgo
    from mzgo.trainer import MuZeroTrainer
    from oracle.make_golden import synthetic_trajectories
    N, C, B, K = 6, 128, 128, 10
    A = N * N + 1
    steps, reps = int(os.environ.get("STEPS", 10)), int(os.environ.get("REPS", 3))
    trajs = synthetic_trajectories(N, B, seed=11)
    replay = mzgo.DeviceReplay(N, B, int(1.5 * N * N), "cuda")
    for t in trajs:
        replay.add(t)
    replay.sample_indices = lambda n: np.arange(n)            # _Buf's sample: the first n games
    start = lambda T: T // 3
    trainers = {}
    for name in ("host", "device"):
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        trainers[name] = MuZeroTrainer(net, mode="batched", start_index=start)
    sources = {"host": _Buf(trajs), "device": replay}
    losses = {}
    for name, tr in trainers.items():                         # warmup (MIOpen picks its kernels here)
        losses[name] = [tr.train(sources[name], B) for _ in range(2)]
    torch.cuda.synchronize()
    times = {"host": [], "device": []}
    for _ in range(reps):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train(sources[name], B)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    # target assembly alone (the weights do not change here: the engine keeps its copy)
    idx = list(range(B))
    starts = [start(len(t["actions"])) for t in trajs]
    th, td = trainers["host"], trainers["device"]
    tgt = {"host": [], "device_wall": [], "device_events": []}
    for _ in range(2):
        th.host_targets(trajs, starts)
        td.device_targets(replay, idx, starts)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            th.host_targets(trajs, starts)
        torch.cuda.synchronize()
        tgt["host"].append((time.perf_counter() - t0) / steps * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(steps):
            td.device_targets(replay, idx, starts)
        e1.record()
        torch.cuda.synchronize()
        tgt["device_wall"].append((time.perf_counter() - t0) / steps * 1e3)
        tgt["device_events"].append(e0.elapsed_time(e1) / steps)
    # what both paths pay after every optimizer step before the bootstrap
    # inference: the engine's weights reloaded from the module (a device-to-host
    # copy of the state_dict, the host repack, one upload)
    eng = td.net.engine()
    reload_ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.set_state_dict(td.net.state_dict())
        torch.cuda.synchronize()
        reload_ms.append((time.perf_counter() - t0) / steps * 1e3)
    out = {"engine_weight_reload_ms": min(reload_ms),
           "what": "one batched trainer step (targets + bootstrap inference + forward unroll + backward + Adam) "
                   "from a host trajectory buffer vs from a DeviceReplay, ms; wall time over STEPS steps, best of "
                   "REPS; and target assembly alone",
           "config": {"board_size": N, "latent_dim": C, "batch": B, "unroll": K, "steps": steps, "reps": reps},
           "step_host_ms": min(times["host"]), "step_device_ms": min(times["device"]),
           "step_host_all_ms": times["host"], "step_device_all_ms": times["device"],
           "targets_host_ms": min(tgt["host"]), "targets_device_ms": min(tgt["device_events"]),
           "targets_device_wall_ms": min(tgt["device_wall"]),
           "targets_host_all_ms": tgt["host"], "targets_device_events_all_ms": tgt["device_events"],
           "warmup_losses": losses}
    out["step_speedup_device_over_host"] = out["step_host_ms"] / out["step_device_ms"]
    out["targets_speedup_device_over_host"] = out["targets_host_ms"] / out["targets_device_wall_ms"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
