"""What sampling on the host costs a batched trainer step on a
``DeviceReplay``, against the device ledger and sampler
(``TrainConfig.device_sampling``; DESIGN §4 "Sampling on the device").
main.py's configuration, scripts/loss_timing.py's protocol: 6x6 board,
latent_dim 128, batch 128 x unroll 10, ``fused_loss`` and ``sample_priorities``
on; the same games and initial weights for every leg; the legs alternate in
one process; best of REPS runs of STEPS steps and the median, every value
kept.  Two store sizes: 512 games and main.py's ``replay_buffer_size`` 5000
(128 distinct synthetic games, repeated).

* step_host_ms     -- (a) ``train`` with the host ledger: ``np.random.choice``
  over the store, ``random.randint`` starts, pinned staging, the per-sample
  losses copied back and written into the Python list;
* step_device_ms   -- (b) ``device_sampling``: sample, batch, step and priority
  update queued on the stream, one copy of the totals;
* step_deferred_ms -- (c) (b) with ``deferred_stats``: no synchronising call in
  ``train`` (one at the end of the STEPS steps);
* sampler_*        -- ``DeviceReplay.sample`` alone (k_replay_sample_build +
  k_replay_sample_draw), by HIP events on the stream and by wall time;
* host_*           -- the host leg's own parts alone, by wall time:
  ``sample_indices`` + the starts, the ``batch`` call (staging, its wait and
  the launch), and the priority loop (``_priorities`` + ``update_priorities``).

Usage (GPU box): python scripts/sample_timing.py [out.json] -> one JSON line
(also written to out.json when given).
"""
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "muzero-go_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, steps):
    """(wall ms, HIP-event ms) per call of ``fn`` over ``steps`` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, e0.elapsed_time(e1) / steps


def measure(games, size, steps, reps):
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    N, C, B, K = 6, 128, 128, 10
    A = N * N + 1
    replay = mzgo.DeviceReplay(N, size, int(1.5 * N * N), "cuda")
    for k in range(size):
        replay.add(games[k % len(games)])
    random.seed(0)
    np.random.seed(0)
    legs = {"host": {}, "device": dict(device_sampling=True),
            "deferred": dict(device_sampling=True, deferred_stats=True)}
    trainers = {}
    for name, extra in legs.items():
        net = mzgo.MuZeroNet(C, A).cuda()
        net.load_state_dict(mzgo.deterministic_state_dict(C, A, 7))
        trainers[name] = MuZeroTrainer(net, TrainConfig(fused_loss=True, sample_priorities=True, **extra),
                                       mode="batched", sample_seed=11)
    warm = {}
    for name, tr in trainers.items():                        # warmup (MIOpen picks its kernels here)
        warm[name] = [float(tr.train(replay, B)) for _ in range(2)]
    torch.cuda.synchronize()
    step = {name: [] for name in trainers}
    for _ in range(reps):
        for name, tr in trainers.items():
            step[name].append(timed(lambda: tr.train(replay, B), steps)[0])
    trainers["deferred"].read_stats()

    # the sampler's two launches alone
    count = [0]

    def sampler():
        count[0] += 1
        replay.sample(B, seed=3, step=count[0])

    sampler()
    samp = [timed(sampler, steps) for _ in range(reps)]

    # the host leg's own parts alone
    tr = trainers["host"]
    drawn = {}

    def host_sample():
        idx = replay.sample_indices(B)
        drawn["idx"], drawn["starts"] = idx, [tr.start_index(replay.lengths[i]) for i in idx]

    def host_batch():
        replay.batch(drawn["idx"], drawn["starts"], K, tr.config.discount)

    tr.last_per_sample = np.full(B, 1.5, np.float32)

    def host_update():
        replay.update_priorities(drawn["idx"], tr._priorities(1.5, B))

    host = {}
    for name, fn in (("sample", host_sample), ("batch_call", host_batch), ("update", host_update)):
        fn()
        host[name] = [timed(fn, steps)[0] for _ in range(reps)]

    best, med = min, statistics.median
    out = {"games": size, "warmup_losses": warm}
    for name in trainers:
        out.update({f"step_{name}_ms": best(step[name]), f"step_{name}_median_ms": med(step[name]),
                    f"step_{name}_all_ms": step[name]})
    wall, ev = [w for w, _ in samp], [e for _, e in samp]
    out.update({"sampler_events_ms": best(ev), "sampler_events_median_ms": med(ev), "sampler_events_all_ms": ev,
                "sampler_wall_ms": best(wall), "sampler_wall_median_ms": med(wall), "sampler_wall_all_ms": wall})
    for name, xs in host.items():
        out.update({f"host_{name}_ms": best(xs), f"host_{name}_median_ms": med(xs), f"host_{name}_all_ms": xs})
    out["host_parts_ms"] = sum(best(xs) for xs in host.values())
    out["skipped_updates"] = replay.skipped_updates()
    out["step_speedup_device_over_host"] = out["step_host_ms"] / out["step_device_ms"]
    out["step_speedup_deferred_over_host"] = out["step_host_ms"] / out["step_deferred_ms"]
    replay.close()
    return out


def main():
    from oracle.make_golden import synthetic_trajectories
    steps, reps = int(os.environ.get("STEPS", 30)), int(os.environ.get("REPS", 5))
    sizes = [int(x) for x in os.environ.get("SIZES", "512,5000").split(",")]
    games = synthetic_trajectories(6, 128, seed=11)
    out = {"what": "the batched trainer step (fused_loss, sample_priorities) from a DeviceReplay of 512 and of 5000 "
                   "games: host ledger and np.random sampling (the default path) vs TrainConfig.device_sampling vs "
                   "device_sampling + deferred_stats; the sampler's two launches alone; the host leg's sampling, "
                   "batch call and priority loop alone; ms per step, best of REPS runs of STEPS steps and the "
                   "median, all runs kept",
           "config": {"board_size": 6, "latent_dim": 128, "batch": 128, "unroll": 10, "steps": steps, "reps": reps},
           "stores": [measure(games, size, steps, reps) for size in sizes]}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
