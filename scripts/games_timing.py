"""Continuous self-play (``play_games_into``: one launch, a device game queue,
k_selfplay_games) against the two ways to put the same games into a
``mzgo.DeviceReplay`` before it, in the modes where the search decides the move.

Two shapes:

* ``main``   main.py's variant at scripts/replay_timing.py's shape -- 6x6,
             latent_dim 128 (``MainSelfPlay``'s search and move cap), 256 slots;
* ``fixed``  9x9, latent_dim 96, 256 slots, 200 simulations, compat "fixed".

For n = G and n = 4 G games, three legs that store the same n games:

(a) ``per_move``    n / G epochs of reset + max_moves single-move launches +
                    ``add_games`` (what ``MainSelfPlay.play_into`` does);
(b) ``whole_game``  n / G epochs of reset + one ``move(max_moves)`` launch, with
                    its default tail helpers, + ``add_games``;
(c) ``queue``       ``play_games_into(n)``.

A shape is one child process (under its own time limit; the first that fails
ends the script) in which the legs alternate, REPS rounds after one warm-up
round; wall time around synchronised calls, since every leg ends with its
lengths on the host.  Reported per leg: best and median ms, games/s and
simulations/s (the engine's counter delta over the time).  Writes
profiles/selfplay_games_timing.json.

    python scripts/games_timing.py [--out profiles/selfplay_games_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "muzero-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {
    "main": dict(board_size=6, latent_dim=128, games=256, simulations=256),
    "fixed": dict(board_size=9, latent_dim=96, games=256, simulations=200),
}
SHAPE_LIMIT_S = {"main": 240, "fixed": 240}
LEGS = ("per_move", "whole_game", "queue")


def _selfplay(name, cfg, seed):
    import mzgo
    from mzgo.trainer import MainSelfPlay
    N, C = cfg["board_size"], cfg["latent_dim"]
    net = mzgo.MuZeroNet(C, N * N + 1).to("cuda:0").eval()
    net.load_state_dict(mzgo.deterministic_state_dict(C, N * N + 1, 0))
    if name == "main":
        return MainSelfPlay(net, cfg["games"], cfg["simulations"], seed=seed).sp
    return mzgo.SelfPlay(net, cfg["games"], cfg["simulations"], seed=seed, compat="fixed")


def _leg(sp, replay, leg, n):
    """store games 0 .. n-1 (slot j % G of epoch j // G) by ``leg``"""
    sp.epoch = 0
    if leg == "queue":
        sp.play_games_into(replay, n)
        return
    for _ in range(n // sp.G):
        sp.reset()
        if leg == "per_move":
            for _ in range(sp.max_moves):
                sp.move()
        else:
            sp.move(sp.max_moves)
        replay.add_games(sp.engine)
        sp.epoch += 1


def run_shape(name, reps, seed):
    import torch

    import mzgo
    cfg = SHAPES[name]
    sp = _selfplay(name, cfg, seed)
    G, S = sp.G, sp.S
    out = dict(cfg, max_moves=sp.max_moves, reps=reps, legs={})
    for mult in (1, 4):
        n = mult * G
        replay = mzgo.DeviceReplay(sp.N, n, sp.max_moves, "cuda:0")
        ms = {leg: [] for leg in LEGS}
        sims, lengths = {}, {}
        for rep in range(reps + 1):                       # round 0 warms up
            for leg in LEGS:
                c0 = sp.engine.counters()["simulations"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _leg(sp, replay, leg, n)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                sims[leg] = sp.engine.counters()["simulations"] - c0
                lengths[leg] = list(replay.lengths[-n:])
                if rep > 0:
                    ms[leg].append(dt)
        # the legs stored the same games
        assert lengths["per_move"] == lengths["whole_game"] == lengths["queue"], "the legs' games differ"
        assert sims["per_move"] == sims["whole_game"] == sims["queue"] == sum(lengths["queue"]) * S
        res = {}
        for leg in LEGS:
            best, med = min(ms[leg]), statistics.median(ms[leg])
            res[leg] = dict(ms=[round(x, 3) for x in ms[leg]], best_ms=round(best, 3), median_ms=round(med, 3),
                            games_per_s=round(n / best * 1e3, 1), simulations_per_s=round(sims[leg] / best * 1e3, 1),
                            median_simulations_per_s=round(sims[leg] / med * 1e3, 1))
        res["games"] = n
        res["moves"] = sum(lengths["queue"])
        res["simulations"] = sims["queue"]
        res["queue_over_whole_game"] = round(res["whole_game"]["best_ms"] / res["queue"]["best_ms"], 4)
        res["queue_over_per_move"] = round(res["per_move"]["best_ms"] / res["queue"]["best_ms"], 4)
        out["legs"]["n=%dG" % mult] = res
        replay.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfplay_games_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="(internal) run one shape in this process")
    ap.add_argument("--work", default=None, help="(internal) the shapes' shared directory")
    args = ap.parse_args()
    if args.shape:
        res = run_shape(args.shape, args.reps, args.seed)
        with open(os.path.join(args.work, args.shape + ".json"), "w") as f:
            json.dump(res, f)
        return 0

    out = dict(what="n games into a DeviceReplay: (a) per-move launches, (b) whole-game launches, (c) one "
                    "play_games_into launch; wall ms, legs alternating in one process per shape, best of REPS "
                    "and the median")
    with tempfile.TemporaryDirectory() as work:
        for shape in ("main", "fixed"):
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--work", work,
                   "--reps", str(args.reps), "--seed", str(args.seed)]
            try:
                rc = subprocess.run(cmd, timeout=SHAPE_LIMIT_S[shape]).returncode
            except subprocess.TimeoutExpired:
                print(f"shape {shape}: no result within {SHAPE_LIMIT_S[shape]} s; stopping", file=sys.stderr)
                return 124
            if rc != 0:
                print(f"shape {shape} failed (exit {rc}); stopping", file=sys.stderr)
                return rc
            with open(os.path.join(work, shape + ".json")) as f:
                out[shape] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
