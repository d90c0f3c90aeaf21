"""Playout cap randomization (``fast_simulations``, ``full_search_prob``) against
full-budget self-play, on continuous self-play (``play_games_into``: one launch,
k_selfplay_games) into a ``mzgo.DeviceReplay``.

Two shapes, scripts/games_timing.py's:

* ``fixed``  9x9, latent_dim 96, 256 slots, 200 simulations, compat "fixed";
* ``main``   main.py's variant -- 6x6, latent_dim 128 (``MainSelfPlay``'s search
             and move cap), 256 slots, 256 simulations.

At each, n = 4 G games by two legs on two engines of one net: ``off`` (every
move searched with S simulations) and ``capped`` (F = S // 5, p = 0.25).  The
games differ between the legs -- a fast search picks other moves -- so each
leg reports its own games, positions and simulations.

One process: at each shape in turn the legs alternate, WINDOWS windows after
one warm-up round; wall time around synchronised calls.  Reported per leg: every window's
ms, the best and the median, and at the best window games/s, positions/s and
simulations/s (the engine's counter deltas over the time); for ``capped`` the
realised fraction of full searches, from the counters: simulations = full * S +
fast * F over ``moves`` moves.  Writes profiles/playout_cap_timing.json.

    python scripts/playout_cap_timing.py [--out profiles/playout_cap_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "muzero-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {
    "fixed": dict(board_size=9, latent_dim=96, games=256, simulations=200),
    "main": dict(board_size=6, latent_dim=128, games=256, simulations=256),
}
LEGS = ("off", "capped")
FULL_PROB = 0.25


def _selfplay(name, cfg, net, seed, caps):
    import mzgo
    from mzgo.trainer import MainSelfPlay
    if name == "main":
        return MainSelfPlay(net, cfg["games"], cfg["simulations"], seed=seed, **caps).sp
    return mzgo.SelfPlay(net, cfg["games"], cfg["simulations"], seed=seed, compat="fixed", **caps)


def run_shape(name, windows, seed):
    import torch

    import mzgo
    cfg = SHAPES[name]
    N, C, S = cfg["board_size"], cfg["latent_dim"], cfg["simulations"]
    F = S // 5
    net = mzgo.MuZeroNet(C, N * N + 1).to("cuda:0").eval()
    net.load_state_dict(mzgo.deterministic_state_dict(C, N * N + 1, 0))
    sps = {"off": _selfplay(name, cfg, net, seed, {}),
           "capped": _selfplay(name, cfg, net, seed, dict(fast_simulations=F, full_search_prob=FULL_PROB))}
    assert sps["off"].engine is not sps["capped"].engine
    n = 4 * cfg["games"]
    replay = mzgo.DeviceReplay(N, n, sps["off"].max_moves, "cuda:0")
    ms = {leg: [] for leg in LEGS}
    sims, moves = {}, {}
    for w in range(windows + 1):                          # round 0 warms up
        for leg in LEGS:
            sp = sps[leg]
            sp.epoch = 0                                  # the same games in every window
            c0 = sp.engine.counters()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp.play_games_into(replay, n)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            c1 = sp.engine.counters()
            s, m = c1["simulations"] - c0["simulations"], c1["moves"] - c0["moves"]
            assert m == sum(replay.lengths[-n:])
            assert sims.setdefault(leg, s) == s and moves.setdefault(leg, m) == m, "a leg's games changed"
            if w > 0:
                ms[leg].append(dt)
    assert sims["off"] == moves["off"] * S
    out = dict(cfg, fast_simulations=F, full_search_prob=FULL_PROB, games_per_call=n, max_moves=sps["off"].max_moves,
               windows=windows, legs={})
    for leg in LEGS:
        best, med = min(ms[leg]), statistics.median(ms[leg])
        out["legs"][leg] = dict(ms=[round(x, 3) for x in ms[leg]], best_ms=round(best, 3), median_ms=round(med, 3),
                                games=n, moves=moves[leg], simulations=sims[leg],
                                simulations_per_move=round(sims[leg] / moves[leg], 3),
                                games_per_s=round(n / best * 1e3, 1), positions_per_s=round(moves[leg] / best * 1e3, 1),
                                simulations_per_s=round(sims[leg] / best * 1e3, 1),
                                median_games_per_s=round(n / med * 1e3, 1),
                                median_positions_per_s=round(moves[leg] / med * 1e3, 1))
    cap = out["legs"]["capped"]
    full = (sims["capped"] - moves["capped"] * F) / (S - F)           # full * S + fast * F = simulations
    cap["full_searches"] = int(round(full))
    cap["full_fraction"] = round(full / moves["capped"], 5)
    off = out["legs"]["off"]
    out["capped_over_off"] = dict(games_per_s=round(cap["games_per_s"] / off["games_per_s"], 4),
                                  positions_per_s=round(cap["positions_per_s"] / off["positions_per_s"], 4),
                                  median_positions_per_s=round(cap["median_positions_per_s"]
                                                               / off["median_positions_per_s"], 4),
                                  simulations_per_move=round(off["simulations_per_move"]
                                                             / cap["simulations_per_move"], 4))
    replay.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_cap_timing.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    out = dict(what="play_games_into(4 G) with the playout caps off against F = S // 5, p = 0.25: wall ms, one "
                    "process, legs alternating, WINDOWS windows after a warm-up round at each shape; rates at the "
                    "best window and at the median")
    for shape in ("fixed", "main"):
        out[shape] = run_shape(shape, args.windows, args.seed)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
