"""GPU parity around a select's arrival at a new parent (9x9, LDS trees).

An arrival is the walk reaching a lazily expanded child X of the last batch's
leaf L: X's policy sums are formed from L's Y (read from the expansion's LDS
copy when it still holds L's), its priors are settled (its rows stay in the
LDS row copy), and X becomes the next parent; after a batch that took all of
a leaf's children and was accepted in full, the next select resumes at that
leaf when the replay showed that its walk comes down to it again.  None of
that may change a tree: the device trees are compared node
for node -- ids in expansion order, actions, visit counts, value sums and
priors -- with the oracle MCTS under the same hooks and the tolerances of
tests/test_gpu_search.py (network outputs differ by fp32 summation order
only: root value 1e-5, priors rtol 1e-4 / atol 1e-7, value sums 1e-4; counts
and structure exact).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C = 9, 96
A = N * N + 1
SEED, GAME = 31, 2

# (name, moves of random play, position seed): a late-game board with 4 legal
# points + pass (deep paths, small batches: sequential and parallel replays
# mixed), a mid-game board with 42 legal points, and the empty board
POSITIONS = {"late": (160, 425), "mid": (40, 140), "empty": (0, 0)}
# S = 64 ends inside a batch on the mid-game and empty boards (the root batch
# of 43 then 21 of a depth-1 leaf's 43 -- every node keeps the root's mask; 64
# of the root's 82); S = 100 ends inside one on the empty board (82, then 18
# of 82) and inside the third batch on the mid-game board (43 + 43 + 14)
SIMS = (64, 100)


def _obs(name):
    from oracle.positions import random_position
    moves, seed = POSITIONS[name]
    return random_position(N, moves, seed) if moves else np.zeros((6, N, N))


def _state_dict(c=C, a=A):
    from oracle.weights import deterministic_state_dict
    return deterministic_state_dict(c, a, 0)


def _net(sd, c=C, a=A):
    import mzgo
    net = mzgo.MuZeroNet(c, a).to("cuda").eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


class _LoggedNet:
    """The oracle network, logging the action of every expansion in order."""

    def __init__(self, net):
        self.net, self.actions = net, []

    def initial_inference(self, obs):
        return self.net.initial_inference(obs)

    def recurrent_inference(self, latent, action):
        self.actions.append(int(action.reshape(-1)[0]))
        return self.net.recurrent_inference(latent, action)


_ORACLE = {}


def _oracle_tree(name, S, move):
    """The oracle's tree of (position, S), computed once and left unchanged."""
    key = (name, S)
    if key not in _ORACLE:
        from oracle.mcts import MCTS
        from oracle.net import OracleNet
        from oracle.rng import SearchHooks, injected_noise
        noise = injected_noise(SEED, GAME, move, A)
        hooks = SearchHooks(SEED, GAME, move)
        onet = _LoggedNet(OracleNet(_state_dict()))
        ref = MCTS(onet, A, S, choice=lambda seq, sim: seq[hooks.choice_index(len(seq), sim)],
                   noise=lambda p, a, e: (1 - e) * p + e * noise)
        with torch.no_grad():
            root, _, value = ref.run(_obs(name))
        _ORACLE[key] = (root, value, onet.actions)
    return _ORACLE[key]


def _compare_trees(tree, r_root, r_actions, n_actions):
    """Device tree (engine.tree) vs the oracle's Node graph, node for node."""
    n = int(tree["n"])
    assert n == len(r_actions) + 1                      # one node per expansion, and the root
    seen = np.zeros(n, bool)
    stack = [(0, r_root, -1)]
    while stack:
        i, ref, act = stack.pop()
        assert not seen[i]
        seen[i] = True
        if i > 0:
            assert act == r_actions[i - 1], (i, act)     # ids in expansion order, with their actions
        assert int(tree["visits"][i]) == ref.visit_count, i
        assert abs(float(tree["value_sum"][i]) - float(ref.value_sum)) < 1e-4, i
        pri = tree["root_prior"] if i == 0 else tree["prior"][i]
        want = np.array([ref.children[a]["prior"] for a in range(n_actions)], np.float64)
        if i == 0:
            np.testing.assert_allclose(pri, want, rtol=1e-5, atol=1e-9)
        else:
            np.testing.assert_allclose(pri, want, rtol=1e-4, atol=1e-7, err_msg=f"node {i}")
        for a in range(n_actions):
            c, rc = int(tree["child"][i][a]), ref.children[a]["node"]
            assert (c >= 0) == (rc is not None), (i, a)
            if c >= 0:
                stack.append((c, rc, a))
    assert seen.all()


@pytest.mark.parametrize("S", SIMS)
@pytest.mark.parametrize("name", list(POSITIONS))
def test_arrival_trees_match_oracle(name, S):
    move = POSITIONS[name][0]
    r_root, r_value, r_actions = _oracle_tree(name, S, move)
    from oracle.rng import injected_noise
    net = _net(_state_dict())
    eng = net.engine(num_games=1, num_simulations=S, seed=SEED, game_base=GAME)
    obs = torch.as_tensor(np.asarray(_obs(name)), dtype=torch.float32).reshape(1, 6, N, N)
    noise = torch.from_numpy(injected_noise(SEED, GAME, move, A))
    _, value = eng.search(obs, noise=noise, move_index=move)
    tree = eng.tree(0)
    assert int(tree["visits"][0]) == S
    assert abs(float(value[0].item()) - r_value) < 1e-5
    _compare_trees(tree, r_root, r_actions, A)


def test_arrival_selfplay_epoch_equals_per_move_launches(monkeypatch):
    """Self-play keeps every batched child's prior row lazy, so its arrivals
    are the lazy ones: the move-parallel epoch (one search queue) against one
    launch per move of the game-per-workgroup kernel at 9x9 / 4 games / 48
    simulations -- byte-identical records, root values and counters."""
    import mzgo
    from mzgo.distributed import pack_engine, unpack
    G, S = 4, 48
    net = _net(_state_dict())
    sp = mzgo.SelfPlay(net, G, S, seed=1234)
    eng = sp.engine
    M = sp.max_moves
    monkeypatch.setenv("MZGO_QUEUE_HELPERS", "0")
    monkeypatch.setenv("MZGO_TAIL_HELPERS", "0")
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MZGO_MOVE_PARALLEL", mode)
        c0 = eng.counters()
        sp.reset(epoch=0)
        if mode == "1":
            sp.move(M)
        else:
            for _ in range(M):
                sp.move()
        c1 = eng.counters()
        arrays = unpack(pack_engine(eng).cpu().numpy(), eng.G, eng.M, eng.N)
        # (the counters of the searches; how many workgroups the launches started differs by design)
        out[mode] = (arrays, {k: c1[k] - c0[k] for k in ("simulations", "moves", "games_finished",
                                                         "dynamics_convs", "prior_rows")})
    (aa, ca), (ab, cb) = out["1"], out["0"]
    assert ca == cb, (ca, cb)
    assert ca["games_finished"] == G and ca["simulations"] == ca["moves"] * S
    assert ca["prior_rows"] > 0 and ca["dynamics_convs"] > 0
    for k in aa:
        np.testing.assert_array_equal(aa[k].view(np.uint8), ab[k].view(np.uint8), err_msg=k)


def test_arrival_main_variant_matches_oracle():
    """search_variant="main" (main.py's select, sqrt(N + 1)) takes the same
    arrival path: one 9x9 mid-game position against oracle.mcts_main."""
    import mzgo
    from oracle.mcts import tree_summary
    from oracle.mcts_main import MCTSMain
    from oracle.net import OracleNet
    from oracle.rng import SearchHooks, injected_noise
    S, seed, game = 64, 17, 1
    moves = POSITIONS["mid"][0]
    obs = _obs("mid")
    noise = injected_noise(seed, game, moves, A)
    hooks = SearchHooks(seed, game, moves)
    sd = _state_dict()
    ref = MCTSMain(OracleNet(sd), A, S, choice=lambda seq, sim: seq[hooks.choice_index(len(seq), sim)],
                   noise=lambda p, a, e: (1 - e) * p + e * noise)
    with torch.no_grad():
        r_root = ref.run(obs)
    m = mzgo.MainMCTS(_net(sd), A, S, seed=seed, game=game)
    root = m.run(obs, move_index=moves, noise=torch.from_numpy(noise))
    np.testing.assert_array_equal(tree_summary(root, A)[0], tree_summary(r_root, A)[0])
    np.testing.assert_array_equal(np.array(tree_summary(root, A)[1]), np.array(tree_summary(r_root, A)[1]))
    assert abs(m.root_value - r_root.value()) < 1e-5
