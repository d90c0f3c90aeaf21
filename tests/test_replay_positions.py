"""Position-level prioritized replay on the CPU, through the host twins
(``mzgo.replay.sample_positions_host`` -> ``mzgo_replay_sample_positions_host``
and ``position_priorities_host`` -> ``mzgo_replay_position_priorities_host``,
which run the kernels' own functions of csrc/mzgo_replay.hpp serially).

``restated_positions`` below restates the sampler in Python ints and numpy
float64 from its rule, not from the C: every group of 64 is added by the
six-step inclusive scan (p[i] <- p[i - d] + p[i], d = 1 .. 32; the sum is
p[63]); a game's weight is the scan over its <= 64 chunk sums, a chunk the scan
over 64 positions, entries past the game's end 0; the 64-ary tree over the
slots is the game sampler's; one u = u01(draw(key, 5, t)) gives target = u x
total, which descends five levels (sums of 64 x 64 slots, of 64 slots, the
slots, the picked game's chunks, the picked chunk's positions) by "the first
non-zero entry whose inclusive prefix exceeds the target, else the last
non-zero entry; target -= the prefix before the pick"; the picked game's leaf
is zeroed and its two ancestors are added again.  The importance weights are
(n_pos w / total0) ** -beta over the batch's largest.

``build_pos_case`` / ``restated_positions`` are shared with
tests/test_gpu_replay_positions.py.
"""
import functools

import numpy as np
import pytest

from test_replay_sample import DOMAIN, TAG_SAMPLE, TAG_SYM, draw, pick64, randbelow, scan64, stream_key, u01

FLT_MIN = float(np.finfo(np.float32).tiny)
M = 130                                                    # max_moves: crosses the chunk edges 64 and 128
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 130)        # the chunk and level boundaries
CAPACITIES = [1, 63, 64, 65, 130, 4097]


def game_weight(row, L):
    """(the game's weight, its 64 chunk sums) from position weights row[:L]."""
    chunks = np.zeros(64)
    for c in range(-(-L // 64)):
        chunks[c] = scan64(row[c * 64:min(L, (c + 1) * 64)])[63]
    return scan64(chunks)[63], chunks


def restated_positions(pprio, length, head, B, seed, step, symmetries=False, beta=0.0):
    """[(index, start, symmetry, slot)] and the f32 importance weights."""
    cap = len(length)
    leaf = np.array([game_weight(pprio[i], int(length[i]))[0] if length[i] > 0 else 0.0 for i in range(cap)])
    n_pos = int(sum(int(x) for x in length if x > 0))
    n1 = -(-cap // 64)
    n2 = -(-n1 // 64)
    l1 = np.zeros(n2 * 64)
    for g in range(n1):
        l1[g] = scan64(leaf[g * 64:(g + 1) * 64])[63]
    l2 = np.zeros(64)
    for g in range(n2):
        l2[g] = scan64(l1[g * 64:(g + 1) * 64])[63]
    key = stream_key(seed, DOMAIN, step)
    out, picked, total0 = [], [], None
    for t in range(B):
        total = scan64(l2)[63]
        total0 = total if total0 is None else total0
        target = u01(draw(key, TAG_SAMPLE, t)) * total
        j2, target = pick64(l2, target)
        j1, target = pick64(l1[j2 * 64:(j2 + 1) * 64], target)
        g1 = j2 * 64 + j1
        j0, target = pick64(leaf[g1 * 64:(g1 + 1) * 64], target)
        slot = g1 * 64 + j0
        leaf[slot] = 0.0
        l1[g1] = scan64(leaf[g1 * 64:(g1 + 1) * 64])[63]
        l2[j2] = scan64(l1[j2 * 64:(j2 + 1) * 64])[63]
        L = int(length[slot])
        _, chunks = game_weight(pprio[slot], L)
        jc, target = pick64(chunks, target)
        jt, target = pick64(pprio[slot][jc * 64:min(L, (jc + 1) * 64)], target)
        start = jc * 64 + jt
        picked.append(pprio[slot][start])
        sym = randbelow(draw(key, TAG_SYM, t), 8) if symmetries else 0
        out.append(((slot - head) % cap, start, sym, slot))
    v = np.array([float(np.float64(n_pos) * w / total0) ** -float(beta) for w in picked])     # (the C library's pow)
    return out, (v / v.max()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def build_pos_case(cap):
    """Per-slot (pprio [cap, M], length [cap], head) for a ring of ``cap``
    slots: lengths drawn from LENGTHS (so some games are empty), weights
    log-uniform over FLT_MIN .. 1e3, and by turns a game with a leading zero
    chunk, one with a trailing run of zeros, one with a single positive
    position and one with zeros sprinkled in; the ring wrapped (head = cap // 3)."""
    r = np.random.default_rng(500 + cap)
    length = r.choice(LENGTHS, cap).astype(np.int32)
    length[r.integers(cap)] = 130                          # (at least one game, of every chunk)
    pprio = 10.0 ** r.uniform(np.log10(FLT_MIN), 3.0, (cap, M))
    for i in range(cap):
        L, kind = int(length[i]), i % 5
        if L < 2:
            continue
        if kind == 0 and L > 64:
            pprio[i, :64] = 0.0                            # a leading zero chunk
        elif kind == 1:
            pprio[i, L // 2:L] = 0.0                       # a trailing zero run
        elif kind == 2:
            one = int(r.integers(L))
            pprio[i, :one] = 0.0                           # a single positive position
            pprio[i, one + 1:] = 0.0
        elif kind == 3:
            pprio[i, r.random(M) < 0.3] = 0.0
            pprio[i, int(r.integers(L))] = 1.0
    pprio.setflags(write=False)
    length.setflags(write=False)
    return pprio, length, cap // 3


def _twin(pprio, length, head, B, seed, step, symmetries=False, beta=0.0):
    from mzgo.replay import sample_positions_host
    return sample_positions_host(pprio, length, head, B, seed=seed, step=step, symmetries=symmetries, beta=beta)


def _assert_twin_equals_restatement(pprio, length, head, B, seed, step, symmetries=False, beta=0.0):
    got = _twin(pprio, length, head, B, seed, step, symmetries, beta)
    want, weight = restated_positions(pprio, length, head, B, seed, step, symmetries, beta)
    assert got["index"].tolist() == [w[0] for w in want]
    assert got["items"][:, 0].tolist() == [w[3] for w in want]
    assert got["items"][:, 1].tolist() == [w[1] for w in want]
    assert got["items"][:, 2].tolist() == [w[2] for w in want]
    assert got["weight"].dtype == np.float32
    np.testing.assert_array_equal(got["weight"].view(np.uint32), weight.view(np.uint32))       # bitwise, as f32
    return got


@pytest.mark.parametrize("cap", CAPACITIES)
def test_twin_equals_the_restatement(cap):
    pprio, length, head = build_pos_case(cap)
    n_valid = int((length > 0).sum())
    assert cap < 63 or (set(LENGTHS) == set(length.tolist()) and head != 0)
    for B, sym, beta in ((1, True, 0.0), (min(n_valid, 7), False, 0.5), (n_valid, True, 1.0)):   # last: the tree drawn empty
        got = _assert_twin_equals_restatement(pprio, length, head, B, 77, cap + B, sym, beta)
        slots, starts = got["items"][:, 0], got["items"][:, 1]
        assert len(set(slots.tolist())) == B                           # distinct games
        assert ((starts >= 0) & (starts < length[slots])).all()
        assert (pprio[slots, starts] > 0).all()                        # never a zero-weight position
        assert ((got["index"] + head) % cap == slots).all()
        assert (got["items"][:, 2] >= 0).all() and (got["items"][:, 2] < 8).all()
        assert sym or (got["items"][:, 2] == 0).all()
        assert got["weight"].max() == 1.0 and (beta > 0 or (got["weight"] == 1.0).all())
    assert sorted(slots.tolist()) == np.flatnonzero(length > 0).tolist()       # B = n_valid: every game once


@pytest.mark.parametrize("cap", CAPACITIES + [5000])
def test_one_move_games_draw_as_the_game_sampler(cap):
    """Both samplers descend one tree.  Where every game has one move and
    pprio[slot][0] = prio[slot], the position twin returns the game twin's
    items, index and weight byte for byte: a one-position game's weight is that
    position's (adding zeros is exact), n_pos = n_valid, the start drawn below 1
    is 0 and the two levels inside the game pick entry 0.  Rows of 1 and of 3
    weights, junk past the one move; B = 1, half and all of the games."""
    from mzgo.replay import sample_host
    r = np.random.default_rng(900 + cap)
    length = (r.random(cap) < 0.85).astype(np.int32)       # some slots empty
    length[r.integers(cap)] = 1
    prio = 10.0 ** r.uniform(-34.0, 1.0, cap)
    n_valid = int(length.sum())
    for Mx in (1, 3):
        pprio = 10.0 ** r.uniform(-34.0, 1.0, (cap, Mx))   # (columns past the length: never read)
        pprio[:, 0] = prio
        for B in sorted({1, max(1, n_valid // 2), n_valid}):
            for beta in (0.0, 0.5):
                draw_ = dict(seed=31, step=cap + B, symmetries=True, beta=beta)
                want = sample_host(prio, length, cap // 3, B, **draw_)
                got = _twin(pprio, length, cap // 3, B, **draw_)
                assert (want["items"][:, 1] == 0).all() and len(set(want["items"][:, 0].tolist())) == B
                for k in ("items", "index", "weight"):
                    assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, Mx, B, beta)


def test_targets_next_to_a_boundary_stay_on_positive_positions():
    """Weights that make every rounding case: 1e-300 next to 1, a zero, then
    1e300 across the chunk edge at 64 (and again at 128, and in a second game
    whose last chunk is all zero).  2000 steps: every draw lands on a positive
    position inside its game, and the twin equals the restatement."""
    cap = 3
    pprio = np.zeros((cap, M))
    length = np.array([130, 66, 129], np.int32)
    pprio[0, 62:66] = [1e-300, 1.0, 0.0, 1e300]            # (63 | 64: the chunk edge)
    pprio[0, 126:130] = [1e-300, 1.0, 0.0, 1e300]
    pprio[1, 62:66] = [1e300, 0.0, 1e-300, 0.0]            # (the last chunk's only weight is 1e-300)
    pprio[2, 0] = 1e-300
    pprio[2, 63] = 1.0
    pprio[2, 64:129] = 0.0                                 # two trailing zero chunks
    seen = set()
    for step in range(2000):
        B = 1 + step % 3
        got = (_assert_twin_equals_restatement if step % 10 == 0 else _twin)(pprio, length, 1, B, 9, step)
        slots, starts = got["items"][:, 0], got["items"][:, 1]
        assert ((starts >= 0) & (starts < length[slots])).all()
        assert (pprio[slots, starts] > 0).all(), (step, got["items"])
        seen.update(zip(slots.tolist(), starts.tolist()))
    assert {(0, 65), (0, 129), (1, 62)} <= seen                        # the heavy ones, of course
    assert seen - {(0, 65), (0, 129), (1, 62)}                         # and, once those games are taken, the others


def test_frequencies_follow_the_position_weights():
    """3 games of lengths 2, 3 and 4 whose 9 positions weigh 1 .. 9, seed 4321,
    steps 0 .. 19999: the first draw's (game, position) has probability w / 45;
    4 sigma bars (binomial)."""
    length = np.array([2, 3, 4], np.int32)
    pprio = np.zeros((3, 4))
    w = np.arange(1.0, 10.0)
    where = [(g, t) for g in range(3) for t in range(int(length[g]))]
    for (g, t), x in zip(where, w):
        pprio[g, t] = x
    n = 20000
    count = np.zeros((3, 4))
    for step in range(n):
        slot, start, _ = _twin(pprio, length, 0, 1, 4321, step)["items"][0]
        count[slot, start] += 1
    P = w / 45.0
    got = np.array([count[g, t] for g, t in where])
    z = (got - n * P) / np.sqrt(n * P * (1 - P))
    print("first-draw |z| max", np.abs(z).max(), "counts", got.tolist())
    assert got.sum() == n and np.abs(z).max() < 4


def _game(L, seed):
    r = np.random.default_rng(seed)
    return r.uniform(-1, 1, L + 1), r.uniform(-1, 1, L)


@pytest.mark.parametrize("L", [1, 2, 9, 65])
def test_td_rule_equals_the_value_targets(L):
    """position_priorities_host = |root value - value_targets_host|, floored
    and raised to alpha: td_steps 1, K and L + 3; alpha 1 exact."""
    from mzgo.replay import position_priorities_host, value_targets_host
    K, discount = 5, 0.97
    reward, rv = _game(L, 40 + L)
    rv[0] = float(np.float32(reward[0] + discount * (rv[1] if L > 1 else reward[1])))     # (an error of exactly 0 at n = 1)
    for n in (1, K, L + 3):
        target = np.concatenate([value_targets_host(reward, rv, s, K, n, discount).astype(np.float64)
                                 for s in range(0, L, K + 1)])[:L]
        err = np.abs(rv - target)
        for floor, fl in ((None, FLT_MIN), (0.25, 0.25)):
            got = position_priorities_host(reward, rv, n, discount, 1.0, floor)
            np.testing.assert_array_equal(got, np.maximum(err, fl))                       # alpha 1: exactly the floored value
            half = position_priorities_host(reward, rv, n, discount, 0.5, floor)
            np.testing.assert_allclose(half, np.maximum(err, fl) ** 0.5, rtol=4e-16)      # (pow: within an ulp of numpy's)
            assert (got >= fl).all() and got.shape == (L,)
        if n == 1:
            assert err[0] == 0.0 and position_priorities_host(reward, rv, 1, discount)[0] == FLT_MIN


def test_twin_refusals():
    from mzgo import MzgoError
    from mzgo.replay import position_priorities_host
    pprio, length, head = build_pos_case(65)
    n_valid = int((length > 0).sum())
    for kwargs, word in ((dict(B=n_valid + 1), "exceeds"), (dict(B=0), "B must be >= 1"), (dict(head=65), "head 65"),
                         (dict(beta=-1.0), "beta")):
        a = dict(pprio=pprio, length=length, head=head, B=4, seed=1, step=0)
        a.update(kwargs)
        with pytest.raises(MzgoError, match=word):
            _twin(**a)
    slot = int(np.flatnonzero(length > 1)[0])
    bad = pprio.copy()
    bad[slot, 1] = -1.0
    with pytest.raises(MzgoError, match="finite and >= 0"):
        _twin(bad, length, head, 4, 1, 0)
    bad = pprio.copy()
    bad[slot, :] = 0.0
    with pytest.raises(MzgoError, match="game's weight"):
        _twin(bad, length, head, 4, 1, 0)
    with pytest.raises(MzgoError, match="max_moves 4097"):
        _twin(np.ones((1, 4097)), np.ones(1, np.int32), 0, 1, 1, 0)
    with pytest.raises(MzgoError, match="td_steps"):
        position_priorities_host([0.0, 1.0], [0.5], 0, 0.99)
    with pytest.raises(MzgoError, match="alpha"):
        position_priorities_host([0.0, 1.0], [0.5], 1, 0.99, alpha=0.0)


def test_position_priorities_refusals_on_the_cpu():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, TrainConfig
    net = mzgo.MuZeroNet(32, 26)
    c = TrainConfig()
    assert (c.position_priorities, c.priority_floor) == (False, 0.0)
    with pytest.raises(ValueError, match="position_priorities needs device_sampling"):
        MuZeroTrainer(net, TrainConfig(position_priorities=True), mode="batched")
    with pytest.raises(ValueError, match="device_sampling"):
        MuZeroTrainer(net, TrainConfig(position_priorities=True, device_sampling=True), mode="reference")
    with pytest.raises(ValueError, match="priority_floor belongs to position_priorities"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True, priority_floor=0.1), mode="batched")
    with pytest.raises(ValueError, match="priority_floor must be finite"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True, position_priorities=True, priority_floor=-1.0),
                      mode="batched")
    tr = MuZeroTrainer(net, TrainConfig(device_sampling=True, position_priorities=True, priority_floor=1e-3),
                       mode="batched", sample_seed=7)
    assert tr.config.position_priorities and tr.sample_step == 0
