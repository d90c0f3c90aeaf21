"""The device sampler's algorithm on the CPU, through its host twin
(``mzgo.replay.sample_host`` -> ``mzgo_replay_sample_host``, which runs the
kernels' own scan / descent / fallback functions of csrc/mzgo_replay.hpp
serially).

``restated_sample`` below is an independent restatement in Python ints and
numpy float64: the counter RNG (``mix64``) on Python ints, the 64-ary sum tree
with every group of 64 added by the documented six-step inclusive scan
(p[i] <- p[i - d] + p[i] for d = 1, 2, 4, 8, 16, 32; a group's sum is p[63]),
the descent (first non-zero entry whose inclusive prefix exceeds the target,
else the last non-zero entry; target -= the prefix before the pick) and the
removal (zero the leaf, add both ancestors again).  The twin must give the
same (index, start, symmetry) bit for bit.

``build_case`` / ``restated_sample`` are shared with tests/test_gpu_replay_sample.py.
"""
import functools

import numpy as np
import pytest

M64 = (1 << 64) - 1
DOMAIN, TAG_SAMPLE, TAG_START, TAG_SYM = 0x53414D50, 5, 6, 7
FLT_MIN = float(np.finfo(np.float32).tiny)
CAPACITIES = [1, 63, 64, 65, 4096, 4097, 5000]


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream_key(seed, game, move):
    return mix64(mix64(seed & M64) ^ ((game << 32) | move))


def draw(key, tag, idx):
    return mix64(key ^ ((tag & 0xFF) << 56) ^ (idx & ((1 << 56) - 1)))


def u01(h):
    return float(h >> 11) * 2.0 ** -53


def randbelow(h, n):
    return ((h >> 32) * n) >> 32


def scan64(x):
    p = np.zeros(64)
    p[:len(x)] = x
    for d in (1, 2, 4, 8, 16, 32):
        q = p.copy()
        q[d:] = p[:-d] + p[d:]
        p = q
    return p


def pick64(x, target):
    p = scan64(x)
    nz = np.flatnonzero(np.asarray(x) > 0)
    over = [i for i in nz if p[i] > target]
    j = int(over[0]) if over else int(nz[-1])
    return j, target - (p[j - 1] if j > 0 else 0.0)


def restated_sample(prio, length, head, B, seed, step, symmetries=False):
    """(index, start, symmetry, slot) lists and the picked weights / total /
    n_valid for the importance weights."""
    cap = len(prio)
    leaf = np.where(np.asarray(length) > 0, np.asarray(prio, dtype=np.float64), 0.0)
    n1 = -(-cap // 64)
    n2 = -(-n1 // 64)
    l1 = np.zeros(n2 * 64)
    for g in range(n1):
        l1[g] = scan64(leaf[g * 64:(g + 1) * 64])[63]
    l2 = np.zeros(64)
    for g in range(n2):
        l2[g] = scan64(l1[g * 64:(g + 1) * 64])[63]
    key = stream_key(seed, DOMAIN, step)
    out, picked_w, total0 = [], [], None
    for t in range(B):
        total = scan64(l2)[63]
        total0 = total if total0 is None else total0
        target = u01(draw(key, TAG_SAMPLE, t)) * total
        j2, target = pick64(l2, target)
        j1, target = pick64(l1[j2 * 64:(j2 + 1) * 64], target)
        g1 = j2 * 64 + j1
        j0, target = pick64(leaf[g1 * 64:(g1 + 1) * 64], target)
        slot = g1 * 64 + j0
        picked_w.append(leaf[slot])
        leaf[slot] = 0.0
        l1[g1] = scan64(leaf[g1 * 64:(g1 + 1) * 64])[63]
        l2[j2] = scan64(l1[j2 * 64:(j2 + 1) * 64])[63]
        sym = randbelow(draw(key, TAG_SYM, t), 8) if symmetries else 0
        out.append(((slot - head) % cap, randbelow(draw(key, TAG_START, t), int(length[slot])), sym, slot))
    return out, np.array(picked_w), total0


@functools.lru_cache(maxsize=None)
def build_case(cap, empty=True, extreme=True):
    """Per-slot (prio, length, head) for a ring of ``cap`` slots: lengths 1..3,
    a third of the slots empty (length 0), weights log-uniform over FLT_MIN ..
    1e3 with both ends present, and the ring wrapped (head = cap // 3)."""
    r = np.random.default_rng(100 + cap)
    length = r.integers(1, 4, cap).astype(np.int32)
    if empty and cap > 1:
        length[r.random(cap) < 1 / 3] = 0
        length[r.integers(cap)] = 2                        # (at least one game)
    if extreme:
        prio = 10.0 ** r.uniform(np.log10(FLT_MIN), 3.0, cap)
        prio[r.integers(cap)] = FLT_MIN
        prio[r.integers(cap)] = 1e3
    else:
        prio = r.uniform(0.1, 4.0, cap)
    prio.setflags(write=False)
    length.setflags(write=False)
    return prio, length, cap // 3


def _twin(prio, length, head, B, seed, step, symmetries=False, beta=0.0):
    from mzgo.replay import sample_host
    return sample_host(prio, length, head, B, seed=seed, step=step, symmetries=symmetries, beta=beta)


def _assert_twin_equals_restatement(prio, length, head, B, seed, step, symmetries):
    got = _twin(prio, length, head, B, seed, step, symmetries)
    want, _, _ = restated_sample(prio, length, head, B, seed, step, symmetries)
    assert got["index"].tolist() == [w[0] for w in want]
    assert got["items"][:, 0].tolist() == [w[3] for w in want]
    assert got["items"][:, 1].tolist() == [w[1] for w in want]
    assert got["items"][:, 2].tolist() == [w[2] for w in want]
    return got


@pytest.mark.parametrize("cap", CAPACITIES)
def test_twin_equals_the_restatement(cap):
    prio, length, head = build_case(cap)
    n_valid = int((length > 0).sum())
    assert cap < 3 or (head != 0 and (length == 0).any())
    assert cap < 3 or (prio.min() == FLT_MIN and prio.max() == 1e3)
    for B, sym in ((1, True), (min(n_valid, 7), False), (n_valid, True)):      # B = every valid game last
        got = _assert_twin_equals_restatement(prio, length, head, B, seed=77, step=cap + B, symmetries=sym)
        slots = got["items"][:, 0]
        assert len(set(got["index"].tolist())) == B                    # distinct
        assert (length[slots] > 0).all()
        assert ((got["items"][:, 1] >= 0) & (got["items"][:, 1] < length[slots])).all()
        assert ((got["index"] + head) % cap == slots).all()
        assert (got["items"][:, 2] >= 0).all() and (got["items"][:, 2] < 8).all()
        if not sym:
            assert (got["items"][:, 2] == 0).all()
    if n_valid > 1:
        assert sorted(slots.tolist()) == np.flatnonzero(length > 0).tolist()       # B = n_valid: every game once


def test_a_group_whose_members_have_all_been_picked():
    """Group 1 (slots 64..127) holds three games a thousand times heavier
    than the rest: they go first, and the draws after them must pass the
    emptied group by."""
    cap = 200
    prio = np.full(cap, 1.0)
    length = np.full(cap, 2, np.int32)
    length[64:128] = 0
    length[[70, 90, 127]] = 3
    prio[[70, 90, 127]] = 1e9
    got = _assert_twin_equals_restatement(prio, length, 5, 40, seed=3, step=0, symmetries=False)
    slots = got["items"][:, 0].tolist()
    assert sorted(slots[:3]) == [70, 90, 127]
    assert all(s < 64 or s >= 128 for s in slots[3:]) and len(set(slots)) == 40


def test_draw_depends_on_seed_and_step_only():
    prio, length, head = build_case(65)
    a = _twin(prio, length, head, 8, 5, 9)
    b = _twin(prio, length, head, 8, 5, 9)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["items"], _twin(prio, length, head, 8, 5, 10)["items"])
    assert not np.array_equal(a["items"], _twin(prio, length, head, 8, 6, 9)["items"])


def test_frequencies_are_successive_sampling():
    """8 games with weights 1..8, B = 2, seed 1234, steps 0..19999: the first
    draw is w / sum, an ordered pair (i, j) has P_i P_j / (1 - P_i); 5 sigma
    bars (binomial)."""
    w = np.arange(1.0, 9.0)
    length = np.ones(8, np.int32)
    n = 20000
    first = np.zeros(8)
    pair = np.zeros((8, 8))
    for step in range(n):
        i, j = _twin(w, length, 0, 2, 1234, step)["index"]
        first[i] += 1
        pair[i, j] += 1
    P = w / w.sum()
    z1 = (first - n * P) / np.sqrt(n * P * (1 - P))
    Pij = P[:, None] * P[None, :] / (1 - P[:, None])
    np.fill_diagonal(Pij, 0.0)
    assert pair.diagonal().sum() == 0
    off = ~np.eye(8, dtype=bool)
    z2 = (pair[off] - n * Pij[off]) / np.sqrt(n * Pij[off] * (1 - Pij[off]))
    print("first-draw |z| max", np.abs(z1).max(), "pair |z| max", np.abs(z2).max())
    assert np.abs(z1).max() < 5 and np.abs(z2).max() < 5 and z2.size == 56


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_importance_weights(beta):
    prio, length, head = build_case(4097, extreme=False)
    B = 64
    got = _twin(prio, length, head, B, 11, 2, beta=beta)
    w = prio[got["items"][:, 0]]
    n_valid = int((length > 0).sum())
    total = np.where(length > 0, prio, 0.0).sum()
    v = (n_valid * w / total) ** (-beta)
    np.testing.assert_allclose(got["weight"].astype(np.float64), v / v.max(), rtol=1e-6)
    assert got["weight"].dtype == np.float32 and got["weight"].max() == 1.0
    if beta == 0.0:
        assert (got["weight"] == 1.0).all()
    else:
        assert len(set(got["weight"].tolist())) > B // 2


def test_twin_refusals():
    from mzgo import MzgoError
    prio, length, head = build_case(65)
    n_valid = int((length > 0).sum())
    for kwargs, word in ((dict(B=n_valid + 1), "exceeds"), (dict(B=0), "B must be >= 1"),
                         (dict(head=65), "head 65"), (dict(beta=-1.0), "beta")):
        a = dict(prio=prio, length=length, head=head, B=4, seed=1, step=0)
        a.update(kwargs)
        with pytest.raises(MzgoError, match=word):
            _twin(**a)
    bad = prio.copy()
    bad[int(np.flatnonzero(length > 0)[0])] = 0.0
    with pytest.raises(MzgoError, match="finite and > 0"):
        _twin(bad, length, head, 4, 1, 0)
    with pytest.raises(MzgoError, match="64\\^3"):
        _twin(np.ones(64 ** 3 + 1), np.ones(64 ** 3 + 1, np.int32), 0, 1, 1, 0)


def test_device_sampling_refusals_on_the_cpu():
    import mzgo
    from mzgo.trainer import MuZeroTrainer, PrioritizedReplayBuffer, TrainConfig
    net = mzgo.MuZeroNet(32, 26)
    c = TrainConfig()
    assert (c.device_sampling, c.importance_beta, c.priority_alpha, c.deferred_stats) == (False, 0.0, 1.0, False)
    with pytest.raises(ValueError, match="device_sampling"):
        MuZeroTrainer(net, TrainConfig(device_sampling=True), mode="reference")
    with pytest.raises(ValueError, match="device_sampling"):
        MuZeroTrainer(net, TrainConfig(deferred_stats=True), mode="batched")
    with pytest.raises(ValueError, match="device_sampling"):
        MuZeroTrainer(net, TrainConfig(importance_beta=0.5), mode="batched")
    tr = MuZeroTrainer(net, TrainConfig(device_sampling=True), mode="batched", sample_seed=7)
    assert tr.sample_seed == 7 and tr.sample_step == 0
    with pytest.raises(ValueError, match="DeviceReplay"):
        tr.train(PrioritizedReplayBuffer(4), 2)
