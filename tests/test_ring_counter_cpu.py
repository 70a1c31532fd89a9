"""The replay ring's 64-bit counter beyond 2^32, the part that needs no GPU: ring_slot's fp64 quotient estimate (csrc/hx_env_dev.h:557) restated
in numpy float64 (tests/_ring_model.ring_slot_estimate) against Python integers, and the host's own handling of `total`
(utils/buffer.py:31-45: int(total.item()), store_rows; utils/checkpoint.py:86-105: replay_state / load_replay_state).
The kernels themselves: tests/test_ring_counter_gpu.py."""
import random

import numpy as np
import pytest
import torch

from tests import _ring_model as R

CAPS = (512, 700, 1000, 1024, 2500, 2600, 4096, 20000, 40000, 1_000_003)
K = 2000  # consecutive multiples of cap per neighbourhood


def multiples(cap):
    """K consecutive multiples of cap from 2^32 on, from 2^40 on, and the last K whose successor is still below 2^52"""
    for m0 in (-(-(1 << 32) // cap), -(-(1 << 40) // cap), (R.TOTAL_BOUND - 2) // cap - K):
        for m in range(m0, m0 + K):
            yield m * cap


def test_model_helpers():
    assert R.slots((1 << 32) - 3, 6, 1000) == [293, 294, 295, 296, 297, 298] and ((1 << 32) - 3) % 1000 == 293
    assert R.slots(5 * 700 - 2, 4, 700) == [698, 699, 0, 1]
    assert R.allowed_slots(400, 700, 150).tolist() == list(range(400))
    assert R.allowed_slots(650, 700, 150).tolist() == list(range(100, 650))
    assert R.allowed_slots((1 << 40) // 700 * 700 + 620, 700, 150).tolist() == list(range(70, 620))
    assert R.allowed_slots(3 * 700 + 620, 700, 150).tolist() == list(range(70, 620))
    for cap, rows in ((1000, 300), (1024, 900), (20000, 8232), (700, 1)):
        e = R.EDGE_TOTALS(cap, rows)
        assert len(e) == len(set(e)) and all(isinstance(t, int) and cap < t and t + 2 * cap < R.TOTAL_BOUND for t in e)
        assert {(1 << 32) - 1, 1 << 32, (1 << 32) + 1, R.TOTAL_BOUND - 2 * cap - 3} <= set(e)
        assert sum(t % cap == 0 and abs(t - (1 << 40)) <= cap // 2 for t in e) == 1 and sum((t + 1) % cap == 0 and abs(t - (1 << 40)) <= cap for t in e) == 1
        if rows > 2:
            assert (1 << 32) - rows // 2 in e and (1 << 32) - (rows - 1) in e
        for t in e:
            small, d = R.twin_offset(t, cap)
            assert cap <= small < 2 * cap and small % cap == t % cap and small + d == t


def test_ring_slot_estimate_equals_integer_modulo():
    """ring_slot's estimate + corrections == total % cap: the ten capacities the suite uses at multiples of cap and their neighbours near 2^32, near
    2^40 and just below 2^52, and 10^5 seeded (total, cap) pairs with 512 <= cap < 2^31, total < 2^52.  Neither correction runs anywhere in that
    set — at these ten capacities fl(1 / cap) is not below 1 / cap, and a random total is never close enough to a multiple."""
    taken, n = [], 0
    for cap in CAPS:
        for m in multiples(cap):
            for tot in (m - 1, m, m + 1):
                assert tot < R.TOTAL_BOUND
                assert R.ring_slot_estimate(tot, cap, taken) == tot % cap, (tot, cap)
                n += 1
    rng = random.Random(20261020)
    for _ in range(100_000):
        cap, tot = rng.randrange(512, 1 << 31), rng.randrange(0, R.TOTAL_BOUND)
        assert R.ring_slot_estimate(tot, cap, taken) == tot % cap, (tot, cap)
    assert n == len(CAPS) * 3 * K * 3
    assert taken == [], taken[:8]


# (total, cap) pairs that DO need a correction below 2^52, found by snapping seeded totals onto multiples of their capacity: where fl(1 / cap) is
# below 1 / cap and total = m * cap with m large, m * cap * fl(1 / cap) rounds to the double below m, the truncation gives m - 1 and r = cap -> the
# "high" step.  A capacity either shows this at the multiples whose m is high in its binade (1006: nine in ten of seeded multiples between 2^32 and
# 2^52, none where m is just above a power of two — as near 2^32, 2^40 and 2^52) or at none (all ten above).
HIGH_PAIRS = ((737339741724906, 1033747074), (1582191345534536, 106567922), (2536230432218868, 26642), (2653221492025864, 12136),
              (46302830020, 1006))


def test_the_high_correction_is_reachable_below_2_52_and_the_low_one_is_not_found():
    """The count the search finds, and the pairs by name.  10^5 seeded pairs snapped onto the multiple of cap at or below total, and its two
    neighbours: the "high" step (estimate one too small) runs at some multiples and nowhere else, the "low" step (estimate one too large)
    never; with the correction the slot is exact every time.  tests/test_ring_counter_gpu.py runs the env step at capacity
    R.CORRECTION_CAP from such a multiple, so the branch is exercised on the device."""
    for tot, cap in HIGH_PAIRS:
        taken = []
        assert tot % cap == 0 and tot < R.TOTAL_BOUND and R.ring_slot_estimate(tot, cap, taken) == 0 and taken == ["high"], (tot, cap, taken)
    rng = random.Random(52)
    high, low, off_multiple = [], [], []
    for _ in range(100_000):
        cap, tot = rng.randrange(512, 1 << 31), rng.randrange(1 << 32, R.TOTAL_BOUND)
        m = tot // cap * cap
        for t in (m - 1, m, m + 1):
            taken = []
            assert R.ring_slot_estimate(t, cap, taken) == t % cap, (t, cap)
            if taken:
                (high if taken == ["high"] else low).append((t, cap))
                if t != m:
                    off_multiple.append((t, cap))
    assert low == [] and off_multiple == [], (low[:4], off_multiple[:4])
    assert 1000 < len(high) < 50_000, len(high)  # (a few per cent of the multiples: what fl(1 / cap) < 1 / cap and the size of m allow)
    # the device cases
    tops = R.CORRECTION_TOTALS()
    assert len(tops) == 3 and (1 << 32) < tops[0] < (1 << 34) and tops[2] > 0.98 * R.TOTAL_BOUND
    for t in tops:
        taken = []
        assert t % R.CORRECTION_CAP == 0 and t + 2 * R.CORRECTION_CAP + 3 < R.TOTAL_BOUND and R.ring_slot_estimate(t, R.CORRECTION_CAP, taken) == 0
        assert taken == ["high"], t


def ring_rows(k, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=(k, 32)).astype(np.float32))


def test_store_rows_across_2_32_on_the_cpu():
    """DeviceReplay.store_rows (utils/buffer.py:36-46) and len() (buffer.py:30-31) on a CPU replay from total = 2^32 - 3: the rows land in
    slots(total, k, cap), everything else keeps its sentinel, total moves by k as a Python integer, len() stays cap."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    cap, t0, k = 1000, (1 << 32) - 3, 10
    rep = DeviceReplay(cap, device="cpu")
    rep.ring.fill_(-7.0)
    rep.success.fill_(55)
    rep.total.fill_(t0)
    assert len(rep) == cap and int(rep.total.item()) == t0
    rows, succ = ring_rows(k, 1), torch.arange(k, dtype=torch.int8) - 4
    rep.store_rows(rows, succ)
    where = R.slots(t0, k, cap)
    assert where == list(range(293, 303))
    assert torch.equal(rep.ring[where], rows) and torch.equal(rep.success[where], succ)
    rest = np.setdiff1d(np.arange(cap), where)
    assert bool((rep.ring[rest] == -7.0).all()) and bool((rep.success[rest] == 55).all())
    assert int(rep.total.item()) == t0 + k == (1 << 32) + 7 and len(rep) == cap and rep.fullEnough(cap)
    # a call that wraps the ring past 2^40
    t1 = ((1 << 40) // cap + 1) * cap - 4
    rep.total.fill_(t1)
    rep.store_rows(rows)
    assert R.slots(t1, k, cap) == [996, 997, 998, 999, 0, 1, 2, 3, 4, 5] and torch.equal(rep.ring[R.slots(t1, k, cap)], rows)
    assert int(rep.total.item()) == t1 + k and len(rep) == cap


def test_replay_checkpoint_round_trip_at_2_40_on_the_cpu():
    """utils/checkpoint.replay_state / load_replay_state (checkpoint.py:86-105) at total = 2^40 + 5: the counter comes back as the same Python
    integer, ring and success in bits, and the next store continues in the same slots.  (A PrioritizedReplay re-sums its blocks with a kernel on
    load: its round trip, `marked` included, is tests/test_ring_counter_gpu.py::test_checkpoint_round_trip_of_a_prioritized_replay.)"""
    from hirl4ucav_amd.utils import checkpoint as C
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    cap, t0 = 700, (1 << 40) + 5
    a = DeviceReplay(cap, device="cpu")
    a.ring.copy_(ring_rows(cap, 2))
    a.success.copy_(torch.arange(cap) % 3 - 1)
    a.total.fill_(t0)
    st = C.replay_state(a)
    assert st["total"] == t0 and type(st["total"]) is int and st["ring"].shape[0] == cap
    b = DeviceReplay(cap, device="cpu")
    C.load_replay_state(b, st)
    assert int(b.total.item()) == t0 and len(b) == cap
    assert torch.equal(a.ring.view(torch.int32), b.ring.view(torch.int32)) and torch.equal(a.success, b.success)
    rows = ring_rows(9, 3)
    for r in (a, b):
        r.store_rows(rows)
    assert torch.equal(a.ring, b.ring) and int(b.total.item()) == t0 + 9
    assert torch.equal(b.ring[R.slots(t0, 9, cap)], rows)
