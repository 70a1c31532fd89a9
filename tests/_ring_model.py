"""The replay ring's slot rule in plain Python integers (include/hirl4ucav.h "Replay ring"): transition number t (0-based, counted by
DeviceReplay.total) lives in slot t % cap.  Counters here are Python `int`s throughout — no numpy type ever holds one — so nothing in this file
can wrap at 32 or 64 bits; tests/test_ring_counter_cpu.py and tests/test_ring_counter_gpu.py hold the kernels and the host code to it."""
import numpy as np

TOTAL_BOUND = 1 << 52  # the documented domain of the counters: total < 2^52 (ring_slot's fp64 quotient, csrc/hx_env_dev.h)


def slots(total, k, cap):
    """the slots of the k transitions stored from counter value `total` on"""
    total, k, cap = int(total), int(k), int(cap)
    return [(total + i) % cap for i in range(k)]


def allowed_slots(tot, cap, guard):
    """The population of a guarded draw, restated: every slot that holds a transition before the env step (slots < min(tot, cap)) and is not one of
    the `guard` slots behind the ring head tot % cap."""
    tot, cap, guard = int(tot), int(cap), int(guard)
    live = np.arange(min(tot, cap))
    window = np.array(slots(tot, guard, cap), dtype=np.int64)
    return np.setdiff1d(live, window)


def ring_slot_estimate(total, cap, taken=None):
    """ring_slot (csrc/hx_env_dev.h) restated: the quotient from ONE fp64 multiply by a host-computed 1.0 / cap and a truncation — numpy's float64
    gives the kernel's bits —, the remainder in integers, one correction step either way.  `taken`: a list that receives "low" (the estimate was
    one too large: r < 0) or "high" (one too small: r >= cap) when a correction ran."""
    total, cap = int(total), int(cap)
    inv_cap = np.float64(1.0) / np.float64(cap)
    q = int(np.float64(total) * inv_cap)  # (unsigned long long)((double)total * inv_cap): truncation
    r = total - q * cap
    if r < 0:
        r += cap
        if taken is not None:
            taken.append("low")
    if r >= cap:
        r -= cap
        if taken is not None:
            taken.append("high")
    return r


# A capacity at which ring_slot's "high" correction DOES run below 2^52: fl(1 / 1006) is below 1 / 1006, and at the multiples m * 1006 whose m is high
# in its binade the product m * 1006 * fl(1 / 1006) rounds to the double below m (tests/test_ring_counter_cpu.py names more such pairs).
CORRECTION_CAP = 1006


def corrected_multiple(cap, start):
    """the first multiple of cap at or above `start` whose quotient estimate needs a correction step"""
    cap = int(cap)
    m = -(-int(start) // cap)
    for k in range(m, m + 64):
        taken = []
        ring_slot_estimate(k * cap, cap, taken)
        if taken:
            return k * cap
    raise ValueError(f"no multiple of {cap} near {start} needs a correction")


def CORRECTION_TOTALS():
    """totals at CORRECTION_CAP whose ring_slot takes the "high" step: m * cap with m just below 2^23 (the first beyond 2^32), 2^31 and 2^42 (the last
    below 2^52) — m high in its binade, where m * 2^-53 is more than half a unit in m's last place"""
    return [corrected_multiple(CORRECTION_CAP, CORRECTION_CAP * ((1 << e) - 64)) for e in (23, 31, 42)]


def EDGE_TOTALS(cap, rows):
    """The totals every GPU test of the counter starts from; `rows` is the most rows one call can insert.
    2^32 - j for j in {1, rows // 2, rows - 1}: the crossing happens inside one call (and, with several workgroups, between two atomicAdds);
    2^32 and 2^32 + 1; the multiple of cap nearest to 2^40 and that value - 1 (the head at slot 0 and at slot cap - 1); 2^52 - 2 cap - 3: the top of
    the documented domain with room for the calls of a test."""
    cap, rows = int(cap), int(rows)
    near = ((1 << 40) + cap // 2) // cap * cap
    out = [(1 << 32) - j for j in (1, rows // 2, rows - 1) if j > 0]
    out += [1 << 32, (1 << 32) + 1, near, near - 1, TOTAL_BOUND - 2 * cap - 3]
    return list(dict.fromkeys(out))


def twin_offset(t_big, cap):
    """-> (T_small, D): the small twin of a ring at t_big — full, the same head h = t_big % cap: T_small = cap + h — and the multiple of cap between"""
    t_big, cap = int(t_big), int(cap)
    t_small = cap + t_big % cap
    d = t_big - t_small
    assert d % cap == 0 and d > 0
    return t_small, d
