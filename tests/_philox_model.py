"""The single host statement of every in-kernel random draw (test infrastructure only; DESIGN.md "Who draws where").

philox4x32_10        Philox4x32-10 (Salmon et al., SC'11) on numpy arrays of counters and keys — csrc/hx_update.h philox4x32_10, its second copy in
                     csrc/hx_env_dev.h and the oracle's ox_philox4x32_10; tests/test_draws_cpu.py holds all the other host copies to this one.
u01                  the uniform of a word IN FLOAT32 AS THE DEVICE FORMS IT: ((float)(u >> 8) + 0.5f) * 2^-24.  From u >> 8 = 2^23 on the sum is not
                     representable and rounds to even; for u >> 8 = 0xFFFFFF it is 2^24 and the uniform is exactly 1.0f (log = 0: both normals of the pair are 0).
normals              Box-Muller on those float32 uniforms, in float64 (the reference the device's logf / sinf / cosf are held to) or in float32 (numpy's libm:
                     the yardstick E32 of tests/test_draws_cpu.py).  Component j uses words j & 2 and (j & 2) + 1, cos for even j, sin for odd.
*_counters           one function per consumer -> (key, counter words [n, 4]).
sample_model         the minibatch draw of sample_kernel (hx_sampler.hip) and draw_fused (hx_update.h) in exact integers.  Neither the hash nor the table size
                     appears: the result does not depend on them."""
import numpy as np

M32 = 0xFFFFFFFF
TAG_ACT, TAG_GAUSS = 0x61637421, 0x53414331           # hx_act_body.h: the deterministic head's exploration noise, the Gaussian head's eps
SMOOTH_ROW, SMOOTH_STREAM = 0xFFFFFFF0, 2             # hx_sampler.hip / hx_update.h smoothing_noise
PER_STREAM = 0x50455231                               # hx_per.hip kPerStream
UPS_STREAM, UPS_FIRE_ROW = 0x55505331, 0xFFFFFFF1     # hx_upsample.hip kUpsStream, kUpsFireRow
BANK_STEP, BANK_INIT = 0x4E4F4900, 0x4E4F4980         # hx_noise.hip: | pole k
SCORE_ROW0, LEARN_NEXT_ROW0 = 0xC0000000, 0x40000000  # hx_score.hip; SAC learn()'s policy.sample(s')
MAX_ROUNDS = 128

_U = np.uint64


def key_of(seed):
    """the two key words of a 64-bit seed (low, high), as every kernel splits it"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & M32, seed >> 32


def philox4x32_10(counter, key):
    """counter [..., 4] and key [..., 2] (any integer arrays that broadcast against each other in the leading dimensions) -> words [..., 4] uint32"""
    c = np.asarray(counter, dtype=np.uint64) & _U(M32)
    k = np.asarray(key, dtype=np.uint64) & _U(M32)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = _U(0xD2511F53) * c0, _U(0xCD9E8D57) * c2  # (32 x 32 bits: the product fits 64)
        c0, c1, c2, c3 = (p1 >> _U(32)) ^ c1 ^ k0, p1 & _U(M32), (p0 >> _U(32)) ^ c3 ^ k1, p0 & _U(M32)
        k0, k1 = (k0 + _U(0x9E3779B9)) & _U(M32), (k1 + _U(0xBB67AE85)) & _U(M32)
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u01(words):
    """float32, every operation in float32 as the device's u01: (float)(u >> 8) is exact, + 0.5f rounds from 2^23 on, * 2^-24 is exact"""
    w = np.asarray(words, dtype=np.uint32)
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def normals(words, dtype=np.float64):
    """words [..., 4] -> standard normals [..., 4] in `dtype`: float64 = the reference; float32 = the same formula with every operation and constant in
    float32 (the device's order: sqrtf(-2 logf(ua)), 6.2831853f * ub)"""
    u = u01(words)
    out = np.empty(u.shape, dtype)
    two_pi = dtype(6.28318530717958647692)
    for p in (0, 2):
        ua, ub = u[..., p].astype(dtype), u[..., p + 1].astype(dtype)
        rad, ang = np.sqrt(dtype(-2.0) * np.log(ua)), two_pi * ub
        out[..., p], out[..., p + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out


def _counters(w0, w1, w2, w3):
    w0 = np.asarray(w0, dtype=np.uint64).reshape(-1)
    out = np.empty((w0.size, 4), np.uint64)
    out[:, 0] = w0 & _U(M32)
    for i, w in ((1, w1), (2, w2), (3, w3)):
        out[:, i] = np.asarray(w, dtype=np.uint64) & _U(M32)
    return out


# ---- who draws where: key and counter words per consumer ---------------------------------------------------------------------------------------------
def act_counters(seed, row0, n, call, tag=TAG_ACT):
    """the acting kernels' deterministic head: ((row0 + row) mod 2^32, call, tag, 0)"""
    return key_of(seed), _counters(int(row0) + np.arange(n, dtype=np.uint64), call, tag, 0)


def gauss_counters(seed, row0, n, call):
    """the Gaussian head (acting, learn() from LEARN_NEXT_ROW0, the scorer from SCORE_ROW0)"""
    return act_counters(seed, row0, n, call, TAG_GAUSS)


def smoothing_counters(seed, call):
    return key_of(seed), _counters([SMOOTH_ROW], call, SMOOTH_STREAM, 0)


def sampler_counters(seed, rows, call, stream, rnd):
    return key_of(seed), _counters(rows, call, stream, rnd)


def per_counters(seed, n, call):
    return key_of(seed), _counters(np.arange(n), call, PER_STREAM, 0)


def upsample_counters(seed, n_main, call, fire=False):
    rows = list(range(n_main)) + ([UPS_FIRE_ROW] if fire else [])
    return key_of(seed), _counters(rows, call, UPS_STREAM, 0)


def bank_counters(seed, row0, n, step, pole, init=False):
    """the AR(1) bank: (row, step lo, step hi, BANK_STEP | k); its initial state (row, 0, 0, BANK_INIT | k)"""
    step = 0 if init else int(step) & 0xFFFFFFFFFFFFFFFF
    return key_of(seed), _counters(int(row0) + np.arange(n, dtype=np.uint64), step & M32, step >> 32, (BANK_INIT if init else BANK_STEP) | int(pole))


def env_reset_counters(seed, env_ids, episodes):
    return key_of(seed), _counters(env_ids, episodes, 0, 0)


def draw_normals(key_counters, dtype=np.float64):
    key, c = key_counters
    return normals(philox4x32_10(c, key), dtype)


def act_normals(seed, row0, n, call, tag=TAG_ACT, dtype=np.float64):
    """[n, 4]: the four draws of rows row0 .. row0 + n - 1 of acting call `call`"""
    return draw_normals(act_counters(seed, row0, n, call, tag), dtype)


def smoothing_normals(seed, call, dtype=np.float64):
    """[4]: the target-smoothing draw of sample call `call` before the factor sigma"""
    return draw_normals(smoothing_counters(seed, call), dtype)[0]


# ---- the draws the quality test looks at, and the float32 yardstick ------------------------------------------------------------------------------------
QUALITY_SEED, QUALITY_ROWS, QUALITY_CALLS = 4, 1 << 16, 16  # (the seed: tests/test_draws_cpu.py test_quality_of_the_models_normals says how it was chosen)
_cache = {}


def quality_words():
    """Philox words [QUALITY_ROWS, QUALITY_CALLS, 4] under the acting tag: rows 0 .., calls 1 .., key QUALITY_SEED"""
    if "words" not in _cache:
        rows, calls = np.meshgrid(np.arange(QUALITY_ROWS, dtype=np.uint64), np.arange(1, QUALITY_CALLS + 1, dtype=np.uint64), indexing="ij")
        c = _counters(rows.reshape(-1), calls.reshape(-1), TAG_ACT, 0)
        _cache["words"] = philox4x32_10(c, key_of(QUALITY_SEED)).reshape(QUALITY_ROWS, QUALITY_CALLS, 4)
    return _cache["words"]


def e32():
    """E32 = max |z32 - z64| over the 2^22 draws of quality_words(): what ONE float32 evaluation of the Box-Muller formula (numpy's libm) is away from the
    float64 one on the same float32 uniforms.  The budget of the device's logf / sinf / cosf normals is a multiple of it (tests/test_draws_gpu.py)."""
    if "e32" not in _cache:
        w = quality_words()
        _cache["e32"] = float(np.abs(normals(w, np.float32).astype(np.float64) - normals(w, np.float64)).max())
    return _cache["e32"]


# ---- the minibatch draw ------------------------------------------------------------------------------------------------------------------------------
def draw_map(total, cap, guard):
    """draw_map (hx_update.h) -> (live, e0, h, jump): the population size and what slot_of_draw needs"""
    tot, cap, guard = int(total), int(cap), int(guard)
    if guard == 0:
        return min(tot, cap), 0, M32, 0
    if tot < cap:
        over = max(tot + guard - cap, 0)
        e0 = min(over, tot)
        return tot - e0, e0, M32, 0
    g = min(guard, cap)
    h = tot % cap
    e0 = max(h + g - cap, 0)
    return cap - g, e0, h, g - e0


def slot_of_draw(m, k):
    """draw k of m[0] -> ring slot: the wrapped part of the guard window shifts every draw up, a draw at or beyond the head jumps the rest of it"""
    _, e0, h, jump = m
    s = np.asarray(k, dtype=np.int64) + e0
    return np.where(s >= h, s + jump, s)


def _draw_stream(lens, groups, stream, seed, call):
    """one index stream: lens / groups [rows] -> (keys without the group bit, rounds run).  Rounds are synchronous: every row still marked duplicate
    redraws with the round as counter word 3, then a row is a duplicate iff it is not the lowest row that has EVER drawn its key."""
    n = len(lens)
    key = np.zeros(n, np.uint64)
    dup = np.ones(n, bool)
    owner = {}
    lens, groups = np.asarray(lens, dtype=np.uint64), np.asarray(groups, dtype=np.uint64)
    for rnd in range(MAX_ROUNDS):
        r = np.flatnonzero(dup)
        w0 = philox4x32_10(sampler_counters(seed, r, call, stream, rnd)[1], key_of(seed))[:, 0].astype(np.uint64)
        key[r] = groups[r] | ((w0 * lens[r]) >> _U(32))  # umulhi(word 0, len); len == 0 gives 0
        for t in r:
            k = int(key[t])
            if owner.get(k, n) > t:
                owner[k] = int(t)
        dup = np.array([owner[int(key[t])] != t for t in range(n)], bool)
        if not dup.any():
            return key & _U(0x7FFFFFFF), rnd + 1
    return key & _U(0x7FFFFFFF), MAX_ROUNDS


def sample_model(total, cap, guard, expert_len, bc_len, batch, n_main, seed, call):
    """-> (idx [batch], idx_bc [batch] or None when bc_len is None, rounds_used).  Stream 0: rows [0, n_main) draw from the `live` slots of the main ring
    (group 0, mapped through the guard), rows [n_main, batch) from the expert ring (group 1); stream 1: every row from the BC table.  Without
    replacement inside a group until MAX_ROUNDS rounds have run; a row that is still a duplicate then keeps its last key.  rounds_used: the rounds the
    longer of the two streams ran (MAX_ROUNDS: the cap was reached)."""
    m = draw_map(total, cap, guard)
    rows = np.arange(batch)
    main = rows < int(n_main)
    keys, used = _draw_stream(np.where(main, m[0], int(expert_len)), np.where(main, 0, 0x80000000), 0, seed, call)
    idx = np.where(main, slot_of_draw(m, keys), keys.astype(np.int64)).astype(np.int32)
    if bc_len is None:
        return idx, None, used
    kb, used_bc = _draw_stream(np.full(batch, int(bc_len)), np.zeros(batch), 1, seed, call)
    return idx, kb.astype(np.int32), max(used, used_bc)
