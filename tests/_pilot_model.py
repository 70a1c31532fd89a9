"""The pursuit pilot and the refresh of the online expert rows in numpy — the rule of include/hirl4ucav.h ("The pilot as a kernel"), operation by
operation in the kernel's order (hx_pilot.hip is built without FMA contraction, with correctly rounded divide and square root, so numpy's fp32
arithmetic gives the same bits), and the same rule in float64 as the yardstick of the fp32 rounding error.  Plus the seeded inputs the tests share.
"""
import numpy as np

OBS, ACT, ROW = 13, 4, 32
ALLY_POS, ALLY_QUAT, OPPO_POS = 0, 6, 13


def levels(state, dtype=np.float32):
    """state [37, n] -> the three stick levels [n, 3] BEFORE noise and clamp, every operation rounded to `dtype`"""
    s = np.asarray(state).astype(dtype)
    one, two = dtype(1), dtype(2)
    w, x, y, z = (s[ALLY_QUAT + i] for i in range(4))
    d0, d1, d2 = (s[OPPO_POS + i] - s[ALLY_POS + i] for i in range(3))
    with np.errstate(all="ignore"):
        ax = (one - two * (y * y + z * z), two * (x * y + w * z), two * (x * z - w * y))
        ay = (two * (x * y - w * z), one - two * (x * x + z * z), two * (y * z + w * x))
        az = (two * (x * z + w * y), two * (y * z - w * x), one - two * (x * x + y * y))
        b0, b1, b2 = ((r[0] * d0 + r[1] * d1) + r[2] * d2 for r in (ax, ay, az))
        nrm = np.sqrt((b0 * b0 + b1 * b1) + b2 * b2)
        nrm = np.where(nrm < dtype(1e-6), dtype(1e-6), nrm)  # (a comparison: a NaN stays a NaN)
        out = np.stack([dtype(-4) * (b1 / nrm), dtype(-2) * (b0 / nrm), dtype(4) * (b0 / nrm)], 1)
    assert out.dtype == dtype
    return out


def norm_of(state, dtype=np.float32):
    """the bearing's norm before the 1e-6 floor (for the tests' own conditions)"""
    s = np.asarray(state).astype(dtype)
    d = np.stack([s[OPPO_POS + i] - s[ALLY_POS + i] for i in range(3)])
    with np.errstate(all="ignore"):
        return np.sqrt((d * d).sum(0))  # (|R^T d| = |d| up to rounding: zero exactly where ally and opponent coincide)


def clamp(v):
    with np.errstate(invalid="ignore"):
        one = v.dtype.type(1)
        return np.where(v < -one, -one, np.where(v > one, one, v))  # (comparisons: a NaN stays a NaN)


def actions(state, obs, noise=None, dtype=np.float32):
    """-> [n, 4]: the clamped levels (+ noise [n, 3] before the clamp) and fire = +1 iff obs[7] > 0 and obs[8] > 0, else -1"""
    lv = levels(state, dtype)
    if noise is not None:
        with np.errstate(invalid="ignore"):
            lv = lv + np.asarray(noise).astype(dtype)
    o = np.asarray(obs)
    with np.errstate(invalid="ignore"):
        fire = np.where((o[:, 7] > 0) & (o[:, 8] > 0), dtype(1), dtype(-1))
    return np.concatenate([clamp(lv), fire[:, None]], 1).astype(dtype)


# ---- the refresh rule (Python integers: exact for every 64-bit call) ------------------------------------------------------------------------
def env_picks(call, n, k):
    return [(call + j * (n // k)) % n for j in range(k)]


def slots(call, k, online_rows, offline_rows):
    return [offline_rows + (call * k + j) % online_rows for j in range(k)]


def initial_table(offline, online_rows):
    """[E0, 32] -> [E0 + M, 32]: online row i starts as offline row i mod E0"""
    offline = np.asarray(offline, np.float32)
    return np.concatenate([offline, offline[np.arange(online_rows) % offline.shape[0]]])


class RefreshModel:
    def __init__(self, table, offline_rows, online_rows, k, call=0):
        self.table, self.e0, self.m, self.k, self.call = np.array(table, np.float32), offline_rows, online_rows, k, call
        assert self.table.shape == (offline_rows + online_rows, ROW)

    def push(self, state, obs):
        """-> the slots that were written"""
        n = obs.shape[0]
        act = actions(state, obs)  # noise-free
        wrote = []
        for e, slot in zip(env_picks(self.call, n, self.k), slots(self.call, self.k, self.m, self.e0)):
            row = np.zeros(ROW, np.float32)
            row[0:OBS], row[OBS:OBS + ACT] = obs[e], act[e]
            if np.isfinite(row[:OBS + ACT]).all():
                self.table[slot] = row
                wrote.append(slot)
        self.call += 1
        return wrote


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
SPECIAL = {"coincide": 1, "nan_state": 2, "inf_state": 3}  # rows planted where n allows (make_inputs)


def make_inputs(n, seed=0, special=True):
    """-> state [37, n] fp32, obs [n, 13] fp32, noise [n, 3] fp32.  Unit-ish quaternions; the opponent mostly ahead of the nose (as in flight: the
    levels are then unclamped in a good share of rows) and anywhere for the rest; ranges from metres to tens of kilometres.  Planted where n allows:
    row 1 — ally and opponent at one point (nrm < 1e-6), row 2 — a NaN state word, row 3 — an infinite one."""
    rng = np.random.default_rng(1000 * seed + n)
    state = rng.uniform(-1, 1, (37, n))
    q = rng.normal(size=(4, n))
    q /= np.linalg.norm(q, axis=0)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])  # body -> world, [3, 3, n]
    body = rng.normal(size=(3, n))
    ahead = rng.random(n) < 0.7
    body[:, ahead] = np.stack([rng.normal(0, 0.08, ahead.sum()), rng.normal(0, 0.04, ahead.sum()), np.ones(ahead.sum())])
    body *= 10.0 ** rng.uniform(0, 4.5, n) / np.linalg.norm(body, axis=0)
    ally = rng.uniform(-5000, 5000, (3, n))
    state[ALLY_POS:ALLY_POS + 3] = ally
    state[ALLY_QUAT:ALLY_QUAT + 4] = q
    state[OPPO_POS:OPPO_POS + 3] = ally + np.einsum("ijn,jn->in", R, body)
    state = state.astype(np.float32)
    obs = rng.uniform(-1, 1, (n, OBS)).astype(np.float32)
    obs[:, 7] = rng.choice([-1.0, 1.0], n)  # locked
    obs[:, 8] = rng.choice([-1.0, 1.0], n)  # missile on the rail
    noise = rng.normal(0, 0.3, (n, 3)).astype(np.float32)
    if special:
        if n > SPECIAL["coincide"]:
            state[OPPO_POS:OPPO_POS + 3, SPECIAL["coincide"]] = state[ALLY_POS:ALLY_POS + 3, SPECIAL["coincide"]]
        if n > SPECIAL["nan_state"]:
            state[ALLY_QUAT + 1, SPECIAL["nan_state"]] = np.nan
        if n > SPECIAL["inf_state"]:
            state[OPPO_POS, SPECIAL["inf_state"]] = np.inf
    return state, obs, noise


def make_offline(rows, seed=0):
    """an offline expert table [rows, 32]: words 0..16 uniform in [-1, 1], fire +-1, words 17..31 zero"""
    rng = np.random.default_rng(77 + seed)
    t = np.zeros((rows, ROW), np.float32)
    t[:, :OBS + ACT] = rng.uniform(-1, 1, (rows, OBS + ACT))
    t[:, OBS + ACT - 1] = rng.choice([-1.0, 1.0], rows)
    return t
