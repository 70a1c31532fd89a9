"""Expert branches on the CPU — the rule of include/hirl4ucav.h ("Expert branches"): picks and slots are hx_pilot_refresh's (tests/_pilot_model.py
env_picks / slots), the action is the pilot's noise-free one (_pilot_model.actions, bit for bit the kernel's), and the ONE step is the C oracle's
(tests/_oracle.step_batch with max_step = 0 and auto_reset = 0, on a COPY of the state: the GPU env step equals it bit for bit,
tests/test_env_gpu.py).  This file assembles the row, the success byte and the non-finite rule, and makes the seeded inputs the tests share.
"""
import numpy as np

from tests import _oracle as ox
from tests import _pilot_model as PM

OBS, ACT, ROW, WORDS = 13, 4, 32, 37
# state words (include/hirl4ucav.h "Env state layout")
ALLY_P, OPP_P, OPP_V, MIS_P, MIS_V, HEALTH, LOCK_TIMER, MIS_AGE, FLAGS, COUNTERS = 0, 13, 16, 26, 29, 32, 33, 34, 35, 36


def step_once(state, obs):
    """state [37, n], obs [n, 13] (both left as they are) -> rows [n, 32], success [n] int8, the stepped state [37, n]: every env flown one step
    under the pilot's noise-free action, no auto-reset, no time limit"""
    state, obs = np.asarray(state, np.float32), np.asarray(obs, np.float32)
    act = PM.actions(state, obs)
    envs, nobs = np.ascontiguousarray(state.T).copy(), obs.copy()
    reward, done, succ = ox.step_batch(envs, act.copy(), nobs, max_step=0, auto_reset=0)
    rows = np.concatenate([obs, act, nobs, reward[:, None], done.astype(np.float32)[:, None]], 1).astype(np.float32)
    assert rows.shape == (obs.shape[0], ROW)
    return rows, succ, np.ascontiguousarray(envs.T)


def initial_ring(rows, success, online_rows):
    """[E0, 32], [E0] -> [E0 + M, 32], [E0 + M]: online row i starts as offline row i mod E0, labels too"""
    rows, success = np.asarray(rows, np.float32), np.asarray(success, np.int8)
    fill = np.arange(online_rows) % rows.shape[0]
    return np.concatenate([rows, rows[fill]]), np.concatenate([success, success[fill]])


class BranchModel:
    def __init__(self, ring, success, offline_rows, online_rows, k, call=0):
        self.ring, self.success = np.array(ring, np.float32), np.array(success, np.int8)
        self.e0, self.m, self.k, self.call = offline_rows, online_rows, k, call
        assert self.ring.shape == (offline_rows + online_rows, ROW) and self.success.shape == (offline_rows + online_rows,)

    def push(self, state, obs):
        """-> [(env, slot)] of the rows that were written"""
        n = obs.shape[0]
        rows, succ, _ = step_once(state, obs)
        wrote = []
        for e, slot in zip(PM.env_picks(self.call, n, self.k), PM.slots(self.call, self.k, self.m, self.e0)):
            if np.isfinite(rows[e]).all():
                self.ring[slot], self.success[slot] = rows[e], succ[e]
                wrote.append((e, slot))
        self.call += 1
        return wrote


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
# env index of each planted edge class (make_inputs plants those that fit into n).  An env's scenario is its index mod 3 (0 straight_line,
# 1 serpentine, 2 circular): serp_phase stands on a serpentine env, circ_phase on a circular one.
CLASSES = {"fire_good": 4, "fire_nolock": 5, "fire_empty": 6, "missile_hit": 7, "alt_low": 8, "alt_high": 9, "band_low": 10, "band_high": 11,
           "nan_state": 12, "serp_phase": 13, "circ_phase": 14, "inf_obs": 15}
assert CLASSES["serp_phase"] % 3 == 1 and CLASSES["circ_phase"] % 3 == 2


def _flags(state, i, set_=0, clear=0):
    f = state[FLAGS].view(np.uint32)
    f[i] = (int(f[i]) | set_) & ~clear & 0xFFFFFFFF


def make_inputs(n, seed=0, special=True, warm=30):
    """-> state [37, n] fp32 (flags / counters bit-cast), obs [n, 13] fp32: n envs of the three scenarios in turn, randomly reset and flown `warm` steps
    under the pilot by the oracle, then the edge classes of CLASSES planted on single envs (where n allows) by editing state words and the STORED
    observation's lock / rail entries (the pilot fires on what the learner saw, the env answers with the latches it holds)."""
    envs, obs = ox.reset_batch(n, np.arange(n) % 3, 1, seed=1000 * seed + n)
    for _ in range(warm):
        ox.step_batch(envs, PM.actions(np.ascontiguousarray(envs.T), obs), obs)
    state = np.ascontiguousarray(envs.T)
    assert np.isfinite(state[:FLAGS]).all() and np.isfinite(obs).all()
    if not special:
        return state, obs
    C = {k: v for k, v in CLASSES.items() if v < n}
    for name in ("fire_good", "fire_nolock", "fire_empty"):
        if name in C:
            obs[C[name], 7], obs[C[name], 8] = 1.0, 1.0  # the pilot fires
    if "fire_good" in C:  # lock held, missile on the rail: step_success +1 (and the missile leaves)
        _flags(state, C["fire_good"], ox.F_LOCKED | ox.F_SLOT | ox.F_SIM_SLOT)
        state[LOCK_TIMER, C["fire_good"]] = 2.0
    if "fire_nolock" in C:  # no lock, missile on the rail: -1
        _flags(state, C["fire_nolock"], ox.F_SLOT | ox.F_SIM_SLOT, ox.F_LOCKED)
        state[LOCK_TIMER, C["fire_nolock"]] = 0.0
    if "fire_empty" in C:  # lock held, empty rail: 0, and the 8 points are still paid
        _flags(state, C["fire_empty"], ox.F_LOCKED, ox.F_SLOT | ox.F_SIM_SLOT)
    if "missile_hit" in C:  # a guided missile 10 m behind the opponent at the opponent's velocity, launched under a lock: hits on this step
        i = C["missile_hit"]
        _flags(state, i, ox.F_M_ACTIVE | ox.F_M_GUIDED | ox.F_FIRE_SUCCESS, ox.F_SLOT | ox.F_SIM_SLOT)
        state[MIS_P:MIS_P + 3, i] = state[OPP_P:OPP_P + 3, i] - np.float32(10.0) * state[OPP_V:OPP_V + 3, i] / np.linalg.norm(state[OPP_V:OPP_V + 3, i])
        state[MIS_V:MIS_V + 3, i] = state[OPP_V:OPP_V + 3, i]
        state[MIS_AGE, i], state[HEALTH, i] = 1.0, 0.2
        obs[i, 8] = -1.0  # (the rail is empty: the pilot does not fire)
    for name, y in (("alt_low", 400.0), ("alt_high", 10500.0), ("band_low", 1500.0), ("band_high", 7500.0)):
        if name in C:
            state[ALLY_P + 1, C[name]] = y
    if "nan_state" in C:
        state[ALLY_P, C["nan_state"]] = np.nan
    if "inf_obs" in C:
        obs[C["inf_obs"], 3] = np.inf
    cnt = state[COUNTERS].view(np.uint32)
    if "serp_phase" in C:  # first leg (250 ticks) at its last tick: the yaw command changes sign on this step
        _flags(state, C["serp_phase"], 0, ox.F_SERP_LONG)
        cnt[C["serp_phase"]] = (int(cnt[C["serp_phase"]]) & 0xFFFF) | (249 << 16)
    if "circ_phase" in C:  # tick 100 of the circle: the pitch command goes from -0.02 to -0.01 on this step
        cnt[C["circ_phase"]] = (int(cnt[C["circ_phase"]]) & 0xFFFF) | (99 << 16)
    return state, obs


def make_offline(rows, seed=0):
    """offline labelled expert rows [rows, 32] (uniform words, fire and done as +-1 / 0-1) and their step_success labels [rows]"""
    rng = np.random.default_rng(177 + seed)
    t = rng.uniform(-1, 1, (rows, ROW)).astype(np.float32)
    t[:, OBS + ACT - 1] = rng.choice([-1.0, 1.0], rows)
    t[:, ROW - 1] = rng.choice([0.0, 1.0], rows)
    return t, rng.choice([-1, 0, 1], rows).astype(np.int8)
