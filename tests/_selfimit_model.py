"""Self-imitation on the CPU (include/hirl4ucav.h "Self-imitation"; hx_self_push / hx_self_reset, hx_selfimit.hip): the rule in numpy, one call at a
time, rows kept as bit patterns (uint32), so every comparison against the device is bit equality.  The model keeps an episode as a per-env list of
steps — it knows nothing of the device's tape, whose layout is the kernel's business — and the ring / success bytes / BC table / cursor / counters as
the header states them.  make_stream builds the seeded synthetic input streams the CPU and the GPU tests share."""
import numpy as np

OBS, ACT, ROW = 13, 4, 32
KILLS, EPISODES, ROWS, DROPPED = range(4)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def finite_bits(w):
    return (np.asarray(w, np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def make_offline(e0, seed=11):
    """e0 offline rows (bit patterns of ordinary floats) and labels"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((e0, ROW)).astype(np.float32), rng.choice([-1, 0, 1], e0).astype(np.int8)


def initial_ring(off, lab, m):
    """[E0 + M][32] float32 and labels: the offline rows, then their cyclic copy (BranchExpert's initial fill)"""
    idx = np.arange(m) % off.shape[0]
    return np.concatenate([off, off[idx]]), np.concatenate([lab, lab[idx]])


class SelfModel:
    """ring: float32 [E0 + M, 32] (copied, kept as uint32), success int8 [E0 + M]; bc: None or float32 [B0 + M, 32]"""

    def __init__(self, ring, success, e0, m, n, L, obs0, ctr0, bc=None, bc_e0=0, cursor=0, call=0):
        assert 1 <= L <= m and ring.shape == (e0 + m, ROW)
        self.ring, self.success = u32(ring).copy(), np.array(success, np.int8)
        self.bc = None if bc is None else u32(bc).copy()
        self.e0, self.m, self.n, self.L, self.bc_e0, self.cursor, self.call = e0, m, n, L, bc_e0, int(cursor), int(call)
        self.counters = [0, 0, 0, 0]
        self.events = {k: 0 for k in ("kill_short", "kill_full", "kill_long", "kill_first", "done_no_kill", "trunc", "same_group", "other_group", "drop_calls",
                                      "wraps", "nonfinite_rows", "calls")}
        self.reset(obs0, ctr0)

    def reset(self, obs, ctr):
        self.steps = [[] for _ in range(self.n)]   # per env: (s bits [13], a bits [4], r bits, step_success), at most L of them
        self.true_len = np.zeros(self.n, np.int64)  # the episode's executed steps, uncapped (the case counters only)
        self.obs_prev, self.last_ctr = u32(obs).copy().reshape(self.n, OBS), np.array(ctr, np.uint32)

    def push(self, obs_new, actions, reward, done, success, ctr):
        """-> the call's accepted episodes as [(env, [slots])] in writing order"""
        n, L, m = self.n, self.L, self.m
        ob, ac, rw = u32(obs_new).reshape(n, OBS), u32(actions).reshape(n, ACT), np.ascontiguousarray(reward, np.float32)
        ctr = np.asarray(ctr, np.uint32)
        kill_eps = []  # (env, rows) in env order
        for e in range(n):
            dn = bool(done[e])
            if ctr[e] != self.last_ctr[e] and not dn:
                self.steps[e], self.true_len[e] = [], 0
                self.events["trunc"] += 1
            else:
                self.steps[e].append((self.obs_prev[e].copy(), ac[e].copy(), rw[e:e + 1].view(np.uint32)[0], np.int8(success[e])))
                self.steps[e] = self.steps[e][-L:]
                self.true_len[e] += 1
                if dn:
                    if rw[e] > np.float32(0):
                        t = int(self.true_len[e])
                        self.events["kill_short" if t < L else "kill_full" if t == L else "kill_long"] += 1
                        self.events["kill_first"] += t == 1
                        st = self.steps[e]
                        rows = np.zeros((len(st), ROW), np.uint32)
                        for j, (s, a, r, _) in enumerate(st):
                            rows[j, 0:13], rows[j, 13:17], rows[j, 30] = s, a, r
                            rows[j, 17:30] = st[j + 1][0] if j + 1 < len(st) else ob[e]
                            rows[j, 31] = np.float32(1.0 if j + 1 == len(st) else 0.0).view(np.uint32)
                        kill_eps.append((e, rows, np.array([b for *_, b in st], np.int8)))
                    else:
                        self.events["done_no_kill"] += 1
                    self.steps[e], self.true_len[e] = [], 0
            self.obs_prev[e], self.last_ctr[e] = ob[e], ctr[e]
        groups = [e // 64 for e, _, _ in kill_eps]
        self.events["same_group"] += len(groups) != len(set(groups))
        self.events["other_group"] += len(set(groups)) > 1
        self.counters[KILLS] += len(kill_eps)
        prefix, k, out, dropped = 0, 0, [], 0
        for e, rows, succ in kill_eps:
            prefix += rows.shape[0]
            if prefix > m:
                dropped += 1
                continue
            assert dropped == 0, "accepted episodes form a leading run"
            slots = []
            for j in range(rows.shape[0]):
                o = (self.cursor + k) % m  # exact arithmetic: the cursor is stored mod 2^64, the sum is not reduced before the mod
                k += 1
                slots.append(self.e0 + o)
                if finite_bits(rows[j]).all():
                    self.ring[self.e0 + o], self.success[self.e0 + o] = rows[j], succ[j]
                    if self.bc is not None:
                        self.bc[self.bc_e0 + o, :17], self.bc[self.bc_e0 + o, 17:] = rows[j, :17], 0
                    self.counters[ROWS] += 1
                else:
                    self.events["nonfinite_rows"] += 1
            out.append((e, slots))
        self.counters[EPISODES] += len(out)
        self.counters[DROPPED] += dropped
        self.events["drop_calls"] += dropped > 0
        self.events["wraps"] += (self.cursor % m) + k >= m and k > 0
        self.cursor = (self.cursor + k) % (1 << 64)
        self.call += 1
        self.events["calls"] += 1
        return out


def make_stream(n, L, calls, seed, mass_kill=(20, 41)):
    """-> (obs0, ctr0, [(obs_new, actions, reward, done, success, episode_ctr)] * calls): every env flies episodes of 1 .. 2 L + 2 steps that end in a
    kill (done, reward near +600), a plain done (reward <= 0) or the time limit (episode_ctr moves without done); at the calls of `mass_kill` EVERY env
    ends in a kill at once; a few words are NaN / Inf.  Arrays are fresh per call (nothing aliases)."""
    rng = np.random.default_rng(seed)
    obs0, ctr = rng.standard_normal((n, OBS)).astype(np.float32), rng.integers(0, 5, n).astype(np.uint32)
    ctr0, left = ctr.copy(), rng.integers(1, 2 * L + 3, n)
    kind = rng.integers(0, 3, n)  # 0 kill, 1 done without a kill, 2 time limit
    out = []
    for c in range(calls):
        obs = rng.standard_normal((n, OBS)).astype(np.float32)
        act = rng.uniform(-1, 1, (n, ACT)).astype(np.float32)
        rew = (-rng.random(n) * 30).astype(np.float32)
        rew[rng.random(n) < 0.1] = 0.0
        done, succ = np.zeros(n, np.uint8), rng.choice([-1, 0, 1], n).astype(np.int8)
        left -= 1
        ends = left <= 0
        if c in mass_kill:
            ends[:], kind[:] = True, 0
        for e in np.nonzero(ends)[0]:
            ctr[e] += 1
            if kind[e] == 0:
                done[e], rew[e] = 1, np.float32(600.0) + rew[e]
            elif kind[e] == 1:
                done[e] = 1
            left[e], kind[e] = rng.integers(1, 2 * L + 3), rng.integers(0, 3)
        bad = rng.random(n) < 0.04
        act[bad, rng.integers(0, ACT)] = np.nan
        obs[rng.random(n) < 0.02, rng.integers(0, OBS)] = np.inf
        out.append((obs, act, rew, done, succ, ctr.copy()))
    return obs0, ctr0, out
