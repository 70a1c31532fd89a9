"""The rule of hx_epstat_push (include/hirl4ucav.h "Episode statistics") in numpy, with the kernel's reduction order; the seeded input stream the
CPU and GPU tests share; and the same statistics from a plain per-env loop written like the reference's training loop (train_all.py:341-387), in
float64.  No GPU, no product import."""
import numpy as np

BINS, SUMS, SLOT = 4, 8, 36
COUNT, N_DONE, N_TIME_LIMIT, SUM_LEN, SUM_RET, SUM_RET_SQ, FIRE_GOOD, FIRE_BAD = range(8)
MAX_STEP = 7  # the stream's time limit


class EpStatModel:
    """Per env: acc (fp32), len, last_ctr.  Per workgroup of 64 envs a slot of 4 bins x 8 float64 sums and 4 x (min, max) fp32.  A call's
    contribution to a word is formed first — c = 0, then the workgroup's lanes 0..63 in order, each into its own bin — and then added to the word."""

    def __init__(self, n):
        self.n, self.groups = n, (n + 63) // 64
        self.acc = np.zeros(n, np.float32)
        self.len = np.zeros(n, np.uint32)
        self.last_ctr = np.zeros(n, np.uint32)
        self.clear()

    def clear(self):
        self.sums = np.zeros((self.groups, BINS, SUMS), np.float64)
        self.min = np.full((self.groups, BINS), np.inf, np.float32)
        self.max = np.full((self.groups, BINS), -np.inf, np.float32)

    def reset(self, ctr):
        self.clear()
        self.acc[:] = 0
        self.len[:] = 0
        self.last_ctr[:] = ctr

    def push(self, flags, reward, done, success, ctr):
        n, G = self.n, self.groups
        done = np.asarray(done) != 0
        ctr = np.asarray(ctr).astype(np.uint32)
        bins = ((np.asarray(flags, np.uint32) >> np.uint32(8)) & np.uint32(3)).astype(np.int64)
        trunc = (ctr != self.last_ctr) & ~done
        ret = np.where(trunc, self.acc, (self.acc + np.asarray(reward, np.float32)).astype(np.float32)).astype(np.float32)
        length = np.where(trunc, self.len, self.len + np.uint32(1)).astype(np.uint32)
        leaves = trunc | done
        self.acc = np.where(leaves, np.float32(0), ret).astype(np.float32)
        self.len = np.where(leaves, np.uint32(0), length).astype(np.uint32)
        self.last_ctr = ctr.copy()
        dret = ret.astype(np.float64)
        vals = np.zeros((G * 64, SUMS), np.float64)  # (lanes behind the last env: bin 0, zeros, +inf / -inf)
        vals[:n, COUNT] = leaves
        vals[:n, N_DONE] = leaves & done
        vals[:n, N_TIME_LIMIT] = leaves & ~done
        vals[:n, SUM_LEN] = np.where(leaves, length, 0)
        vals[:n, SUM_RET] = np.where(leaves, dret, 0.0)
        vals[:n, SUM_RET_SQ] = np.where(leaves, dret * dret, 0.0)
        vals[:n, FIRE_GOOD] = np.asarray(success) == 1
        vals[:n, FIRE_BAD] = np.asarray(success) == -1
        lane_bin = np.zeros(G * 64, np.int64)
        lane_bin[:n] = bins
        lane_min = np.full(G * 64, np.inf, np.float32)
        lane_max = np.full(G * 64, -np.inf, np.float32)
        lane_min[:n] = np.where(leaves, ret, np.float32(np.inf))
        lane_max[:n] = np.where(leaves, ret, np.float32(-np.inf))
        vals, lane_bin, lane_min, lane_max = vals.reshape(G, 64, SUMS), lane_bin.reshape(G, 64), lane_min.reshape(G, 64), lane_max.reshape(G, 64)
        g = np.arange(G)
        c = np.zeros((G, BINS, SUMS), np.float64)
        for lane in range(64):
            b = lane_bin[:, lane]
            c[g, b] = c[g, b] + vals[:, lane]
            self.min[g, b] = np.where(lane_min[:, lane] < self.min[g, b], lane_min[:, lane], self.min[g, b])
            self.max[g, b] = np.where(lane_max[:, lane] > self.max[g, b], lane_max[:, lane], self.max[g, b])
        self.sums = self.sums + c

    def part_words(self):
        """the partials as the device holds them: [groups][36] 8-byte words"""
        w = np.zeros((self.groups, SLOT), np.uint64)
        w[:, :BINS * SUMS] = self.sums.reshape(self.groups, -1).view(np.uint64)
        w[:, BINS * SUMS:] = self.min.view(np.uint32).astype(np.uint64) | (self.max.view(np.uint32).astype(np.uint64) << np.uint64(32))
        return w

    def totals(self):
        """(sums [4, 8], min [4], max [4]): the workgroups added in index order, in float64"""
        s = np.zeros((BINS, SUMS), np.float64)
        for k in range(self.groups):
            s = s + self.sums[k]
        return s, self.min.min(0), self.max.max(0)


def scenario_bins(n):
    """the stream's scenario ids: the mixed rule (sorted thirds) — and thirds of every 64 from 64 envs on, so that the first workgroup holds all three"""
    b = np.sort(np.arange(n) % 3)
    if n >= 64:
        b[:64] = np.sort(np.arange(64) % 3)
    return b.astype(np.uint32)


def make_stream(n, calls=40, seed=0):
    """-> (ctr0 [n], [(flags, reward, done, success, ctr, time_limit_step)] per call): what an auto-resetting env leaves behind each acting launch.
    An episode ends by done (p = 0.12) or at its MAX_STEP-th step (the time-limit step; done may be raised ON it); episode_ctr moves at either.
    time_limit_step is the ground truth the reference-style loop reads; the rule itself must find it from ctr and done.  Forced: env 0 raises done at
    calls 2, 3 and 4 (two one-step episodes in a row); the envs of scenario 2 raise no done before call 6 (call 0..5: that bin ends nothing); env
    n - 1 raises done on its first time-limit step."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    bins = scenario_bins(n)
    ctr = rng.integers(0, 5, n).astype(np.uint32)
    ctr0 = ctr.copy()
    t = np.zeros(n, np.int64)
    out = []
    for call in range(calls):
        t += 1
        done = rng.random(n) < 0.12
        if call < 6:
            done[bins == 2] = False
        if n > 1 and call < MAX_STEP:
            done[n - 1] = call == MAX_STEP - 1
        if call in (2, 3, 4):
            done[0] = True
        tl = t == MAX_STEP
        ended = done | tl
        ctr = (ctr + ended).astype(np.uint32)
        t[ended] = 0
        reward = (rng.standard_normal(n) * 3).astype(np.float32)
        success = rng.choice(np.array([-1, 0, 0, 0, 1], np.int8), n)
        flags = (rng.integers(0, 256, n).astype(np.uint32) | (bins << np.uint32(8)) | (rng.integers(0, 32, n).astype(np.uint32) << np.uint32(10)))
        out.append((flags, reward, done.astype(np.uint8), success, ctr.copy(), tl.copy()))
    return ctr0, out


def reference_loop(n, stream):
    """The same statistics from a per-env loop written like the reference's (train_all.py:341-387): totalReward = 0; for step in range(maxStep):
    act, env.step; if step is the last one: break (BEFORE totalReward += reward); totalReward += reward; if done: break — in float64, python lists.
    A done on the last allowed step ends the episode as a done (st_tl's rule in hx_env_block.h).  -> (per-bin dict of lists, fires [4, 2])"""
    bins = scenario_bins(n)
    eps = {b: {"ret": [], "len": [], "done": 0, "time_limit": 0} for b in range(BINS)}
    fires = np.zeros((BINS, 2), np.int64)
    for i in range(n):
        b = int(bins[i])
        total, steps = 0.0, 0
        for flags, reward, done, success, ctr, tl in stream:
            fires[b, 0] += success[i] == 1
            fires[b, 1] += success[i] == -1
            if tl[i] and not done[i]:
                eps[b]["ret"].append(total)
                eps[b]["len"].append(steps)
                eps[b]["time_limit"] += 1
                total, steps = 0.0, 0
                continue
            total += float(reward[i])
            steps += 1
            if done[i]:
                eps[b]["ret"].append(total)
                eps[b]["len"].append(steps)
                eps[b]["done"] += 1
                total, steps = 0.0, 0
    return eps, fires
