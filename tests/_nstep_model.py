"""numpy model of the n-step rule (include/hirl4ucav.h "n-step returns"): the same buffers as hx_nstep_push keeps — win[field][head][env], hc,
obs_prev[13][env], last_ctr — the same fp32 arithmetic in the same order, the same row order (by env, then oldest head first).  Beside the
buffers it keeps, per pending head, the rewards it has taken in, so that a test can hold every emitted row to the float64 sum."""
import numpy as np

FIELDS, F_A, F_ACC, F_BOOT, F_SUCC = 20, 13, 17, 18, 19


class NStepModel:
    def __init__(self, n_envs, n, gamma):
        self.N, self.n, self.gamma = int(n_envs), int(n), np.float32(gamma)
        self.win = np.zeros((FIELDS, self.n, self.N), np.float32)
        self.hc = np.zeros(self.N, np.uint32)
        self.obs_prev = np.zeros((13, self.N), np.float32)
        self.last_ctr = np.zeros(self.N, np.uint32)
        self.total = 0
        self.rewards = [[] for _ in range(self.N)]  # per env: one list of rewards per pending head, oldest first
        self.pushed = 0                             # steps that were not truncated

    def reset(self, obs, episode_ctr):
        self.win[:] = 0
        self.hc[:] = 0
        self.obs_prev[:] = np.asarray(obs, np.float32).reshape(self.N, 13).T
        self.last_ctr[:] = np.asarray(episode_ctr).astype(np.uint32)
        self.rewards = [[] for _ in range(self.N)]

    def pending(self):
        return int((self.hc >> 8).sum())

    def push(self, obs_new, actions, reward, done, success, episode_ctr):
        """-> rows [k, 32] float32, success [k] int8, meta: per row (env, m = steps in the row, its rewards, "trunc" | "done" | "full",
        heads pending before the step)"""
        n, g = self.n, self.gamma
        obs_new = np.asarray(obs_new, np.float32).reshape(self.N, 13)
        actions = np.asarray(actions, np.float32).reshape(self.N, 4)
        reward, ctr = np.asarray(reward, np.float32), np.asarray(episode_ctr).astype(np.uint32)
        rows, succ, meta = [], [], []
        for i in range(self.N):
            dn = bool(done[i])
            trunc = bool(ctr[i] != self.last_ctr[i]) and not dn
            head, count = int(self.hc[i] & 0xff), int(self.hc[i] >> 8)
            before = count
            op = self.obs_prev[:, i].copy()

            def emit(j, s_next, d, kind):
                pos = (head + j) % n
                row = np.zeros(32, np.float32)
                row[0:17], row[17:30], row[30], row[31] = self.win[0:17, pos, i], s_next, self.win[F_ACC, pos, i], d
                rows.append(row)
                succ.append(np.int8(self.win[F_SUCC, pos, i]))
                meta.append((i, len(self.rewards[i][j]), list(self.rewards[i][j]), kind, before))

            if trunc:
                for j in range(count):
                    emit(j, op, np.float32(1.0) - self.win[F_BOOT, (head + j) % n, i], "trunc")
                head = count = 0
                self.rewards[i] = []
            else:
                self.pushed += 1
                pos = (head + count) % n
                self.win[0:13, pos, i], self.win[13:17, pos, i] = op, actions[i]
                self.win[F_ACC, pos, i], self.win[F_BOOT, pos, i], self.win[F_SUCC, pos, i] = 0.0, 0.0, np.float32(success[i])
                self.rewards[i].append([])
                count += 1
                for j in range(count):
                    pos = (head + j) % n
                    age = count - 1 - j
                    w = np.float32(1.0) if age == 0 else np.float32(self.win[F_BOOT, pos, i] * g)
                    self.win[F_ACC, pos, i] = np.float32(self.win[F_ACC, pos, i] + np.float32(w * reward[i]))
                    self.win[F_BOOT, pos, i] = w
                    self.rewards[i][j].append(float(reward[i]))
                if dn:
                    for j in range(count):
                        emit(j, obs_new[i], np.float32(1.0), "done")
                    head = count = 0
                    self.rewards[i] = []
                elif count == n:
                    emit(0, obs_new[i], np.float32(1.0) - self.win[F_BOOT, head, i], "full")
                    head, count = (head + 1) % n, count - 1
                    self.rewards[i].pop(0)
            self.hc[i] = head | (count << 8)
            self.obs_prev[:, i] = obs_new[i]
            self.last_ctr[i] = ctr[i]
        self.total += len(rows)
        return (np.array(rows, np.float32).reshape(-1, 32), np.array(succ, np.int8), meta)


def live_window(win, hc):
    """the pending heads of a window buffer, oldest first: [env][j][field], zeros beyond an env's count (what a popped head leaves behind in
    the buffer is not part of the state)"""
    win, hc = np.asarray(win), np.asarray(hc).astype(np.uint32)
    f, n, N = win.shape
    out = np.zeros((N, n, f), win.dtype)
    for i in range(N):
        head, count = int(hc[i] & 0xff), int(hc[i] >> 8)
        for j in range(count):
            out[i, j] = win[:, (head + j) % n, i]
    return out


def sort_rows(rows, succ):
    """rows with their step_success as one bit pattern per row, sorted: the order-free comparison of what a call wrote"""
    rows = np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 32)).view(np.uint32)
    both = np.concatenate([rows, np.asarray(succ).astype(np.int8).astype(np.uint32).reshape(-1, 1)], 1)
    return both[np.lexsort(both.T[::-1])] if len(both) else both


def make_inputs(n_envs, n, calls, seed=0):
    """seeded synthetic steps for `calls` calls: per call (obs_new, actions, reward, done, success, episode_ctr) as an auto-resetting env would
    leave them — the counter moves on every done and on every time-limit step; rewards are negative, as a pursuit's mostly are (one sign: the
    float64 check of a row's sum is then a relative one).  Episode ends are planted: env e sees nothing end before call a = e % n, so a heads are
    pending there; at call a it is done (blocks of n envs 0, 2, 4, ...) or truncated (blocks 1, 3, ...), and in three blocks of four another end
    follows on the very next step (a done in blocks 0 and 1 of four, a truncation in block 3).  From call a + 2 on, ends are random (6 % each)."""
    rng = np.random.default_rng(1000 * n + n_envs + seed)
    ctr = np.zeros(n_envs, np.uint32)
    obs0 = rng.normal(size=(n_envs, 13)).astype(np.float32)
    steps = []
    for c in range(calls):
        done = rng.random(n_envs) < 0.06
        limit = (rng.random(n_envs) < 0.06) & ~done
        for e in range(n_envs):  # planted ends: with an empty window at call 0, `a` pushes precede the end -> it meets a pending heads
            a = e % n
            if c <= a + 1:
                done[e], limit[e] = False, False
            if c == a:                       # a heads pending: done (even envs) or truncation (odd envs of the next block of n)
                if (e // n) % 2 == 0:
                    done[e] = True
                else:
                    limit[e] = True
            if c == a + 1 and (e // n) % 4 < 2:  # ... and an end on the very next step: a done after a done / a truncation
                done[e] = True
            if c == a + 1 and (e // n) % 4 == 3:
                limit[e] = True
        ctr = ctr + (done | limit).astype(np.uint32)
        steps.append((rng.normal(size=(n_envs, 13)).astype(np.float32), rng.uniform(-1, 1, (n_envs, 4)).astype(np.float32),
                      rng.uniform(-2.0, -0.01, n_envs).astype(np.float32), done.astype(np.uint8), rng.integers(-1, 2, n_envs).astype(np.int8), ctr.copy()))
    return obs0, steps
