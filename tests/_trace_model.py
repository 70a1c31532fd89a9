"""The episode record's rule (include/hirl4ucav.h "Episode record", hx_trace.hip) restated in numpy, and the seeded synthetic stream the CPU
and GPU tests drive it with.  The score is summed with np.float32 adds in step order."""
import numpy as np

FIELDS, W_ALLY, W_OPPO, W_FLAGS, ENV_WORDS = 8, 0, 13, 35, 37
STREAM_SEED = 2  # chosen on the CPU: test_trace_cpu.py asserts the coverage conditions of this stream


class TraceModel:
    def __init__(self, k, cap_steps, env_ids=None):
        self.k, self.cap = int(k), int(cap_steps)
        self.ids = np.arange(self.k) if env_ids is None else np.asarray(env_ids, np.int64)
        self.log = np.zeros((FIELDS, self.cap, self.k), np.uint32)  # (reset leaves the log as it is)
        self.reset()

    def reset(self):
        k = self.k
        self.total, self.nrec, self.end_step = np.zeros(k, np.float32), np.zeros(k, np.int32), np.full(k, -1, np.int32)
        self.end_flags, self.launches, self.hits = np.zeros(k, np.uint32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        self.alive = k

    def push(self, state, reward, done, success, t):
        """state [37, stride] uint32 words; reward fp32, done u8, success i8 [n]"""
        assert 0 <= t < self.cap
        for j, i in enumerate(self.ids):
            if self.end_step[j] >= 0:
                continue
            flags = np.uint32(state[W_FLAGS, i])
            self.log[0:3, t, j] = state[W_ALLY:W_ALLY + 3, i]
            self.log[3:6, t, j] = state[W_OPPO:W_OPPO + 3, i]
            self.log[6, t, j] = np.float32(reward[i]).view(np.uint32)
            self.log[7, t, j] = (flags & np.uint32(0xFFFF)) | (np.uint32(np.uint8(np.int8(success[i]).view(np.uint8))) << np.uint32(16))
            self.total[j] = np.float32(self.total[j]) + np.float32(reward[i])
            self.nrec[j] = t + 1
            self.launches[j] += success[i] != 0
            self.hits[j] += success[i] == 1
            if done[i] != 0:
                self.end_step[j], self.end_flags[j] = t, flags
                self.alive -= 1

    def summaries(self):
        return {"total": self.total, "nrec": self.nrec, "end_step": self.end_step, "end_flags": self.end_flags, "launches": self.launches,
                "hits": self.hits}


def stream(n=300, stride=320, steps=24, seed=STREAM_SEED):
    """-> dict of per-step arrays: state [steps, 37, stride] uint32 (random bit patterns, NaN payloads among them), reward [steps, n] fp32
    (integer-valued: fp32 and float64 sums agree exactly), done [steps, n] u8 (mostly 0; 1 or 2 when raised, and raised again later),
    success [steps, n] i8 in {-1, 0, 1}"""
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 1 << 32, (steps, ENV_WORDS, stride), dtype=np.uint64).astype(np.uint32)
    state[:, W_ALLY, 0] = np.uint32(0x7FC12345)  # a quiet NaN with a payload, a signalling one and an infinity among the positions
    state[:, W_OPPO + 1, 1] = np.uint32(0x7F800001)
    state[:, W_ALLY + 2, 2] = np.uint32(0xFF800000)
    reward = rng.integers(-20, 21, (steps, n)).astype(np.float32)
    done = np.where(rng.random((steps, n)) < 0.06, rng.integers(1, 3, (steps, n)), 0).astype(np.uint8)
    success = rng.choice(np.array([-1, 0, 1], np.int8), (steps, n), p=[0.15, 0.7, 0.15])
    return {"state": state, "reward": reward, "done": done, "success": success}


def run(model, s, steps=None):
    model.reset()
    for t in range(len(s["reward"]) if steps is None else steps):
        model.push(s["state"][t], s["reward"][t], s["done"][t], s["success"][t], t)
    return model
