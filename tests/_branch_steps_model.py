"""Expert branches of up to H steps on the CPU — the conveyor rule of include/hirl4ucav.h ("Expert branches", hx_pilot_branch_steps): the step is
tests/_branch_model.step_once (the pilot model plus the C oracle's step on a copy), picks and slots are hx_pilot_refresh's (tests/_pilot_model.py),
and this file keeps the bookkeeping: the resident columns, their ages, the three counters per lane, and the workspace's byte image.
"""
import numpy as np

from tests import _branch_model as BM
from tests import _oracle as ox
from tests import _pilot_model as PM

WORDS, OBS, ROW = BM.WORDS, BM.OBS, BM.ROW
BYTES_PER_COLUMN = (WORDS + OBS + 1) * 4 + 3 * 8  # 228


def kpad(k):
    return (k + 63) // 64 * 64


def workspace_bytes(k):
    return kpad(k) * BYTES_PER_COLUMN


def is_kill(stepped_state_column):
    """the comparison wrap_step pays the +600 on, on the state words the step left: health < 0.1f and the fire-success latch"""
    flags = int(np.asarray(stepped_state_column[BM.FLAGS:BM.FLAGS + 1], np.float32).view(np.uint32)[0])
    with np.errstate(invalid="ignore"):
        return bool(np.float32(stepped_state_column[BM.HEALTH]) < np.float32(0.1)) and bool(flags & ox.F_FIRE_SUCCESS)


class StepsModel:
    """ring [E0 + M, 32], success [E0 + M]; k branches of up to H steps.  work: None (zeros) or the uint8 image of the workspace to start from.
    push(state, obs) is one hx_pilot_branch_steps call; `events` collects what the coverage assertions count."""

    def __init__(self, ring, success, offline_rows, online_rows, k, max_steps, call=0, work=None):
        self.ring, self.success = np.array(ring, np.float32), np.array(success, np.int8)
        self.e0, self.m, self.k, self.h, self.call = offline_rows, online_rows, k, max_steps, call
        assert self.ring.shape == (offline_rows + online_rows, ROW) and self.success.shape == (offline_rows + online_rows,)
        assert 1 <= max_steps <= 65535
        self.kpad = kpad(k)
        img = np.zeros(workspace_bytes(k), np.uint8) if work is None else np.array(work, np.uint8)
        assert img.shape == (workspace_bytes(k),)
        kp, w = self.kpad, img.view(np.uint32)
        self.bstate = w[:WORDS * kp].view(np.float32).reshape(WORDS, kp).copy()
        self.bobs = w[WORDS * kp:(WORDS + OBS) * kp].view(np.float32).reshape(OBS, kp).copy()
        self.age = w[(WORDS + OBS) * kp:(WORDS + OBS + 1) * kp].copy()
        self.cnt = img[(WORDS + OBS + 1) * kp * 4:].view(np.uint64).reshape(3, kp).copy()
        self.events = {"rows": 0, "done": 0, "kills": 0, "skips": 0, "cap": 0, "seeds": 0, "max_age": 0}

    def image(self):
        """the workspace as the kernel lays it out: bstate[37][kpad] bobs[13][kpad] age[kpad] counters[3][kpad]"""
        return np.concatenate([self.bstate.view(np.uint8).ravel(), self.bobs.view(np.uint8).ravel(), self.age.view(np.uint8).ravel(),
                               self.cnt.view(np.uint8).ravel()])

    def counters(self):
        return tuple(int(self.cnt[i, :self.k].sum()) for i in range(3))

    def push(self, state, obs):
        """-> [(lane, env or None, slot)] of the rows that were written (env None: a resident step)"""
        state, obs = np.asarray(state, np.float32), np.asarray(obs, np.float32)
        n, k, resident = obs.shape[0], self.k, self.h > 1
        picks, slots = PM.env_picks(self.call, n, k), PM.slots(self.call, k, self.m, self.e0)
        age = self.age[:k].copy() if resident else np.zeros(k, np.uint32)
        src_s, src_o = np.empty((WORDS, k), np.float32), np.empty((k, OBS), np.float32)
        for j in range(k):
            if age[j] == 0:
                src_s[:, j], src_o[j] = state[:, picks[j]], obs[picks[j]]
            else:
                src_s[:, j], src_o[j] = self.bstate[:, j], self.bobs[:, j]
        rows, succ, stepped = BM.step_once(src_s, src_o)
        wrote, ev = [], self.events
        for j in range(k):
            ok = bool(np.isfinite(rows[j]).all())
            done = bool(rows[j, ROW - 1] != 0)
            ev["seeds"] += int(age[j] == 0)
            if ok:
                self.ring[slots[j]], self.success[slots[j]] = rows[j], succ[j]
                wrote.append((j, picks[j] if age[j] == 0 else None, slots[j]))
                kill = done and is_kill(stepped[:, j])
                self.cnt[0, j] += np.uint64(1)
                self.cnt[1, j] += np.uint64(done)
                self.cnt[2, j] += np.uint64(kill)
                ev["rows"] += 1
                ev["done"] += int(done)
                ev["kills"] += int(kill)
            else:
                ev["skips"] += 1
            if resident:
                if ok and not done and int(age[j]) + 1 < self.h:
                    self.bstate[:, j], self.bobs[:, j] = stepped[:, j], rows[j, OBS + BM.ACT:OBS + BM.ACT + OBS]
                    self.age[j] = age[j] + 1
                    ev["max_age"] = max(ev["max_age"], int(self.age[j]))
                else:
                    ev["cap"] += int(ok and not done)
                    self.age[j] = 0
        self.call += 1
        return wrote
