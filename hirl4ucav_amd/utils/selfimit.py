"""Self-imitation: the learner's own kill episodes join the labelled expert ring (an extension after Oh et al. 2018; the reference's expert rows are
recordings and nothing else).

utils/pilot.py widened where expert rows come from three times — relabelled states, one-step branches, resident flights — and every one of those rows is
still the scripted pursuit pilot's action.  SelfExpert keeps what a long run produces on its own: behind every acting launch hx_self_push
(hx_selfimit.hip) records the step of every env on a device tape of the last L steps, and an episode that ends in a kill (done with reward > 0) is
written, oldest step first, as full transitions over the oldest rows of the online region of the labelled expert ring — the region BranchExpert
builds, with the same initial cyclic fill — and optionally as (s, a) rows into the online region of the BC table, OnlineExpert's region.  In HIRL
--type soft the BC weight is the share of rows where the critic prefers the demonstrated action, so self-demonstrations pull on the policy only where
the critic says they are better.  The rule is stated in include/hirl4ucav.h ("Self-imitation"); the helpers in front of the class are host-only.
"""
from .. import _lib
from .pilot import BRANCH_SLACK, branch_layout_refusal, initial_fill_index

SELF_MAX_STEPS, SELF_FIELDS, SELF_COUNTERS = (_lib.DEFINES[k] for k in ("HX_SELF_MAX_STEPS", "HX_SELF_FIELDS", "HX_SELF_COUNTERS"))
COUNTER_NAMES = ("kills", "episodes_written", "rows_written", "episodes_dropped")  # HX_SELF_KILLS .. HX_SELF_DROPPED


# ---- host-only helpers (plain values: unit-tested without a GPU) ----------------------------------------------------------------------------
def self_args_refusal(n_envs, offline_rows, online_rows, steps):
    """why a tape of `steps` steps per env over `n_envs` envs cannot feed an online region of `online_rows` rows, or None"""
    if online_rows < 1:
        return f"online_rows {online_rows}: the online region holds at least one row"
    if offline_rows < 1:
        return "the offline table is empty: the online region starts as a copy of its rows"
    if not 1 <= n_envs < 2 ** 31:
        return f"n_envs {n_envs}: 1 <= n_envs < 2^31"
    if not 1 <= steps <= SELF_MAX_STEPS:
        return f"steps {steps}: 1 <= steps <= {SELF_MAX_STEPS} (the episode counter's range)"
    if steps > online_rows:
        return f"steps {steps} > online_rows {online_rows}: an episode of `steps` rows must fit into the online region"
    if offline_rows + online_rows >= 2 ** 31:
        return f"{offline_rows} + {online_rows} rows: fewer than 2^31 rows in all"
    return None


def tape_bytes(n_envs, steps):
    """bytes of the episode tape: 19 words (s[13] a[4] r step_success) per env and step = 76 L n"""
    return 4 * SELF_FIELDS * int(steps) * int(n_envs)


def workspace_layout(n_envs, steps):
    """word offsets of the workspace's parts as include/hirl4ucav.h states them -> dict name -> (offset, words), and "words": the total
    (== hx_self_workspace_words)"""
    n, L = int(n_envs), int(steps)
    g = (n + 63) // 64
    gp = (g + 1) // 2 * 2
    at, out = 0, {}
    for name, words in (("tape", SELF_FIELDS * L * n), ("obs_prev", _lib.OBS_DIM * n), ("len", n), ("last_ctr", n), ("klen", n), ("wcount", gp), ("wkills", gp)):
        out[name], at = (at, words), at + words
    at = (at + 1) // 2 * 2
    for name, words in (("cursor", 4), ("counters", 2 * SELF_COUNTERS * g)):
        out[name], at = (at, words), at + words
    out["words"], out["groups"] = at, g
    return out


def counter_sums(counters_host):
    """the four sums (kills seen, episodes written, rows written, episodes dropped) of a host copy of the per-group counters (int64 [4 G])"""
    return tuple(int(v) for v in counters_host.reshape(SELF_COUNTERS, -1).sum(1))


class SelfExpert:
    """The labelled expert ring as a DeviceReplay of capacity E0 + M + 10 (`ring`), built exactly as BranchExpert builds it: the first E0 rows and
    labels are the offline ones (never touched), the last M start as their cyclic copy and are rewritten by the learner's own kill episodes.  With
    bc_table_offline the BC table is widened the same way (`table`, what OnlineExpert builds) and takes the same rows as (s, a, zeros).  push(actions)
    behind every acting launch, reset() after env.reset(); both only enqueue on the current torch stream.  counters() is one device-to-host copy.
    (Building the ring and the state round trip are plain tensor code; push() and reset() need the GPU.)"""

    def __init__(self, env, rows_offline, success_offline, online_rows, steps, bc_table_offline=None, device=None):
        import torch

        from .buffer import DeviceReplay

        why = branch_layout_refusal(tuple(rows_offline.shape), rows_offline.dtype, tuple(success_offline.shape), success_offline.dtype)
        if why:
            raise ValueError("SelfExpert: " + why)
        self.env, self.offline_rows, self.online_rows, self.steps = env, int(rows_offline.shape[0]), int(online_rows), int(steps)
        why = self_args_refusal(env.n, self.offline_rows, self.online_rows, self.steps)
        if why:
            raise ValueError("SelfExpert: " + why)
        device = rows_offline.device if device is None else device
        fill = torch.tensor(initial_fill_index(self.offline_rows, self.online_rows), dtype=torch.int64, device=rows_offline.device)
        self.ring = DeviceReplay(self.offline_rows + self.online_rows + BRANCH_SLACK, device)
        self.ring.store_rows(rows_offline, success_offline)
        self.ring.store_rows(rows_offline[fill], success_offline[fill])
        assert self.ring.fixed_len == self.offline_rows + self.online_rows < self.ring.capacity  # (slot = row index: the ring has not wrapped)
        self.table, self.bc_offline_rows = None, 0
        if bc_table_offline is not None:
            t = bc_table_offline
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != _lib.ROW_WORDS or t.shape[0] < 1:
                raise ValueError(f"SelfExpert: the offline BC table is fp32 [rows >= 1, {_lib.ROW_WORDS}]")
            self.bc_offline_rows = int(t.shape[0])
            bfill = torch.tensor(initial_fill_index(self.bc_offline_rows, self.online_rows), dtype=torch.int64, device=t.device)
            self.table = torch.cat([t, t[bfill]]).contiguous()
        self.call = 0
        self.layout = workspace_layout(env.n, self.steps)
        self.work = torch.zeros(self.layout["words"], dtype=torch.int32, device=self.ring.ring.device)  # every len 0, cursor 0, counters 0
        self.checked = False

    def _part(self, name):
        at, words = self.layout[name]
        return self.work[at:at + words]

    def _work(self):
        """the workspace's address; on first use the layout here is held to the library's word count"""
        if not self.checked:
            words = int(_lib.load().hx_self_workspace_words(self.env.n, self.steps))
            if words != self.layout["words"]:
                raise _lib.HxError(f"ABI mismatch: the self-imitation workspace is {self.layout['words']} words here, {words} in {_lib.SO_PATH}")
            self.checked = True
        return self.work.data_ptr()

    def _gpu(self, what):
        if self.env.device.type != "cuda" or not self.ring.ring.is_cuda:
            raise _lib.HxError(f"SelfExpert.{what} runs on the GPU only (there is no CPU path in the product)")

    def reset(self):
        """after env.reset(), and after a snapshot came back: every episode empty, the next step starts from env.obs; cursor and counters stay"""
        self._gpu("reset")
        e = self.env
        _lib.call("hx_self_reset", self._work(), self.layout["words"], e.n, self.steps, _lib.ptr(e.obs), _lib.ptr(e.episode_ctr), _lib.stream_ptr())

    def push_arrays(self, obs_new, actions, reward, done, success, episode_ctr):
        r = self.ring
        _lib.call("hx_self_push", self._work(), self.layout["words"], self.env.n, self.steps, _lib.ptr(obs_new), _lib.ptr(actions), _lib.ptr(reward), _lib.ptr(done), _lib.ptr(success),
                  _lib.ptr(episode_ctr), _lib.ptr(r.ring), _lib.ptr(r.success), self.offline_rows, self.online_rows, _lib.ptr(self.table),
                  self.bc_offline_rows, self.call, _lib.stream_ptr())
        self.call += 1

    def push(self, actions):
        """the step env has just taken with `actions` [n, 4] (fp32, contiguous, on the device), as an acting launch or env.step left it"""
        import torch

        self._gpu("push")
        e = self.env
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.numel() != e.n * _lib.ACT_DIM or not actions.is_cuda:
            raise ValueError("SelfExpert.push: actions are a contiguous fp32 [num_envs, 4] tensor on the device")
        self.push_arrays(e.obs, actions, e.reward, e.done, e.success, e.episode_ctr)

    def cursor(self):
        """the 64-bit cursor as the next call will read it (one device-to-host copy)"""
        import torch

        return int(self._part("cursor").cpu().view(torch.int64)[self.call & 1]) & (2 ** 64 - 1)

    def set_cursor(self, value):
        import torch

        v = int(value) & (2 ** 64 - 1)
        self._part("cursor").view(torch.int64)[self.call & 1] = torch.tensor(v - 2 ** 64 if v >= 2 ** 63 else v, dtype=torch.int64)

    def counters(self):
        """(kills seen, episodes written, rows written, episodes dropped) since the workspace was zeroed: ONE device-to-host copy"""
        import torch

        return counter_sums(self._part("counters").cpu().view(torch.int64))

    def state_dict(self):
        """the online region(s), success bytes, cursor, counters and call — NOT the tape (76 L n bytes do not belong in a snapshot)"""
        lo, hi = self.offline_rows, self.offline_rows + self.online_rows
        st = {"online": self.ring.ring[lo:hi].cpu().clone(), "success": self.ring.success[lo:hi].cpu().clone(), "call": self.call,
              "online_rows": self.online_rows, "steps": self.steps, "offline_rows": self.offline_rows, "bc": self.table is not None,
              "cursor": self.cursor(), "counters": self._part("counters").cpu().clone()}
        if self.table is not None:
            st["bc_online"], st["bc_offline_rows"] = self.table[self.bc_offline_rows:].cpu().clone(), self.bc_offline_rows
        return st

    def load_state_dict(self, st):
        """what state_dict wrote; the caller calls reset() next (every env's len starts at 0: an episode in flight contributes only its steps after
        the resume)"""
        was = (st["online_rows"], st["steps"], bool(st["bc"]))
        if was != (self.online_rows, self.steps, self.table is not None):
            raise ValueError(f"snapshot was written under --expert_self {was[0]} --expert_self_steps {was[1]}{' --expert_self_bc' if was[2] else ''}, this run "
                             f"has --expert_self {self.online_rows} --expert_self_steps {self.steps}{' --expert_self_bc' if self.table is not None else ''}")
        if st["offline_rows"] != self.offline_rows:
            raise ValueError(f"snapshot's self-imitation rows stand behind {st['offline_rows']} offline expert rows, this run's ring has {self.offline_rows}")
        if st["counters"].numel() != self._part("counters").numel():
            raise ValueError(f"snapshot's self-imitation counters cover {st['counters'].numel() // (2 * SELF_COUNTERS)} groups of 64 envs, this run has "
                             f"{self.layout['groups']}")
        lo, hi = self.offline_rows, self.offline_rows + self.online_rows
        self.ring.ring[lo:hi].copy_(st["online"])
        self.ring.success[lo:hi].copy_(st["success"])
        if self.table is not None:
            if st["bc_offline_rows"] != self.bc_offline_rows:
                raise ValueError(f"snapshot's self-imitation BC rows stand behind {st['bc_offline_rows']} offline rows, this run's table has {self.bc_offline_rows}")
            self.table[self.bc_offline_rows:].copy_(st["bc_online"])
        self.call = int(st["call"])
        self._part("counters").copy_(st["counters"])
        self.set_cursor(st["cursor"])
