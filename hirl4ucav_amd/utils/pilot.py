"""The scripted pursuit pilot on the device, and an expert table that follows the learner (an extension: the reference's expert is Harfang's IA inside
an external simulator and can only be replayed from recordings).

data/expert_pilot.py pursuit_actions is a closed-form law on state words that already lie in HBM, so it can be asked what it would do in ANY state
the learner reaches.  OnlineExpert does that behind every acting launch (hx_pilot_refresh, hx_pilot.hip): a few envs of the population are
relabelled by the pilot and their (s, a) rows replace the oldest rows of an online region appended to the BC table — dataset aggregation (DAgger), the
standard remedy for a BC term computed on the recordings' state distribution only.  The table keeps its length, so the sampler and every kernel that
reads it are untouched.  The rule is stated in include/hirl4ucav.h ("The pilot as a kernel"); the helpers in front of the classes are host-only.

BranchExpert does the same for the LABELLED EXPERT RING, which holds full transitions (s, a, s', r, done) + step_success and is what HIRL's expert rows,
E-SAC's expert rows and ISAC's expert batch are drawn from: behind every acting launch hx_pilot_branch (hx_branch.hip) loads a few envs' whole state
into registers, flies each ONE step under the pilot's noise-free action with the env's own step, and writes that branch over the oldest rows of an
online region appended to the ring.  Nothing is stored back to the env: the learner's trajectory is untouched, and any (s, a, r, s') of the true
dynamics is valid off-policy data.  With steps = H > 1 the branches stay RESIDENT in a device workspace (hx_pilot_branch_steps, hx_branch_steps.hip):
every push() advances each of them one step, and a branch that ends — done, a non-finite row, H steps — is reseeded from the learner's envs, so the
ring also gets the rows in which the pursuit pays off, hundreds of steps behind the state it started from.  The rule is stated in
include/hirl4ucav.h ("Expert branches").
"""
from .. import _lib


# ---- host-only helpers (plain values: unit-tested without a GPU) ----------------------------------------------------------------------------
def online_args_refusal(n_envs, offline_rows, online_rows, per_step):
    """why an online region of `online_rows` rows refreshed `per_step` rows per call cannot be built over `n_envs` envs, or None"""
    if online_rows < 1:
        return f"online_rows {online_rows}: the online region holds at least one row"
    if offline_rows < 1:
        return "the offline table is empty: the online region starts as a copy of its rows"
    if not 1 <= per_step <= min(n_envs, online_rows):
        return f"per_step {per_step}: 1 <= per_step <= min(envs, online_rows) = {min(n_envs, online_rows)} (the picks of a call are distinct envs and distinct slots)"
    return None


def initial_fill_index(offline_rows, online_rows):
    """the offline row online row i starts as: i mod offline_rows (the draw over the whole table then starts as the offline distribution)"""
    return [i % offline_rows for i in range(online_rows)]


def rows_written(call, per_step, online_rows):
    """online slots that have been handed to the pilot at least once after `call` pushes (host arithmetic, no device read)"""
    return min(call * per_step, online_rows)


def device_pilot_actions(env, noise=None, out=None):
    """pursuit_actions(env.state, env.obs) as ONE launch (hx_pilot_act) -> actions [n, 4].  noise: None or a [n, 3] fp32 device tensor that is added
    to the three levels before the clamp (already scaled by its std).  Enqueues on the current torch stream."""
    import torch

    if env.device.type != "cuda":
        raise _lib.HxError("device_pilot_actions runs on the GPU only (data.expert_pilot.pursuit_actions is the torch form)")
    if noise is not None and (noise.dtype != torch.float32 or tuple(noise.shape) != (env.n, 3) or not noise.is_contiguous() or noise.device != env.obs.device):
        raise ValueError(f"device_pilot_actions: noise is a contiguous fp32 [{env.n}, 3] tensor on the env's device")
    if out is None:
        out = torch.empty((env.n, _lib.ACT_DIM), dtype=torch.float32, device=env.obs.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (env.n, _lib.ACT_DIM) or not out.is_contiguous():
        raise ValueError(f"device_pilot_actions: out is a contiguous fp32 [{env.n}, 4] tensor")
    _lib.call("hx_pilot_act", _lib.ptr(env.state), env.n, env.pitch, _lib.ptr(env.obs), _lib.ptr(noise), _lib.ptr(out), _lib.stream_ptr())
    return out


class OnlineExpert:
    """A BC table [E0 + M][32] whose first E0 rows are the offline expert rows (never touched) and whose last M rows are refreshed by the pilot:
    push() behind every acting launch relabels `per_step` envs of `env` (FIFO over the online region).  `table` is what sample() / step_learn() are
    given as bc_table.  push() only enqueues on the current torch stream; state_dict() is the one device-to-host copy.  (Building the table and
    the state round trip are plain tensor code; only push() needs the GPU.)"""

    def __init__(self, env, bc_table_offline, online_rows, per_step):
        import torch

        t = bc_table_offline
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != _lib.ROW_WORDS:
            raise ValueError(f"OnlineExpert: the offline table is fp32 [rows, {_lib.ROW_WORDS}]")
        self.env, self.offline_rows, self.online_rows, self.per_step = env, int(t.shape[0]), int(online_rows), int(per_step)
        why = online_args_refusal(env.n, self.offline_rows, self.online_rows, self.per_step)
        if why:
            raise ValueError("OnlineExpert: " + why)
        fill = torch.tensor(initial_fill_index(self.offline_rows, self.online_rows), dtype=torch.int64, device=t.device)
        self.table = torch.cat([t, t[fill]]).contiguous()
        self.call = 0

    def push(self):
        e = self.env
        if e.device.type != "cuda" or not self.table.is_cuda:
            raise _lib.HxError("OnlineExpert.push runs on the GPU only (there is no CPU path in the product)")
        _lib.call("hx_pilot_refresh", _lib.ptr(e.state), e.n, e.pitch, _lib.ptr(e.obs), _lib.ptr(self.table), self.offline_rows, self.online_rows,
                  self.per_step, self.call, _lib.stream_ptr())
        self.call += 1

    def rows_written(self):
        return rows_written(self.call, self.per_step, self.online_rows)

    def state_dict(self):
        return {"online": self.table[self.offline_rows:].cpu().clone(), "call": self.call, "online_rows": self.online_rows, "per_step": self.per_step,
                "offline_rows": self.offline_rows}

    def load_state_dict(self, st):
        if (st["online_rows"], st["per_step"]) != (self.online_rows, self.per_step):
            raise ValueError(f"snapshot was written under --expert_online {st['online_rows']} --expert_online_per_step {st['per_step']}, this run has "
                             f"--expert_online {self.online_rows} --expert_online_per_step {self.per_step}")
        if st["offline_rows"] != self.offline_rows:
            raise ValueError(f"snapshot's online region stands behind {st['offline_rows']} offline expert rows, this run's table has {self.offline_rows}")
        self.table[self.offline_rows:].copy_(st["online"])
        self.call = int(st["call"])


# ---- expert branches -------------------------------------------------------------------------------------------------------------------------
BRANCH_SLACK = 10  # the labelled expert ring is built 10 rows longer than it is filled (train_all.load_expert_tables): never full, never wrapped


BRANCH_MAX_STEPS = 65535  # hx_pilot_branch_steps' max_steps: the episode counter's range
BRANCH_COLUMN_BYTES = (37 + 13 + 1) * 4 + 3 * 8  # a workspace column: bstate[37] bobs[13] age, three 64-bit counters (include/hirl4ucav.h)


def branch_steps_refusal(steps):
    """why branches of `steps` steps cannot be built, or None"""
    if not 1 <= steps <= BRANCH_MAX_STEPS:
        return f"steps {steps}: 1 (one step per pick) <= steps <= {BRANCH_MAX_STEPS}"
    return None


def branch_counter_sums(counters_host, per_step):
    """the three sums (rows written, rows with done, kills) of a host copy of the workspace's counters (uint8 [24 kpad]: uint64 [3][kpad]) over its
    first per_step lanes"""
    import torch

    cnt = counters_host.contiguous().view(torch.int64).reshape(3, -1)[:, :per_step]
    return tuple(int(v) for v in cnt.sum(1))


def branch_layout_refusal(rows_shape, rows_dtype, success_shape, success_dtype):
    """why (rows, step_success) are not what train_all.label_expert builds and DeviceReplay.store_rows takes — fp32 [E0, 32] rows in the column order
    [s 0..12 | a 13..16 | s' 17..29 | r 30 | done 31], which is the order hx_pilot_branch writes, and int8 [E0] labels —, or None"""
    if str(rows_dtype) != "torch.float32" or len(rows_shape) != 2 or rows_shape[1] != _lib.ROW_WORDS:
        return f"the offline rows are fp32 [rows, {_lib.ROW_WORDS}], got {rows_dtype} {list(rows_shape)}"
    if _lib.OBS_DIM + _lib.ACT_DIM + _lib.OBS_DIM + 2 != _lib.ROW_WORDS:
        return f"a row is s[{_lib.OBS_DIM}] a[{_lib.ACT_DIM}] s'[{_lib.OBS_DIM}] r done = {_lib.ROW_WORDS} words"
    if str(success_dtype) != "torch.int8" or list(success_shape) != [rows_shape[0]]:
        return f"the step_success labels are int8 [{rows_shape[0]}], got {success_dtype} {list(success_shape)}"
    return None


class BranchExpert:
    """The labelled expert ring as a DeviceReplay of capacity E0 + M + 10 (`ring`): its first E0 rows and labels are the offline ones (never touched),
    its last M rows start as their cyclic copy (row E0 + i = row i mod E0, labels too) and are rewritten by the pilot's branches: push() behind every
    acting launch flies `per_step` envs of `env` one step each in registers (FIFO over the online region).  total = E0 + M for good, so every
    sampler and every kernel that reads the ring is untouched, and the draw starts as the offline distribution.  push() only enqueues on the current
    torch stream; state_dict() is the one device-to-host copy.  (Building the ring and the state round trip are plain tensor code; only push()
    needs the GPU.)  steps = 1: that object and nothing else.  steps = H > 1: the per_step branches are resident in `work` (the workspace of
    hx_pilot_branch_steps, zeroed here), push() flies each one step further, counters() reads what they have written."""

    def __init__(self, env, rows_offline, success_offline, online_rows, per_step, device=None, steps=1):
        import torch

        from .buffer import DeviceReplay

        why = branch_layout_refusal(tuple(rows_offline.shape), rows_offline.dtype, tuple(success_offline.shape), success_offline.dtype)
        if why:
            raise ValueError("BranchExpert: " + why)
        self.env, self.offline_rows, self.online_rows, self.per_step = env, int(rows_offline.shape[0]), int(online_rows), int(per_step)
        self.steps = int(steps)
        why = online_args_refusal(env.n, self.offline_rows, self.online_rows, self.per_step) or branch_steps_refusal(self.steps)  # (the BC table's region rule)
        if why:
            raise ValueError("BranchExpert: " + why)
        device = rows_offline.device if device is None else device
        fill = torch.tensor(initial_fill_index(self.offline_rows, self.online_rows), dtype=torch.int64, device=rows_offline.device)
        self.ring = DeviceReplay(self.offline_rows + self.online_rows + BRANCH_SLACK, device)
        self.ring.store_rows(rows_offline, success_offline)
        self.ring.store_rows(rows_offline[fill], success_offline[fill])
        assert self.ring.fixed_len == self.offline_rows + self.online_rows < self.ring.capacity  # (slot = row index: the ring has not wrapped)
        self.call = 0
        self.work = None
        if self.steps > 1:  # every age 0: the first push() seeds every branch
            self.kpad = (self.per_step + 63) // 64 * 64
            self.work = torch.zeros(self.kpad * BRANCH_COLUMN_BYTES, dtype=torch.uint8, device=self.ring.ring.device)

    def push(self):
        e, r = self.env, self.ring
        if e.device.type != "cuda" or not r.ring.is_cuda:
            raise _lib.HxError("BranchExpert.push runs on the GPU only (there is no CPU path in the product)")
        if self.steps == 1:
            _lib.call("hx_pilot_branch", _lib.ptr(e.state), e.n, e.pitch, _lib.ptr(e.obs), _lib.ptr(r.ring), _lib.ptr(r.success), self.offline_rows,
                      self.online_rows, self.per_step, self.call, _lib.stream_ptr())
        else:
            _lib.call("hx_pilot_branch_steps", _lib.ptr(e.state), e.n, e.pitch, _lib.ptr(e.obs), _lib.ptr(r.ring), _lib.ptr(r.success), self.offline_rows,
                      self.online_rows, self.per_step, self.steps, self.call, _lib.ptr(self.work), self.kpad, _lib.stream_ptr())
        self.call += 1

    def counters(self):
        """(rows written, rows with done, kills) of the resident branches since the workspace was zeroed: ONE device-to-host copy"""
        if self.work is None:
            raise _lib.HxError("BranchExpert.counters: one-step branches (steps = 1) keep no counters; rows_written() is host arithmetic")
        return branch_counter_sums(self.work[(BRANCH_COLUMN_BYTES - 24) * self.kpad:].cpu(), self.per_step)

    def rows_written(self):
        return rows_written(self.call, self.per_step, self.online_rows)

    def state_dict(self):
        lo, hi = self.offline_rows, self.offline_rows + self.online_rows
        st = {"online": self.ring.ring[lo:hi].cpu().clone(), "success": self.ring.success[lo:hi].cpu().clone(), "call": self.call,
              "online_rows": self.online_rows, "per_step": self.per_step, "offline_rows": self.offline_rows}
        if self.steps > 1:  # (steps = 1 writes the record it always wrote)
            st["steps"], st["work"] = self.steps, self.work.cpu().clone()
        return st

    def load_state_dict(self, st):
        if (st["online_rows"], st["per_step"]) != (self.online_rows, self.per_step):
            raise ValueError(f"snapshot was written under --expert_branch {st['online_rows']} --expert_branch_per_step {st['per_step']}, this run has "
                             f"--expert_branch {self.online_rows} --expert_branch_per_step {self.per_step}")
        if int(st.get("steps", 1)) != self.steps:
            raise ValueError(f"snapshot was written under --expert_branch_steps {int(st.get('steps', 1))}, this run has --expert_branch_steps {self.steps}")
        if st["offline_rows"] != self.offline_rows:
            raise ValueError(f"snapshot's branch rows stand behind {st['offline_rows']} offline expert rows, this run's ring has {self.offline_rows}")
        lo, hi = self.offline_rows, self.offline_rows + self.online_rows
        self.ring.ring[lo:hi].copy_(st["online"])
        self.ring.success[lo:hi].copy_(st["success"])
        if self.steps > 1:
            self.work.copy_(st["work"])
        self.call = int(st["call"])
