"""The scripted pursuit pilot on the device, and an expert table that follows the learner (an extension: the reference's expert is Harfang's IA inside
an external simulator and can only be replayed from recordings).

data/expert_pilot.py pursuit_actions is a closed-form law on state words that already lie in HBM, so it can be asked what it would do in ANY state
the learner reaches.  OnlineExpert does that behind every acting launch (hx_pilot_refresh, hx_pilot.hip): a few envs of the population are
relabelled by the pilot and their (s, a) rows replace the oldest rows of an online region appended to the BC table — dataset aggregation (DAgger), the
standard remedy for a BC term computed on the recordings' state distribution only.  The table keeps its length, so the sampler and every kernel that
reads it are untouched.  The rule is stated in include/hirl4ucav.h ("The pilot as a kernel"); the helpers in front of the classes are host-only.
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
