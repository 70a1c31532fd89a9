"""The record of validation episodes (validate() with --plot: train_all.py:22-102, train_sac.py:24-91 of the reference).

The reference collects the last validation episode's track on the host, one get_pos() per step_test.  Here validation steps all its episodes
in one launch and the state stays on the device, so EpisodeRecorder puts one small launch behind every env step (hx_trace_push, hx_trace.hip):
it appends the step of every tracked env whose episode is still running to a device log and latches what the reference reads when it sees
done.  The rule is stated in include/hirl4ucav.h ("Episode record"); the helpers in front of the class are host-only and work on arrays.
"""
import csv
import ctypes
import os

import numpy as np

from .. import _lib
from .plot import plot_3d_trajectories, plot_distance

SUMMARY_NAMES = ("total", "nrec", "end_step", "end_flags", "launches", "hits")
_SUMMARY_DTYPES = (np.float32, np.int32, np.int32, np.uint32, np.int32, np.int32)


# ---- host-only helpers (arrays in, arrays out: unit-tested without a GPU) ---------------------------------------------------------------
def check_env_ids(env_ids, n):
    """-> the tracked env ids as an int32 array (None: all envs, no list), or ValueError: distinct ids in [0, n)."""
    if env_ids is None:
        return None
    ids = np.asarray(env_ids)
    if ids.ndim != 1 or ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"EpisodeRecorder: env_ids is a non-empty list of integer env ids, got {env_ids!r}")
    if ids.min() < 0 or ids.max() >= n:
        raise ValueError(f"EpisodeRecorder: env ids lie in [0, {n}), got {int(ids.min())} .. {int(ids.max())}")
    if np.unique(ids).size != ids.size:
        raise ValueError("EpisodeRecorder: env_ids holds an env twice")
    return ids.astype(np.int32)


def workspace_layout(k, cap_steps):
    """word offsets of the workspace's parts -> ({"log": 0, "total": ..., ..., "alive": ...}, words) — hx_trace_workspace_words(k, cap_steps)"""
    off, at = {"log": 0}, _lib.TRACE_FIELDS * cap_steps * k
    for name in SUMMARY_NAMES:
        off[name] = at
        at += k
    off["alive"] = at
    return off, at + 1


def trace_struct(ws, k, cap_steps):
    """HxTrace over the first hx_trace_workspace_words(k, cap_steps) words of `ws`, a 4-byte device tensor"""
    off, words = workspace_layout(k, cap_steps)
    if ws.element_size() != 4 or ws.numel() < words:
        raise ValueError(f"trace_struct: the workspace is {words} 4-byte words, got {ws.numel()} of {ws.element_size()} bytes")
    base = ws.data_ptr()
    return _lib.HxTrace(*[base + 4 * off[name] for name in ("log",) + SUMMARY_NAMES + ("alive",)], k, cap_steps)


def split_summary(words, k):
    """the 6 k summary words behind the log (uint32) -> dict of the six typed arrays"""
    words = np.ascontiguousarray(words, np.uint32).reshape(len(SUMMARY_NAMES), k)
    return {name: words[i].view(dt).copy() for i, (name, dt) in enumerate(zip(SUMMARY_NAMES, _SUMMARY_DTYPES))}


def summary_masks(end_flags):
    """(kill, fire_success) — env.episode_success / env.fire_success as validate() reads them at the step that raised done"""
    f = np.asarray(end_flags, np.uint32)
    return (f & np.uint32(_lib.F_EPISODE_SUCCESS)) != 0, (f & np.uint32(_lib.F_FIRE_SUCCESS)) != 0


def decode_episode(log):
    """log [8, T] uint32 words of one env -> the lists validate() collects (train_all.py:26-54): positions [T, 3] as float64, the distance in
    float64 from the fp32 positions (environments/HarfangEnv_GYM.py _pull), the reward, and the steps with iffire / locked / beforeaction."""
    log = np.ascontiguousarray(log, np.uint32)
    with np.errstate(invalid="ignore"):  # (a signalling NaN among the words is a test's doing; it converts quietly)
        pos = log[0:6].view(np.float32).astype(np.float64)
    self_pos, oppo_pos = pos[0:3].T.copy(), pos[3:6].T.copy()
    d = self_pos - oppo_pos
    flags = log[7]
    steps = (lambda bit: np.nonzero(flags & np.uint32(bit))[0].tolist())
    return {"self_pos": self_pos, "oppo_pos": oppo_pos, "distance": np.sqrt((d * d).sum(1)), "reward": log[6].view(np.float32).copy(),
            "fire": steps(_lib.F_FIRED), "lock": steps(_lib.F_LOCKED_PREV), "missile": steps(_lib.F_SLOT_PREV),
            "success": ((flags >> np.uint32(16)) & np.uint32(0xFF)).astype(np.uint8).view(np.int8)}


def write_episode_files(ep, plot_dir, tag):
    """The reference's file set for one episode (train_all.py:70-89): trajectories_{tag}.png and distance_{tag}.png in plot_dir, and
    self_pos / oppo_pos (three columns), fire / lock / distance (one column) as {name}{tag}.csv in plot_dir/csv, written with csv.writer."""
    self_pos, oppo_pos = [[float(x) for x in p] for p in ep["self_pos"]], [[float(x) for x in p] for p in ep["oppo_pos"]]
    distance, fire, lock, missile = [float(x) for x in ep["distance"]], list(ep["fire"]), list(ep["lock"]), list(ep["missile"])
    os.makedirs(os.path.join(plot_dir, "csv"), exist_ok=True)
    for name, rows in (("self_pos", self_pos), ("oppo_pos", oppo_pos), ("fire", [[i] for i in fire]), ("lock", [[i] for i in lock]),
                       ("distance", [[x] for x in distance])):
        with open(os.path.join(plot_dir, "csv", f"{name}{tag}.csv"), "w", newline="") as f:
            csv.writer(f).writerows(rows)
    plot_3d_trajectories(self_pos, oppo_pos, fire, lock, plot_dir, f"trajectories_{tag}.png")
    plot_distance(distance, lock, missile, fire, plot_dir, f"distance_{tag}.png")


def validation_recorder(episodes, scenario, seed, if_random, max_steps, device):
    """--plot in the drivers: the env of one batched validation, built and reset as train_all.validate / validate_all.validate_round build theirs, and a
    recorder over its LAST episode — the reference's e == validationEpisodes - 1 (train_all.py:52-54) -> (env, recorder) for their env= / recorder="""
    from ..environments.batched import BatchedHarfangEnv

    env = BatchedHarfangEnv(episodes, scenario=scenario, device=device, seed=seed, auto_reset=False, random_reset=if_random, collect_stats=False)
    env.reset()
    return env, EpisodeRecorder(env, [episodes - 1], max_steps=max_steps)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
class EpisodeRecorder:
    """Records the episodes of `env_ids` (None: every env) of a BatchedHarfangEnv that runs WITHOUT auto reset: reset() when the episodes
    start, push() behind every env.step.  Every method but alive() / summary() / episode() only enqueues on the current torch stream."""

    def __init__(self, env, env_ids=None, max_steps=1500, device=None):
        import torch

        self.env = env
        self.device = torch.device(device) if device is not None else env.device
        if self.device.type != "cuda" or env.device.type != "cuda":
            raise _lib.HxError("EpisodeRecorder runs on the GPU only (there is no CPU path in the product)")
        ids = check_env_ids(env_ids, env.n)
        self.k = env.n if ids is None else int(ids.size)
        self.max_steps = int(max_steps)
        if self.max_steps <= 0:
            raise ValueError(f"EpisodeRecorder: max_steps > 0, got {max_steps}")
        L = _lib.load()
        if L.hx_trace_sizeof() != ctypes.sizeof(_lib.HxTrace):
            raise _lib.HxError(f"ABI mismatch: HxTrace is {ctypes.sizeof(_lib.HxTrace)} bytes here, {L.hx_trace_sizeof()} in {_lib.SO_PATH}")
        self._off, words = workspace_layout(self.k, self.max_steps)
        if int(L.hx_trace_workspace_words(self.k, self.max_steps)) != words:
            raise _lib.HxError(f"ABI mismatch: the record of {self.k} envs x {self.max_steps} steps is {words} words here, "
                               f"{L.hx_trace_workspace_words(self.k, self.max_steps)} in {_lib.SO_PATH}")
        self.ws = torch.zeros(words, dtype=torch.int32, device=self.device)
        self.env_ids = None if ids is None else torch.from_numpy(ids).to(self.device)
        self.tr = trace_struct(self.ws, self.k, self.max_steps)
        self.t = 0
        self.reset()

    def reset(self):
        _lib.call("hx_trace_reset", ctypes.byref(self.tr), _lib.stream_ptr())
        self.t = 0

    def push(self):
        e = self.env
        _lib.call("hx_trace_push", ctypes.byref(self.tr), _lib.ptr(e.state), e.n, e.pitch, _lib.ptr(e.reward), _lib.ptr(e.done), _lib.ptr(e.success),
                  _lib.ptr(self.env_ids), self.t, _lib.stream_ptr())  # (t == max_steps: HxError, nothing launched)
        self.t += 1

    def alive(self):
        """tracked envs whose episode is still running (one word, one synchronisation)"""
        return int(self.ws[self._off["alive"]])

    def summary(self):
        a = self._off["total"]
        out = split_summary(self.ws[a:a + len(SUMMARY_NAMES) * self.k].cpu().numpy().view(np.uint32), self.k)
        out["kill"], out["fire_success"] = summary_masks(out["end_flags"])
        return out

    def episode(self, j):
        """tracked env j's record as the reference's validate() collects it: see decode_episode"""
        if not 0 <= j < self.k:
            raise IndexError(f"EpisodeRecorder.episode: tracked env {j} of {self.k}")
        T = int(self.ws[self._off["nrec"] + j])
        log = self.ws[:_lib.TRACE_FIELDS * self.max_steps * self.k].view(_lib.TRACE_FIELDS, self.max_steps, self.k)
        return decode_episode(log[:, :T, j].contiguous().cpu().numpy().view(np.uint32))

    def write_reference_files(self, plot_dir, tag, j=None):
        """the reference's five CSVs and two figures (write_episode_files) for tracked env j (default: the last one)"""
        write_episode_files(self.episode(self.k - 1 if j is None else j), plot_dir, tag)
