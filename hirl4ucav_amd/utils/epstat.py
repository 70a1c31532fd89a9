"""Per-episode training statistics, binned by scenario (the reference's totalReward / step of an episode, train_all.py:341-354, 383-385).

The vector loop steps N auto-resetting envs whose episodes end at different steps, so EpisodeStats puts one small launch behind every acting launch
(hx_epstat_push, hx_epstat.hip): it keeps each env's running return and length on the device and, when an episode leaves, adds them to the
statistics of the env's scenario.  read_and_clear() is the one device-to-host copy.  The rule is stated in include/hirl4ucav.h ("Episode
statistics"); the helpers in front of the class are host-only and work on arrays.
"""
import ctypes
import math
from collections import deque

import numpy as np

from .. import _lib

SUM_NAMES = ("count", "n_done", "n_time_limit", "sum_len", "sum_ret", "sum_ret_sq", "fire_good", "fire_bad")
SCENARIO_NAMES = ("straight_line", "serpentine", "circular")  # bin = scenario id (environments.batched.SCENARIOS); bin 3 is never used


# ---- host-only helpers (arrays in, plain values out: unit-tested without a GPU) -------------------------------------------------------
def workspace_layout(n_envs):
    """word offsets (4-byte words) of the workspace's parts -> ({"part": 0, "acc": ..., "len": ..., "last_ctr": ...}, words, workgroups)
    — hx_epstat_workspace_words(n_envs)"""
    groups = (n_envs + 63) // 64
    at = groups * 2 * _lib.EPSTAT_SLOT_WORDS
    return {"part": 0, "acc": at, "len": at + n_envs, "last_ctr": at + 2 * n_envs}, at + 3 * n_envs, groups


def combine_partials(part_words):
    """the partials as copied from the device (4-byte words, [workgroups * 72]) -> (sums [4, 8] float64, min [4], max [4] fp32): the workgroups
    added in index order, in float64"""
    w = np.ascontiguousarray(part_words).view(np.uint64).reshape(-1, _lib.EPSTAT_SLOT_WORDS)
    ns = _lib.EPSTAT_BINS * _lib.EPSTAT_SUMS
    sums = np.zeros(ns, np.float64)
    for row in w[:, :ns].view(np.float64):  # (index order, one add per workgroup: np.sum would add pairwise)
        sums = sums + row
    mm = w[:, ns:]
    mn = (mm & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).min(0)
    mx = (mm >> np.uint64(32)).astype(np.uint32).view(np.float32).max(0)
    return sums.reshape(_lib.EPSTAT_BINS, _lib.EPSTAT_SUMS), mn, mx


def summarize(sums, mn, mx):
    """-> {scenario: {count, done, time_limit, mean, std, min, max, mean_len, sum_ret, sum_len, fire_good, fire_bad}} for the three scenarios;
    std is the population std of the returns, sqrt(E[x^2] - mean^2) clamped at 0; a scenario in which no episode ended has count 0 and NaN means"""
    out = {}
    for b, name in enumerate(SCENARIO_NAMES):
        s = dict(zip(SUM_NAMES, (float(v) for v in sums[b])))
        c = s["count"]
        mean = s["sum_ret"] / c if c else math.nan
        out[name] = {"count": int(c), "done": int(s["n_done"]), "time_limit": int(s["n_time_limit"]), "mean": mean,
                     "std": math.sqrt(max(s["sum_ret_sq"] / c - mean * mean, 0.0)) if c else math.nan,
                     "min": float(mn[b]), "max": float(mx[b]), "mean_len": s["sum_len"] / c if c else math.nan,
                     "sum_ret": s["sum_ret"], "sum_len": s["sum_len"], "fire_good": int(s["fire_good"]), "fire_bad": int(s["fire_bad"])}
    return out


class Last100:
    """Training/Last 100 Episode Average Reward (train_all.py:384) for a vector loop: the count-weighted mean return over the last 100 DRIVER
    episodes, held as (sum of returns, episodes ended) pairs."""

    def __init__(self, pairs=(), window=100):
        self.pairs = deque(((float(s), int(c)) for s, c in pairs), maxlen=window)

    def add(self, sum_ret, count):
        self.pairs.append((float(sum_ret), int(count)))

    def mean(self):
        c = sum(c for _, c in self.pairs)
        return sum(s for s, _ in self.pairs) / c if c else math.nan

    def state(self):
        return [list(p) for p in self.pairs]


# ---- the device side ------------------------------------------------------------------------------------------------------------------------
class EpisodeStats:
    """Statistics of the episodes of a BatchedHarfangEnv that runs WITH auto reset: reset() after env.reset(), push() behind every acting launch.
    Every method but read_and_clear() / state() only enqueues on the current torch stream."""

    def __init__(self, env):
        import torch

        if env.device.type != "cuda":
            raise _lib.HxError("EpisodeStats runs on the GPU only (there is no CPU path in the product)")
        if not env.auto_reset:
            raise ValueError("EpisodeStats: the env was built with auto_reset=False — the rule reads an episode's end off the auto-reset "
                             "(episode_ctr moving); a validation env is recorded by utils.trace.EpisodeRecorder")
        self.env, self.n = env, env.n
        L = _lib.load()  # (checks hx_epstat_sizeof)
        self._off, words, self.groups = workspace_layout(self.n)
        if int(L.hx_epstat_workspace_words(self.n)) != words:
            raise _lib.HxError(f"ABI mismatch: the statistics of {self.n} envs are {words} words here, {L.hx_epstat_workspace_words(self.n)} in {_lib.SO_PATH}")
        self.ws = torch.zeros(words, dtype=torch.int32, device=env.device)
        self.es = epstat_struct(self.ws, self.n)
        self.reset()

    def reset(self):
        _lib.call("hx_epstat_reset", ctypes.byref(self.es), _lib.ptr(self.env.episode_ctr), _lib.stream_ptr())

    def clear(self):
        _lib.call("hx_epstat_clear", ctypes.byref(self.es), _lib.stream_ptr())

    def push(self):
        e = self.env
        _lib.call("hx_epstat_push", ctypes.byref(self.es), _lib.ptr(e.state), e.n, e.pitch, _lib.ptr(e.reward), _lib.ptr(e.done), _lib.ptr(e.success),
                  _lib.ptr(e.episode_ctr), _lib.stream_ptr())

    def read(self):
        """the statistics since the last clear (one device-to-host copy) -> summarize()'s dict"""
        return summarize(*combine_partials(self.ws[:self.groups * 2 * _lib.EPSTAT_SLOT_WORDS].cpu().numpy()))

    def read_and_clear(self):
        out = self.read()
        self.clear()
        return out

    def state(self):
        return {"n": self.n, "ws": self.ws.cpu().clone()}

    def load_state(self, st):
        if st["n"] != self.n or st["ws"].numel() != self.ws.numel():
            raise ValueError(f"snapshot holds the episode statistics of {st['n']} envs, this run has {self.n}")
        self.ws.copy_(st["ws"])


def epstat_struct(ws, n_envs):
    """HxEpStat over the first hx_epstat_workspace_words(n_envs) words of `ws`, a 4-byte device tensor whose storage is 8-byte aligned"""
    off, words, _ = workspace_layout(n_envs)
    if ws.element_size() != 4 or ws.numel() < words or ws.data_ptr() % 8:
        raise ValueError(f"epstat_struct: the workspace is {words} 4-byte words, 8-byte aligned, got {ws.numel()} of {ws.element_size()} bytes")
    base = ws.data_ptr()
    return _lib.HxEpStat(*[base + 4 * off[name] for name in ("part", "acc", "len", "last_ctr")], n_envs)
