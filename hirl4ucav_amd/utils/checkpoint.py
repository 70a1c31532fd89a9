"""Whole-run snapshots for true resume.

The reference only writes the four network state_dicts (HIRL.py:336-350), so a restarted run loses the Adam moments,
the replay contents, the update counters and the episode progress.  A snapshot here holds everything the next vector
step reads: the engine arena (all networks, gradients, Adam moments, soft weight), the engine's call counters (they key
the Philox streams of the sampler and of the exploration noise), the env state words + episode counters + statistics,
the filled part of the replay ring, the host RNGs, and the driver's own scalars.  A run resumed from a snapshot
continues bit-identically to the run that was never stopped (tests/test_facade_gpu.py).
"""
import os
import random

import numpy as np
import torch

from ..agents import engine as E

ENGINE_COUNTERS = ("critic_step", "actor_step", "update_count", "actor_trainable", "sample_calls", "act_calls", "learning_steps")


def engine_state(eng):
    st = {"arena": eng.arena.detach().cpu().clone(), "counters": {k: getattr(eng, k) for k in ENGINE_COUNTERS if hasattr(eng, k)}}
    if hasattr(eng, "acting_format"):
        st["acting_format"] = eng.acting_format()  # the run's arithmetic is part of its state (train_all.py: --dtype; here: what the flag does not say)
    if getattr(eng, "imitative", False):  # SAC's imitative branch only (a plain SAC snapshot stays as it was): the frozen BC actor and the expert-draw counter
        st["imitative"] = {"bc_actor": eng.bc_actor.detach().cpu().clone(), "bc_slope": eng.bc_slope, "expert_calls": eng.expert_calls}
    if getattr(eng, "prioritized", None) is not None:  # (a plain snapshot carries no such key)
        st["prioritized"] = True
        if hasattr(eng, "per_calls"):  # (HirlEngine: the call word of its prioritized draws keys their Philox stream)
            st["per_calls"] = eng.per_calls
        if getattr(eng, "per_new_rows", "max") != "max":  # (a snapshot of a run whose new rows enter at pmax stays as it was)
            st["per_new_rows"] = eng.per_new_rows
    if getattr(eng, "grad_clip", None) is not None:  # (a snapshot of an unclipped run with entropy tuning carries neither key)
        st["grad_clip"] = float(eng.grad_clip)
    if not getattr(eng, "entropy_tuning", True):
        st["fixed_alpha"] = float(eng.ent_coef)
    if getattr(eng, "multi_step", None) is not None:  # (a one-step snapshot carries no such key) the n-step inserter's windows, obs_prev and counters
        st["multi_step"] = eng.multi_step.state()
    if upsample_flags(eng) != (False, False):  # (a snapshot of a run without the two switches carries no such key)
        st["upsample"] = {"buffer": eng.upsampler.state() if eng.upsampler is not None else None, "expert": eng.fire_idx is not None,
                          "calls": eng.upsample_calls}
    return st


def upsample_flags(eng):
    """(buffer_upsample, expert_upsample) as the engine runs them (HirlEngine.set_upsample)"""
    return getattr(eng, "upsampler", None) is not None, getattr(eng, "fire_idx", None) is not None


def check_upsample(eng, st):
    ups = st.get("upsample")
    was = (ups["buffer"] is not None, bool(ups["expert"])) if ups else (False, False)
    now = upsample_flags(eng)
    for name, w, n in (("--buffer_upsample", was[0], now[0]), ("--expert_upsample", was[1], now[1])):
        if w != n:
            raise ValueError(f"snapshot was written {'under' if w else 'without'} {name}, this run is {'under' if n else 'without'} it: resume with the "
                             "flags the run was started with")
    if was[0] and int(ups["buffer"]["boost"]) != eng.upsampler.boost:
        raise ValueError(f"snapshot was written under --upsample_boost {ups['buffer']['boost']}, this run has --upsample_boost {eng.upsampler.boost}: "
                         "resume with the value the run was started with")


def load_engine_state(eng, st):
    if st["arena"].numel() != eng.arena.numel():
        raise ValueError(f"snapshot arena has {st['arena'].numel()} words, this engine {eng.arena.numel()} (different agent or batch size)")
    was, now = st.get("acting_format"), (eng.acting_format() if hasattr(eng, "acting_format") else None)
    if now is not None and was != now:
        import warnings

        # (a snapshot from before round 6 carries no format: round 5's default, or round 4's x9_rows = 16,384 with nine terms — it cannot tell)
        warnings.warn(f"snapshot was written under acting format {was if was is not None else 'unrecorded (a round <= 5 snapshot)'}, this engine "
                      f"acts under {now}: the run continues under other acting arithmetic (fp32 results up to summation order)", stacklevel=2)
    if bool(st.get("prioritized", False)) != (getattr(eng, "prioritized", None) is not None):
        raise ValueError(f"snapshot and engine disagree about prioritized replay ({getattr(eng, 'per_flag', '--per')}): resume with the flag the run was "
                         "started with")
    if st.get("per_new_rows", "max") != getattr(eng, "per_new_rows", "max"):
        raise ValueError(f"snapshot was written under --per_new {st.get('per_new_rows', 'max')}, this engine runs under --per_new "
                         f"{getattr(eng, 'per_new_rows', 'max')}: resume with the flag the run was started with")
    if st.get("grad_clip") != getattr(eng, "grad_clip", None):
        flag = getattr(eng, "grad_clip_flag", "--grad_clip")  # (HirlEngine: --hirl_grad_clip)
        raise ValueError(f"snapshot was written under {flag} {st.get('grad_clip')}, this engine clips at {getattr(eng, 'grad_clip', None)}: "
                         "resume with the flag the run was started with")
    now_fixed = None if getattr(eng, "entropy_tuning", True) else float(eng.ent_coef)
    if st.get("fixed_alpha") != now_fixed:
        raise ValueError(f"snapshot was written under --fixed_alpha {st.get('fixed_alpha')}, this engine runs under {now_fixed} (None: entropy tuning): "
                         "resume with the flag the run was started with")
    was_n = st["multi_step"]["n"] if "multi_step" in st else 1
    now_n = eng.multi_step.n if getattr(eng, "multi_step", None) is not None else 1
    if was_n != now_n or ("multi_step" in st) != (getattr(eng, "multi_step", None) is not None):
        flag = getattr(eng, "multi_step_flag", "--multi_step")  # (HirlEngine: --hirl_multi_step)
        raise ValueError(f"snapshot was written under {flag} {was_n}, this engine runs under {flag} {now_n}: resume with the flag the run was "
                         "started with")
    if ("imitative" in st) != bool(getattr(eng, "imitative", False)):
        raise ValueError("snapshot and engine disagree about SAC's imitative branch (--type ISAC): resume with the type the run was started with")
    check_upsample(eng, st)
    eng.arena.copy_(st["arena"])
    if "per_calls" in st:
        eng.per_calls = st["per_calls"]
    if "upsample" in st:
        eng.upsample_calls = st["upsample"]["calls"]
    if "multi_step" in st:
        eng.multi_step.load_state(st["multi_step"])
    if "imitative" in st:
        eng.bc_actor.copy_(st["imitative"]["bc_actor"])
        eng.expert_calls = st["imitative"]["expert_calls"]
    if hasattr(eng, "needs_reload"):
        eng.needs_reload = False  # host counters and device state agree again from here
    if hasattr(eng, "front_reset"):
        eng.front_reset()
    if hasattr(eng, "refresh_bf16"):
        eng.refresh_bf16()  # the bf16 image of the actor's W2 follows the restored fp32 parameters
    for k, v in st["counters"].items():
        setattr(eng, k, v)


def replay_state(replay):
    n = min(int(replay.total.item()), replay.capacity)
    st = {"capacity": replay.capacity, "total": int(replay.total.item()), "ring": replay.ring[:n].cpu().clone(),
          "success": replay.success[:n].cpu().clone()}
    if hasattr(replay, "prio"):  # a prioritized replay only (a plain snapshot stays as it was): the block sums are recomputed on load
        st["per"] = {"prio": replay.prio[:n].cpu().clone(), "pmax": replay.pmax_t.cpu().clone(), "marked": replay.marked, "beta": replay.beta,
                     "alpha": replay.alpha, "beta_annealing": replay.beta_annealing}
        if replay.score_calls:  # (score_new was never called: the snapshot stays as it was)
            st["per"]["score_calls"], st["per"]["score_chunk"] = replay.score_calls, replay.score_chunk  # (a row's score depends on the chunk)
    return st


def load_replay_state(replay, st):
    if st["capacity"] != replay.capacity:
        raise ValueError(f"snapshot replay capacity {st['capacity']} != {replay.capacity}")
    if ("per" in st) != hasattr(replay, "prio"):
        raise ValueError("snapshot and replay disagree about prioritized replay (--per): resume with the flag the run was started with")
    n = st["ring"].shape[0]
    replay.ring[:n].copy_(st["ring"])
    replay.success[:n].copy_(st["success"])
    replay.total.fill_(st["total"])
    if "per" in st:
        replay.prio.zero_()
        replay.prio[:n].copy_(st["per"]["prio"])
        replay.pmax_t.copy_(st["per"]["pmax"])
        replay.marked_t.fill_(st["per"]["marked"])
        replay.beta = st["per"]["beta"]
        replay.score_calls = st["per"].get("score_calls", 0)
        replay.score_chunk = st["per"].get("score_chunk", replay.score_chunk)
        replay.resum()


def env_state(env):
    return {"state": env.state.cpu().clone(), "obs": env.obs.cpu().clone(), "episode_ctr": env.episode_ctr.cpu().clone(),
            "stats": None if env.stats is None else env.stats.cpu().clone()}


def load_env_state(env, st):
    if tuple(st["state"].shape) != tuple(env.state.shape):
        raise ValueError(f"snapshot holds {st['state'].shape[1]} envs, this run {env.n}")
    env.state.copy_(st["state"])
    env.obs.copy_(st["obs"])
    env.episode_ctr.copy_(st["episode_ctr"])
    if env.stats is not None and st["stats"] is not None:
        if tuple(st["stats"].shape) == tuple(env.stats.shape):
            env.stats.copy_(st["stats"])
        else:  # a snapshot from before the counters were kept HX_STAT_WAYS times (and possibly with fewer statistics): its totals go into way 0
            old = st["stats"].reshape(-1)
            k = min(env.stats.shape[1], old.numel())
            env.stats.zero_()
            env.stats[0, :k].copy_(old[:k])


def save_run(path, eng, env, replay, driver):
    """Written to a temporary file and renamed: a kill during the ~130 MB write leaves the previous snapshot intact."""
    torch.cuda.synchronize()
    tmp = path + ".tmp"
    torch.save({"engine": engine_state(eng), "env": env_state(env), "replay": replay_state(replay), "driver": dict(driver),
                "rng": {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state(),
                        "torch_cuda": torch.cuda.get_rng_state(env.device)}}, tmp)
    os.replace(tmp, path)


def read_run(path):
    """the snapshot as stored (its driver dict carries the run's seed: the caller needs it BEFORE it builds the env)"""
    return torch.load(path, map_location="cpu", weights_only=False)


def load_run(path, eng, env, replay):
    snap = path if isinstance(path, dict) else read_run(path)
    load_engine_state(eng, snap["engine"])
    load_env_state(env, snap["env"])
    load_replay_state(replay, snap["replay"])
    if getattr(eng, "upsampler", None) is not None:  # the counts are formed again from the restored labels
        eng.upsampler.load_state(snap["engine"]["upsample"]["buffer"])
    random.setstate(snap["rng"]["python"])
    np.random.set_state(snap["rng"]["numpy"])
    torch.set_rng_state(snap["rng"]["torch"])
    torch.cuda.set_rng_state(snap["rng"]["torch_cuda"], env.device)
    return snap["driver"]


# ---- the reference's four network files (Agent.saveCheckpoints / loadCheckpoints, HIRL.py:336-350): <dir>/<tag><name>Harfang_GYM ----
HIRL_NETS = (("Critic_", "critic", E.CRITIC_LAYOUT, E.CRITIC_SIZE), ("Actor_", "actor", E.ACTOR_LAYOUT, E.ACTOR_SIZE),  # (name, attribute, layout, size)
             ("TargetCritic_", "target_critic", E.CRITIC_LAYOUT, E.CRITIC_SIZE), ("TargetActor_", "target_actor", E.ACTOR_LAYOUT, E.ACTOR_SIZE))
ALL_NETS = tuple(net[0] for net in HIRL_NETS)


def save_hirl_nets(eng, model_dir, tag, names=ALL_NETS):
    """the state_dicts of a HirlEngine's networks `names` under the reference's key names, one file each"""
    for name, attr, layout, _ in HIRL_NETS:
        if name in names:
            torch.save({k: v.cpu().clone() for k, v in E.unpack(getattr(eng, attr), layout).items()}, os.path.join(model_dir, tag + name + "Harfang_GYM"))


def load_hirl_nets(eng, src_dir, tag, names=ALL_NETS, missing="{} not found"):
    """the files save_hirl_nets writes into the engine's networks `names`; `missing`: the FileNotFoundError's text, {} standing for the file"""
    for name, attr, layout, size in HIRL_NETS:
        if name in names:
            f = os.path.join(src_dir, tag + name + "Harfang_GYM")
            if not os.path.exists(f):
                raise FileNotFoundError(missing.format(f))
            flat = getattr(eng, attr)
            flat.copy_(E.pack(torch.load(f, map_location="cpu"), layout, size, flat.device))
    eng.refresh_bf16()
