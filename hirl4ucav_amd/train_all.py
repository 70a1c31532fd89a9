#!/usr/bin/env python3
"""Vectorised counterpart of the reference training driver (hirl/train_all.py, HIRL and TD3 branches, :261-487):
the same schedule — random exploration, expert-buffer labelling, per-step act / step / store / learn, expert_num decay,
linear / fixed / soft BC-weight schedules, periodic validation and checkpoints — with the single socket env replaced
by `--num_envs` GPU-resident envs per process and every per-step call replaced by a HIP launch.

    python -m hirl4ucav_amd.train_all --agent HIRL --type soft --env straight_line --random --num_envs 4096
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m hirl4ucav_amd.train_all ...   (one process per GPU)

What "one step" means here: the reference does one learn() per single env step (train_all.py:360-361).  With N envs a
vector step yields N transitions; this driver keeps ONE learn() of the reference's batch size per vector step by
default (`--updates_per_step` raises it).  That ratio is a stated design parameter, not something the reference fixes.
"""
import argparse
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .agents import engine as E
from .agents.HIRL import init_actor_state_dict, init_critic_state_dict
from .environments.batched import SCENARIOS, BatchedHarfangEnv
from .utils import checkpoint as CK
from .utils.buffer import DeviceReplay
from .utils.data_processor import read_data
from .utils.scalars import make_writer
from .utils.seed import set_seed

MAX_STEP = {"straight_line": 1500, "serpentine": 1500, "circular": 1900}  # train_all.py:159-183
MIXED = "mixed"  # --env mixed: one population over all of SCENARIOS (BASELINE.json configs[4]); an extension, the reference trains one scenario per run
MIXED_MAX_STEP = max(MAX_STEP.values())  # HxStepOpts.max_step is one word: a mixed population trains under the longest of its scenarios' limits
BATCH = 128  # train_all.py:190-208: the minibatch of every agent


# ---- pure host logic (unit-tested on CPU) ----------------------------------------------------------------------------
def mixed_scenarios(n, env_id0=0):
    """per-env scenario ids of a mixed shard of n envs whose first env has the global id env_id0: contiguous thirds, so that wavefronts never
    mix scenarios (the rule of bench.py --scenario mixed)"""
    return np.sort((env_id0 + np.arange(n)) % 3)


def scenarios_of(env_type):
    """the scenario names a --env value covers, in bin order"""
    return list(SCENARIOS) if env_type == MIXED else [env_type]


def default_max_step(env_type):
    return MIXED_MAX_STEP if env_type == MIXED else MAX_STEP[env_type]


def expert_paths(arg):
    """--expert_csv: one path, or a comma-separated list of them (one file per scenario, say) -> the list; empty items are an error"""
    if not arg:
        return []
    paths = [p.strip() for p in arg.split(",")]
    if any(not p for p in paths):
        raise ValueError(f"--expert_csv {arg!r}: an empty item in the list")
    return paths


def pool_validation(results, episodes=50):
    """The reference's four validation numbers over several validate() calls of `episodes` episodes each, from their (mean, std, successes, fire
    successes) tuples alone -> the same tuple for the pooled episodes: the mean of means, the population std of the pooled scores
    (sqrt(mean(std_k^2 + mean_k^2) - mean^2), equal groups), the summed counts (the caller divides by len(results) * episodes)."""
    means = np.asarray([r[0] for r in results], np.float64)
    stds = np.asarray([r[1] for r in results], np.float64)
    mean = float(means.mean())
    var = float((stds * stds + means * means).mean() - mean * mean)
    return mean, math.sqrt(max(var, 0.0)), int(sum(r[2] for r in results)), int(sum(r[3] for r in results))


def mixed_refusal(config):
    """why `--env mixed` cannot run as asked, or None"""
    if config.env == MIXED and config.num_envs < len(SCENARIOS):
        return f"--env mixed with --num_envs {config.num_envs}: a mixed population holds every scenario, so at least {len(SCENARIOS)} envs"
    return None


def bc_weight_schedule(hirl_type, episode, bc_weight, bc_warm_up=False):
    """(bc_weight_now, bc_warm_up_weight) at the start of `episode` — train_all.py:328-339."""
    warm = 0.0
    if hirl_type == "linear":
        return max(bc_weight - episode / 5000, 0), warm
    if hirl_type == "fixed":
        return bc_weight, warm
    if hirl_type == "soft":
        if bc_warm_up:
            warm = max(0.3 - episode / 1000, 0)
        return 100, warm
    raise ValueError(hirl_type)


def expert_num_after(expert_num, step, warm_up_rate=10, floor=0):
    """train_all.py:356-357: one expert row fewer whenever step % warm_up_rate == 0, down to 0.  floor (--expert_floor, a departure: DESIGN.md
    section 5): never below `floor` rows, so the expert rows outlive the warm-up; floor = 0 is the reference's rule."""
    after = expert_num - 1 if (step % warm_up_rate == 0 and expert_num != 0) else expert_num
    return after if floor == 0 else max(after, floor)


def next_expert_num(run, step):
    """expert_num behind this step's decay, under the run's --expert_floor (without one: the reference's call, argument for argument)"""
    floor = getattr(run, "expert_floor", 0)
    return expert_num_after(run.expert_num, step, run.warm_up_rate, floor=floor) if floor else expert_num_after(run.expert_num, step, run.warm_up_rate)


def expert_pair_indices(done):
    """Which (i, i+1) pairs the reference turns into expert-buffer transitions (train_all.py:289-306): it walks i over the
    expert rows and skips one extra row after a terminal pair.  done[i] = get_termination(states[i+1])."""
    out, i, n = [], 0, len(done) + 1
    while i + 1 < n:
        out.append(i)
        if done[i]:
            i += 1
        i += 1
    return np.asarray(out, np.int64)


def resolve_dtype(sac, requested, snap_driver=None):
    """The --dtype a run computes in, given the agent, the flag and the driver record of the snapshot it resumes (None: a fresh run).
    -> (dtype, warning or None, refusal or None, mark).  The run's arithmetic is part of its state: a snapshot taken under one --dtype does not
    continue under another (the flag changed meaning before: round 2's "bf16" was policy inference only, since round 3 it is the policy AND
    learn()'s 256 <-> 512 products).  SAC / E-SAC have no exact-split format (f32x9 runs fp32, with a warning), and before they had a bf16 path
    a SAC run given --dtype bf16 ran and stored "f32": a SAC snapshot without the `dtype_honoured` mark resumes in fp32 with that old warning,
    so that such a run keeps resuming with its own command line.  `mark`: whether this run's snapshots carry the mark — not while that legacy
    fallback applies (a snapshot it writes stays unmarked, and the next resume with the same command line takes the same branch)."""
    dtype, warning = requested, None
    marked = snap_driver is not None and bool(snap_driver.get("dtype_honoured"))
    legacy = sac and requested in ("bf16", "bf16_policy") and snap_driver is not None and not marked
    if sac and (requested == "f32x9" or legacy):
        dtype = "f32"
        warning = f"--dtype {requested} has no effect on " + ("the SAC / E-SAC agents (no exact-split format): running fp32" if requested == "f32x9" else
                                                              "a SAC run resumed from a snapshot that ran fp32: running fp32")
    snap_dtype = snap_driver.get("dtype") if snap_driver is not None else None
    if snap_dtype is not None and snap_dtype != dtype:
        return dtype, warning, f"was run with --dtype {snap_dtype}, --dtype {dtype} given", not legacy
    return dtype, warning, None, not legacy


def checkpoint_tag(arttir, success, episodes, mean_score):
    return "Agent{}_{}_{}_".format(arttir, round(success / episodes * 100), round(mean_score))  # train_all.py:69


# ---- device side -----------------------------------------------------------------------------------------------------
def label_expert(states, actions, device):
    """Expert replay rows [k, 32] + step_success from consecutive expert states, labelled on the GPU
    (HarfangEnv.get_reward / get_termination, HarfangEnv_GYM.py:299-336)."""
    rows, succ, _keep = label_expert_pairs(states, actions, device)
    return rows, succ


def label_expert_pairs(states, actions, device):
    """label_expert with the pair indices it kept (expert_pair_indices): utils.buffer.segment_last reads a file's segments off them"""
    s = torch.as_tensor(np.asarray(states[:-1], np.float32), device=device).contiguous()
    a = torch.as_tensor(np.asarray(actions[:-1], np.float32), device=device).contiguous()
    ns = torch.as_tensor(np.asarray(states[1:], np.float32), device=device).contiguous()
    m = s.shape[0]
    r = torch.zeros(m, device=device)
    sc = torch.zeros(m, dtype=torch.int8, device=device)
    dn = torch.zeros(m, dtype=torch.uint8, device=device)
    _lib.call("hx_label_transitions", s.data_ptr(), a.data_ptr(), ns.data_ptr(), m, r.data_ptr(), sc.data_ptr(), dn.data_ptr(), _lib.stream_ptr())
    keep = torch.as_tensor(expert_pair_indices(dn.cpu().numpy().astype(bool)), device=device)
    rows = torch.cat([s, a, ns, r[:, None], dn.float()[:, None]], 1)[keep]
    return rows, sc[keep], keep


def validate(engine, scenario, episodes, max_step, if_random, seed, device, sac=False, env=None, recorder=None):
    """validate() of train_all.py:22-102 (train_sac.py:24-68 for SAC) as ONE batch: `episodes` envs stepped with
    chooseActionNoNoise / exploit until done or the step limit.  The kernels keep simulating an env after its `done` (no auto
    reset here), so everything the reference reads when it SEES done — the score so far, env.episode_success, env.fire_success
    (train_all.py:59-64) — is latched at the first step with done != 0: a missile that is still in flight when the aircraft leaves
    the altitude band must not turn that episode into a kill afterwards.  `env`: a prepared BatchedHarfangEnv (tests, --plot).
    `recorder`: an EpisodeRecorder over `env` (utils/trace.py) — one more launch behind every env step; None: none, and the return is the same."""
    if env is None:
        env = BatchedHarfangEnv(episodes, scenario=scenario, device=device, seed=seed, auto_reset=False, random_reset=if_random, collect_stats=False)
        obs = env.reset()
    else:
        obs = env.obs
    calls = getattr(engine, "act_calls", None)  # validation must not move the training run's exploration-noise counter
    total = torch.zeros(episodes, device=device)
    alive = torch.ones(episodes, dtype=torch.bool, device=device)
    kill = torch.zeros(episodes, dtype=torch.bool, device=device)
    fired = torch.zeros(episodes, dtype=torch.bool, device=device)
    if recorder is not None:
        recorder.reset()
    for step in range(max_step):
        a = engine.act(obs, explore=False) if sac else engine.act(obs)
        obs, r, d, s = env.step(a)
        if recorder is not None:
            recorder.push()
        total += torch.where(alive, r, torch.zeros_like(r))
        ending = alive & (d != 0)
        flags = env.state[35].view(torch.int32)
        kill |= ending & ((flags & _lib.F_EPISODE_SUCCESS) != 0)
        fired |= ending & ((flags & _lib.F_FIRE_SUCCESS) != 0)
        alive &= d == 0
        if step % 64 == 63 and not bool(alive.any()):
            break
    if calls is not None:
        engine.act_calls = calls
    scores = total.cpu().numpy()
    return float(scores.mean()), float(scores.std()), int(kill.sum()), int(fired.sum())


def validate_plotting(plot, engine, scenario, episodes, max_step, if_random, seed, device, sac=False):
    """validate(), and with --plot the record of its last episode -> (validate()'s tuple, the EpisodeRecorder or None).  Without --plot: the call as it
    always was, no launch more."""
    if not plot:
        return validate(engine, scenario, episodes, max_step, if_random, seed, device, sac), None
    from .utils.trace import validation_recorder

    env, rec = validation_recorder(episodes, scenario, seed, if_random, max_step, device)
    return validate(engine, scenario, episodes, max_step, if_random, seed, device, sac, env=env, recorder=rec), rec


def validate_mixed(plot, engine, episodes, if_random, seed, device, sac=False):
    """--env mixed: the existing validate() once per scenario — `episodes` episodes each, that scenario's OWN step limit (MAX_STEP), the same seed — so
    every tuple is what a single-scenario run would get from the same networks -> ({scenario: validate()'s tuple}, {scenario: recorder or None})."""
    results, recorders = {}, {}
    for name in SCENARIOS:
        results[name], recorders[name] = validate_plotting(plot, engine, name, episodes, MAX_STEP[name], if_random, seed, device, sac)
    return results, recorders


def validate_env(config, engine, env_type, max_step, seed, device, sac=False, episodes=50):
    """The periodic validation of a training run -> (the tuple the checkpoint rule reads, {scenario: tuple}, {scenario: recorder or None}).
    One scenario: validate_plotting as ever.  mixed: validate_mixed, pooled over the three scenarios' episodes (pool_validation)."""
    if env_type != MIXED:
        res, rec = validate_plotting(config.plot, engine, env_type, episodes, max_step, config.random, seed, device, sac)
        return res, {env_type: res}, {env_type: rec}
    results, recorders = validate_mixed(config.plot, engine, episodes, config.random, seed, device, sac)
    return pool_validation([results[k] for k in SCENARIOS], episodes), results, recorders


def write_validation_plots(recorders, plot_dir, arttir):
    """--plot: the last validation episode's files beside a checkpoint; under mixed one set per scenario with the tag <arttir>_<scenario>"""
    for name, rec in recorders.items():
        if rec is not None:
            rec.write_reference_files(plot_dir, arttir if len(recorders) == 1 else f"{arttir}_{name}")


def log_validation_by_scenario(writer, episode, results, episodes=50):
    """mixed: Validation/<scenario>/{Avg Reward, Std Reward, Success Rate, Fire Success Rate} beside the four pooled reference tags"""
    if writer is None or len(results) == 1:
        return
    for name, (mean, std, succ, fire) in results.items():
        for tag, v in (("Avg Reward", mean), ("Std Reward", std), ("Success Rate", succ / episodes), ("Fire Success Rate", fire / episodes)):
            writer.add_scalar(f"Validation/{name}/{tag}", v, episode)


def log_episode_stats(writer, episode, stats, last100):
    """The per-scenario Training/* scalars of one driver episode from EpisodeStats.read_and_clear(), for every scenario in which an episode ended,
    and Training/Last 100 Episode Average Reward (train_all.py:384) from the (sum, count) window, to which this episode is added first."""
    last100.add(sum(s["sum_ret"] for s in stats.values()), sum(s["count"] for s in stats.values()))
    if writer is None:
        return
    for name, s in stats.items():
        if not s["count"]:
            continue
        writer.add_scalar(f"Training/{name}/Episode Reward", s["mean"], episode)
        writer.add_scalar(f"Training/{name}/Episode Reward Std", s["std"], episode)
        writer.add_scalar(f"Training/{name}/Episode Length", s["mean_len"], episode)
        writer.add_scalar(f"Training/{name}/Average Step Reward", s["sum_ret"] / max(s["sum_len"], 1.0), episode)
        writer.add_scalar(f"Training/{name}/Ended By Done", s["done"], episode)
        writer.add_scalar(f"Training/{name}/Ended By Time Limit", s["time_limit"], episode)
    if not math.isnan(last100.mean()):
        writer.add_scalar("Training/Last 100 Episode Average Reward", last100.mean(), episode)


def load_expert_files(config):
    """load_expert per file of --expert_csv's list -> [(states, actions), ...]: each file is read, and later labelled, on its own, so that no
    transition spans two files.  One path (or none: --synthetic_expert) gives the one table load_expert gives."""
    paths = expert_paths(config.expert_csv)
    if len(paths) <= 1:
        return [load_expert(config)]
    out = []
    for p in paths:
        if not os.path.exists(p):
            raise FileNotFoundError(f"--expert_csv {p}: no such file")
        out.append(read_data(p))
    return out


def load_expert(config, rng_seed=0):
    """read_data(data_dir) (train_all.py:222-228).  The reference raises when the file is missing, and so does this: a mistyped path must
    not turn into a run that trains on noise.  `--synthetic_expert` (benchmarks, tests; the Drive data is not available, README.md:6,30)
    asks for a uniform-random stand-in of the same shape explicitly, and says so loudly."""
    if config.expert_csv:
        if not os.path.exists(config.expert_csv):
            raise FileNotFoundError(f"--expert_csv {config.expert_csv}: no such file")
        return read_data(config.expert_csv)
    if not getattr(config, "synthetic_expert", False):
        raise ValueError("HIRL / E-SAC / BC need expert data: pass --expert_csv FILE (hirl4ucav_amd.data.ai_data_col writes one), or "
                         "--synthetic_expert to run on a uniform-random stand-in (throughput runs and tests only)")
    print("WARNING: --synthetic_expert: the expert table is UNIFORM RANDOM noise - throughput / plumbing runs only", flush=True)
    rng = np.random.default_rng(rng_seed)
    es = rng.uniform(-1, 1, (20000, 13))
    es[:, 7:9] = np.where(rng.random((20000, 2)) < 0.5, 1, -1)
    es[:, 12] = rng.uniform(0, 0.2, 20000)
    ea = rng.uniform(-1, 1, (20000, 4))
    ea[:, 3] = np.where(rng.random(20000) < 1e-3, 1, -1)
    return es, ea


def shared_value(value, world):
    """rank 0's `value` on every rank (one broadcast_object_list)"""
    if world <= 1:
        return value
    box = [value]
    torch.distributed.broadcast_object_list(box, src=0)
    return box[0]


def save_hparams(log_dir, **kw):
    """save_parameters_to_txt (train_all.py:104-109,233): log1.txt, one key=value per line"""
    with open(os.path.join(log_dir, "log1.txt"), "w") as f:
        for k, v in kw.items():
            f.write(f"{k}={v}\n")


def log_validation(writer, episode, mean, std, success_rate, fire_rate):
    """the four Validation/* scalars of train_all.py:97-100"""
    writer.add_scalar("Validation/Avg Reward", mean, episode)
    writer.add_scalar("Validation/Std Reward", std, episode)
    writer.add_scalar("Validation/Success Rate", success_rate, episode)
    writer.add_scalar("Validation/Fire Success Rate", fire_rate, episode)
    if hasattr(writer, "flush"):
        writer.flush()


def train_bc(config, device, seed, max_step):
    """The BC branch of train_all.py:244-260: maxStep train_actor() calls per 'episode' on the expert (s, a) table, validation
    every checkpoint_rate episodes from --bc_validate_from on, actor checkpoints with the reference's tag and file name."""
    env_type, batch = config.env, 128
    eng = E.HirlEngine(batch=batch, lr_actor=1e-3, slope=0.01, use_bc=True, device=device)  # BC.py:129-135 leaky_relu
    eng.load_params(init_actor_state_dict(), init_critic_state_dict())
    tables = load_expert_files(config)
    es, ea = np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables])
    tab = np.zeros((es.shape[0], 32), np.float32)
    tab[:, 0:13], tab[:, 13:17] = es, ea
    bc_table = torch.from_numpy(tab).to(device)
    table = DeviceReplay(es.shape[0], device)  # the sampler wants a main ring as well; the BC step reads only the BC rows
    table.store_rows(bc_table)
    if hirl_per_refusal(config) or upsample_refusal(config) or expert_online_refusal(config) or expert_branch_refusal(config) or expert_self_refusal(config) or expert_floor_refusal(config) or explore_refusal(config):
        raise SystemExit("train_all: " + (hirl_per_refusal(config) or upsample_refusal(config) or expert_online_refusal(config) or expert_branch_refusal(config)
                                          or expert_self_refusal(config) or expert_floor_refusal(config) or explore_refusal(config)))
    if getattr(config, "expert_upsample", False):  # BC.py:152-158, 171-176: one row of every minibatch is a fire row
        from .utils.buffer import fire_rows

        fire = fire_rows(bc_table)
        if upsample_refusal(config, n_fire=fire.numel()):
            raise SystemExit("train_all: " + upsample_refusal(config, n_fire=fire.numel()))
        eng.set_upsample(None, fire)
    log_dir = os.path.join(config.result_dir, env_type, config.agent, config.model_name, time.strftime("%Y_%m_%d_%H_%M"))
    model_dir = os.path.join(log_dir, "model")
    os.makedirs(model_dir, exist_ok=True)
    plot_dir = os.path.join(log_dir, "plot")  # train_all.py:217-219: beside model and summary
    if config.plot:
        os.makedirs(plot_dir, exist_ok=True)
    save_hparams(log_dir, actorLR=1e-3, batchSize=batch, maxStep=max_step, hiddenLayer1=256, hiddenLayer2=512, agent="BC", model_dir=model_dir,
                 data_dir=config.expert_csv)
    writer = make_writer(os.path.join(log_dir, "summary"))
    high_score, success_rate, arttir = -math.inf, 0.0, 1
    for episode in range(config.episodes):
        for _ in range(max_step):
            eng.sample(table, None, bc_table, seed=seed + 2)
            eng.bc_train_actor()
        bc_loss = eng.losses_host()[2]
        writer.add_scalar("Loss/BC_Loss", bc_loss, (episode + 1) * max_step)  # train_all.py:250-251
        print(f"Episode {episode + 1}: bc_loss {bc_loss:.6f}", flush=True)
        if (episode + 1) % config.checkpoint_rate == 0 and (episode + 1) >= config.bc_validate_from:  # train_all.py:259
            (mean, std, succ, fire), by_scenario, recs = validate_env(config, eng, env_type, max_step, seed + 12345, device)
            val_n = 50 * len(by_scenario)  # (mixed: the pooled episodes of the three scenarios)
            if mean > high_score or succ / val_n >= success_rate or arttir % 5 == 0:
                CK.save_hirl_nets(eng, model_dir, checkpoint_tag(arttir, succ, val_n, mean), names=("Actor_",))
                write_validation_plots(recs, plot_dir, arttir)  # train_all.py:70-89: only beside a checkpoint
                high_score, success_rate = max(high_score, mean), max(success_rate, succ / val_n)
            print(f"Validation {arttir}: avg reward {mean:.2f} (std {std:.2f}) success {succ / val_n:.2f} fire success {fire / val_n:.2f}", flush=True)
            log_validation_by_scenario(writer, episode, by_scenario)
            log_validation(writer, episode, mean, std, succ / val_n, fire / val_n)
            arttir += 1
    writer.close()
    return log_dir


def launch_ranks(n, argv):
    """`--gpus N` without a launcher environment: start the N ranks as a CHILD torch.distributed.run (this process has not touched a
    GPU and only relays the exit code); refuse when fewer than N GPUs are visible."""
    import socket
    import subprocess
    import sys

    have = torch.cuda.device_count()  # counting does not initialise the GPU
    if have < n and os.environ.get("HX_DIST_BACKEND", "nccl") == "nccl":
        sys.stderr.write(f"train_all: {n} GPUs requested, {have} visible\n")
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
                            "--master-port", str(port), "-m", "hirl4ucav_amd.train_all"] + list(argv), env=env)


# ---- the training run: one plain state object, filled by the functions below in main()'s order -----------------------------------------------------
Run = SimpleNamespace  # config, rank / world / device / seed, the agent flags, env / replay / inserter / eng / expert tables, writer and directories, driver scalars


def start_run(config):
    """process / device / process-group setup, the seed and snapshot negotiation, the step limit -> Run"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if getattr(config, "gpus", None) and config.gpus != world:
        raise SystemExit(f"train_all: --gpus {config.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if not torch.cuda.is_available():
        raise SystemExit("train_all needs a GPU: the product has no CPU path")
    if world > torch.cuda.device_count() and os.environ.get("HX_DIST_BACKEND", "nccl") == "nccl":
        raise SystemExit(f"train_all: {world} ranks but {torch.cuda.device_count()} GPUs visible")
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL over xGMI; HX_DIST_BACKEND=gloo exists only to exercise this path where all ranks share one GPU (tests)
        backend = os.environ.get("HX_DIST_BACKEND", "nccl")
        torch.distributed.init_process_group(backend, **({"device_id": device} if backend == "nccl" else {}))
    # no --seed: rank 0 draws one and every rank uses it (the replicas must start from identical networks either way); it is printed
    # and written to log1.txt, so that "unseeded" differs from --seed 0 and is still reproducible after the fact
    # --resume: the run's seed comes from the snapshot (the Philox keys of acting noise, sampling and random_reset must not change mid-run);
    # an explicit --seed that differs is an error
    snap = CK.read_run(os.path.join(config.resume, f"state_rank{rank}.pt")) if config.resume else None
    snap_seed = snap["driver"].get("seed") if snap is not None else None
    if snap_seed is not None and config.seed is not None and int(config.seed) != int(snap_seed):
        raise SystemExit(f"train_all: --resume {config.resume} was run with seed {snap_seed}, --seed {config.seed} given")
    seed = shared_value(snap_seed if snap_seed is not None else
                        (config.seed if config.seed is not None else int.from_bytes(os.urandom(4), "little") & 0x7FFFFFFF), world)
    set_seed(seed + rank)
    if rank == 0:
        print(f"seed {seed}" + (" (from the snapshot)" if snap_seed is not None else "" if config.seed is not None else " (drawn: no --seed given)"), flush=True)
    env_type = config.env
    max_step = (int(config.max_step) if getattr(config, "max_step", None) else default_max_step(env_type)) * (8 if config.render else 1)
    if mixed_refusal(config):
        raise SystemExit("train_all: " + mixed_refusal(config))
    snap_env = snap["driver"].get("env") if snap is not None else None  # (a snapshot from before --env mixed does not record it: it is not a mixed one)
    if snap is not None and (snap_env != env_type if snap_env is not None else env_type == MIXED):
        raise SystemExit(f"train_all: --resume {config.resume} was run with --env {snap_env if snap_env is not None else 'of one scenario (unrecorded)'}, "
                         f"--env {env_type} given")
    return Run(config=config, rank=rank, world=world, device=device, seed=seed, snap=snap, env_type=env_type, n=config.num_envs, max_step=max_step)


def check_agent_flags(run):
    """the agent flags, each with its refusal check"""
    config, world = run.config, run.world
    run.sac, run.hirl = config.agent == "SAC", config.agent == "HIRL"
    run.esac = run.sac and config.type == "ESAC"
    run.isac = run.sac and config.type == "ISAC"  # SacAgent(imitative=True): the BC-gated policy loss; the minibatch is NOT expert-mixed
    if run.isac and (world > 1 or getattr(config, "dtype", "f32") != "f32" or not config.bc_actor):
        raise SystemExit("train_all: " + isac_refusal(config, world))
    run.per = bool(getattr(config, "per", False))  # SacAgent(per=True): prioritized replay, the importance weights through the three losses
    # --hirl_per: HirlEngine.set_prioritized (an extension) on the same store — the replay, the marking of new rows behind every acting
    # launch and the stats/per_* scalars are --per's (run.per); what differs hangs on run.hirl_per
    run.hirl_per = bool(getattr(config, "hirl_per", False))
    run.per = run.per or run.hirl_per
    run.per_new = getattr(config, "per_new", "max")  # how a step's rows get their first priority: at pmax, or at a TD error of their own (agent.py:234-246)
    run.multi_step = int(getattr(config, "multi_step", 1))  # SacAgent(multi_step=n): truncated n-step returns (utils.buffer.NStepInserter)
    # --hirl_multi_step: HirlEngine.set_multi_step (an extension) on the same inserter — the env without a ring, the push behind every
    # acting launch and the bound of mark_new are --multi_step's (run.multi_step, run.inserter); what differs hangs on run.hirl_multi_step
    run.hirl_multi_step = int(getattr(config, "hirl_multi_step", 1)) if not run.sac else 1
    if run.hirl_multi_step != 1:
        run.multi_step = run.hirl_multi_step
    run.grad_clip, run.fixed_alpha = getattr(config, "grad_clip", None), getattr(config, "fixed_alpha", None)  # SacAgent(grad_clip=c) / (entropy_tuning=False, ent_coef=x)
    if not run.sac:  # HIRL / TD3: --hirl_grad_clip, an extension (HirlEngine.set_grad_clip); --grad_clip itself is refused for them (clip_refusal)
        run.grad_clip = getattr(config, "hirl_grad_clip", None)
    # the reference's two sampling switches (HIRL.py:184-185): success rows of the replay drawn 10 : 1, one fire row forced into the BC minibatch
    run.buffer_upsample, run.expert_upsample = bool(getattr(config, "buffer_upsample", False)), bool(getattr(config, "expert_upsample", False))
    run.upsampler = None
    for refusal in (per_refusal, hirl_per_refusal, nstep_refusal, hirl_multi_step_refusal, clip_refusal, hirl_clip_refusal, upsample_refusal, expert_online_refusal, expert_branch_refusal, expert_self_refusal, expert_floor_refusal, explore_refusal):  # (per_refusal without --per: --per_new td on its own)
        if refusal(config, world):
            raise SystemExit("train_all: " + refusal(config, world))
    if hirl_per_resume_refusal(config, getattr(run, "snap", None)):
        raise SystemExit(f"train_all: --resume {config.resume} " + hirl_per_resume_refusal(config, run.snap))
    if hirl_multi_step_resume_refusal(config, getattr(run, "snap", None)):
        raise SystemExit(f"train_all: --resume {config.resume} " + hirl_multi_step_resume_refusal(config, run.snap))
    run.batch = BATCH  # train_all.py:190-208
    run.expert_floor = int(getattr(config, "expert_floor", 0))  # --expert_floor: expert_num stops there instead of at 0 (expert_num_after)
    run.warm_up_rate = 20 if run.sac else 10  # train_sac.py:203 / train_all.py:207


def build_env(run):
    """replay ring, envs, the n-step inserter and the episode statistics"""
    config, device, n, env_type = run.config, run.device, run.n, run.env_type
    if run.per:  # SAC/agent.py:112-118 (alpha 0.6, beta 0.4, beta_annealing 0.0001 are the reference's defaults)
        from .utils.buffer import PrioritizedReplay, score_chunk_for

        run.replay = PrioritizedReplay(config.buffer_size, device, alpha=config.per_alpha, beta=config.per_beta, beta_annealing=config.per_beta_annealing)
        run.replay.score_chunk = score_chunk_for(n)  # --per_new td: rows per chunk of the scoring pass, by the envs per step (measured: DESIGN.md section 8)
    else:
        run.replay = DeviceReplay(config.buffer_size, device)
    run.env = BatchedHarfangEnv(n, scenario=mixed_scenarios(n, run.rank * n).astype(np.int32) if env_type == MIXED else env_type, device=device, seed=run.seed,
                                max_step=run.max_step, auto_reset=True, random_reset=config.random, env_id0=run.rank * n,
                                replay=run.replay if run.multi_step == 1 else None)
    if run.buffer_upsample:  # UniformMemory(capacity, upsample=True), HIRL.py:189: the counts beside the ring, kept current behind every acting launch
        from .utils.buffer import SuccessUpsampler

        run.upsampler = SuccessUpsampler(run.replay, int(config.upsample_boost))
    run.inserter = None
    if run.multi_step > 1:  # the acting launches run without a ring; the inserter's launch behind each step writes the finished n-step rows
        from .utils.buffer import NStepInserter

        run.inserter = NStepInserter(run.replay, n, run.multi_step, 0.99)  # (SacEngine's gamma, SAC/agent.py:60; HirlEngine's, HIRL.py:162: set_multi_step checks it)
    # Episode statistics by scenario (utils/epstat.py): one small launch behind every acting launch.  On under --env mixed, opt-in (--episode_stats) for
    # one scenario; off, the run is launch for launch what it was.  Every rank keeps its own shard's statistics; rank 0 writes its own.
    run.estats = run.last100 = None
    if env_type == MIXED or getattr(config, "episode_stats", False):
        from .utils.epstat import EpisodeStats, Last100

        run.estats, run.last100 = EpisodeStats(run.env), Last100()


def build_engine(run):
    """the engine of either agent family, with the networks every rank starts from"""
    torch.manual_seed(run.seed)  # identical initial networks on every rank
    if run.sac:  # train_sac.py:187-215: lr 1e-3, hidden [256, 512], batch 128, target_update_interval 3
        from .agents import sac_engine as SE
        from .agents.SAC.agent import _xavier_mlp

        eng = SE.SacEngine(batch=run.batch, lr=1e-3, device=run.device)
        eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
        if run.per:
            eng.set_prioritized(run.replay, new_rows=run.per_new)
        if run.grad_clip is not None:  # update_params(..., grad_clip), SAC/agent.py:310-320
            eng.set_grad_clip(run.grad_clip)
        if run.fixed_alpha is not None:  # SAC/agent.py:108-110
            eng.set_entropy_tuning(False, run.fixed_alpha)
        if run.inserter is not None:
            eng.set_multi_step(run.inserter)
    else:
        eng = E.HirlEngine(batch=run.batch, slope=0.0 if run.hirl else 0.01, use_bc=run.hirl, device=run.device)
        eng.load_params(init_actor_state_dict(), init_critic_state_dict(), init_actor_state_dict() if run.hirl else None)
        if run.grad_clip is not None:  # an extension (the reference's HIRL / TD3 have no clip): clip_grad_norm_ once per optimizer, DESIGN.md section 5
            eng.set_grad_clip(run.grad_clip)
        if run.hirl_per:  # an extension too: proportional draws of the replay rows, importance weights through the critic loss, |Q1 - y| back as priorities
            eng.set_prioritized(run.replay)
        if run.inserter is not None:  # an extension too (--hirl_multi_step): n-step rows in the ring, the row's discount in its done column
            eng.set_multi_step(run.inserter)
    run.eng = eng


def load_expert_tables(run):
    """HIRL / E-SAC / ISAC: the labelled expert ring, the BC (s, a) table and the frozen bc_actor"""
    config, device, eng = run.config, run.device, run.eng
    run.expert = run.bc_table = run.fire_idx = run.online = run.branch = run.selfx = None
    if run.upsampler is not None:  # (TD3 has no expert table: the engine hears of the upsampler here)
        eng.set_upsample(run.upsampler, None)
    if not (run.hirl or run.esac or run.isac):
        return
    why = (expert_branch_resume_refusal(config, run.snap["driver"] if run.snap is not None else None)
           or expert_self_resume_refusal(config, run.snap["driver"] if run.snap is not None else None)
           or expert_floor_resume_refusal(config, run.snap["driver"] if run.snap is not None else None))
    if why:
        raise SystemExit(f"train_all: --resume {config.resume} {why}")
    tables = load_expert_files(config)
    labelled = [label_expert_pairs(es_k, ea_k, device) for es_k, ea_k in tables]  # each file on its own: no transition spans two files
    rows, succ = torch.cat([r for r, _, _ in labelled]), torch.cat([s_ for _, s_, _ in labelled])
    if run.hirl and getattr(run, "hirl_multi_step", 1) > 1:
        # --hirl_multi_step: the offline expert rows become n-step rows too (hx_nstep_label), before they are stored — and so before BranchExpert copies
        # them.  Row j stays row j: succ, fire_idx and the ring's layout stay valid.  Each file ends a segment.  (E-SAC's rows under --multi_step stay one-step.)
        from .utils.buffer import nstep_relabel, segment_last

        last = np.concatenate([segment_last(r[:, 31], keep) for r, _, keep in labelled])
        rows = nstep_relabel(rows, last, run.hirl_multi_step, float(eng.hyper.gamma))
    es, ea = np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables])
    if int(getattr(config, "expert_branch", 0)) > 0:
        # An extension (utils/pilot.py): the ring grows by an online region that starts as a cyclic copy of the labelled rows and is rewritten behind
        # every acting launch by branches of the learner's envs under the pilot: one step per pick, or (--expert_branch_steps H > 1) resident flights of
        # up to H steps that advance one step per launch.  Its length stays E0 + ROWS: the samplers are untouched.
        from .utils.pilot import BranchExpert

        run.branch = BranchExpert(run.env, rows, succ, int(config.expert_branch), int(config.expert_branch_per_step), device,
                                  steps=int(getattr(config, "expert_branch_steps", 1)))
        run.expert = run.branch.ring
    elif int(getattr(config, "expert_self", 0)) <= 0:
        run.expert = DeviceReplay(rows.shape[0] + 10, device)
        run.expert.store_rows(rows, succ)
    tab = np.zeros((es.shape[0], 32), np.float32)
    tab[:, 0:13], tab[:, 13:17] = es, ea
    run.bc_table = torch.from_numpy(tab).to(device)
    if int(getattr(config, "expert_self", 0)) > 0:
        # An extension (utils/selfimit.py): the same online region, rewritten by the LEARNER's own episodes that ended in a kill (hx_self_push behind
        # every acting launch: a device tape of the last --expert_self_steps steps per env).  --expert_self_bc: the BC table grows by the same region and
        # takes the same rows as (s, a).  Under --hirl_multi_step the self rows stay one-step rows, as branch rows do.
        from .utils.selfimit import SelfExpert

        run.selfx = SelfExpert(run.env, rows, succ, int(config.expert_self), int(config.expert_self_steps),
                               bc_table_offline=run.bc_table if getattr(config, "expert_self_bc", False) else None, device=device)
        run.expert = run.selfx.ring
    if (run.hirl or run.isac) and config.bc_actor and not os.path.exists(config.bc_actor):  # agent.load_bc_actor: a missing file is an error, as in the reference
        raise FileNotFoundError(f"--bc_actor {config.bc_actor}: no such file")
    if run.hirl and config.bc_actor:  # agent.load_bc_actor (train_all.py:311-312)
        eng.bc_actor.copy_(E.pack(torch.load(config.bc_actor, map_location="cpu"), E.ACTOR_LAYOUT, E.ACTOR_SIZE, device))
    elif run.hirl and config.type == "soft" and run.rank == 0:
        print("WARNING: HIRL-soft without --bc_actor: the soft weight is estimated against a randomly initialised bc_actor", flush=True)
    if run.isac:  # agent.load_bc_actor (SAC/agent.py:158-160)
        eng.set_imitative(torch.load(config.bc_actor, map_location="cpu"), slope=0.01)
    if run.expert_upsample:  # target_indices, HIRL.py:217-219
        from .utils.buffer import fire_rows

        run.fire_idx = fire_rows(run.bc_table)
        if upsample_refusal(config, run.world, n_fire=run.fire_idx.numel()):
            raise SystemExit("train_all: " + upsample_refusal(config, run.world, n_fire=run.fire_idx.numel()))
        eng.set_upsample(run.upsampler, run.fire_idx)
    why = expert_online_resume_refusal(config, run.snap["driver"] if run.snap is not None else None)
    if why:
        raise SystemExit(f"train_all: --resume {config.resume} {why}")
    if int(getattr(config, "expert_online", 0)) > 0:
        # An extension (utils/pilot.py): the table grows by an online region that starts as a cyclic copy of the offline rows and is relabelled by the
        # pilot behind every acting launch.  fire_idx above was taken from the offline rows, which stay where they are: it stays valid.
        from .utils.pilot import OnlineExpert

        run.online = OnlineExpert(run.env, run.bc_table, int(config.expert_online), int(config.expert_online_per_step))
        run.bc_table = run.online.table
    if run.selfx is not None and run.selfx.table is not None:  # --expert_self_bc: the widened table (fire_idx above was taken from the offline rows, likewise)
        run.bc_table = run.selfx.table


def set_dtype(run):
    """--dtype against the agent and the snapshot, then the engine's acting / update formats; the sharded update's transport"""
    config, eng = run.config, run.eng
    run.dtype, warning, refusal, mark = resolve_dtype(run.sac, getattr(config, "dtype", "f32"), run.snap["driver"] if run.snap is not None else None)
    run.dtype_mark = {"dtype_honoured": True} if mark else {}  # (in every snapshot's driver record)
    if warning and run.rank == 0:
        print(f"WARNING: {warning}", flush=True)
    if refusal:
        raise SystemExit(f"train_all: --resume {config.resume} {refusal}")
    if run.world > 1 and os.environ.get("HX_DIST_BACKEND", "nccl") == "nccl" and hasattr(eng, "use_rccl_direct"):
        eng.use_rccl_direct()  # ncclAllReduce enqueued by the library on the engine's stream (hx_rccl_*): no torch.distributed call inside learn()
    if run.dtype == "f32x9" and not run.sac:  # fp32, the acting kernel's 256 -> 512 product through the exact three-way bf16 split of both operands (engine.set_act_dtype)
        eng.set_act_dtype("f32x9")
    elif run.dtype in ("bf16", "bf16_policy"):  # bf16: policy AND critics (BASELINE.json configs[4]; SAC: SacEngine's bf16 path); bf16_policy: policy inference only
        eng.set_act_dtype("bf16")
        if run.dtype == "bf16":
            eng.set_update_dtype("bf16")


def open_run_dir(run):
    """the run directory, log1.txt and the writer (rank 0); --load_model"""
    config = run.config
    # ONE run directory for all ranks: rank 0 names it (a minute boundary between ranks would scatter the state_rank<r>.pt shards)
    run.log_dir = shared_value(os.path.join(config.result_dir, run.env_type, config.agent, config.model_name, time.strftime("%Y_%m_%d_%H_%M")), run.world)
    run.model_dir = os.path.join(run.log_dir, "model")
    os.makedirs(run.model_dir, exist_ok=True)
    run.plot_dir = os.path.join(run.log_dir, "plot")  # train_all.py:217-219: beside model and summary
    run.writer = None
    if run.rank == 0:
        if config.plot:
            os.makedirs(run.plot_dir, exist_ok=True)
        save_hparams(run.log_dir, bufferSize=config.buffer_size, criticLR=1e-3, actorLR=1e-3, batchSize=run.batch, maxStep=run.max_step, validationStep=run.max_step,
                     hiddenLayer1=256, hiddenLayer2=512, agent=config.agent, model_dir=run.model_dir, hirl_type=config.type, data_dir=config.expert_csv,
                     num_envs=run.n, world=run.world, seed=run.seed, dtype=getattr(config, "dtype", "f32"))
        run.writer = make_writer(os.path.join(run.log_dir, "summary"))
    if config.load_model and not run.sac:  # agent.loadCheckpoints(tag, model_dir), train_all.py:239-240 (the reference hard-codes the tag)
        CK.load_hirl_nets(run.eng, config.load_dir or run.model_dir, config.load_tag,
                          missing="--load_model: {} not found (--load_dir / --load_tag name the checkpoint)")


def build_explore(run):
    """--explore_*: the scale of the learner's action noise and, for any colour but white or a ladder of scales, the generator that draws it (an
    extension).  white at one scale: run.explore stays None and the acting kernels draw as ever, call for call."""
    config = run.config
    why = explore_resume_refusal(config, run.snap["driver"] if run.snap is not None else None)
    if why:
        raise ValueError(f"train_all: --resume {config.resume} {why}")
    e = explore_settings(config)
    run.act_sigma, run.explore = float(e["explore_sigma"]), None
    if not explore_uses_generator(config):
        return
    from .utils.noise import ColoredNoise, lag_autocorr

    # SAC / ESAC / ISAC: unit-variance eps for the Gaussian head (the policy's log-std scales it).  Seed + 4: the acting kernels key seed + 1, the draws
    # seed + 2 + rank, the scoring pass seed + 3 + rank; the generator's counters carry the env id, so every rank takes the same key
    gen = ColoredNoise(run.n, e["explore_noise"], tau=e["explore_tau"], octaves=e["explore_octaves"], sigma=1.0 if run.sac else run.act_sigma,
                       sigma_max=e["explore_sigma_max"], seed=run.seed + 4, env_id0=run.env.env_id0, chunk=e["explore_chunk"], device=run.device)
    run.explore = gen
    if run.writer is not None:
        lo, hi = gen.sigma_range()
        for tag, v in (("Explore/Sigma Min", lo), ("Explore/Sigma Max", hi), ("Explore/Lag1 Autocorr", lag_autocorr(gen.a, gen.w, 1))):
            run.writer.add_scalar(tag, v, 0)


def stats_record(run):
    """what every snapshot's driver record carries beside the driver's scalars"""
    rec = {"env": run.env_type}
    if run.estats is not None:
        rec["episode_stats"] = {"device": run.estats.state(), "last100": run.last100.state()}
    if getattr(run, "online", None) is not None:  # (a snapshot of a run without --expert_online carries no such key)
        rec["expert_online"] = run.online.state_dict()
    if getattr(run, "branch", None) is not None:  # (likewise without --expert_branch)
        rec["expert_branch"] = run.branch.state_dict()
    if getattr(run, "selfx", None) is not None:  # (likewise without --expert_self)
        rec["expert_self"] = run.selfx.state_dict()
    if getattr(run, "expert_floor", 0):  # (likewise without --expert_floor)
        rec["expert_floor"] = run.expert_floor
    flags = {k: v for (k, default), v in zip(EXPLORE_FLAGS, explore_settings(getattr(run, "config", None)).values()) if v != default}
    if flags:  # (likewise without any --explore_* flag)
        rec["explore"] = {"flags": flags, "generator": run.explore.state_dict() if getattr(run, "explore", None) is not None else None}
    return rec


def restore_stats(run, record):
    """after CK.load_run: the statistics workspace and the last-100 window of the snapshot; a snapshot without them starts them at zero.  The online
    region of the expert table and its call counter come back here too (load_expert_tables has refused a snapshot without them)."""
    if getattr(run, "online", None) is not None:
        run.online.load_state_dict(record["expert_online"])
    if getattr(run, "branch", None) is not None:
        run.branch.load_state_dict(record["expert_branch"])
    if getattr(run, "selfx", None) is not None:  # the tape is not in the snapshot: every env's episode starts empty at the restored env's observation
        run.selfx.load_state_dict(record["expert_self"])
        run.selfx.reset()
    if getattr(run, "explore", None) is not None:  # the bank's state, the chunk and the step counter: the noise goes on as if the run had never stopped
        run.explore.load_state_dict(record["explore"]["generator"])
    if run.estats is None:
        return
    st = record.get("episode_stats")
    run.last100.pairs.clear()
    if st is None:
        run.estats.reset()
        return
    run.estats.load_state(st["device"])
    for s_, c_ in st["last100"]:
        run.last100.add(s_, c_)


def driver_record(run, episode):
    """the driver's part of a whole-run snapshot taken with `episode` episodes finished"""
    return {"episode": episode, "expert_num": run.expert_num, "high_score": run.high_score, "success_rate": run.success_rate, "arttir": run.arttir,
            "seed": run.seed, "dtype": run.dtype, **run.dtype_mark, **stats_record(run)}


def adopt_record(run, record):
    """the driver scalars of a driver record (a fresh run's, or a loaded snapshot's); the throughput clock and the env counters' baseline start here"""
    run.expert_num, run.high_score, run.success_rate, run.arttir = record["expert_num"], record["high_score"], record["success_rate"], record["arttir"]
    run.episode = run.episode0 = record["episode"]
    run.t0, run.last_stats = time.time(), run.env.stats_dict()


def restore_or_explore(run):
    """--resume: this rank's shard of the snapshot; a fresh run: the reference's random exploration"""
    config, env, eng, inserter, estats, n = run.config, run.env, run.eng, run.inserter, run.estats, run.n
    record = {"episode": 0, "expert_num": run.batch if (run.hirl or run.esac) else 0, "high_score": -math.inf, "success_rate": 0.0, "arttir": 1}
    if config.resume:  # every rank restores its own shard: <resume>/state_rank<r>.pt
        record = CK.load_run(run.snap, eng, env, run.replay)
        restore_stats(run, record)
    else:
        # RANDOM EXPLORATION: 20 episodes of uniform actions in the reference (train_all.py:266-282) = 20*maxStep transitions
        env.reset()
        if inserter is not None:
            inserter.reset(env)
        if estats is not None:
            estats.reset()
        if getattr(run, "selfx", None) is not None:
            run.selfx.reset()
        for _ in range(math.ceil(20 * run.max_step / (n * run.world))):
            a0 = torch.rand((n, 4), device=run.device) * 2 - 1
            env.step(a0)
            if inserter is not None:
                inserter.push(env, a0)
            if estats is not None:
                estats.push()
            if getattr(run, "online", None) is not None:
                run.online.push()
            if getattr(run, "branch", None) is not None:
                run.branch.push()
            if getattr(run, "selfx", None) is not None:
                run.selfx.push(a0)
            if getattr(run, "upsampler", None) is not None:
                run.upsampler.mark_new(n if inserter is None else inserter.max_rows)
        if run.per and run.per_new == "td":  # the exploration rows are appended with an error of their own too (SAC/agent.py:176-177, 234-246: the start_steps rows are scored as well)
            eng.score_new(run.replay, math.ceil(20 * run.max_step / (n * run.world)) * n, seed=run.seed + 3 + run.rank)
        elif run.per:
            run.replay.mark_new()  # the exploration rows enter at the starting maximum priority
    run.snap = None  # (the snapshot's tensors are not kept for the length of the run)
    adopt_record(run, record)


def choose_loop(run):
    """which form the vector step takes, the "vector loop: ..." line, and the starting snapshot a front trip can go back to"""
    config, world, rank, sac = run.config, run.world, run.rank, run.sac
    run.actions = torch.zeros((run.n, 4), device=run.device)
    run.log_rate = 300  # train_all.py:208
    run.ret = torch.zeros(run.n, device=run.device) if config.log_rewards else None
    # --loop front (default where it applies: HIRL / TD3 in fp32 or bf16 actor + critic, SAC / E-SAC on one GPU at every number of envs — up to 8,192 the
    # per-tile acting role measured faster than the reference's order in every size class; batch <= 256, one update per step): the env
    # step and the first two launches of learn() (SAC: its first forward launch) as ONE launch (HirlEngine / SacEngine.step_learn) — the minibatch is then drawn from the ring as it stood before
    # this step's insert.  --loop reference: the reference's order on every step (act -> env step -> insert -> draw -> learn)
    # ... and only with ONE process per GPU: the in-launch waits of the front launch are argued for a chip of its own (include/hirl4ucav.h hx_hirl_front —
    # the waiting workgroups of processes that share a GPU add up; eight front-loop ranks on one GPU tripped in round 5).  HX_FRONT_SHARED_GPU=1 takes it
    # anyway (soak tests); the status word + fallback below stay armed either way.
    shared_gpu = world > torch.cuda.device_count() and not os.environ.get("HX_FRONT_SHARED_GPU")
    upsampled = tuple(flag for flag in ("buffer_upsample", "expert_upsample") if getattr(run, flag, False))  # the weighted draw is a launch behind the plain one
    run.front = (config.loop == "front" and not sac and not config.separate_launches and config.updates_per_step == 1 and run.batch <= 256
                 and getattr(config, "dtype", "f32") in ("f32", "f32x9", "bf16") and not shared_gpu and not upsampled and not getattr(run, "hirl_per", False)
                 and (run.inserter is None or run.n <= 8192))  # (--hirl_multi_step: the env has no ring, so the front launch acts per tile: up to 8,192 envs)
    run.front_sac = (config.loop == "front" and sac and world == 1 and not config.separate_launches and config.updates_per_step == 1 and run.batch <= 256 and not run.per
                     and run.grad_clip is None and run.inserter is None and getattr(run, "explore", None) is None)
    if rank == 0:
        which = "front launch (env step + first launches of learn() in one launch; draw before the insert)" if (run.front or run.front_sac) else "reference order"
        if run.per:  # the front loop draws before the step's insert: update_priority could then hit slots the step has overwritten
            which += f" ({'--hirl_per' if getattr(run, 'hirl_per', False) else '--per'}: the front launch draws before the step's insert, so the priorities of the drawn rows could be written into overwritten slots)"
        if run.inserter is not None and sac:  # the front launch's acting workgroups insert one-step rows themselves
            which += f" (--multi_step {run.multi_step}: the n-step rows are written by a launch of their own behind the acting launch)"
        if run.inserter is not None and not sac:  # HIRL / TD3: the front launch takes an env without a ring up to 8,192 envs (per-tile acting workgroups)
            which += (f" (--hirl_multi_step {run.multi_step}: the n-step rows are written by a launch of their own behind " +
                      ("the front launch's call; the minibatch is drawn before the previous step's rows" if run.front else "the acting launch") +
                      ("; more than 8,192 envs: the front launch's persistent and streaming acting roles need a ring in the env" if run.n > 8192 and config.loop == "front" else "") + ")")
        if upsampled:  # the front launch draws uniformly, inside the launch and before the step's insert
            which += f" ({' '.join('--' + flag for flag in upsampled)}: the upsampled draw is a launch of its own between the acting launch and learn(), after the step's insert)"
        if sac and run.grad_clip is not None and not run.per:  # the clipped update is the staged sequence (gradients -> norm -> clipped step): its first launch is its own
            which += " (--grad_clip: the clipped update runs as stages, which have no front form)"
        if sac and getattr(run, "explore", None) is not None:  # SacEngine.step_learn draws its eps in-kernel; act / act_step take the generator's
            which += (f" (--explore_noise {run.explore.params['kind']}: the coloured draws are the Gaussian head's eps, which act_step takes and the front "
                      "launch does not)")
        if not sac and run.grad_clip is not None:  # HIRL / TD3: the stages run behind the front launch as they do on a sharded rank
            which += (f" (--hirl_grad_clip {run.grad_clip:g}: the clipped update runs as stages" +
                      (" behind the front launch" if run.front else "") + ", a norm launch in front of each optimizer step)")
        print(f"vector loop: {which}" + (f" ({world} ranks share a GPU: the front launch is for one process per GPU)" if (shared_gpu and config.loop == "front") else ""),
              flush=True)
    # The front launch's in-launch waits (launch B for launch A's rows, launch C for both) assume that the workgroups of ONE launch start in index order —
    # observed on gfx950, promised by nobody.  A wait that gives up sets a sticky status word: it is read every --status_check_every vector steps (one host
    # sync; every rank takes the same decision), and on a trip every rank goes back to the newest snapshot and continues in the reference's order INSIDE this
    # process (--on_front_trip fallback, the default), or the run exits with code 3 (no snapshot yet, or --on_front_trip exit).
    run.check_every = max(int(config.status_check_every), 0)
    run.steps_since_check = 0
    run.snap_path = os.path.join(config.resume, f"state_rank{rank}.pt") if config.resume else None  # the newest whole-run snapshot this process can go back to
    if run.front and run.check_every and config.on_front_trip == "fallback" and config.snapshot_every and run.snap_path is None:
        # a trip before the first periodic snapshot would leave nothing to go back to: take one of the starting state (every rank its shard)
        write_snapshot(run, run.episode0)


def write_snapshot(run, episode):
    """whole-run state for --resume and for the way back after a front trip: one file per rank, `episode` episodes finished"""
    if run.world > 1:
        torch.distributed.barrier()  # every shard of a snapshot comes from the same episode ...
    path = os.path.join(run.log_dir, f"state_rank{run.rank}.pt")
    CK.save_run(path, run.eng, run.env, run.replay, driver_record(run, episode))
    if run.world > 1:
        torch.distributed.barrier()  # ... and nobody runs ahead while a shard is still being written
    run.snap_path = path


def branch_has_reader(run):
    """whether anything still draws from the expert ring: ISAC's expert batch for the whole run; HIRL's and E-SAC's expert rows only while expert_num > 0
    (train_all.py:356-357: one row fewer every warm_up_rate steps, 0 after batch * warm_up_rate vector steps, for good).  Behind that the branches would
    be written for nobody: the launch is dropped, the ring keeps what it holds."""
    return bool(run.isac) or run.expert_num > 0


# ---- the vector step: two hooks every form shares, three forms --------------------------------------------------------------------------------------
def after_env_step(run, step, pushed=False):
    """Behind every acting launch, in this order: the n-step rows, the episode statistics, the pilot's relabelled rows, the pilot's branches, the learner's own kill episodes, the new
    rows' first priorities, the reward sum.  (SAC's front form runs without an inserter, every front form without --per: choose_loop.)  pushed: the
    step's n-step rows are in the ring already — HirlEngine.step_learn pushes behind its own launches; one push per env step."""
    if run.inserter is not None and not pushed:
        run.inserter.push(run.env, run.actions)  # this step's finished n-step rows (at most multi_step * n of them)
    if run.estats is not None:
        run.estats.push()
    if getattr(run, "online", None) is not None:
        run.online.push()  # --expert_online: per_step envs relabelled by the pilot into the online region of bc_table (one launch, no host sync)
    if getattr(run, "branch", None) is not None and branch_has_reader(run):
        run.branch.push()  # --expert_branch: per_step envs flown one step by the pilot, in registers, into the online region of the expert ring (likewise)
    if getattr(run, "selfx", None) is not None and branch_has_reader(run):
        run.selfx.push(run.actions)  # --expert_self: the step goes onto the episode tape; kill episodes leave for the same region (two launches, no host sync)
    if run.per and run.per_new == "td":
        replay, n, writer = run.replay, run.n, run.writer
        log_new = writer is not None and step % run.log_rate == 0
        marked0 = replay.marked if log_new else 0  # (a host read, at the logging step only)
        run.eng.score_new(replay, n, seed=run.seed + 3 + run.rank)  # this step's rows enter at |Q1(s, a) - y| of their own (no host sync)
        if log_new:  # the mean over the rows this call covered (a step stores at most n)
            k = min(max(replay.marked - marked0, 1), n)
            writer.add_scalar("stats/per_mean_new_error", float(replay.errors[:k].mean()), step + run.episode * run.max_step)
    elif run.per:
        run.replay.mark_new(run.n if run.inserter is None else run.inserter.max_rows)  # this step's rows enter at the running maximum priority (one launch, no host sync)
    if getattr(run, "upsampler", None) is not None:
        run.upsampler.mark_new(run.n if run.inserter is None else run.inserter.max_rows)  # the blocks this step's rows fell into are recounted (one launch, no host sync)
    if run.ret is not None:
        run.ret += run.env.reward


def log_step_scalars(run, step):
    """Behind a step's learn(), every log_rate steps on rank 0.  (SAC's front form writes neither grad norms nor stats/per_*: it never runs with
    --grad_clip or --per, choose_loop; HIRL's and TD3's front form keeps its clip, --hirl_grad_clip, and writes their norms.)"""
    writer, eng = run.writer, run.eng
    if writer is None or step % run.log_rate != 0:
        return
    at = step + run.episode * run.max_step
    if not run.sac:  # Loss/* every 300 steps, train_all.py:362-367
        c_, a_, b_, r__, f_, _w = eng.losses_host()
        for tag, v in (("Loss/Critic_Loss", c_), ("Loss/Actor_Loss", a_), ("Loss/BC_Loss", b_), ("Loss/RL_Loss", r__), ("Loss/BC_Fire_Loss", f_)):
            writer.add_scalar(tag, v, at)
    if run.isac:  # SAC/agent.py:353-359
        log_imitative(writer, eng, at)
    if run.sac and run.grad_clip is not None:
        for tag, v in zip(("q1", "q2", "policy"), eng.grad_norms_host()[0]):
            writer.add_scalar("stats/grad_norm_" + tag, v, at)
    if not run.sac and run.grad_clip is not None:  # (the actor's norm is that of the last actor call: every second learn())
        for tag, v in zip(("critic", "actor"), eng.grad_norms_host()[0]):
            writer.add_scalar("stats/grad_norm_" + tag, v, at)
    if run.per:
        writer.add_scalar("stats/per_beta", run.replay.beta, at)
        writer.add_scalar("stats/per_max_priority", run.replay.pmax, at)


def explore_kw(run, key):
    """{key: this step's [n, 4] slice of the generator's chunk} under coloured noise or a ladder of scales; {} without a generator: the acting call is
    then word for word the one it was (Philox draws inside the acting kernel)"""
    gen = getattr(run, "explore", None)
    return {key: gen.next()} if gen is not None else {}


def step_front_hirl(run, step, w_now, warm):
    """HIRL / TD3: env step + the first two launches of learn() as one launch (HirlEngine.step_learn)"""
    run.expert_num = next_expert_num(run, step)
    run.eng.step_learn(run.env, run.expert, run.bc_table, n_main=run.batch - run.expert_num, **explore_kw(run, "act_noise"), act_sigma=getattr(run, "act_sigma", 0.1),
                       act_seed=run.seed + 1, out=run.actions, sample_seed=run.seed + 2 + run.rank, bc_weight_now=w_now, bc_warm_up_weight=warm)
    after_env_step(run, step, pushed=run.inserter is not None)
    log_step_scalars(run, step)


def step_front_sac(run, step):
    """SAC / E-SAC / ISAC: explore + env step + the first forward launch of learn() in one launch (SacEngine.step_learn); ISAC's expert batch rides in it"""
    run.expert_num = next_expert_num(run, step)
    run.eng.step_learn(run.env, run.expert if (run.esac or run.isac) else None, n_main=run.batch - run.expert_num, act_seed=run.seed + 1, out=run.actions,
                       sample_seed=run.seed + 2 + run.rank)
    after_env_step(run, step)
    log_step_scalars(run, step)


def step_reference(run, step, w_now, warm):
    """the reference's order: act -> env step -> insert -> draw -> learn (--updates_per_step times); an episode's last step only acts"""
    config, eng, env, seed, sac = run.config, run.eng, run.env, run.seed, run.sac
    noise = explore_kw(run, "eps" if sac else "noise")  # coloured noise: per-row additive noise (HIRL / TD3, noise_mode 2), the Gaussian head's eps (SAC)
    if config.separate_launches:  # chooseAction, then env.step: two launches
        eng.act(env.obs, **noise, seed=seed + 1, row0=env.env_id0, out=run.actions) if sac else eng.act(env.obs, **noise, sigma=getattr(run, "act_sigma", 0.1), seed=seed + 1, row0=env.env_id0, out=run.actions)
        env.step(run.actions)
    elif sac:                     # the same in ONE launch (identical values; only the order in which a step's rows enter the
        eng.act_step(env, **noise, seed=seed + 1, out=run.actions)     # replay ring depends on the workgroup schedule)
    else:
        eng.act_step(env, **noise, sigma=getattr(run, "act_sigma", 0.1), seed=seed + 1, out=run.actions)
    after_env_step(run, step)
    if step == run.max_step - 1:
        return
    run.expert_num = next_expert_num(run, step)
    n_main, sample_seed = run.batch - run.expert_num, seed + 2 + run.rank
    for _ in range(config.updates_per_step):
        if sac:  # train_sac.py:270-273 (SAC) / :401-403 (E-SAC: expert rows mixed in while expert_num > 0)
            eng.sample(run.replay, run.expert if run.esac else None, n_main=n_main, seed=sample_seed, defer=True)
            if run.isac:  # expert_memory.sample(batch_size), SAC/agent.py:392: the second batch, drawn inside learn() too
                eng.sample_expert(run.expert, seed=sample_seed, defer=True)
            eng.learn()
            continue
        eng.sample(run.replay, run.expert, run.bc_table, n_main=n_main, seed=sample_seed, defer=True)  # drawn inside learn()'s first launch
        eng.learn(bc_weight_now=w_now, bc_warm_up_weight=warm)
        w_now = None  # afterwards learn()'s own returned weight is fed back (train_all.py:361): the stored device value
    log_step_scalars(run, step)


def front_tripped(run):
    """the front launch's status word, the worst over the ranks (0: no in-launch wait gave up)"""
    code = run.eng.front_status()
    if run.world > 1:
        t = torch.tensor([code], dtype=torch.int32, device=run.device if torch.distributed.get_backend() == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        code = int(t.item())
    return code


def run_episode(run):
    """max_step vector steps, each in the form that applies -> the front launch's status word (non-zero: the episode was left at that read)"""
    config, max_step = run.config, run.max_step
    w_now, warm = bc_weight_schedule(config.type, run.episode, config.bc_weight) if run.hirl else (0.0, 0.0)
    front = run.front  # (read every episode: a trip turns it off)
    for step in range(max_step):
        if front and run.check_every:
            run.steps_since_check += 1
            if run.steps_since_check >= run.check_every:
                run.steps_since_check = 0
                tripped = front_tripped(run)
                if tripped:
                    return tripped
        if front and step < max_step - 1:  # (the last step of an episode has no learn() behind it, train_all.py:346-347: it only acts)
            step_front_hirl(run, step, w_now, warm)
        elif run.front_sac and step < max_step - 1:
            step_front_sac(run, step)
        else:
            step_reference(run, step, w_now, warm)
        w_now = None  # given to an episode's first learn(); afterwards learn()'s own returned weight is fed back (train_all.py:361): the stored device value
    return front_tripped(run) if front else 0  # ... and at every episode's end: nothing of a tripped episode reaches a validation, a checkpoint or a snapshot


def roll_back(run, tripped):
    """An in-launch wait of the front launch gave up: back to the newest snapshot and on in the reference's order, or exit code 3"""
    config, eng, rank, snap_path = run.config, run.eng, run.rank, run.snap_path
    why = (f"front launch: an in-launch wait gave up (status word {tripped}: " + " and ".join(w for b_, w in ((1, "launch B waiting for launch A's rows"),
           (2, "launch C waiting for launches A / B")) if tripped & b_) + f") in episode {run.episode + 1} — the minibatches read since the last check are suspect")
    if config.on_front_trip != "fallback" or snap_path is None or not os.path.exists(snap_path):
        if rank == 0:
            print(why + "; " + ("--on_front_trip exit" if config.on_front_trip != "fallback" else "no snapshot to go back to (--snapshot_every)") +
                  ": stopping.  `--loop reference` runs the same update without in-launch waits", flush=True)
        raise SystemExit(3)
    record = CK.load_run(snap_path, eng, run.env, run.replay)  # every rank its own shard; all shards of a snapshot come from the same episode
    restore_stats(run, record)
    eng.front_reset()
    adopt_record(run, record)
    run.front = False
    if run.ret is not None:
        run.ret.zero_()
    if rank == 0:
        print(why + f": back to the snapshot of episode {run.episode} ({snap_path}), continuing in the REFERENCE's order (no in-launch waits)", flush=True)
        if run.dtype == "f32" and eng.front_x9 and (eng.x9_rows is None or run.n < eng.x9_rows):  # [ADVICE r5] say what else changes with the loop
            print(f"note: the front launch acted in the exact-split format at every size; in the reference's order {run.n} envs act on fp32 MFMA "
                  f"(the split applies from {eng.x9_rows} rows on): fp32 results up to summation order from here on", flush=True)
        print(f"note: scalars and checkpoints written for episodes {run.episode + 1}.. before the trip are written again from here", flush=True)
        if run.writer is not None:
            run.writer.add_scalar("Others/Front_trip_rollback_to_episode", run.episode, run.episode)


# ---- an episode's end ---------------------------------------------------------------------------------------------------------------------------------
def log_scenario_stats(run):
    """the env episodes that ended during this driver episode, by scenario (one device-to-host copy, then the partials are cleared)"""
    if run.estats is None:
        return
    by_scenario = run.estats.read_and_clear()
    log_episode_stats(run.writer, run.episode, by_scenario, run.last100)
    if run.rank == 0:
        print(f"Episode {run.episode + 1}: " + " | ".join(f"{k} ended {v['count']} (done {v['done']}, time limit {v['time_limit']}) return {v['mean']:.2f} "
                                                          f"length {v['mean_len']:.1f}" for k, v in by_scenario.items() if v["count"]), flush=True)


def log_episode(run):
    """rank 0: the `Episode N:` line, Training/* and Others/*"""
    if run.rank != 0:
        return
    episode, writer, ret = run.episode, run.writer, run.ret
    c, a, b, r_, f, w = run.eng.losses_host()
    st = run.env.stats_dict()
    sps = (episode + 1 - run.episode0) * run.max_step * run.n * run.world / (time.time() - run.t0)
    names = ("q1", "q2", "policy", "entropy_loss", "alpha") if run.sac else ("critic", "actor", "bc", "rl", "bc_weight")
    print(f"Episode {episode + 1}: " + " ".join(f"{k} {v:.4f}" for k, v in zip(names, (c, a, b, r_, w))) + f" | episodes {st['episodes']} "
          f"kills {st['kills']} fire-success {st['fire_success_episodes']} | {sps:,.0f} env steps/s", flush=True)
    if writer is not None:  # Training/* per episode, train_all.py:383-388: rates over the env episodes that ENDED during this driver episode
        ended = max(st["episodes"] - run.last_stats["episodes"], 1)
        writer.add_scalar("Training/Last 50 Episode Train success rate", (st["kills"] - run.last_stats["kills"]) / ended, episode)
        writer.add_scalar("Training/Last 50 Episode Fire success rate", (st["fire_success_episodes"] - run.last_stats["fire_success_episodes"]) / ended, episode)
        writer.add_scalar("Others/BC_weight", w, episode)
        writer.add_scalar("Others/Nonfinite_actions", st.get("nonfinite_actions", 0), episode)
        if getattr(run, "online", None) is not None:
            writer.add_scalar("Expert/Online Rows Written", run.online.rows_written(), episode)  # (host arithmetic: no device read)
        if getattr(run, "branch", None) is not None:
            writer.add_scalar("Expert/Branch Rows Written", run.branch.rows_written(), episode)  # (likewise)
            if run.branch.steps > 1:  # the resident flights' own counters: one device-to-host copy per driver episode
                _, ended_rows, kill_rows = run.branch.counters()
                writer.add_scalar("Expert/Branch Episodes Ended", ended_rows, episode)
                writer.add_scalar("Expert/Branch Kills", kill_rows, episode)
        if getattr(run, "selfx", None) is not None:  # the device counters: one device-to-host copy per driver episode
            for tag, v in zip(("Kills", "Episodes Written", "Rows Written", "Episodes Dropped"), run.selfx.counters()):
                writer.add_scalar("Expert/Self " + tag, v, episode)
        if ret is not None:
            tot = float(ret.mean())
            writer.add_scalar("Training/Episode Reward", tot, episode)
            writer.add_scalar("Training/Average Step Reward", tot / run.max_step, episode)
            ret.zero_()
        run.last_stats = st


def validate_and_checkpoint(run):
    """rank 0: VALIDATION, train_all.py:400-402 / train_sac.py:431-433, and the checkpoint where the reference's rule asks for one"""
    config, eng, episode, arttir = run.config, run.eng, run.episode, run.arttir
    (mean, std, succ, fire), val_by_scenario, recs = validate_env(config, eng, run.env_type, run.max_step, run.seed + 12345, run.device, run.sac)
    val_n = 50 * len(val_by_scenario)  # (mixed: the pooled episodes of the three scenarios)
    if mean > run.high_score or succ / val_n >= run.success_rate or arttir % 5 == 0:
        tag = checkpoint_tag(arttir, succ, val_n, mean)
        write_validation_plots(recs, run.plot_dir, arttir)  # train_all.py:70-89: the last validation episode's track, only beside a checkpoint
        if run.sac:  # SacAgent.save_models, SAC/agent.py:440-444
            eng.save_models(run.model_dir, tag)
        else:    # Agent.saveCheckpoints, HIRL.py:336-342
            CK.save_hirl_nets(eng, run.model_dir, tag)
        run.high_score, run.success_rate = max(run.high_score, mean), max(run.success_rate, succ / val_n)
    print(f"Validation {arttir}: avg reward {mean:.2f} (std {std:.2f}) success {succ / val_n:.2f} fire success {fire / val_n:.2f}", flush=True)
    if len(val_by_scenario) > 1:
        for k_, (m_, s_, k2_, f_) in val_by_scenario.items():
            print(f"  {k_}: avg reward {m_:.2f} (std {s_:.2f}) success {k2_ / 50:.2f} fire success {f_ / 50:.2f}", flush=True)
    log_validation_by_scenario(run.writer, episode, val_by_scenario)
    log_validation(run.writer, episode, mean, std, succ / val_n, fire / val_n)
    run.arttir += 1


def check_replicas(run):
    """sharded run: the replicas must not have drifted apart"""
    mine = torch.tensor([run.eng.replica_checksum()], dtype=torch.int64, device=run.device)
    every = [torch.zeros_like(mine) for _ in range(run.world)]
    torch.distributed.all_gather(every, mine)
    if any(int(c.item()) != int(mine.item()) for c in every):
        raise RuntimeError(f"rank {run.rank}: network replicas diverged at episode {run.episode + 1}")


def main(config):
    run = start_run(config)
    if config.agent == "BC":
        return train_bc(config, run.device, run.seed, run.max_step)
    for phase in (check_agent_flags, build_env, build_engine, load_expert_tables, set_dtype, open_run_dir, build_explore, restore_or_explore, choose_loop):
        phase(run)
    while run.episode < config.episodes:
        tripped = run_episode(run)
        if tripped:
            roll_back(run, tripped)
            continue
        log_scenario_stats(run)
        log_episode(run)
        done = run.episode + 1
        validation_due = done % config.checkpoint_rate == 0
        if validation_due and run.rank == 0:
            validate_and_checkpoint(run)
        if run.world > 1 and (validation_due or (config.replica_check_every and done % config.replica_check_every == 0)):
            check_replicas(run)
        if config.snapshot_every and done % config.snapshot_every == 0:
            write_snapshot(run, done)
        run.episode += 1
    if run.writer is not None:
        run.writer.close()
    if run.world > 1:
        torch.distributed.destroy_process_group()
    return run.log_dir


def log_imitative(writer, eng, at):
    """loss/bc and loss/bc_weight of the imitative SAC branch (SAC/agent.py:353-359)"""
    bc_loss, bc_weight = eng.imitative_losses_host()
    writer.add_scalar("loss/bc", bc_loss, at)
    writer.add_scalar("loss/bc_weight", bc_weight, at)


def isac_refusal(config, world=1):
    """why `--agent SAC --type ISAC` cannot run as asked, or None"""
    if config.agent != "SAC" or config.type != "ISAC":
        return None
    if getattr(config, "dtype", "f32") != "f32":
        return f"--type ISAC with --dtype {config.dtype}: the imitative branch is fp32 only (its kernels have no bf16 form): drop --dtype"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--type ISAC runs on one GPU (the gate's count is not exchanged between ranks): use --gpus 1"
    if not config.bc_actor:
        return "--type ISAC needs --bc_actor FILE: the frozen actor a `--agent BC` run writes"
    if not config.expert_csv and not getattr(config, "synthetic_expert", False):
        return "--type ISAC needs an expert table: --expert_csv FILE or --synthetic_expert"
    return None


def per_refusal(config, world=1):
    """why `--per` / `--per_new` cannot run as asked, or None"""
    if not getattr(config, "per", False):
        if getattr(config, "per_new", "max") != "max":
            return f"--per_new {config.per_new} goes with --per (it says how the rows of prioritized replay get their first priority): add --per"
        return None
    if config.agent != "SAC":
        return f"--per goes with --agent SAC --type SAC (prioritized replay is SacAgent's: SAC/agent.py:112-118), not --agent {config.agent}"
    if config.type == "ESAC":
        return "--per with --type ESAC: the reference's learn() drops the expert rows when per is on (SAC/agent.py:281-284): use --type SAC"
    if config.type == "ISAC":
        return "--per with --type ISAC: prioritized replay with the imitative branch is not built: use --type SAC"
    if config.type != "SAC":
        return f"--per goes with --agent SAC --type SAC, not --type {config.type}"
    if getattr(config, "dtype", "f32") != "f32":
        return f"--per with --dtype {config.dtype}: the weighted update is fp32 only (its kernels have no bf16 form): drop --dtype"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--per runs on one GPU (priorities and block sums are not exchanged between ranks): use --gpus 1"
    return None


def nstep_refusal(config, world=1):
    """why `--multi_step` cannot run as asked, or None"""
    n = getattr(config, "multi_step", 1)
    if n == 1:
        return None
    if not 2 <= n <= 8:
        return f"--multi_step {n}: the number of steps is 1 (off) or 2..8"
    if config.agent != "SAC":
        return (f"--multi_step goes with --agent SAC (n-step returns are SacAgent's: SAC/agent.py:121-124), not --agent {config.agent}" +
                (": HIRL and TD3 have --hirl_multi_step N" if config.agent in ("HIRL", "TD3") else ""))
    if config.type == "ISAC":
        return "--multi_step with --type ISAC: n-step returns with the imitative branch are not built: use --type SAC or ESAC"
    if config.type not in ("SAC", "ESAC"):
        return f"--multi_step goes with --agent SAC --type SAC | ESAC, not --type {config.type}"
    if getattr(config, "per_new", "max") != "max":
        return f"--multi_step with --per_new {config.per_new}: scoring n-step rows at insert is not built: use --per_new max"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--multi_step runs on one GPU (the per-env windows are not built for sharded ranks): use --gpus 1"
    return None


def upsample_refusal(config, world=1, n_fire=None):
    """why `--buffer_upsample` / `--expert_upsample` cannot run as asked, or None.  n_fire: the fire rows of the expert table, once it has been read"""
    buf, exp = getattr(config, "buffer_upsample", False), getattr(config, "expert_upsample", False)
    if not buf and not exp:
        return None
    flag = "--buffer_upsample" if buf else "--expert_upsample"
    if config.agent == "SAC":
        return (f"{flag} goes with --agent HIRL | TD3{'' if buf else ' | BC'} (the two switches are the HIRL agent's: HIRL.py:184-185; SacAgent has --per), "
                "not --agent SAC")
    if buf and config.agent == "BC":
        return "--buffer_upsample goes with --agent HIRL | TD3 (BC has no replay ring); --expert_upsample is BC's switch (BC.py:152-158)"
    if exp and config.agent == "TD3":
        return "--expert_upsample goes with --agent HIRL | BC (TD3 reads no expert table)"
    if (config.gpus and config.gpus > 1) or world > 1:
        return f"{flag} runs on one GPU (the draw is rank-local and untested on sharded ranks): use --gpus 1"
    boost = getattr(config, "upsample_boost", 10)
    if buf and not 2 <= boost <= 255:
        return f"--upsample_boost {boost}: the weight of a success row against 1 is 2..255 (10 = the reference's 1.0 : 0.1)"
    if exp and n_fire is not None and n_fire == 0:
        return "--expert_upsample: the expert table holds no row whose fire action is 1 (target_indices would be empty: HIRL.py:217-219)"
    return None


def expert_online_refusal(config, world=1):
    """why `--expert_online` / `--expert_online_per_step` cannot run as asked, or None"""
    rows, k = int(getattr(config, "expert_online", 0)), int(getattr(config, "expert_online_per_step", 64))
    if rows == 0:
        return None
    if rows < 0:
        return f"--expert_online {rows}: the rows of the online region, 0 (off) or more"
    if config.agent == "SAC":
        return (f"--expert_online goes with --agent HIRL (SAC / ESAC / ISAC draw expert TRANSITIONS from the labelled ring, not from the BC table, and "
                f"relabelling r, s' and done there is not built), not --agent SAC --type {config.type}")
    if config.agent == "TD3":
        return "--expert_online goes with --agent HIRL (TD3 reads no expert table)"
    if config.agent == "BC":
        return "--expert_online goes with --agent HIRL (--agent BC has no rollouts whose states the pilot could label)"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--expert_online runs on one GPU (the refresh is rank-local and untested on sharded ranks): use --gpus 1"
    if not 1 <= k <= min(rows, int(config.num_envs)):
        return (f"--expert_online_per_step {k}: 1 <= rows per step <= min(--expert_online, --num_envs) = {min(rows, int(config.num_envs))} (the picks of a step "
                "are distinct envs and distinct slots)")
    return None


def expert_online_resume_refusal(config, driver):
    """why a snapshot's driver record cannot be resumed under this run's --expert_online / --expert_online_per_step, or None (driver None: a fresh run)"""
    if driver is None:
        return None
    was = driver.get("expert_online")
    was_rows, was_k = (int(was["online_rows"]), int(was["per_step"])) if was is not None else (0, None)
    rows, k = int(getattr(config, "expert_online", 0)), int(getattr(config, "expert_online_per_step", 64))
    if was_rows != rows:
        return f"was run with --expert_online {was_rows}, --expert_online {rows} given"
    if rows and was_k != k:
        return f"was run with --expert_online_per_step {was_k}, --expert_online_per_step {k} given"
    return None


def expert_branch_refusal(config, world=1):
    """why `--expert_branch` / `--expert_branch_per_step` / `--expert_branch_steps` cannot run as asked, or None"""
    rows, k = int(getattr(config, "expert_branch", 0)), int(getattr(config, "expert_branch_per_step", 64))
    steps = int(getattr(config, "expert_branch_steps", 1))
    if not 1 <= steps <= 65535:
        return f"--expert_branch_steps {steps}: the steps of a resident branch, 1 (one step per pick) to 65,535 (the episode counter's range)"
    if rows <= 0 and steps != 1:
        return f"--expert_branch_steps {steps} goes with --expert_branch ROWS > 0 (there are no branches to fly without it)"
    if rows == 0:
        return None
    if rows < 0:
        return f"--expert_branch {rows}: the rows of the expert ring's online region, 0 (off) or more"
    takes = "--expert_branch goes with --agent HIRL, --agent SAC --type ESAC and --agent SAC --type ISAC"
    if config.agent == "SAC" and config.type not in ("ESAC", "ISAC"):
        return f"{takes} (--agent SAC --type {config.type} reads no expert ring)"
    if config.agent == "TD3":
        return f"{takes} (TD3 reads no expert ring)"
    if config.agent == "BC":
        return f"{takes} (--agent BC reads no expert ring and has no rollouts the pilot could branch from)"
    if getattr(config, "per", False):
        return "--expert_branch does not go with --per (the weighted call drops the expert rows: the branch rows would never be drawn)"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--expert_branch runs on one GPU (the branches are rank-local and untested on sharded ranks): use --gpus 1"
    if not 1 <= k <= min(rows, int(config.num_envs)):
        return (f"--expert_branch_per_step {k}: 1 <= rows per step <= min(--expert_branch, --num_envs) = {min(rows, int(config.num_envs))} (the picks of a step "
                "are distinct envs and distinct slots)")
    return None


def expert_branch_resume_refusal(config, driver):
    """why a snapshot's driver record cannot be resumed under this run's --expert_branch / --expert_branch_per_step, or None (driver None: a fresh run)"""
    if driver is None:
        return None
    was = driver.get("expert_branch")
    was_rows, was_k = (int(was["online_rows"]), int(was["per_step"])) if was is not None else (0, None)
    rows, k = int(getattr(config, "expert_branch", 0)), int(getattr(config, "expert_branch_per_step", 64))
    if was_rows != rows:
        return f"was run with --expert_branch {was_rows}, --expert_branch {rows} given"
    if rows and was_k != k:
        return f"was run with --expert_branch_per_step {was_k}, --expert_branch_per_step {k} given"
    was_steps, steps = (int(was.get("steps", 1)) if was is not None else 1), int(getattr(config, "expert_branch_steps", 1))
    if rows and was_steps != steps:
        return f"was run with --expert_branch_steps {was_steps}, --expert_branch_steps {steps} given"
    return None


def expert_self_refusal(config, world=1):
    """why `--expert_self` / `--expert_self_steps` / `--expert_self_bc` cannot run as asked, or None"""
    rows, steps, bc = int(getattr(config, "expert_self", 0)), int(getattr(config, "expert_self_steps", 256)), bool(getattr(config, "expert_self_bc", False))
    if rows == 0:
        if bc:
            return "--expert_self_bc goes with --expert_self ROWS > 0 (there are no self rows to mirror without it)"
        return None
    if rows < 0:
        return f"--expert_self {rows}: the rows of the expert ring's online region, 0 (off) or more"
    if not 1 <= steps <= 65535:
        return f"--expert_self_steps {steps}: the steps of an episode the tape keeps, 1 to 65,535 (the episode counter's range)"
    takes = "--expert_self goes with --agent HIRL, --agent SAC --type ESAC and --agent SAC --type ISAC"
    if config.agent == "SAC" and config.type not in ("ESAC", "ISAC"):
        return f"{takes} (--agent SAC --type {config.type} reads no expert ring)"
    if config.agent == "TD3":
        return f"{takes} (TD3 reads no expert ring)"
    if config.agent == "BC":
        return f"{takes} (--agent BC reads no expert ring and has no rollouts whose kills could be kept)"
    if int(getattr(config, "expert_branch", 0)) > 0:
        return "--expert_self does not go with --expert_branch (both want the online region of the expert ring): drop one of the two"
    if bc and config.agent != "HIRL":
        return "--expert_self_bc goes with --agent HIRL (SAC / ESAC / ISAC read no BC table)"
    if bc and int(getattr(config, "expert_online", 0)) > 0:
        return "--expert_self_bc does not go with --expert_online (both want the online region of the BC table): drop one of the two"
    if getattr(config, "per", False):
        return "--expert_self does not go with --per (the weighted call drops the expert rows: the self rows would never be drawn)"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--expert_self runs on one GPU (the tape is rank-local and untested on sharded ranks): use --gpus 1"
    if steps > rows:
        return f"--expert_self_steps {steps} > --expert_self {rows}: an episode of L rows must fit into the online region (L <= ROWS)"
    return None


def expert_self_resume_refusal(config, driver):
    """why a snapshot's driver record cannot be resumed under this run's --expert_self / --expert_self_steps / --expert_self_bc, or None (driver None: a
    fresh run)"""
    if driver is None:
        return None
    was = driver.get("expert_self")
    was_rows, was_steps, was_bc = (int(was["online_rows"]), int(was["steps"]), bool(was["bc"])) if was is not None else (0, None, False)
    rows, steps, bc = int(getattr(config, "expert_self", 0)), int(getattr(config, "expert_self_steps", 256)), bool(getattr(config, "expert_self_bc", False))
    if was_rows != rows:
        return f"was run with --expert_self {was_rows}, --expert_self {rows} given"
    if rows and was_steps != steps:
        return f"was run with --expert_self_steps {was_steps}, --expert_self_steps {steps} given"
    if rows and was_bc != bc:
        return f"was run {'with' if was_bc else 'without'} --expert_self_bc, this run is {'with' if bc else 'without'} it"
    return None


def expert_floor_refusal(config, world=1):
    """why `--expert_floor` cannot run as asked, or None"""
    floor = int(getattr(config, "expert_floor", 0))
    if floor == 0:
        return None
    if not 0 <= floor <= BATCH:
        return f"--expert_floor {floor}: the expert rows of a minibatch that stay after the warm-up, 0 (off) to the batch of {BATCH}"
    takes = "--expert_floor goes with --agent HIRL and --agent SAC --type ESAC"
    if config.agent == "SAC" and config.type != "ESAC":
        return f"{takes} (--agent SAC --type {config.type} mixes no expert rows into its minibatch: there is no expert_num to hold)"
    if config.agent in ("TD3", "BC"):
        return f"{takes} (--agent {config.agent} mixes no expert rows into its minibatch: there is no expert_num to hold)"
    if getattr(config, "per", False):
        return "--expert_floor does not go with --per (the weighted call drops the expert rows)"
    return None


def expert_floor_resume_refusal(config, driver):
    """why a snapshot's driver record cannot be resumed under this run's --expert_floor, or None (driver None: a fresh run)"""
    if driver is None:
        return None
    was, floor = int(driver.get("expert_floor", 0)), int(getattr(config, "expert_floor", 0))
    if was != floor:
        return f"was run with --expert_floor {was}, --expert_floor {floor} given"
    return None


EXPLORE_FLAGS = (("explore_noise", "white"), ("explore_tau", 16.0), ("explore_octaves", 6), ("explore_sigma", 0.1), ("explore_sigma_max", None), ("explore_chunk", 16))


def explore_settings(config):
    """the six --explore_* values of a config (a namespace from before the flags has the defaults)"""
    return {k: getattr(config, k, default) for k, default in EXPLORE_FLAGS}


def explore_uses_generator(config):
    """whether the action noise comes from utils.noise.ColoredNoise: any colour but white, or a ladder of scales"""
    e = explore_settings(config)
    return e["explore_noise"] != "white" or e["explore_sigma_max"] is not None


def explore_refusal(config, world=1):
    """why the `--explore_*` flags cannot run as asked, or None.  Every --dtype, both loop forms of HIRL / TD3, any number of envs and --gpus N are fine
    (each rank has its own generator, keyed by its envs' ids)."""
    e = explore_settings(config)
    given = [k for k, default in EXPLORE_FLAGS if e[k] != default]
    if not given:
        return None
    noise, tau, octaves, sigma, sigma_max, chunk = (e[k] for k, _ in EXPLORE_FLAGS)
    if config.agent == "BC":
        return f"--{given[0]} goes with --agent HIRL, TD3 or SAC, not --agent BC (behaviour cloning never acts while it trains)"
    if not (math.isfinite(tau) and tau > 0):
        return f"--explore_tau {tau:g}: the OU process's correlation time in vector steps, > 0"
    if not 1 <= octaves <= 8:
        return f"--explore_octaves {octaves}: the poles of the 1 / f bank, 1..8"
    if not 1 <= chunk <= 64:
        return f"--explore_chunk {chunk}: the vector steps of one generator launch, 1..64"
    if tau != 16.0 and noise != "ou":
        return "--explore_tau goes with --explore_noise ou"
    if octaves != 6 and noise != "pink":
        return "--explore_octaves goes with --explore_noise pink"
    if config.agent == "SAC" and (sigma != 0.1 or sigma_max is not None):
        return ("--explore_sigma / --explore_sigma_max go with --agent HIRL or TD3: SAC's noise scale is the policy's own log-std (the generator feeds the "
                "Gaussian head unit-variance eps)")
    if not (math.isfinite(sigma) and sigma >= 0):
        return f"--explore_sigma {sigma:g}: the action noise's standard deviation, >= 0"
    if sigma_max is not None and not (math.isfinite(sigma_max) and 0 < sigma <= sigma_max):
        return f"--explore_sigma_max {sigma_max:g} with --explore_sigma {sigma:g}: the ladder runs from --explore_sigma > 0 up to --explore_sigma_max >= it"
    if chunk != 16 and not explore_uses_generator(config):
        return "--explore_chunk goes with --explore_noise ou or pink, or --explore_sigma_max (white noise of one scale is drawn inside the acting kernels)"
    return None


def explore_resume_refusal(config, driver):
    """why a snapshot's driver record cannot be resumed under this run's --explore_* flags, or None (driver None: a fresh run; a record from before the
    flags was run with their defaults)"""
    if driver is None:
        return None
    was, now = {**dict(EXPLORE_FLAGS), **driver.get("explore", {}).get("flags", {})}, explore_settings(config)
    for k, _ in EXPLORE_FLAGS:
        if was[k] != now[k]:
            return f"was run with --{k} {was[k]}, --{k} {now[k]} given: resume with the flag the run was started with"
    return None


def clip_refusal(config, world=1):
    """why `--grad_clip` / `--fixed_alpha` cannot run as asked, or None"""
    clip, fixed = getattr(config, "grad_clip", None), getattr(config, "fixed_alpha", None)
    if clip is None and fixed is None:
        return None
    flag = "--grad_clip" if clip is not None else "--fixed_alpha"
    if config.agent != "SAC":
        return (f"{flag} goes with --agent SAC (gradient clipping and the fixed entropy coefficient are SacAgent's: SAC/agent.py:108-110, 310-320), "
                f"not --agent {config.agent}" + (": HIRL and TD3 clip with --hirl_grad_clip C" if clip is not None and config.agent in ("HIRL", "TD3") else ""))
    if clip is not None and not (clip > 0 and math.isfinite(clip)):
        return f"--grad_clip {clip}: the maximum gradient norm is a positive number"
    if fixed is not None and not (fixed >= 0 and math.isfinite(fixed)):
        return f"--fixed_alpha {fixed}: the entropy coefficient is a number >= 0"
    if clip is not None and ((config.gpus and config.gpus > 1) or world > 1):
        return "--grad_clip runs on one GPU (the norm is taken over one rank's gradient, before any exchange): use --gpus 1"
    return None


def hirl_clip_refusal(config, world=1):
    """why `--hirl_grad_clip` cannot run as asked, or None.  (A flag of its own: `--grad_clip` is SacAgent's keyword and stays refused for every other
    agent.)  HirlEngine.set_grad_clip puts the clip into the stages of the update, behind any exchange: both loop forms, every --dtype, any number of ranks."""
    clip = getattr(config, "hirl_grad_clip", None)
    if clip is None:
        return None
    if config.agent == "BC":
        return ("--hirl_grad_clip goes with --agent HIRL or TD3, not --agent BC (behaviour cloning steps its actor inside ONE fused call, hx_bc_train_actor: "
                "there is no launch boundary between its gradient and its step for a norm to sit at)")
    if config.agent not in ("HIRL", "TD3"):
        return f"--hirl_grad_clip goes with --agent HIRL or TD3, not --agent {config.agent}: SAC clips with --grad_clip C (SacAgent(grad_clip=C))"
    if not (clip > 0 and math.isfinite(clip)):
        return f"--hirl_grad_clip {clip}: the maximum gradient norm is a positive number"
    return None


def hirl_per_refusal(config, world=1):
    """why `--hirl_per` cannot run as asked, or None.  (A flag of its own: `--per` is SacAgent's keyword and stays refused for every other agent.)
    HirlEngine.set_prioritized: every --type, --dtype bf16, --hirl_grad_clip, --expert_floor / --expert_branch* / --expert_online, --env mixed and
    --separate_launches are fine; the vector loop takes the reference's order (choose_loop)."""
    if not getattr(config, "hirl_per", False):
        return None
    if config.agent == "SAC":
        return "--hirl_per goes with --agent HIRL or TD3, not --agent SAC: SAC has --per (SacAgent(per=True))"
    if config.agent == "BC":
        return "--hirl_per goes with --agent HIRL or TD3, not --agent BC (behaviour cloning draws from the expert table alone: there is no replay ring to prioritize)"
    if config.agent not in ("HIRL", "TD3"):
        return f"--hirl_per goes with --agent HIRL or TD3, not --agent {config.agent}"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--hirl_per runs on one GPU (priorities and block sums are not exchanged between ranks): use --gpus 1"
    for flag in ("buffer_upsample", "expert_upsample"):
        if getattr(config, flag, False):
            return f"--hirl_per does not go with --{flag} (both redraw the same rows of the minibatch; untested together): drop one of the two"
    if int(getattr(config, "buffer_size", 0)) > (1 << 24):
        return f"--hirl_per with --buffer_size {config.buffer_size}: prioritized replay holds at most 2^24 = 16,777,216 slots (the sampler scans 16,384 block sums)"
    return None


def hirl_multi_step_refusal(config, world=1):
    """why `--hirl_multi_step` cannot run as asked, or None.  (A flag of its own: `--multi_step` is SacAgent's keyword and stays refused for every other
    agent.)  HirlEngine.set_multi_step: every --type and --dtype, --separate_launches, --hirl_grad_clip, --hirl_per, --buffer_upsample / --expert_upsample,
    --expert_floor, --expert_online, --expert_branch[_steps] (branch rows stay one-step rows) and --env mixed are fine."""
    n = int(getattr(config, "hirl_multi_step", 1))
    if n == 1:
        return None
    if config.agent == "SAC":
        return "--hirl_multi_step goes with --agent HIRL or TD3, not --agent SAC: SAC has --multi_step (SacAgent(multi_step=N))"
    if config.agent == "BC":
        return "--hirl_multi_step goes with --agent HIRL or TD3, not --agent BC (behaviour cloning has no replay ring and no TD target)"
    if config.agent not in ("HIRL", "TD3"):
        return f"--hirl_multi_step goes with --agent HIRL or TD3, not --agent {config.agent}"
    if not 2 <= n <= 8:
        return f"--hirl_multi_step {n}: the number of steps is 1 (off) or 2..8"
    if (config.gpus and config.gpus > 1) or world > 1:
        return "--hirl_multi_step runs on one GPU (the per-env windows are rank-local and untested on sharded ranks): use --gpus 1"
    if int(getattr(config, "buffer_size", 0)) < n * int(config.num_envs):
        return (f"--hirl_multi_step {n} with --buffer_size {config.buffer_size}: one step can store N * --num_envs = {n * int(config.num_envs)} rows: "
                "use a larger --buffer_size")
    return None


def hirl_multi_step_resume_refusal(config, snap):
    """why a snapshot cannot be resumed under this run's --hirl_multi_step, or None (snap None: a fresh run)"""
    if snap is None or config.agent not in ("HIRL", "TD3"):
        return None
    was = int(snap["engine"]["multi_step"]["n"]) if "multi_step" in snap["engine"] else 1
    now = int(getattr(config, "hirl_multi_step", 1))
    if was != now:
        return f"was run with --hirl_multi_step {was}, --hirl_multi_step {now} given: resume with the flag the run was started with"
    return None


def hirl_per_resume_refusal(config, snap):
    """why a snapshot cannot be resumed under this run's --hirl_per, or None (snap None: a fresh run)"""
    if snap is None:
        return None
    was, now = bool(snap["engine"].get("prioritized", False)), bool(getattr(config, "hirl_per", False))
    if was != now and config.agent in ("HIRL", "TD3"):
        return f"was run {'with' if was else 'without'} --hirl_per, this run is {'with' if now else 'without'} it: resume with the flag the run was started with"
    return None


def parse_args(argv=None):
    """parser().parse_args with the cross-flag checks that are argparse errors"""
    p = parser()
    cfg = p.parse_args(argv)
    why = per_refusal(cfg) or hirl_per_refusal(cfg) or clip_refusal(cfg) or hirl_clip_refusal(cfg) or nstep_refusal(cfg) or hirl_multi_step_refusal(cfg) or mixed_refusal(cfg) or upsample_refusal(cfg) or expert_online_refusal(cfg) or expert_branch_refusal(cfg) or expert_self_refusal(cfg) or expert_floor_refusal(cfg) or explore_refusal(cfg)
    if why:
        p.error(why)
    if cfg.type == "ISAC" and cfg.agent != "SAC":
        p.error("--type ISAC goes with --agent SAC")
    why = isac_refusal(cfg)
    if why:
        p.error(why)
    return cfg


def parser():
    p = argparse.ArgumentParser()  # the reference's flags, train_all.py:489-513
    p.add_argument("--agent", type=str, default="HIRL", choices=["HIRL", "TD3", "BC", "SAC"])  # SAC: the train_sac.py path (D2)
    p.add_argument("--port", type=int, default=None)
    p.add_argument("--type", type=str, default="soft", choices=["soft", "linear", "fixed", "SAC", "ESAC", "ISAC"])  # SAC / ESAC: train_sac.py:440-458; ISAC: SacAgent(imitative=True)
    p.add_argument("--bc_weight", type=float, default=0.5)
    p.add_argument("--model_name", type=str, default="model")
    p.add_argument("--load_model", action="store_true")
    p.add_argument("--render", action="store_true")
    p.add_argument("--plot", action="store_true")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--env", type=str, default="straight_line", choices=list(SCENARIOS) + [MIXED],
                   help="mixed (an extension): one population over all three scenarios in contiguous thirds (mixed_scenarios), under the longest step limit "
                        "(1,900) unless --max_step says otherwise; episode statistics and validation are reported per scenario and pooled")
    p.add_argument("--random", action="store_true")
    # additions of the vectorised driver
    p.add_argument("--num_envs", type=int, default=4096)
    p.add_argument("--episodes", type=int, default=6000)
    p.add_argument("--updates_per_step", type=int, default=1)
    p.add_argument("--buffer_size", type=int, default=1 << 20)
    p.add_argument("--expert_csv", type=str, default=None, help="the expert table; a comma-separated list of files is read and labelled file by file "
                                                                "(no transition spans two files) and concatenated")
    p.add_argument("--bc_actor", type=str, default=None)
    p.add_argument("--result_dir", type=str, default="results")
    p.add_argument("--checkpoint_rate", type=int, default=25, help="episodes between validations (train_all.py:206)")
    p.add_argument("--bc_validate_from", type=int, default=1000, help="BC: first episode with validation (train_all.py:259)")
    p.add_argument("--loop", type=str, default="front", choices=["front", "reference"],
                   help="front (default where it applies AND every rank has a GPU of its own: HIRL / TD3 in fp32 or bf16 actor + critic, SAC / E-SAC at every number of envs on "
                        "one GPU (fp32, or bf16 for acting AND update; ISAC and bf16_policy keep the reference's order inside it); batch <= 256, one update per step; ranks that share a GPU run the reference's order): env step + the first "
                        "launches of learn() as one launch; the minibatch is drawn from the ring as it stood before the step's insert, without the slots it may "
                        "overwrite.  reference: act -> env step -> insert -> draw -> learn on every step (the minibatch sees this step's transitions)")
    p.add_argument("--separate_launches", action="store_true",
                   help="chooseAction and env.step as two launches (default: one fused launch). With <= 256 envs this keeps the replay "
                        "insert order, and so the whole run, reproducible bit for bit")
    p.add_argument("--snapshot_every", type=int, default=25, help="episodes between whole-run snapshots (0: never)")
    p.add_argument("--resume", type=str, default=None, help="run directory holding state_rank<r>.pt to continue from")
    p.add_argument("--gpus", type=int, default=None, help="ranks = GPUs of this node; without a launcher environment the driver starts them itself")
    p.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16", "bf16_policy", "f32x9"],
                   help="f32 (default): fp32 everywhere — from 4,096 envs per GPU on, the ACTING kernel forms its fp32 256->512 product as the exact "
                        "three-way bf16 split of both operands on the bf16 matrix cores (engine.x9_rows); f32x9: that format at every size; bf16: policy inference AND the "
                        "256<->512 products of learn() on bf16 MFMA (fp32 accumulate, fp32 master weights / Adam / LayerNorm / dynamics); bf16_policy: "
                        "policy inference only.  SAC / E-SAC: bf16 and bf16_policy as above (the Gaussian head stays fp32), f32x9 runs fp32 with a warning.  "
                        "Stored in the snapshot: --resume refuses another value (a SAC snapshot from before SAC had bf16 resumes in fp32)")
    p.add_argument("--synthetic_expert", action="store_true", help="uniform-random stand-in for the expert CSV (throughput runs and tests ONLY)")
    p.add_argument("--load_dir", type=str, default=None, help="--load_model: directory of the checkpoint files (default: this run's model dir)")
    p.add_argument("--load_tag", type=str, default="Agent20_successRate0.64", help="--load_model: checkpoint tag (train_all.py:240 hard-codes this one)")
    p.add_argument("--log_rewards", action="store_true", help="also log Training/Episode Reward (one more small launch per vector step)")
    p.add_argument("--episode_stats", action="store_true",
                   help="per-episode training statistics by scenario (return, length, how the episode ended: Training/<scenario>/*, Training/Last 100 Episode "
                        "Average Reward): one small launch behind every acting launch (utils/epstat.py).  Always on under --env mixed")
    p.add_argument("--per", action="store_true", help="SAC: prioritized replay (SacAgent(per=True)): proportional draws with importance weights, priorities from "
                                                      "|Q1 - y|; fp32, one GPU, --type SAC; the vector loop runs in the reference's order")
    p.add_argument("--per_new", choices=("max", "td"), default="max",
                   help="--per: the priority a newly stored row enters at.  max (default): the running maximum priority; td: a TD error of its own, "
                        "|Q1(s, a) - y| with the networks as they stand, as the reference's train_episode computes it for every append "
                        "(SAC/agent.py:234-246): one scoring pass over the step's rows per vector step (fp32, one GPU)")
    p.add_argument("--per_alpha", type=float, default=0.6, help="--per / --hirl_per: priority exponent (SAC/agent.py:62)")
    p.add_argument("--per_beta", type=float, default=0.4, help="--per / --hirl_per: importance-weight exponent at the start (SAC/agent.py:62)")
    p.add_argument("--per_beta_annealing", type=float, default=0.0001, help="--per / --hirl_per: beta <- min(1, beta + this) per sample call (SAC/agent.py:63)")
    p.add_argument("--hirl_per", action="store_true",
                   help="HIRL (every --type) and TD3 (an extension: the reference's prioritized branch is dead code, HIRL.py:236,283): prioritized replay — the "
                        "replay rows of a minibatch are drawn proportionally to (|Q1 - y| + 1e-4)^alpha with replacement and weigh (n p / S)^-beta / max in the "
                        "critic loss; expert rows weigh 1 and are kept, the actor loss is unweighted.  New rows enter at the running maximum priority.  Every "
                        "--dtype, --hirl_grad_clip, --expert_floor / --expert_branch / --expert_online, --env mixed; one GPU, the reference's step order, not with "
                        "--buffer_upsample / --expert_upsample, --buffer_size <= 2^24.  (--per is SacAgent's and stays SAC's.)  Stored in the snapshot: "
                        "--resume refuses the other setting")
    p.add_argument("--buffer_upsample", action="store_true",
                   help="HIRL (every --type) and TD3: the reference's UniformMemory(upsample=True) (HIRL.py:184, 189): a replay row whose step_success is 1 "
                        "is drawn --upsample_boost times as often as any other, with replacement.  TD3 is an extension (the same engine draws for both).  "
                        "The vector loop takes the reference's order")
    p.add_argument("--expert_upsample", action="store_true",
                   help="HIRL and BC: the reference's `bc fire upsample` (HIRL.py:185, 253-257; BC.py:171-176): one row of every BC minibatch is replaced "
                        "by a uniformly chosen expert row whose fire action is 1")
    p.add_argument("--upsample_boost", type=int, default=10, help="--buffer_upsample: the integer weight of a success row against 1, 2..255 "
                                                                  "(10 = the reference's 1.0 : 0.1)")
    p.add_argument("--expert_online", type=int, default=0, metavar="ROWS",
                   help="HIRL (every --type, every --dtype, both loops; an extension, the reference can only replay recordings): the BC table grows by ROWS "
                        "rows that start as a cyclic copy of the expert CSV's and are relabelled by the scripted pursuit pilot in the states the learner "
                        "reaches (dataset aggregation): one small launch behind every acting launch (utils/pilot.py).  0 (default): off, the run is launch "
                        "for launch what it was.  One GPU.  Stored in the snapshot: --resume refuses another value")
    p.add_argument("--expert_branch", type=int, default=0, metavar="ROWS",
                   help="an extension: ROWS rows are appended to the labelled expert ring (HIRL's expert rows, E-SAC's, ISAC's expert batch) and rewritten "
                        "behind every acting launch by BRANCHES of the learner's own envs: K envs are each flown one step by the scripted pursuit pilot, in "
                        "registers, and (s, a_E, s'_E, r, done) + step_success replace the K oldest of those rows; the envs themselves are untouched.  "
                        "0 (default): off.  HIRL, E-SAC and ISAC, every --dtype / loop, one GPU, not with --per")
    p.add_argument("--expert_branch_per_step", type=int, default=64, metavar="K",
                   help="--expert_branch: envs branched per acting launch, 1 <= K <= min(ROWS, --num_envs)")
    p.add_argument("--expert_branch_steps", type=int, default=1, metavar="H",
                   help="--expert_branch: the K branches stay resident on the device and fly up to H steps, one step per acting launch (the launch's cost "
                        "does not depend on H); a branch that ends (done, a non-finite row, H steps) is reseeded from the learner's envs.  1 (default): one "
                        "step per pick.  1..65535.  Stored in the snapshot: --resume refuses another value")
    p.add_argument("--expert_self", type=int, default=0, metavar="ROWS",
                   help="HIRL (every --type), ESAC, ISAC: self-imitation (an extension) — the labelled expert ring grows by ROWS online rows that the learner's "
                        "own episodes rewrite: every env's last --expert_self_steps steps are kept on a device tape, and an episode that ends in a kill (done "
                        "with reward > 0) is written, oldest step first, as full transitions over the oldest online rows.  0 (default): off.  Not with "
                        "--expert_branch, --per, --gpus > 1")
    p.add_argument("--expert_self_steps", type=int, default=256, metavar="L",
                   help="--expert_self: steps of an episode the tape keeps, 1 <= L <= min(ROWS, 65535); the tape takes 76 L num_envs bytes of device memory")
    p.add_argument("--expert_self_bc", action="store_true",
                   help="--expert_self, HIRL only: the BC table grows by the same ROWS and takes the same rows as (s, a).  Not with --expert_online")
    p.add_argument("--expert_floor", type=int, default=0, metavar="N",
                   help="HIRL and --type ESAC (a departure from the reference, whose expert rows end with the warm-up): the expert rows of a minibatch never "
                        "fall below N, 0 <= N <= 128, so the expert ring (and --expert_branch's rows) is read for the whole run.  0 (default): the "
                        "reference's rule.  Not with --per.  Stored in the snapshot: --resume refuses another value")
    p.add_argument("--expert_online_per_step", type=int, default=64, metavar="K",
                   help="--expert_online: envs relabelled per acting launch, 1 <= K <= min(ROWS, --num_envs); they replace the K oldest online rows")
    p.add_argument("--explore_noise", type=str, default="white", choices=["white", "ou", "pink"],
                   help="HIRL / TD3 / SAC (an extension, the reference's exploration noise is white): the colour of the learner's action noise.  white "
                        "(default): drawn fresh per env, component and step inside the acting kernels, as ever.  ou: an Ornstein-Uhlenbeck process of "
                        "correlation time --explore_tau.  pink: 1 / f noise from --explore_octaves octave-spaced AR(1) poles.  ou and pink come from a "
                        "generator launch every --explore_chunk steps and are not reset at episode ends; SAC, ESAC and ISAC take them as the Gaussian "
                        "head's eps, in the reference's order.  Stored in the snapshot: --resume refuses another value.  Not --agent BC")
    p.add_argument("--explore_tau", type=float, default=16.0, metavar="STEPS", help="--explore_noise ou: the correlation time in vector steps, a = exp(-1 / tau) (default 16)")
    p.add_argument("--explore_octaves", type=int, default=6, metavar="K", help="--explore_noise pink: the poles a[k] = exp(-2^-k) of the bank, 1..8 (default 6)")
    p.add_argument("--explore_sigma", type=float, default=0.1, metavar="S",
                   help="HIRL / TD3: the standard deviation of the action noise (default 0.1, the reference's).  SAC's noise scale is the policy's own: refused")
    p.add_argument("--explore_sigma_max", type=float, default=None, metavar="S",
                   help="HIRL / TD3: a ladder of noise scales over the envs, sigma_i = S0 (S / S0)^(u_i) with S0 = --explore_sigma and u_i a fixed hash of the env "
                        "id in [0, 1); the noise then comes from the generator whatever its colour")
    p.add_argument("--explore_chunk", type=int, default=16, metavar="STEPS", help="vector steps one generator launch fills, 1..64 (default 16)")
    p.add_argument("--multi_step", type=int, default=1,
                   help="SAC / E-SAC: truncated n-step returns (SacAgent(multi_step=N)), N in 2..8; 1 (default): one-step rows.  A launch of its own behind "
                        "every acting launch keeps the last N steps per env and stores finished rows with r = sum gamma^k r_k and the row's discount folded "
                        "into the done column; no transition is dropped.  Any --dtype, --per with --per_new max; one GPU; the vector loop runs in the "
                        "reference's order.  Stored in the snapshot: --resume refuses another value")
    p.add_argument("--hirl_multi_step", type=int, default=1,
                   help="HIRL / TD3: truncated n-step returns, N in 2..8; 1 (default): one-step rows.  An extension (the reference's HIRL and TD3 learn from "
                        "one-step rows): the env runs without a ring, a launch of its own behind every acting launch stores finished rows with r = sum gamma^k "
                        "r_k and the row's discount folded into the done column, and HIRL's offline expert rows are relabelled the same way (expert branch "
                        "rows stay one-step rows).  Every --type and --dtype, both loop forms up to 8,192 envs (the reference's order beyond), "
                        "--hirl_grad_clip, --hirl_per, the upsampling switches; one GPU.  Stored in the snapshot: --resume refuses another value")
    p.add_argument("--grad_clip", type=float, default=None, help="SAC: clip each network's gradient (Q1, Q2, policy) to this global L2 norm before its Adam step "
                                                                 "(SacAgent(grad_clip=C), SAC/utils.py:15-21); one GPU; the vector loop runs in the reference's "
                                                                 "order.  Stored in the snapshot: --resume refuses another value")
    p.add_argument("--hirl_grad_clip", type=float, default=None, metavar="C",
                   help="HIRL / TD3 (an extension, the reference has none): clip_grad_norm_ once per optimizer — the critic's two heads and LayerNorms under ONE "
                        "norm, the whole actor — in front of its Adam step, in both loop forms, at every --dtype and under --gpus N (the norm of the averaged "
                        "gradient); norms under stats/grad_norm_critic / _actor.  Not --agent BC; SAC has --grad_clip.  Stored in the snapshot: --resume refuses "
                        "another value")
    p.add_argument("--fixed_alpha", type=float, default=None, help="SAC: a constant entropy coefficient alpha = X and no log-alpha optimiser "
                                                                   "(SacAgent(entropy_tuning=False, ent_coef=X), SAC/agent.py:108-110).  Stored in the snapshot: "
                                                                   "--resume refuses another value")
    p.add_argument("--max_step", type=int, default=None, help="steps per episode (default: the scenario's, train_all.py:159-183: 1500 / 1500 / 1900); short rehearsal runs")
    p.add_argument("--status_check_every", type=int, default=256,
                   help="front loop: vector steps between reads of the front launch's status word (one host sync each; 0: only at every episode's end)")
    p.add_argument("--on_front_trip", type=str, default="fallback", choices=["fallback", "exit"],
                   help="a front launch's in-launch wait gave up: fallback = reload the newest snapshot and continue with --loop reference inside this process "
                        "(exit code 3 when there is no snapshot yet); exit = always exit with code 3")
    p.add_argument("--replica_check_every", type=int, default=5, help="sharded runs: episodes between replica checksum comparisons (0: only at validation)")
    return p


if __name__ == "__main__":
    import sys

    cfg = parse_args()
    if cfg.gpus and cfg.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(cfg.gpus, sys.argv[1:]))
    main(cfg)
