"""The reference's stand-alone validation drivers (hirl/validate_all.py, hirl/validate_sac.py) on the batched GPU env: load a checkpoint, run `nums`
rounds of `episodes` validation episodes with the noise-free policy, print what the reference prints.

    python -m hirl4ucav_amd.validate_all --agent HIRL --model_dir <run>/model --model_name Agent3_100_5_ --random [--infinite]
    python -m hirl4ucav_amd.validate_all --agent SAC  --model_dir <run>/model --model_name <tag> --random [--infinite]

What the reference does (validate_all.py:79-212, validate_sac.py:79-186) and what is kept:
  * whatever --env says, the episodes run in the SERPENTINE scenario with validationStep = 1200 (validate_all.py:184-190) — kept as the default; `--scenario`
    validates somewhere else (an extension);
  * `nums = 2` rounds of 50 episodes (:192), mean and SAMPLE standard deviation over the rounds (statistics.stdev, :200-204);
  * `--infinite`: HarfangSerpentineInfiniteEnv (HarfangEnv_GYM.py:476-535) — the missile is put back on the rail every 60th step_test call (:484-486) and the
    figure of merit is the share of launches made WITH the target locked, infinite_total_success / infinite_total_fire (:517-527), pooled over the round's episodes;
  * the checkpoint: the reference hard-codes a Windows path and a tag (validate_all.py:181-183); here --model_dir / --model_name name them.
One deviation, forced by batching: the reference's every-60th-call counter runs on across the episodes of a round (an env attribute, never reset), so an
episode's first re-arm comes 60 - (steps of the episodes before it) mod 60 calls in; here every episode is its own env and re-arms at ITS steps 60, 120, ...
(the first episode of a reference round does exactly that).  An episode that is still running at the step limit counts neither as a kill nor as a fire success
(validate_all.py:59-66: both are read only when `done` is seen).
An extension: the reference collects the last episode's track in validate() with --plot but never writes it (validate_all.py:30-58); here `--plot` writes it per
round — the reference's five CSVs and two figures of train_all.py:70-89 with the tag round<k> — into `--plot_dir` (default <model_dir>/../plot), from the device
record of utils/trace.py.
Another: `--scenario mixed` runs every round over the three scenarios (`episodes` episodes each, the same seed), prints a line per scenario and the pooled
line, and the final statistics are over the rounds' pooled numbers; it has no --infinite form (that env is the serpentine one).  main()'s returned lists then hold the
pooled numbers of each round."""
import argparse
import os
import statistics

import torch

from . import _lib
from .agents import engine as E
from .agents.HIRL import init_actor_state_dict, init_critic_state_dict
from .environments.batched import BatchedHarfangEnv
from .utils import checkpoint as CK
from .utils.seed import set_seed

VALIDATION_STEP = 1200   # validate_all.py:187,190
SCENARIO_NAMES = ("straight_line", "serpentine", "circular")
MIXED = "mixed"
REARM_EVERY = 60         # HarfangEnv_GYM.py:484-486


def validate_round(engine, episodes, steps, if_random, seed, device, infinite=False, sac=False, scenario="serpentine", env=None, recorder=None):
    """validate() of validate_all.py:25-77 / validate_sac.py:26-77 as ONE batch of `episodes` envs -> (mean score, fire-success rate, locked launches per launch or 0).
    An env is simulated on after its `done` (no auto reset), so score and counters only accumulate while its episode lasts.
    `recorder`: an EpisodeRecorder over `env` (utils/trace.py) — one more launch behind every env step; None: none, and the return is the same."""
    if env is None:
        env = BatchedHarfangEnv(episodes, scenario=scenario, device=device, seed=seed, auto_reset=False, random_reset=if_random, collect_stats=False)
        obs = env.reset()
    else:
        obs = env.obs
    calls = getattr(engine, "act_calls", None)  # validation must not move a training run's exploration-noise counter
    total = torch.zeros(episodes, device=device)
    alive = torch.ones(episodes, dtype=torch.bool, device=device)
    fire_success = torch.zeros(episodes, dtype=torch.bool, device=device)
    launches = torch.zeros((), dtype=torch.int64, device=device)
    hits = torch.zeros((), dtype=torch.int64, device=device)
    if recorder is not None:
        recorder.reset()
    for step in range(steps):
        if infinite and (step + 1) % REARM_EVERY == 0:  # the call counter is incremented first, then tested (:483-486)
            env.rearm(alive.to(torch.uint8))
        a = engine.act(obs, explore=False) if sac else engine.act(obs)  # exploit / chooseActionNoNoise
        obs, r, d, s = env.step(a)
        if recorder is not None:
            recorder.push()
        total += torch.where(alive, r, torch.zeros_like(r))
        launches += (alive & (s != 0)).sum()   # success != 0: a missile left the rail on this step (:517, :523)
        hits += (alive & (s == 1)).sum()       # ... with the target locked (:524)
        ending = alive & (d != 0)
        if step < steps - 1:                   # `done` raised by the LAST allowed step is never looked at (:59-60 break first)
            flags = env.state[35].view(torch.int32)
            fire_success |= ending & ((flags & _lib.F_FIRE_SUCCESS) != 0)
        alive &= d == 0
        if step % 64 == 63 and not bool(alive.any()):
            break
    if calls is not None:
        engine.act_calls = calls
    n_launch = int(launches)
    rate = (int(hits) / n_launch) if (infinite and n_launch > 0) else 0.0  # (the reference divides by zero when nothing was launched)
    return float(total.mean()), int(fire_success.sum()) / episodes, rate


def plot_dir_of(config):
    """--plot_dir, or `plot` beside the checkpoint directory (the run layout of train_all: <run>/model, <run>/summary, <run>/plot)"""
    return config.plot_dir or os.path.normpath(os.path.join(config.model_dir, os.pardir, "plot"))


def load_agent(config, device):
    """The networks validate_all.py:166-183 builds and loads (HIRL / BC / TD3: agent.loadCheckpoints(tag, dir), HIRL.py:344-350; SAC: agent.load_models)."""
    if config.agent == "SAC":
        from .agents import sac_engine as SE
        from .agents.SAC.agent import _xavier_mlp

        eng = SE.SacEngine(batch=128, lr=1e-3, device=device)
        eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
        eng.load_models(config.model_dir, config.model_name)
        if config.dtype == "bf16":  # the policy's 256 -> 512 product on bf16 MFMA, the Gaussian head in fp32 (SacEngine.set_act_dtype)
            eng.set_act_dtype("bf16")
        elif config.dtype != "f32":
            print(f"WARNING: --dtype {config.dtype} has no effect on the SAC agent (no exact-split format): running fp32", flush=True)
        return eng, True
    hirl = config.agent == "HIRL"
    eng = E.HirlEngine(batch=128, slope=0.0 if hirl else 0.01, use_bc=False, device=device)  # HIRL: ReLU; TD3 / BC: LeakyReLU(0.01)
    eng.load_params(init_actor_state_dict(), init_critic_state_dict(), None)
    CK.load_hirl_nets(eng, config.model_dir, config.model_name, names=("Actor_",),  # validation acts with the actor alone
                      missing="{} not found (--model_dir / --model_name name the checkpoint, e.g. Agent3_100_5_)")
    if config.dtype != "f32":
        eng.set_act_dtype("f32x9" if config.dtype == "f32x9" else "bf16")
    return eng, False


def main(config):
    _lib.load()  # fails loudly without the HIP library
    device = torch.device("cuda", 0)
    seed = config.seed if config.seed is not None else int.from_bytes(os.urandom(4), "little") & 0x7FFFFFFF
    set_seed(seed)
    print(("random" if config.random else "fixed") + f" initial positions; seed {seed}" + ("" if config.seed is not None else " (drawn: no --seed given)"), flush=True)
    eng, sac = load_agent(config, device)
    scenario = config.scenario or "serpentine"
    why = mixed_refusal(config)
    if why:
        raise SystemExit("validate_all: " + why)
    returns, success, hit_rate = [], [], []

    def one_round(k, scenario, tag):
        env = rec = None
        if config.plot:
            from .utils.trace import validation_recorder

            env, rec = validation_recorder(config.episodes, scenario, seed + 12345 + k, config.random, config.validation_step, device)
        out = validate_round(eng, config.episodes, config.validation_step, config.random, seed + 12345 + k, device, infinite=config.infinite, sac=sac,
                             scenario=scenario, env=env, recorder=rec)
        if rec is not None:
            rec.write_reference_files(plot_dir_of(config), tag)
        return out

    for k in range(config.nums):
        if scenario == MIXED:  # every scenario with the round's seed; the round's numbers are the pooled ones (equal groups: the mean of the three)
            per = {name: one_round(k, name, f"round{k + 1}_{name}") for name in SCENARIO_NAMES}
            for name, (r, s, _) in per.items():
                print(f"round {k + 1} {name}: avg reward {r:.2f} fire success {s:.2f}", flush=True)
            r, s, f = statistics.mean(v[0] for v in per.values()), statistics.mean(v[1] for v in per.values()), 0.0
        else:
            r, s, f = one_round(k, scenario, f"round{k + 1}")
        returns.append(r)
        success.append(s)
        hit_rate.append(f)
        print(f"round {k + 1}: avg reward {r:.2f} fire success {s:.2f}" + (f" locked launches per launch {f:.3f}" if config.infinite else ""), flush=True)
    sd = (lambda v: statistics.stdev(v) if len(v) > 1 else 0.0)
    if config.infinite:  # validate_all.py:199-200
        print(statistics.mean(hit_rate), sd(hit_rate))
    else:                # :202-204
        print(statistics.mean(returns), sd(returns))
        print(statistics.mean(success), sd(success))
    return returns, success, hit_rate


def mixed_refusal(config):
    """why `--scenario mixed` cannot run as asked, or None"""
    if config.scenario == MIXED and config.infinite:
        return "--scenario mixed with --infinite: the re-arming env is the serpentine one (HarfangSerpentineInfiniteEnv): drop one of the two"
    return None


def parse_args(argv=None):
    """parser().parse_args with the cross-flag check that is an argparse error"""
    p = parser()
    cfg = p.parse_args(argv)
    if mixed_refusal(cfg):
        p.error(mixed_refusal(cfg))
    return cfg


def parser():
    p = argparse.ArgumentParser()  # the reference's flags, validate_all.py:214-227
    p.add_argument("--agent", type=str, default="HIRL", choices=["HIRL", "TD3", "BC", "SAC"])  # SAC: the validate_sac.py path
    p.add_argument("--port", type=int, default=None)
    p.add_argument("--type", type=str, default="linear")
    p.add_argument("--bc_weight", type=float, default=1)
    p.add_argument("--model_name", type=str, required=True, help="checkpoint tag, e.g. Agent3_100_5_ (SAC: the tag of save_models)")
    p.add_argument("--load_model", action="store_true")
    p.add_argument("--render", action="store_true")
    p.add_argument("--plot", action="store_true")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--env", type=str, default="straight_line")  # read and, as in the reference, not used for the validation episodes
    p.add_argument("--random", action="store_true")
    p.add_argument("--infinite", action="store_true")
    # not in the reference
    p.add_argument("--model_dir", type=str, required=True, help="directory of the checkpoint files (the reference hard-codes one)")
    p.add_argument("--plot_dir", type=str, default=None, help="--plot: where the last episode's CSVs and figures of every round go (default: <model_dir>/../plot)")
    p.add_argument("--scenario", type=str, default=None, choices=list(SCENARIO_NAMES) + [MIXED],
                   help="validate here instead of in serpentine; mixed: every round over all three, per-scenario and pooled lines")
    p.add_argument("--nums", type=int, default=2)
    p.add_argument("--episodes", type=int, default=50)
    p.add_argument("--validation_step", type=int, default=VALIDATION_STEP)
    p.add_argument("--dtype", type=str, default="f32", choices=["f32", "f32x9", "bf16"], help="policy inference arithmetic (SAC: f32 or bf16)")
    return p


if __name__ == "__main__":
    main(parse_args())
