"""The order of host calls within a vector step of train_all (act -> n-step push -> statistics push -> first priorities -> reward sum -> draw -> expert
draw -> learn), pinned without a GPU: the step functions and hooks run over a hand-built Run whose engine, env, replay, inserter, statistics and writer
are stubs that append (name, positional arguments, keyword arguments) to one list.  The expected lists are written out from the driver as it stood before
its main() was split; nothing here calls the code under test to produce them."""
from types import SimpleNamespace

import pytest

from hirl4ucav_amd import train_all as T

SEED, RANK, N, BATCH = 7, 2, 4, 128  # acting seed 8, sampling seed 11, scoring seed 12


class Eng:
    def __init__(self, log, status=()):
        self.log, self.status = log, list(status)

    def act(self, *a, **kw):
        self.log.append(("eng.act", a, kw))

    def act_step(self, *a, **kw):
        self.log.append(("eng.act_step", a, kw))

    def step_learn(self, *a, **kw):
        self.log.append(("eng.step_learn", a, kw))

    def sample(self, *a, **kw):
        self.log.append(("eng.sample", a, kw))

    def sample_expert(self, *a, **kw):
        self.log.append(("eng.sample_expert", a, kw))

    def learn(self, *a, **kw):
        self.log.append(("eng.learn", a, kw))

    def score_new(self, *a, **kw):
        self.log.append(("eng.score_new", a, kw))

    def front_status(self):
        self.log.append(("eng.front_status", (), {}))
        return self.status.pop(0) if self.status else 0

    def losses_host(self):
        return 1.0, 2.0, 3.0, 4.0, 5.0, 6.0


class Env:
    obs, env_id0, reward = "obs", 8, "reward"

    def __init__(self, log):
        self.log = log

    def step(self, *a, **kw):
        self.log.append(("env.step", a, kw))


class Replay:
    def __init__(self, log):
        self.log = log

    def mark_new(self, *a, **kw):
        self.log.append(("replay.mark_new", a, kw))


class Inserter:
    max_rows = 12

    def __init__(self, log):
        self.log = log

    def push(self, *a, **kw):
        self.log.append(("inserter.push", a, kw))


class Stats:
    def __init__(self, log):
        self.log = log

    def push(self, *a, **kw):
        self.log.append(("estats.push", a, kw))


class Ret:
    def __init__(self, log):
        self.log = log

    def __iadd__(self, other):
        self.log.append(("ret +=", (other,), {}))
        return self


class Writer:
    def __init__(self, log):
        self.log = log

    def add_scalar(self, tag, value, at):
        self.log.append(("writer.add_scalar", (tag, at), {}))


@pytest.fixture
def log(monkeypatch):
    out, real = [], T.expert_num_after
    monkeypatch.setattr(T, "expert_num_after", lambda *a: out.append(("expert_num_after", a, {})) or real(*a))
    return out


def make_run(log, agent="HIRL", max_step=3, **over):
    """a Run as main() leaves it before the first episode, on rank 2 (no writer) unless told otherwise"""
    sac = agent in ("SAC", "ESAC", "ISAC")
    run = T.Run(config=SimpleNamespace(type="soft", bc_weight=0.5, separate_launches=False, updates_per_step=1), rank=RANK, world=1, seed=SEED,
                sac=sac, hirl=agent == "HIRL", esac=agent == "ESAC", isac=agent == "ISAC", per=False, per_new="max", multi_step=1, grad_clip=None,
                n=N, batch=BATCH, max_step=max_step, warm_up_rate=20 if sac else 10, env=Env(log), replay=Replay(log), inserter=None, eng=Eng(log),
                expert=None if agent in ("SAC", "TD3") else "expert", bc_table="bc_table" if agent == "HIRL" else None, estats=None, writer=None,
                actions="actions", log_rate=300, ret=Ret(log), episode=0, expert_num=BATCH if agent in ("HIRL", "ESAC") else 0,
                front=False, front_sac=False, check_every=0, steps_since_check=0)
    for k, v in over.items():
        setattr(run.config if hasattr(run.config, k) else run, k, v)
    return run


def test_hirl_front_episode(log):
    """steps 0 and 1: the decay, ONE step_learn (the schedule's weight on the first, None afterwards), the hooks; step 2, the episode's last, only acts"""
    run = make_run(log, front=True, estats=Stats(log))
    hooks = [("estats.push", (), {}), ("ret +=", ("reward",), {})]

    def step_learn(w):
        return ("eng.step_learn", (run.env, "expert", "bc_table"), dict(n_main=1, act_sigma=0.1, act_seed=8, out="actions", sample_seed=11, bc_weight_now=w,
                                                                        bc_warm_up_weight=0.0))

    assert T.run_episode(run) == 0
    assert log == ([("expert_num_after", (128, 0, 10), {}), step_learn(100)] + hooks + [("expert_num_after", (127, 1, 10), {}), step_learn(None)] + hooks +
                   [("eng.act_step", (run.env,), dict(sigma=0.1, seed=8, out="actions"))] + hooks + [("eng.front_status", (), {})])
    assert run.expert_num == 127


def test_hirl_reference_order_with_two_updates_per_step(log):
    run = make_run(log, updates_per_step=2, max_step=2)
    sample = ("eng.sample", (run.replay, "expert", "bc_table"), dict(n_main=1, seed=11, defer=True))
    act = ("eng.act_step", (run.env,), dict(sigma=0.1, seed=8, out="actions"))
    assert T.run_episode(run) == 0
    assert log == [act, ("ret +=", ("reward",), {}), ("expert_num_after", (128, 0, 10), {}),
                   sample, ("eng.learn", (), dict(bc_weight_now=100, bc_warm_up_weight=0.0)),
                   sample, ("eng.learn", (), dict(bc_weight_now=None, bc_warm_up_weight=0.0)),
                   act, ("ret +=", ("reward",), {})]  # (the last step: no draw, no learn)


@pytest.mark.parametrize("agent, kw", [("SAC", {}), ("HIRL", {"sigma": 0.1})])
def test_separate_launches(log, agent, kw):
    run = make_run(log, agent, separate_launches=True, max_step=1, ret=None)
    T.run_episode(run)
    assert log == [("eng.act", ("obs",), dict(kw, seed=8, row0=8, out="actions")), ("env.step", ("actions",), {})]


@pytest.mark.parametrize("agent, drawn_with, expert_num, n_main", [("SAC", None, 0, 128), ("ESAC", "expert", 128, 1), ("ISAC", None, 0, 128)])
def test_sac_families_in_the_reference_order(log, agent, drawn_with, expert_num, n_main):
    """the minibatch is expert-mixed for ESAC only; ISAC draws its expert batch by sample_expert, under the sampling seed"""
    run = make_run(log, agent, max_step=2, ret=None)
    act = ("eng.act_step", (run.env,), dict(seed=8, out="actions"))
    second = [("eng.sample_expert", ("expert",), dict(seed=11, defer=True))] if agent == "ISAC" else []
    T.run_episode(run)
    assert log == [act, ("expert_num_after", (expert_num, 0, 20), {}),
                   ("eng.sample", (run.replay, drawn_with), dict(n_main=n_main, seed=11, defer=True))] + second + [("eng.learn", (), {}), act]


@pytest.mark.parametrize("agent, passed, expert_num, n_main", [("SAC", None, 0, 128), ("ESAC", "expert", 128, 1), ("ISAC", "expert", 0, 128)])
def test_sac_front_passes_the_expert_ring_for_esac_and_isac(log, agent, passed, expert_num, n_main):
    run = make_run(log, agent, max_step=2, ret=None, front_sac=True)
    T.run_episode(run)
    assert log == [("expert_num_after", (expert_num, 0, 20), {}),
                   ("eng.step_learn", (run.env, passed), dict(n_main=n_main, act_seed=8, out="actions", sample_seed=11)),
                   ("eng.act_step", (run.env,), dict(seed=8, out="actions"))]  # (no status read: that word is the HIRL front launch's)


@pytest.mark.parametrize("per_new, inserter", [("max", True), ("max", False), ("td", False)])
def test_hook_order_after_the_env_step(log, per_new, inserter):
    """acting call, n-step push, statistics push, the new rows' first priorities, the reward sum — and only then the draw"""
    run = make_run(log, "SAC", max_step=2, per=True, per_new=per_new, estats=Stats(log), inserter=Inserter(log) if inserter else None)
    first = ("eng.score_new", (run.replay, N), dict(seed=12)) if per_new == "td" else ("replay.mark_new", (12 if inserter else N,), {})
    T.run_episode(run)
    step0 = ([("eng.act_step", (run.env,), dict(seed=8, out="actions"))] + ([("inserter.push", (run.env, "actions"), {})] if inserter else []) +
             [("estats.push", (), {}), first, ("ret +=", ("reward",), {}), ("expert_num_after", (0, 0, 20), {}),
              ("eng.sample", (run.replay, None), dict(n_main=128, seed=11, defer=True)), ("eng.learn", (), {})])
    assert log[:len(step0)] == step0
    assert [name for name, _, _ in log].count("replay.mark_new") == (0 if per_new == "td" else 2)  # (the last step's rows are marked too)


def test_status_word_is_read_every_check_every_steps_across_episodes(log):
    """check_every = 2, three steps per episode: the count carries over the episode boundary; one more read at every episode's end; a non-zero word
    leaves the episode before that step's launches, and the end-of-episode read is not repeated"""
    run = make_run(log, front=True, check_every=2, ret=None, eng=Eng(log, status=[0, 0, 2]))
    names = lambda: [name for name, _, _ in log if name.startswith("eng.")]  # noqa: E731
    assert T.run_episode(run) == 0
    assert names() == ["eng.step_learn", "eng.front_status", "eng.step_learn", "eng.act_step", "eng.front_status"] and run.steps_since_check == 1
    del log[:]
    assert T.run_episode(run) == 2
    assert names() == ["eng.front_status"] and run.steps_since_check == 0


@pytest.mark.parametrize("agent, expected", [("HIRL", [1] * 10 + [2] * 10 + [3] * 5), ("ESAC", [1] * 20 + [2] * 5)])
def test_expert_rows_decay_once_per_learning_step(log, agent, expected):
    """n_main = 128 - expert_num, one expert row fewer every warm_up_rate steps (10; SAC: 20), advanced before the draw"""
    run = make_run(log, agent, max_step=26, ret=None)
    T.run_episode(run)
    assert [kw["n_main"] for name, _, kw in log if name == "eng.sample"] == expected
    assert [a[1] for name, a, _ in log if name == "expert_num_after"] == list(range(25))


def test_expert_rows_stop_at_zero(log):
    run = make_run(log, "HIRL", max_step=22, ret=None, front=True, expert_num=2)
    T.run_episode(run)
    assert [kw["n_main"] for name, _, kw in log if name == "eng.step_learn"] == [127] * 10 + [128] * 11 and run.expert_num == 0


@pytest.mark.parametrize("argv, rate", [(["--agent", "SAC", "--type", "ESAC"], 20), (["--agent", "HIRL"], 10), (["--agent", "TD3"], 10)])
def test_warm_up_rate_by_agent(argv, rate):
    run = T.Run(config=T.parser().parse_args(argv), world=1)
    T.check_agent_flags(run)
    assert (run.warm_up_rate, run.batch) == (rate, 128)


def test_step_scalars_on_rank_0(log):
    """Loss/* behind the learn of every log_rate-th step, at step + episode * max_step"""
    run = make_run(log, front=True, rank=0, writer=Writer(log), ret=None, episode=2)
    T.run_episode(run)
    tags = [("writer.add_scalar", (t, 6), {}) for t in ("Loss/Critic_Loss", "Loss/Actor_Loss", "Loss/BC_Loss", "Loss/RL_Loss", "Loss/BC_Fire_Loss")]
    assert log[2:7] == tags and [e for e in log if e[0] == "writer.add_scalar"] == tags


def test_driver_record_keys():
    run = T.Run(expert_num=5, high_score=1.5, success_rate=0.25, arttir=3, seed=SEED, dtype="f32", dtype_mark={}, env_type="serpentine", estats=None)
    assert T.driver_record(run, 4) == {"episode": 4, "expert_num": 5, "high_score": 1.5, "success_rate": 0.25, "arttir": 3, "seed": SEED, "dtype": "f32",
                                       "env": "serpentine"}
    run.dtype_mark = {"dtype_honoured": True}
    run.estats, run.last100 = SimpleNamespace(state=lambda: "device"), SimpleNamespace(state=lambda: "last100")
    assert list(T.driver_record(run, 4)) == ["episode", "expert_num", "high_score", "success_rate", "arttir", "seed", "dtype", "dtype_honoured", "env",
                                             "episode_stats"]
    assert T.driver_record(run, 4)["episode_stats"] == {"device": "device", "last100": "last100"}
