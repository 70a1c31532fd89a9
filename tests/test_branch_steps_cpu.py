"""Host-side tests of expert branches of up to H steps (no GPU): the conveyor model of tests/_branch_steps_model.py on its seeded inputs — its coverage is
asserted, so that the GPU comparison cannot pass on an empty case —, H = 1 against tests/_branch_model.BranchModel, the counters, expert_num_after with a
floor, BranchExpert(steps=...)'s workspace and state round trip, the parser's defaults and every refusal of --expert_branch_steps / --expert_floor by
name."""
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hirl4ucav_amd import train_all as T  # noqa: E402
from hirl4ucav_amd.utils import pilot as P  # noqa: E402
from tests import _branch_model as B  # noqa: E402
from tests import _branch_steps_model as S  # noqa: E402
from tests import _pilot_model as PM  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def static_case(n=16, k=16, h=400, m=64, e0=8, calls=420, seed=0):
    state, obs = B.make_inputs(n, seed=seed, special=True)
    off, lab = B.make_offline(e0)
    ring, success = B.initial_ring(off, lab, m)
    model = S.StepsModel(ring, success, e0, m, k, h)
    wrote = [model.push(state, obs) for _ in range(calls)]
    return model, wrote, (state, obs, ring, success)


@pytest.fixture(scope="module")
def flown():
    return static_case()


def test_the_seeded_case_covers_every_way_a_branch_ends(flown):
    """make_inputs(16, seed=0, special=True) held static, k = 16, H = 400, M = 64, E0 = 8, 420 calls (measured: 2 kills, 7 done rows, 2 non-finite skips,
    15 reseeds by the step cap, a largest age of 399): at least one of each"""
    model, wrote, _ = flown
    ev = model.events
    assert ev["kills"] >= 1 and ev["done"] >= 1 and ev["skips"] >= 1 and ev["cap"] >= 1 and ev["max_age"] == 399
    assert ev["done"] > ev["kills"]  # (a done row that is no kill: an altitude edge)
    assert ev["seeds"] > 16  # (reseeds beyond the first call's)
    assert sum(len(w) for w in wrote) == ev["rows"] == 420 * 16 - ev["skips"]
    assert any(env is None for w in wrote for _, env, _ in w) and model.call == 420


def test_counters_are_the_events(flown):
    model, wrote, _ = flown
    ev = model.events
    assert model.counters() == (ev["rows"], ev["done"], ev["kills"])
    assert not model.cnt[:, 16:].any() and not model.age[16:].any() and not model.bstate[:, 16:].any() and not model.bobs[:, 16:].any()
    assert model.image().shape == (S.workspace_bytes(16),) and S.workspace_bytes(16) == 64 * 228 and S.workspace_bytes(65) == 128 * 228
    # the image round-trips through the constructor
    again = S.StepsModel(model.ring, model.success, 8, 64, 16, 400, call=model.call, work=model.image())
    assert np.array_equal(again.image(), model.image())


def test_a_kill_pays_600_and_is_counted_once(flown):
    """every done row the model wrote with a kill carries the +600 (reward > 500), every other done row does not"""
    state, obs = B.make_inputs(16, seed=0, special=True)
    off, lab = B.make_offline(8)
    ring, success = B.initial_ring(off, lab, 64)
    model = S.StepsModel(ring, success, 8, 64, 16, 400)
    kills = dones = 0
    for _ in range(420):
        before = model.counters()
        wrote = model.push(state, obs)
        rows = [model.ring[slot] for _, _, slot in wrote]
        d = sum(1 for r in rows if r[31] == 1)
        kl = sum(1 for r in rows if r[31] == 1 and r[30] > 500)
        after = model.counters()
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (len(wrote), d, kl)
        kills, dones = kills + kl, dones + d
    assert kills >= 1 and dones > kills


@pytest.mark.parametrize("n,k", [(16, 5), (16, 16), (7, 1)])
def test_one_step_is_the_branch_model(n, k):
    """H = 1 reproduces BranchModel.push exactly and leaves bstate / bobs / age as they were: only the counters move"""
    state, obs = B.make_inputs(n, seed=1, special=True)
    off, lab = B.make_offline(8)
    ring, success = B.initial_ring(off, lab, 23)
    fill = np.full(S.workspace_bytes(k), 0xA5, np.uint8)
    a, b = S.StepsModel(ring, success, 8, 23, k, 1, work=fill), B.BranchModel(ring, success, 8, 23, k)
    for _ in range(40):
        wa, wb = a.push(state, obs), b.push(state, obs)
        assert [(e, s) for _, e, s in wa] == wb
        assert np.array_equal(bits(a.ring), bits(b.ring)) and np.array_equal(a.success, b.success)
    img, kp = a.image(), S.kpad(k)
    assert (img[:51 * 4 * kp] == 0xA5).all()
    base = int(np.full(8, 0xA5, np.uint8).view(np.uint64)[0])
    assert int(a.cnt[0, 0]) > base and (a.cnt[:, k:] == np.uint64(base)).all()


def test_short_flights_and_spread_picks():
    """H = 8 and k = 5 over 16 envs (floor(n / k) = 3): a resident flight of 8 steps, then the reseed from the env the window has moved to"""
    model, wrote, (state, obs, ring, success) = static_case(k=5, h=8, m=64, calls=40)
    assert PM.env_picks(0, 16, 5) == [0, 3, 6, 9, 12] and PM.env_picks(8, 16, 5) == [8, 11, 14, 1, 4]
    lane0 = [(c, env) for c, w in enumerate(wrote) for lane, env, _ in w if lane == 0]
    assert [env for _, env in lane0[:9]] == [0] + [None] * 7 + [8]  # seeded at call 0, flown 7 more steps, reseeded at call 8 from env (8 + 0) mod 16
    assert model.events["cap"] >= 5 and model.events["max_age"] == 7
    # the first row of a flight is the one-step branch's row of that env; the second starts where the first ended
    rows, succ, stepped = B.step_once(state, obs)
    slot0, slot1 = PM.slots(0, 5, 64, 8)[0], PM.slots(1, 5, 64, 8)[0]
    m2 = S.StepsModel(ring, success, 8, 64, 5, 8)
    m2.push(state, obs)
    assert np.array_equal(bits(m2.ring[slot0]), bits(rows[0])) and np.array_equal(bits(m2.bstate[:, 0]), bits(stepped[:, 0])) and m2.age[0] == 1
    assert np.array_equal(bits(m2.bobs[:, 0]), bits(rows[0, 17:30]))
    m2.push(state, obs)
    rows2, _, _ = B.step_once(stepped[:, :1], rows[:1, 17:30])
    assert np.array_equal(bits(m2.ring[slot1]), bits(rows2[0])) and np.array_equal(bits(m2.ring[slot1, 0:13]), bits(rows[0, 17:30]))
    # lane 4 seeds on env 12 (a NaN state word): nothing written, not resident, reseeded on the next call
    assert all(lane != 4 for lane, _, _ in wrote[0]) and any(lane == 4 and env == 13 for lane, env, _ in wrote[1])


def test_the_inputs_stand():
    state, obs = B.make_inputs(16, seed=0, special=True)
    s0, o0 = state.copy(), obs.copy()
    off, lab = B.make_offline(8)
    ring, success = B.initial_ring(off, lab, 64)
    model = S.StepsModel(ring, success, 8, 64, 16, 8)
    for _ in range(20):
        model.push(state, obs)
    assert np.array_equal(bits(state), bits(s0)) and np.array_equal(bits(obs), bits(o0))
    assert np.array_equal(bits(model.ring[:8]), bits(off)) and np.array_equal(model.success[:8], lab)


# ---- expert_num_after with a floor ----------------------------------------------------------------------------------------------------------
def test_expert_num_floor():
    e, f, trace, ftrace = 128, 128, [], []
    for step in range(1500):
        e, f = T.expert_num_after(e, step), T.expert_num_after(f, step, 10, floor=32)
        trace.append(e)
        ftrace.append(f)
    # floor = 0: the trace of tests/test_host_logic.py
    assert trace[0] == 127 and trace[9] == 127 and trace[10] == 126 and trace[1269] == 1 and trace[1270] == 0 and trace[-1] == 0
    assert [T.expert_num_after(v, s, 10, floor=0) for s, v in enumerate([128] + trace[:-1])] == trace
    # 128 -> 32 and stays
    assert ftrace[:951] == trace[:951] and ftrace[949] == 33 and ftrace[950] == 32 and set(ftrace[950:]) == {32} and trace[960] == 31
    assert T.expert_num_after(32, 10, 10, floor=32) == 32 and T.expert_num_after(128, 0, 20, floor=128) == 128
    assert T.branch_has_reader(types.SimpleNamespace(isac=False, expert_num=ftrace[-1]))
    assert T.BATCH - ftrace[-1] == 96


# ---- BranchExpert ---------------------------------------------------------------------------------------------------------------------------
def branch_expert(e0=5, m=12, k=4, n_envs=8, **kw):
    off, lab = B.make_offline(e0)
    env = types.SimpleNamespace(n=n_envs, device=torch.device("cpu"))
    return P.BranchExpert(env, torch.from_numpy(off), torch.from_numpy(lab), m, k, **kw)


def test_steps_1_is_the_parents_object():
    for be in (branch_expert(), branch_expert(steps=1)):
        assert be.steps == 1 and be.work is None
        assert set(be.state_dict()) == {"online", "success", "call", "online_rows", "per_step", "offline_rows"}
        with pytest.raises(Exception, match="steps = 1"):
            be.counters()


def test_workspace_and_state_round_trip():
    a = branch_expert(steps=8)
    assert a.steps == 8 and a.kpad == 64 and a.work.dtype == torch.uint8 and a.work.numel() == 64 * 228 == S.workspace_bytes(4) and not bool(a.work.any())
    assert branch_expert(m=80, k=65, n_envs=70, steps=2).work.numel() == 128 * 228
    assert a.counters() == (0, 0, 0)
    model = S.StepsModel(np.zeros((17, 32), np.float32), np.zeros(17, np.int8), 5, 12, 4, 8)
    model.cnt[:, :6] = np.arange(18, dtype=np.uint64).reshape(3, 6) + np.uint64(2 ** 33)  # (lanes 4, 5 are beyond k: not summed)
    model.age[:4] = [1, 7, 0, 3]
    a.work.copy_(torch.from_numpy(model.image()))
    assert a.counters() == model.counters() == tuple(4 * 2 ** 33 + sum(range(6 * i, 6 * i + 4)) for i in range(3))
    a.call = 2 ** 33 + 7
    st = a.state_dict()
    assert set(st) == {"online", "success", "call", "online_rows", "per_step", "offline_rows", "steps", "work"} and st["steps"] == 8
    assert not st["work"].is_cuda and np.array_equal(st["work"].numpy(), model.image())
    a.work.zero_()  # (the snapshot is a copy)
    b = branch_expert(steps=8)
    b.load_state_dict(st)
    assert b.call == 2 ** 33 + 7 and np.array_equal(b.work.numpy(), model.image()) and b.counters() == model.counters()
    with pytest.raises(ValueError, match="--expert_branch_steps 8, this run has --expert_branch_steps 9"):
        branch_expert(steps=9).load_state_dict(st)
    with pytest.raises(ValueError, match="--expert_branch_steps 8, this run has --expert_branch_steps 1"):
        branch_expert().load_state_dict(st)
    with pytest.raises(ValueError, match="--expert_branch_steps 1, this run has --expert_branch_steps 8"):
        branch_expert(steps=8).load_state_dict(branch_expert().state_dict())
    for steps in (0, -1, 65536):
        with pytest.raises(ValueError, match=f"BranchExpert: steps {steps}"):
            branch_expert(steps=steps)
    assert branch_expert(steps=65535).steps == 65535
    with pytest.raises(Exception, match="GPU only"):
        a.push()


# ---- the driver's flags ---------------------------------------------------------------------------------------------------------------------
HIRL = ["--agent", "HIRL", "--type", "soft", "--num_envs", "32"]
ESAC = ["--agent", "SAC", "--type", "ESAC", "--synthetic_expert", "--num_envs", "32"]
ISAC = ["--agent", "SAC", "--type", "ISAC", "--synthetic_expert", "--bc_actor", "x", "--num_envs", "32"]
ON = ["--expert_branch", "64", "--expert_branch_per_step", "8"]
STEPS = ON + ["--expert_branch_steps", "8"]


def test_parser_defaults():
    cfg = T.parse_args(HIRL)
    assert cfg.expert_branch_steps == 1 and cfg.expert_floor == 0
    assert T.expert_branch_refusal(cfg) is None and T.expert_floor_refusal(cfg) is None
    cfg = T.parse_args(HIRL + ON)
    assert cfg.expert_branch_steps == 1 and T.expert_branch_refusal(cfg) is None


def test_expert_branch_steps_is_taken_where_expert_branch_is():
    for base in (HIRL, ESAC, ISAC):
        cfg = T.parse_args(base + STEPS)
        assert cfg.expert_branch_steps == 8 and T.expert_branch_refusal(cfg) is None
    for extra in (["--type", "linear"], ["--type", "fixed"], ["--dtype", "bf16"], ["--dtype", "f32x9"], ["--loop", "reference"], ["--separate_launches"],
                  ["--env", "mixed"], ["--expert_online", "64", "--expert_online_per_step", "8"], ["--expert_floor", "32"]):
        assert T.expert_branch_refusal(T.parse_args(HIRL + STEPS + extra)) is None, extra
    for extra in (["--dtype", "bf16"], ["--loop", "reference"], ["--separate_launches"], ["--env", "mixed"], ["--expert_floor", "32"]):
        assert T.expert_branch_refusal(T.parse_args(ESAC + STEPS + extra)) is None, extra
    for h in ("1", "2", "1500", "65535"):
        assert T.expert_branch_refusal(T.parse_args(HIRL + ON + ["--expert_branch_steps", h])) is None


def test_expert_branch_steps_refusals():
    cases = [(HIRL + ["--expert_branch_steps", "8"], r"--expert_branch_steps 8 goes with --expert_branch ROWS > 0"),
             (HIRL + ON + ["--expert_branch_steps", "0"], r"--expert_branch_steps 0: .*1 .* to 65,535"),
             (HIRL + ON + ["--expert_branch_steps", "-3"], r"--expert_branch_steps -3"),
             (HIRL + ON + ["--expert_branch_steps", "65536"], r"--expert_branch_steps 65536"),
             (HIRL + ["--expert_branch_steps", "0"], r"--expert_branch_steps 0"),
             (["--agent", "TD3", "--num_envs", "32"] + STEPS, r"\(TD3 reads no expert ring\)"),
             (["--agent", "SAC", "--type", "SAC", "--num_envs", "32"] + STEPS, r"--agent SAC --type SAC reads no expert ring"),
             (ESAC + STEPS + ["--per"], "--expert_branch does not go with --per"),
             (HIRL + STEPS + ["--gpus", "2"], "--expert_branch runs on one GPU")]
    for argv, why in cases:
        got = T.expert_branch_refusal(T.parser().parse_args(argv))
        assert got is not None and re.search(why, got), (argv, got)
        with pytest.raises(SystemExit):
            T.parse_args(argv)


def test_expert_floor_is_taken_and_refused_by_name():
    for base in (HIRL, HIRL + ["--type", "linear"], HIRL + ["--type", "fixed"], ESAC, HIRL + ON, ESAC + STEPS, HIRL + ["--loop", "reference"],
                 HIRL + ["--dtype", "bf16"], HIRL + ["--env", "mixed"]):
        for n in ("0", "1", "32", "128"):
            cfg = T.parse_args(base + ["--expert_floor", n])
            assert cfg.expert_floor == int(n) and T.expert_floor_refusal(cfg) is None
    cases = [(["--agent", "TD3", "--num_envs", "32", "--expert_floor", "32"], r"--expert_floor goes with --agent HIRL and --agent SAC --type ESAC \(--agent TD3"),
             (["--agent", "BC", "--num_envs", "32", "--expert_floor", "32"], r"--expert_floor goes with .*\(--agent BC"),
             (["--agent", "SAC", "--type", "SAC", "--num_envs", "32", "--expert_floor", "32"], r"--expert_floor goes with .*\(--agent SAC --type SAC"),
             (ISAC + ["--expert_floor", "32"], r"--expert_floor goes with .*\(--agent SAC --type ISAC .*no expert_num"),
             (ESAC + ["--per", "--expert_floor", "32"], "--expert_floor does not go with --per"),
             (HIRL + ["--expert_floor", "-1"], "--expert_floor -1"),
             (HIRL + ["--expert_floor", "129"], "--expert_floor 129: .* to the batch of 128")]
    for argv, why in cases:
        got = T.expert_floor_refusal(T.parser().parse_args(argv))
        assert got is not None and re.search(why, got), (argv, got)
        with pytest.raises(SystemExit):
            T.parse_args(argv)


def test_resume_refusals():
    cfg = lambda *a_: T.parser().parse_args(HIRL + list(a_))  # noqa: E731
    on = ("--expert_branch", "12", "--expert_branch_per_step", "4")
    one, eight = {"episode": 1, "expert_branch": branch_expert().state_dict()}, {"episode": 1, "expert_branch": branch_expert(steps=8).state_dict()}
    assert T.expert_branch_resume_refusal(cfg(*on), one) is None and T.expert_branch_resume_refusal(cfg(*on, "--expert_branch_steps", "8"), eight) is None
    assert T.expert_branch_resume_refusal(cfg(*on, "--expert_branch_steps", "8"), None) is None
    assert "--expert_branch_steps 8, --expert_branch_steps 1 given" in T.expert_branch_resume_refusal(cfg(*on), eight)
    assert "--expert_branch_steps 8, --expert_branch_steps 9 given" in T.expert_branch_resume_refusal(cfg(*on, "--expert_branch_steps", "9"), eight)
    assert "--expert_branch_steps 1, --expert_branch_steps 8 given" in T.expert_branch_resume_refusal(cfg(*on, "--expert_branch_steps", "8"), one)
    assert "--expert_branch 12, --expert_branch 0 given" in T.expert_branch_resume_refusal(cfg(), eight)
    # --expert_floor
    assert T.expert_floor_resume_refusal(cfg(), {"episode": 1}) is None and T.expert_floor_resume_refusal(cfg("--expert_floor", "32"), None) is None
    assert T.expert_floor_resume_refusal(cfg("--expert_floor", "32"), {"episode": 1, "expert_floor": 32}) is None
    assert "--expert_floor 0, --expert_floor 32 given" in T.expert_floor_resume_refusal(cfg("--expert_floor", "32"), {"episode": 1})
    assert "--expert_floor 32, --expert_floor 0 given" in T.expert_floor_resume_refusal(cfg(), {"episode": 1, "expert_floor": 32})
    assert "--expert_floor 32, --expert_floor 16 given" in T.expert_floor_resume_refusal(cfg("--expert_floor", "16"), {"episode": 1, "expert_floor": 32})


def test_the_snapshot_record_carries_both():
    run = types.SimpleNamespace(env_type="straight_line", estats=None, online=None, branch=branch_expert(steps=8), expert_floor=32)
    rec = T.stats_record(run)
    assert rec["expert_floor"] == 32 and rec["expert_branch"]["steps"] == 8
    run = types.SimpleNamespace(env_type="straight_line", estats=None, online=None, branch=branch_expert(), expert_floor=0)
    rec = T.stats_record(run)
    assert "expert_floor" not in rec and "steps" not in rec["expert_branch"]
