"""Host-side tests of expert branches (no GPU): the CPU model of tests/_branch_model.py on its seeded inputs — every edge class is met by a pick and
does what its name says, checked here against the C oracle's step —, the picks and slots at 64-bit call counts, BranchExpert's ring (initial cyclic
fill with labels, total, state round trip), the parser's flags and every refusal of --expert_branch by name; --expert_online's refusals as before."""
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hirl4ucav_amd import train_all as T  # noqa: E402
from hirl4ucav_amd.utils import pilot as P  # noqa: E402
from tests import _branch_model as B  # noqa: E402
from tests import _oracle as ox  # noqa: E402
from tests import _pilot_model as PM  # noqa: E402

N = 300


@pytest.fixture(scope="module")
def stepped():
    state, obs = B.make_inputs(N)
    state0, obs0 = state.copy(), obs.copy()
    rows, succ, after = B.step_once(state, obs)
    # the model works on a copy: the inputs stand, bit for bit
    assert np.array_equal(state.view(np.uint32), state0.view(np.uint32)) and np.array_equal(obs.view(np.uint32), obs0.view(np.uint32))
    return state, obs, rows, succ, after


def flags(state, i):
    return int(state[B.FLAGS].view(np.uint32)[i])


def script(state, i):
    return int(state[B.COUNTERS].view(np.uint32)[i]) >> 16


def test_every_class_is_picked():
    """with k = n every env is a pick of call 0; with k = 64 every planted env is picked within n calls (pick 0 walks the population)"""
    assert sorted(PM.env_picks(0, N, N)) == list(range(N))
    seen = set()
    for call in range(N):
        seen.update(PM.env_picks(call, N, 64))
    assert set(B.CLASSES.values()) <= seen and max(B.CLASSES.values()) < N


def test_fire_with_lock_and_loaded_rail(stepped):
    state, obs, rows, succ, after = stepped
    i = B.CLASSES["fire_good"]
    assert rows[i, 16] == 1 and succ[i] == 1 and flags(after, i) & ox.F_FIRE_SUCCESS and flags(after, i) & ox.F_M_ACTIVE and not flags(after, i) & ox.F_SIM_SLOT
    assert np.isfinite(rows[i]).all()


def test_fire_without_lock(stepped):
    state, obs, rows, succ, after = stepped
    i = B.CLASSES["fire_nolock"]
    assert rows[i, 16] == 1 and succ[i] == -1 and not flags(after, i) & ox.F_FIRE_SUCCESS and np.isfinite(rows[i]).all()


def test_fire_on_an_empty_rail_still_pays(stepped):
    """step_success 0, no missile leaves, and the reward is 8 below the same env's reward when the stored observation shows the empty rail"""
    state, obs, rows, succ, after = stepped
    i = B.CLASSES["fire_empty"]
    assert rows[i, 16] == 1 and succ[i] == 0 and not flags(after, i) & ox.F_M_ACTIVE and np.isfinite(rows[i]).all()
    quiet = obs.copy()
    quiet[i, 8] = -1.0
    rows_q, succ_q, _ = B.step_once(state, quiet)
    assert rows_q[i, 16] == -1 and succ_q[i] == 0 and rows[i, 30] == np.float32(rows_q[i, 30] - np.float32(8.0))


def test_missile_in_flight_hits_on_this_step(stepped):
    state, obs, rows, succ, after = stepped
    i = B.CLASSES["missile_hit"]
    assert flags(state, i) & ox.F_M_ACTIVE and state[B.HEALTH, i] == np.float32(0.2)
    assert not flags(after, i) & ox.F_M_ACTIVE and after[B.HEALTH, i] == 0 and rows[i, 29] == 0  # s'[12]: the opponent's health
    assert rows[i, 31] == 1 and flags(after, i) & ox.F_EPISODE_SUCCESS and rows[i, 16] == -1 and succ[i] == 0
    unlatched = state.copy()  # the same step without the fire-success latch: the kill pays nothing
    unlatched[B.FLAGS].view(np.uint32)[i] &= ~np.uint32(ox.F_FIRE_SUCCESS)
    rows_u, _, _ = B.step_once(unlatched, obs)
    assert rows_u[i, 31] == 1 and rows[i, 30] > 500 and rows[i, 30] == np.float32(rows_u[i, 30] + np.float32(600.0))  # (the reward's last operation)


def fma32(a, b, c):
    """fmaf on fp32 values (the product of two fp32 values is exact in float64)"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def reward_of(after, row, i):
    """_get_reward (HarfangEnv_GYM.py:101-137) of env i restated in fp32, operation by operation in wrap_step's order, from the stepped state and the row's
    own entries -> (reward, how many 4-point altitude penalties it holds)"""
    f32 = np.float32
    d = [f32(after[B.OPP_P + c, i] - after[B.ALLY_P + c, i]) for c in range(3)]
    dist = np.sqrt(fma32(d[2], d[2], fma32(d[1], d[1], f32(d[0] * d[0]))))
    r = f32(f32(0.0) - f32(f32(0.0001) * dist))
    r = f32(r - f32(row[23] * f32(10.0)))  # s'[6]: the target angle / 180
    alt, bands = after[B.ALLY_P + 1, i], 0
    for hit in (alt < f32(2000.0), alt > f32(7000.0)):
        if hit:
            r, bands = f32(r - f32(4.0)), bands + 1
    if row[16] > 0:
        r = f32(r - f32(8.0))
    return r, bands


@pytest.mark.parametrize("name,done", [("alt_low", 1.0), ("alt_high", 1.0), ("band_low", 0.0), ("band_high", 0.0)])
def test_altitude_edges(stepped, name, done):
    """below 500 / above 10,000: done; 1,500 / 7,500: not done; each pays exactly ONE 4-point penalty: the row's reward equals the reward rule
    restated in fp32 on the stepped state, bit for bit — and so does every other finite row that has no kill in it, most of them with no penalty"""
    state, obs, rows, succ, after = stepped
    i = B.CLASSES[name]
    assert rows[i, 31] == done and bool(flags(after, i) & ox.F_DONE) == bool(done) and np.isfinite(rows[i]).all()
    want, bands = reward_of(after, rows[i], i)
    assert bands == 1 and rows[i, 30] == want, (name, rows[i, 30], want)
    plain = [e for e in range(N) if np.isfinite(rows[e]).all() and after[B.HEALTH, e] >= np.float32(0.1)]
    got = [reward_of(after, rows[e], e) for e in plain]
    assert len(plain) == N - 3 and all(rows[e, 30] == w for e, (w, _) in zip(plain, got))
    assert sum(1 for _, b_ in got if b_ == 0) > N // 2 and sorted(e for e, (_, b_) in zip(plain, got) if b_) == sorted(B.CLASSES[k] for k in ("alt_low", "alt_high", "band_low", "band_high"))


@pytest.mark.parametrize("name", ["nan_state", "inf_obs"])
def test_non_finite_rows_are_skipped(stepped, name):
    state, obs, rows, succ, after = stepped
    i = B.CLASSES[name]
    assert not np.isfinite(rows[i]).all()
    off, lab = B.make_offline(7)
    ring, success = B.initial_ring(off, lab, N + 1)
    model = B.BranchModel(ring, success, 7, N + 1, N)
    wrote = model.push(state, obs)
    slot = PM.slots(0, N, N + 1, 7)[PM.env_picks(0, N, N).index(i)]
    assert (i, slot) not in wrote and np.array_equal(model.ring[slot], ring[slot]) and model.success[slot] == success[slot]
    assert len(wrote) == N - 2 and np.isfinite(model.ring).all() and model.call == 1
    assert np.array_equal(model.ring[:7], off) and np.array_equal(model.success[:7], lab)
    assert set(np.unique(model.success[7:])) == {-1, 0, 1}
    e, s = wrote[0]
    assert np.array_equal(model.ring[s], rows[e]) and model.success[s] == succ[e]


def test_each_scenario_and_the_script_phase_changes(stepped):
    state, obs, rows, succ, after = stepped
    scen = (state[B.FLAGS].view(np.uint32) >> ox.F_SCEN_SHIFT) & 3
    assert np.array_equal(scen, np.arange(N) % 3)
    i = B.CLASSES["serp_phase"]
    assert scen[i] == 1 and script(state, i) == 249 and script(after, i) == 0
    assert (flags(state, i) ^ flags(after, i)) & ox.F_SERP_POS and flags(after, i) & ox.F_SERP_LONG and not flags(state, i) & ox.F_SERP_LONG
    j = B.CLASSES["circ_phase"]
    assert scen[j] == 2 and script(state, j) == 99 and script(after, j) == 100
    other = [e for e in range(N) if e % 3 == 1 and e != i]
    assert all(script(after, e) == script(state, e) + 1 for e in other)  # (no other serpentine env changes phase)
    assert np.isfinite(rows[i]).all() and np.isfinite(rows[j]).all()


def test_row_layout(stepped):
    """[s | a_E | s' | r | done]; the action is the pilot's on the state words, the fire entry follows the STORED observation"""
    state, obs, rows, succ, after = stepped
    act = PM.actions(state, obs)
    ok = np.isfinite(rows).all(1)
    assert ok.sum() == N - 2
    assert np.array_equal(rows[ok, 0:13], obs[ok]) and np.array_equal(rows[ok, 13:17], act[ok])
    assert np.array_equal(rows[ok, 16] == 1, (obs[ok, 7] > 0) & (obs[ok, 8] > 0)) and set(np.unique(rows[ok, 31])) == {0.0, 1.0}
    assert np.array_equal(rows[ok, 29], after[B.HEALTH, ok]) and (np.abs(rows[ok, 13:16]) <= 1).all()


@pytest.mark.parametrize("n,k,m,e0", [(300, 7, 50, 40), (65, 64, 100, 5), (300, 130, 131, 1)])
def test_picks_and_slots_at_large_calls(n, k, m, e0):
    assert m % k
    for call in (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40):
        picks, slots = PM.env_picks(call, n, k), PM.slots(call, k, m, e0)
        assert picks == [(call % n + j * (n // k)) % n for j in range(k)] and len(set(picks)) == k
        assert slots == [e0 + ((call % m) * k % m + j) % m for j in range(k)] and len(set(slots)) == k  # (the residues the host forms)
        nxt = PM.slots(call + 1, k, m, e0)
        assert nxt[0] - e0 == (slots[-1] - e0 + 1) % m  # FIFO across the wrap
    assert P.rows_written(0, k, m) == 0 and P.rows_written(1, k, m) == k and P.rows_written(2 ** 40, k, m) == m


def branch_expert(e0=5, m=12, k=4, n_envs=8):
    off, lab = B.make_offline(e0)
    env = types.SimpleNamespace(n=n_envs, device=torch.device("cpu"))
    return P.BranchExpert(env, torch.from_numpy(off), torch.from_numpy(lab), m, k), off, lab


def test_branch_expert_initial_fill():
    be, off, lab = branch_expert()
    ring, success = B.initial_ring(off, lab, 12)
    assert be.ring.capacity == 5 + 12 + 10 and int(be.ring.total.item()) == 17 == len(be.ring) == be.ring.fixed_len
    assert np.array_equal(be.ring.ring[:17].numpy(), ring) and np.array_equal(be.ring.success[:17].numpy(), success)
    for i in range(12):
        assert np.array_equal(be.ring.ring[5 + i].numpy(), off[i % 5]) and int(be.ring.success[5 + i]) == int(lab[i % 5])
    assert bool((be.ring.ring[17:] == 0).all()) and be.call == 0 and be.rows_written() == 0
    with pytest.raises(Exception, match="GPU only"):
        be.push()
    env = types.SimpleNamespace(n=8, device=torch.device("cpu"))
    for rows, labels, m, k, why in ((torch.zeros(5, 31), torch.zeros(5, dtype=torch.int8), 12, 4, "fp32 .rows, 32"),
                                    (torch.zeros(5, 32, dtype=torch.float64), torch.zeros(5, dtype=torch.int8), 12, 4, "fp32 .rows, 32"),
                                    (torch.zeros(5, 32), torch.zeros(4, dtype=torch.int8), 12, 4, "int8 .5"),
                                    (torch.zeros(5, 32), torch.zeros(5, dtype=torch.int32), 12, 4, "int8 .5"),
                                    (torch.zeros(5, 32), torch.zeros(5, dtype=torch.int8), 0, 1, "online_rows 0"),
                                    (torch.zeros(5, 32), torch.zeros(5, dtype=torch.int8), 12, 0, "per_step 0"),
                                    (torch.zeros(5, 32), torch.zeros(5, dtype=torch.int8), 12, 9, "per_step 9"),
                                    (torch.zeros(5, 32), torch.zeros(5, dtype=torch.int8), 4, 5, "per_step 5"),
                                    (torch.zeros(0, 32), torch.zeros(0, dtype=torch.int8), 4, 2, "offline table is empty")):
        with pytest.raises(ValueError, match="BranchExpert: .*" + why):
            P.BranchExpert(env, rows, labels, m, k)


def test_branch_expert_state_round_trip():
    a, off, lab = branch_expert()
    a.ring.ring[5:17] = torch.arange(12 * 32, dtype=torch.float32).view(12, 32)
    a.ring.success[5:17] = torch.tensor([-1, 0, 1] * 4, dtype=torch.int8)
    a.call = 2 ** 33 + 7
    st = a.state_dict()
    assert set(st) == {"online", "success", "call", "online_rows", "per_step", "offline_rows"} and not st["online"].is_cuda
    assert (st["online_rows"], st["per_step"], st["offline_rows"]) == (12, 4, 5) and st["success"].dtype == torch.int8
    a.ring.ring[5:17] = 0  # (the snapshot is a copy)
    a.ring.success[5:17] = 0
    b, _, _ = branch_expert()
    b.load_state_dict(st)
    assert b.call == 2 ** 33 + 7 and torch.equal(b.ring.ring[5:17], torch.arange(12 * 32, dtype=torch.float32).view(12, 32))
    assert torch.equal(b.ring.success[5:17], torch.tensor([-1, 0, 1] * 4, dtype=torch.int8))
    assert np.array_equal(b.ring.ring[:5].numpy(), off) and np.array_equal(b.ring.success[:5].numpy(), lab) and int(b.ring.total.item()) == 17
    with pytest.raises(ValueError, match="--expert_branch 12 --expert_branch_per_step 4"):
        branch_expert(k=3)[0].load_state_dict(st)
    with pytest.raises(ValueError, match="--expert_branch 12"):
        branch_expert(m=16)[0].load_state_dict(st)
    with pytest.raises(ValueError, match="offline expert rows"):
        branch_expert(e0=6)[0].load_state_dict(st)


HIRL = ["--agent", "HIRL", "--type", "soft", "--num_envs", "32"]
ESAC = ["--agent", "SAC", "--type", "ESAC", "--synthetic_expert", "--num_envs", "32"]
ISAC = ["--agent", "SAC", "--type", "ISAC", "--synthetic_expert", "--bc_actor", "x", "--num_envs", "32"]
ON = ["--expert_branch", "64", "--expert_branch_per_step", "8"]


def test_parser_flags_and_refusals():
    cfg = T.parse_args(HIRL)
    assert cfg.expert_branch == 0 and cfg.expert_branch_per_step == 64 and T.expert_branch_refusal(cfg) is None
    for base in (HIRL, ESAC, ISAC):
        cfg = T.parse_args(base + ON)
        assert (cfg.expert_branch, cfg.expert_branch_per_step) == (64, 8) and T.expert_branch_refusal(cfg) is None
    for extra in (["--type", "linear"], ["--type", "fixed"], ["--dtype", "bf16"], ["--dtype", "f32x9"], ["--loop", "reference"], ["--separate_launches"],
                  ["--env", "mixed"], ["--expert_online", "64", "--expert_online_per_step", "8"]):
        assert T.expert_branch_refusal(T.parse_args(HIRL + ON + extra)) is None, extra
    for extra in (["--dtype", "bf16"], ["--loop", "reference"], ["--separate_launches"], ["--env", "mixed"]):
        assert T.expert_branch_refusal(T.parse_args(ESAC + ON + extra)) is None, extra
    cases = [(["--agent", "TD3", "--num_envs", "32"] + ON, r"--expert_branch goes with --agent HIRL, .*\(TD3 reads no expert ring\)"),
             (["--agent", "BC", "--num_envs", "32"] + ON, r"--expert_branch goes with --agent HIRL, .*\(--agent BC reads no expert ring"),
             (["--agent", "SAC", "--type", "SAC", "--num_envs", "32"] + ON, r"--expert_branch goes with .*\(--agent SAC --type SAC reads no expert ring\)"),
             (ESAC + ON + ["--per"], "--expert_branch does not go with --per .the weighted call drops the expert rows"),
             (HIRL + ON + ["--gpus", "2"], "--expert_branch runs on one GPU"),
             (HIRL + ["--expert_branch", "-1"], "--expert_branch -1"),
             (HIRL + ["--expert_branch", "64", "--expert_branch_per_step", "0"], "--expert_branch_per_step 0"),
             (HIRL + ["--expert_branch", "16", "--expert_branch_per_step", "17"], "--expert_branch_per_step 17"),
             (HIRL + ["--expert_branch", "64", "--expert_branch_per_step", "33"], "--expert_branch_per_step 33")]
    for argv, why in cases:
        got = T.expert_branch_refusal(T.parser().parse_args(argv))
        assert got is not None and re.search(why, got), (argv, got)
        with pytest.raises(SystemExit):
            T.parse_args(argv)
    assert "--gpus" in T.expert_branch_refusal(T.parser().parse_args(HIRL + ON), world=2)


def test_resume_refusals():
    st = branch_expert()[0].state_dict()
    driver = {"episode": 1, "expert_branch": st}
    cfg = lambda *a_: T.parser().parse_args(HIRL + list(a_))  # noqa: E731
    assert T.expert_branch_resume_refusal(cfg("--expert_branch", "12", "--expert_branch_per_step", "4"), driver) is None
    assert T.expert_branch_resume_refusal(cfg("--expert_branch", "12", "--expert_branch_per_step", "4"), None) is None
    assert "--expert_branch 12, --expert_branch 16 given" in T.expert_branch_resume_refusal(cfg("--expert_branch", "16", "--expert_branch_per_step", "4"), driver)
    assert "--expert_branch_per_step 4, --expert_branch_per_step 2 given" in T.expert_branch_resume_refusal(cfg("--expert_branch", "12", "--expert_branch_per_step", "2"), driver)
    assert "--expert_branch 12, --expert_branch 0 given" in T.expert_branch_resume_refusal(cfg(), driver)
    assert "--expert_branch 0, --expert_branch 12 given" in T.expert_branch_resume_refusal(cfg("--expert_branch", "12", "--expert_branch_per_step", "4"), {"episode": 1})
    assert T.expert_branch_resume_refusal(cfg(), {"episode": 1}) is None
    # a snapshot of --expert_online alone is one without branches, and the other way round
    assert T.expert_branch_resume_refusal(cfg(), {"episode": 1, "expert_online": {"online_rows": 12, "per_step": 4}}) is None
    assert T.expert_online_resume_refusal(cfg(), driver) is None


def test_expert_online_refusals_are_as_before():
    """--expert_online keeps its words: still refused for the SAC family by the sentence that names what was not built for it"""
    on = ["--num_envs", "32", "--expert_online", "64", "--expert_online_per_step", "8"]
    for argv, why in ((["--agent", "SAC", "--type", "ESAC", "--synthetic_expert"] + on, "--expert_online goes with --agent HIRL .SAC / ESAC / ISAC draw expert TRANSITIONS"),
                      (["--agent", "SAC", "--type", "SAC"] + on, "relabelling r, s' and done there is not built"),
                      (["--agent", "TD3"] + on, "--expert_online goes with --agent HIRL .TD3 reads no expert table"),
                      (["--agent", "BC"] + on, "--expert_online goes with --agent HIRL .--agent BC has no rollouts"),
                      (HIRL + ["--gpus", "2", "--expert_online", "64", "--expert_online_per_step", "8"], "--expert_online runs on one GPU"),
                      (HIRL + ["--expert_online", "16", "--expert_online_per_step", "17"], "--expert_online_per_step 17")):
        got = T.expert_online_refusal(T.parser().parse_args(argv))
        assert got is not None and re.search(why, got), (argv, got)
    assert T.expert_online_refusal(T.parse_args(HIRL + ["--expert_online", "64", "--expert_online_per_step", "8"] + ON)) is None


def test_branches_are_pushed_only_while_the_ring_has_a_reader():
    """after_env_step: HIRL and E-SAC push while expert_num > 0 and no longer once the warm-up's expert rows have run out; ISAC's expert batch reads the
    ring for the whole run"""
    pushes = []
    branch = types.SimpleNamespace(push=lambda: pushes.append(1))
    run = types.SimpleNamespace(inserter=None, estats=None, online=None, branch=branch, per=False, per_new="max", upsampler=None, ret=None, isac=False,
                                expert_num=2)
    for expert_num, isac, want in ((2, False, 1), (1, False, 2), (0, False, 2), (0, True, 3), (0, False, 3)):
        run.expert_num, run.isac = expert_num, isac
        T.after_env_step(run, 5)
        assert len(pushes) == want, (expert_num, isac)
    assert T.branch_has_reader(types.SimpleNamespace(isac=False, expert_num=128)) and not T.branch_has_reader(types.SimpleNamespace(isac=False, expert_num=0))
    n = 128
    for step in range(1, 1281):  # expert_num_after: 0 after batch * warm_up_rate steps, for good
        n = T.expert_num_after(n, step, 10)
    assert n == 0 and T.expert_num_after(0, 10, 10) == 0
