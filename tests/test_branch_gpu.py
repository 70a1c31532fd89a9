"""GPU tests of expert branches (hx_pilot_branch; utils.pilot.BranchExpert; train_all --expert_branch) against the CPU model of the rule,
tests/_branch_model.py (the pilot's numpy model + the C oracle's env step), and against the product's own hx_pilot_act + hx_env_step — bit for bit
everywhere but the engines' logged losses (sums of float atomics: rtol 1e-6 / atol 1e-7, the bar identical launches are held to elsewhere in the suite).
Smallest shapes that can still go wrong: 1 env, 63, one full workgroup (64), one pick more (65), 130 and 300 (ragged tails); the state at a pitch
(320) that is not the number of envs; online regions that are no multiple of the picks per call, so the FIFO wraps inside a call."""
import functools
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _branch_model as B  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _pilot_model as PM  # noqa: E402

STRIDE, GUARD, POISON = 320, 64, 0x7FC0DEAD


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import pilot

    return pilot


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def inputs(n, seed):
    return B.make_inputs(n, seed=seed)


def padded_state(state):
    """[37, n] -> a device tensor [37, STRIDE] (int32 bits) whose columns behind n are poison"""
    full = np.full((37, STRIDE), POISON, np.int32)
    full[:, :state.shape[1]] = state.view(np.int32)
    return dev(full)


def branch_call(s, n, o, ring, success, e0, m, k, call):
    from hirl4ucav_amd import _lib

    _lib.call("hx_pilot_branch", s.data_ptr(), n, STRIDE, o.data_ptr(), ring.data_ptr(), success.data_ptr(), e0, m, k, call, _lib.stream_ptr())
    torch.cuda.synchronize()


class RawBranch:
    """hx_pilot_branch over a ring with guard rows behind it and success bytes with guard bytes behind them, fed from arrays (no env)"""

    def __init__(self, n, k, m, e0, call=0):
        self.n, self.k, self.m, self.e0, self.call = n, k, m, e0, call
        off, lab = B.make_offline(e0)
        ring0, succ0 = B.initial_ring(off, lab, m)
        self.model = B.BranchModel(ring0, succ0, e0, m, k, call)
        full = np.full((e0 + m + 2, 32), POISON, np.int32)
        full[:e0 + m] = ring0.view(np.int32)
        sfull = np.full(e0 + m + GUARD, 0x5A, np.int8)
        sfull[:e0 + m] = succ0
        self.ring, self.success, self.off, self.lab = dev(full), dev(sfull), off, lab

    def push(self, state, obs):
        s, o = padded_state(state), dev(obs)
        s0, o0 = s.clone(), o.clone()
        branch_call(s, self.n, o, self.ring, self.success, self.e0, self.m, self.k, self.call)
        assert torch.equal(s, s0) and torch.equal(bits(o), bits(o0)), "state / obs were written"
        self.call += 1
        return self.model.push(state, obs)

    def check(self, what):
        t, b, end = self.ring.cpu().numpy(), self.success.cpu().numpy(), self.e0 + self.m
        assert (t[end:] == POISON).all() and (b[end:] == 0x5A).all(), what + ": guard rows / bytes"
        assert np.array_equal(t[:self.e0], self.off.view(np.int32)) and np.array_equal(b[:self.e0], self.lab), what + ": offline rows / labels"
        assert np.array_equal(t[self.e0:end], self.model.ring[self.e0:].view(np.int32)), what + ": online rows"
        assert np.array_equal(b[self.e0:end], self.model.success[self.e0:]), what + ": online success bytes"


# (n, k, M, E0): k from 1 to min(n, M); M no multiple of k wherever k > 1
CASES = [(1, 1, 3, 2), (63, 63, 100, 5), (64, 64, 100, 5), (65, 1, 3, 2), (65, 64, 100, 5), (65, 65, 66, 3), (130, 7, 50, 40), (130, 130, 137, 1), (300, 64, 100, 5),
         (300, 300, 301, 7)]


@pytest.mark.parametrize("n,k,m,e0", CASES)
def test_branch_equals_the_model(P, n, k, m, e0):
    """enough calls to wrap the online region twice (at most 9); after EVERY call ring, success bytes, offline part, guards, state and obs bit for bit"""
    assert k == 1 or m % k
    raw = RawBranch(n, k, m, e0)
    raw.check("start")
    calls, wrote_all, skipped = min(2 * -(-m // k) + 1, 9), 0, 0
    for c in range(calls):
        state, obs = inputs(n, c % 3)
        wrote = raw.push(state, obs)
        raw.check(f"call {c}")
        wrote_all, skipped = wrote_all + len(wrote), skipped + k - len(wrote)
    assert wrote_all > 0 and raw.call == calls
    if k == n >= 16:
        assert skipped == 2 * calls  # the NaN state word and the infinite observation word, every call
        assert set(np.unique(raw.model.success[e0:])) == {-1, 0, 1} and (raw.model.ring[e0:, 31] == 1).any() and (raw.model.ring[e0:, 30] > 500).any()


@pytest.mark.parametrize("call0", [2 ** 32 - 2, 2 ** 40])
@pytest.mark.parametrize("n,k,m,e0", [(65, 64, 100, 5), (300, 7, 50, 40)])
def test_branch_at_large_call_counts(P, n, k, m, e0, call0):
    """call is a 64-bit count: carried across 2^32 (2^32 - 2 .. 2^32 + 1), and 2^40 .. 2^40 + 3"""
    raw = RawBranch(n, k, m, e0, call=call0)
    for c in range(4):
        raw.push(*inputs(n, c % 3))
        raw.check(f"call {call0} + {c}")
    assert raw.call == call0 + 4


def product_step(s, n, o):
    """hx_pilot_act (no noise) + hx_env_step with no ring, no auto-reset and no time limit on CLONES -> actions, next obs, reward, done, success"""
    from hirl4ucav_amd import _lib

    sc, oc = s.clone(), o.clone()
    act = torch.zeros((n, 4), device="cuda")
    reward, done, succ = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int8, device="cuda")
    _lib.call("hx_pilot_act", sc.data_ptr(), n, sc.shape[1], oc.data_ptr(), None, act.data_ptr(), _lib.stream_ptr())
    _lib.call("hx_env_step", sc.data_ptr(), n, sc.shape[1], act.data_ptr(), oc.data_ptr(), reward.data_ptr(), done.data_ptr(), succ.data_ptr(), None, _lib.stream_ptr())
    return act, oc, reward, done, succ


def mismatches(rows, byte, o, act, nobs, reward, done, succ):
    """per env: the branch row [s | a | s' | r | done] and its success byte against the product's own launches, bit for bit -> bool [n] (True: differs)"""
    want = torch.cat([bits(o), bits(act), bits(nobs), bits(reward)[:, None], bits(done.float())[:, None]], 1)
    return (bits(rows) != want).any(1) | (byte != succ)


def test_branch_equals_the_products_own_step_on_edge_states(P):
    """k = n = 300, call 0: pick j is env j and its slot is E0 + j.  Every row that was written equals hx_pilot_act + hx_env_step on clones bit for
    bit; the two non-finite envs left their slots alone (the ring starts as poison there)"""
    n, e0 = 300, 4
    state, obs = inputs(n, 0)
    s, o = padded_state(state), dev(obs)
    ring = torch.full((e0 + n + 1, 32), POISON, dtype=torch.int32, device="cuda")
    success = torch.full((e0 + n + 1,), 0x5A, dtype=torch.int8, device="cuda")
    branch_call(s, n, o, ring, success, e0, n + 1, n, 0)
    act, nobs, reward, done, succ = product_step(s.view(torch.float32), n, o)
    rows, byte = ring[e0:e0 + n].view(torch.float32), success[e0:e0 + n]
    written = ~(ring[e0:e0 + n] == POISON).all(1)
    bad = sorted({B.CLASSES["nan_state"], B.CLASSES["inf_obs"]})
    assert (~written).nonzero().flatten().tolist() == bad and bool((byte[~written] == 0x5A).all())
    assert not bool(mismatches(rows, byte, o, act, nobs, reward, done, succ)[written].any())
    assert bool((ring[:e0] == POISON).all()) and bool((ring[e0 + n:] == POISON).all()) and bool((success[:e0] == 0x5A).all()) and bool((success[e0 + n:] == 0x5A).all())
    got = {name: (float(rows[i, 30]), float(rows[i, 31]), int(byte[i])) for name, i in B.CLASSES.items() if i not in bad}
    assert got["fire_good"][2] == 1 and got["fire_nolock"][2] == -1 and got["fire_empty"][2] == 0 and got["missile_hit"][0] > 500 and got["missile_hit"][1] == 1
    assert got["alt_low"][1] == 1 and got["alt_high"][1] == 1 and got["band_low"][1] == 0 and got["band_high"][1] == 0


@pytest.mark.parametrize("scenario", ["straight_line", "serpentine", "circular", "mixed"])
def test_branch_equals_the_products_own_step_in_flight(P, scenario):
    """64 real envs flown by the pilot: 700 steps without a look (the approach), then 500 steps with a branch of EVERY env before each step, compared on
    the device with hx_pilot_act + hx_env_step on clones (no auto-reset there; the flight itself resets its envs).  One host read at the end: no row
    differs, every row was written, and locks, launches under a lock and kills all occurred in the branch rows"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    n, e0, m = 64, 3, 65
    scen = (np.arange(n) % 3).astype(np.int32) if scenario == "mixed" else scenario
    env = BatchedHarfangEnv(n, scenario=scen, seed=7, auto_reset=True, random_reset=True)
    env.reset()
    for _ in range(700):
        env.step(P.device_pilot_actions(env))
    off, lab = B.make_offline(e0)
    be = P.BranchExpert(env, dev(off), dev(lab), m, n)
    differ = torch.zeros((), dtype=torch.int64, device="cuda")
    unwritten, locks, launches, kills, dones = (torch.zeros((), dtype=torch.int64, device="cuda") for _ in range(5))
    for t in range(500):
        state0, obs0 = env.state.clone(), env.obs.clone()
        slots = torch.tensor(PM.slots(be.call, n, m, e0), device="cuda")
        picks = torch.tensor(PM.env_picks(be.call, n, n), device="cuda")
        be.ring.ring[slots] = float("nan")
        be.push()
        act, nobs, reward, done, succ = product_step(env.state, n, env.obs)
        rows, byte = be.ring.ring[slots], be.ring.success[slots]
        differ += mismatches(rows, byte, env.obs[picks], act[picks], nobs[picks], reward[picks], done[picks], succ[picks]).sum()
        unwritten += torch.isnan(rows).any(1).sum()
        locks, launches = locks + (rows[:, 7] > 0).sum(), launches + (byte == 1).sum()
        kills, dones = kills + ((rows[:, 30] > 300) & (rows[:, 31] == 1) & (rows[:, 29] == 0)).sum(), dones + (rows[:, 31] == 1).sum()
        differ += (bits(env.state) != bits(state0)).sum() + (bits(env.obs) != bits(obs0)).sum()  # the branch left the flight alone
        env.step(act)
    got = [int(v) for v in (differ, unwritten, locks, launches, kills, dones)]
    print(f"{scenario}: rows that differ {got[0]}, unwritten {got[1]}, locked rows {got[2]}, launches under a lock {got[3]}, kills {got[4]}, done rows {got[5]}")
    assert got[0] == 0 and got[1] == 0 and got[2] > 0 and got[3] > 0 and got[4] > 0 and got[5] >= got[4]  # (every kill is a done row)
    assert torch.equal(be.ring.ring[:e0], dev(off)) and torch.equal(be.ring.success[:e0], dev(lab)) and be.call == 500


def test_branch_refusals(P):
    from hirl4ucav_amd import _lib

    n, k, m, e0 = 65, 64, 100, 5
    raw = RawBranch(n, k, m, e0)
    state, obs = inputs(n, 0)
    s, o, t, b = padded_state(state), dev(obs), raw.ring, raw.success
    good = (s.data_ptr(), n, STRIDE, o.data_ptr(), t.data_ptr(), b.data_ptr(), e0, m, k, 0, _lib.stream_ptr())

    def swap(i, v):
        return good[:i] + (v,) + good[i + 1:]

    for bad in (swap(0, None), swap(1, 0), swap(1, -1), swap(2, n - 1), good[:1] + (1 << 31, 1 << 31) + good[3:], swap(3, None), swap(4, None),
                swap(4, t.data_ptr() + 64), swap(4, t.data_ptr() + 4), swap(5, None), swap(6, -1), swap(6, (1 << 31) - m), swap(7, 0), swap(7, 1 << 31), swap(8, 0),
                swap(8, -3), swap(8, n + 1), good[:7] + (32, 33) + good[9:], good[:7] + (64, 65) + good[9:]):
        with pytest.raises(_lib.HxError, match=r"hx_pilot_branch failed \(-1\)"):
            _lib.call("hx_pilot_branch", *bad)
    torch.cuda.synchronize()
    raw.check("after the refusals")  # nothing was written
    env = types.SimpleNamespace(n=8, device=torch.device("cuda"))
    off, lab = B.make_offline(5)
    for rows, per in ((0, 1), (4, 5), (16, 9), (4, 0)):
        with pytest.raises(ValueError, match="BranchExpert"):
            P.BranchExpert(env, dev(off), dev(lab), rows, per)


# ---- engines ---------------------------------------------------------------------------------------------------------------------------------
HIRL_NETS = ("actor", "target_actor", "bc_actor", "critic", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic", "wstate", "soft_count")
HIRL_COUNTERS = ("critic_step", "actor_step", "update_count", "sample_calls", "upsample_calls", "actor_trainable")
SAC_STATE = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i")
SAC_COUNTERS = ("learning_steps", "sample_calls", "expert_calls")


def ring_copy(r):
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    c = DeviceReplay(r.capacity)
    c.ring.copy_(r.ring)
    c.success.copy_(r.success)
    c.total.copy_(r.total)
    c.fixed_len = r.fixed_len
    return c


def live_branches(P, online=1024, per=32):
    """a main ring, a BC table, and a BranchExpert over the shared expert rows behind a real env of 96"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    data = D.make_data(2)
    rep = DeviceReplay(D.N_REPLAY)
    rep.store_rows(torch.from_numpy(data["replay"]))
    bc = np.zeros((D.N_EXPERT, 32), np.float32)
    bc[:, 0:13], bc[:, 13:17] = data["expert_s"], data["expert_a"]
    env = BatchedHarfangEnv(96, scenario="straight_line", seed=5, auto_reset=True, random_reset=True, max_step=40)
    env.reset()
    labels = torch.from_numpy(np.random.default_rng(3).choice([-1, 0, 1], D.N_EXPERT_ROWS).astype(np.int8))
    be = P.BranchExpert(env, torch.from_numpy(data["expert_rows"]).cuda(), labels.cuda(), online, per)
    return rep, torch.from_numpy(bc).cuda(), env, be


def fly_and_push(P, env, be, call, g):
    for _ in range(5):
        env.step(P.device_pilot_actions(env) if call == 2 else torch.rand((96, 4), device="cuda", generator=g) * 2 - 1)
        be.push()


def assert_losses(live, ref, what):
    la, lb = np.asarray(live.losses.cpu().numpy(), np.float32), np.asarray(ref.losses.cpu().numpy(), np.float32)
    print(f"{what}: losses bit-equal {np.array_equal(la.view(np.uint32), lb.view(np.uint32))}, max |diff| {np.abs(la - lb).max():.3g}")
    np.testing.assert_allclose(la, lb, rtol=1e-6, atol=1e-7)


def reached(rows, be, start):
    """minibatch rows that equal a REWRITTEN online row of the live ring"""
    lo, hi = be.offline_rows, be.offline_rows + be.rows_written()
    changed = be.ring.ring[lo:hi][(bits(be.ring.ring[lo:hi]) != bits(start[lo:hi])).any(1)]
    return int((bits(rows.view(-1, 32))[:, None, :] == bits(changed)[None]).all(-1).any(1).sum())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_hirl_engine_reads_the_live_ring(P, dtype):
    """after some pushes through a real env, sample() + learn() with the live branch ring equal the same calls on a copy of it: networks, moments,
    soft weight and counters bit for bit, the logged losses at rtol 1e-6 / atol 1e-7.  The expert rows of the minibatch reach into rewritten rows."""
    from hirl4ucav_amd.agents import engine as E

    params = D.make_params(1)
    rep, bc_table, env, be = live_branches(P)
    start = be.ring.ring.clone()
    assert be.ring.ring.data_ptr() % 128 == 0 and len(be.ring) == D.N_EXPERT_ROWS + 1024
    engines = []
    for _ in range(2):
        eng = E.HirlEngine(batch=128)
        eng.load_params(params["actor"], params["critic"], params["bc_actor"])
        if dtype == "bf16":
            eng.set_act_dtype("bf16")
            eng.set_update_dtype("bf16")
        engines.append(eng)
    live, ref = engines
    g, hits = torch.Generator(device="cuda").manual_seed(4), 0
    for call in (1, 2, 3):
        fly_and_push(P, env, be, call, g)
        copy = ring_copy(be.ring)
        for eng, expert in ((live, be.ring), (ref, copy)):
            eng.sample(rep, expert, bc_table, n_main=40, seed=21, defer=(call != 1))
            eng.learn(bc_weight_now=100 if call == 1 else None)
        torch.cuda.synchronize()
        assert torch.equal(live._idx, ref._idx) and torch.equal(bits(live.rows), bits(ref.rows)), call
        hits += reached(live.rows.view(-1, 32)[40:], be, start)
        for name in HIRL_NETS:
            assert torch.equal(bits(getattr(live, name)), bits(getattr(ref, name))), (call, name)
        assert [getattr(live, c) for c in HIRL_COUNTERS] == [getattr(ref, c) for c in HIRL_COUNTERS]
        assert_losses(live, ref, f"HIRL {dtype} call {call}")
    e0 = D.N_EXPERT_ROWS
    assert hits > 0 and be.call == 15 and be.rows_written() == 480
    assert torch.equal(be.ring.ring[:e0], start[:e0]) and torch.equal(be.ring.ring[e0 + 480:], start[e0 + 480:]) and bool(torch.isfinite(be.ring.ring).all())
    other = P.BranchExpert(env, start[:e0], be.ring.success[:e0], 1024, 32)
    other.load_state_dict(be.state_dict())
    assert other.call == 15 and torch.equal(bits(other.ring.ring), bits(be.ring.ring)) and torch.equal(other.ring.success, be.ring.success)


@pytest.mark.parametrize("kind", ["ESAC", "ISAC"])
def test_sac_engine_reads_the_live_ring(P, kind):
    """the same for SacEngine: E-SAC's expert rows in the minibatch, ISAC's second batch — networks, moments, alpha state, counters bit for bit"""
    from hirl4ucav_amd.agents import sac_engine as SE
    from tests.test_isac_gpu import bc_actor_params
    from tests.test_oracle_sac import sac_params

    params = sac_params()
    rep, _, env, be = live_branches(P)
    start = be.ring.ring.clone()
    engines = []
    for _ in range(2):
        eng = SE.SacEngine(batch=128)
        eng.load_params(params["policy"], params["q1"], params["q2"])
        if kind == "ISAC":
            eng.set_imitative(bc_actor_params(), slope=0.01)
        engines.append(eng)
    live, ref = engines
    g, hits = torch.Generator(device="cuda").manual_seed(4), 0
    for call in (1, 2, 3):
        fly_and_push(P, env, be, call, g)
        copy = ring_copy(be.ring)
        for eng, expert in ((live, be.ring), (ref, copy)):
            eng.sample(rep, expert if kind == "ESAC" else None, n_main=40, seed=21, defer=(call != 1))
            if kind == "ISAC":
                eng.sample_expert(expert, seed=21, defer=(call != 1))
            eng.learn()
        torch.cuda.synchronize()
        assert torch.equal(bits(live.rows), bits(ref.rows)), call
        if kind == "ISAC":
            assert torch.equal(live._expert_idx, ref._expert_idx) and torch.equal(bits(live.expert_rows), bits(ref.expert_rows)), call
        hits += reached(live.expert_rows if kind == "ISAC" else live.rows.view(-1, 32)[40:], be, start)
        for name in SAC_STATE:
            assert torch.equal(bits(getattr(live, name)), bits(getattr(ref, name))), (call, name)
        assert [getattr(live, c) for c in SAC_COUNTERS] == [getattr(ref, c) for c in SAC_COUNTERS]
        assert_losses(live, ref, f"{kind} call {call}")
    assert hits > 0 and be.call == 15 and bool(torch.isfinite(be.ring.ring).all())


# ---- train_all -------------------------------------------------------------------------------------------------------------------------------
COMMON = ["--env", "straight_line", "--random", "--seed", "3", "--num_envs", "64", "--buffer_size", "4096", "--max_step", "12", "--checkpoint_rate", "1000",
          "--snapshot_every", "1", "--synthetic_expert"]
HIRL = ["--agent", "HIRL", "--type", "soft"] + COMMON
BRANCH = ["--expert_branch", "96", "--expert_branch_per_step", "40"]  # (96 is no multiple of 40: the FIFO wraps inside the third call)
EXPLORE = 4  # ceil(20 * 12 / 64) exploration steps


class Recorder:
    """stands in for the scalar writer: every add_scalar call"""

    def __init__(self, *_):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass

    def close(self):
        pass


def spy(monkeypatch):
    """-> (names of every library call, the runs' states as load_expert_tables left them with a copy of the expert ring, the writers)"""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd import train_all as T

    names, runs, writers, real_call, real_load = [], [], [], _lib.call, T.load_expert_tables

    def load(run):
        real_load(run)
        runs.append((run, run.expert.ring.clone(), run.expert.success.clone()))

    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real_call(name, *a))
    monkeypatch.setattr(T, "load_expert_tables", load)
    monkeypatch.setattr(T, "make_writer", lambda d: writers.append(Recorder()) or writers[-1])
    return names, runs, writers


def agent_args(kind, tmp_path):
    if kind == "ESAC":
        return ["--agent", "SAC", "--type", "ESAC"] + COMMON
    if kind == "ISAC":
        from tests.test_isac_gpu import bc_actor_params

        f = tmp_path / "bc_actor.pth"
        torch.save({k: torch.from_numpy(v) for k, v in bc_actor_params().items()}, f)
        return ["--agent", "SAC", "--type", "ISAC", "--bc_actor", str(f)] + COMMON
    return HIRL + ["--loop", kind]


@pytest.mark.parametrize("kind", ["front", "reference", "ESAC", "ISAC"])
def test_train_all_expert_branch(P, tmp_path, monkeypatch, capsys, kind):
    """2 driver episodes of 12 steps at 64 envs: one branch launch behind every acting launch, exploration included; the online region has left its
    initial fill, the offline rows and labels stand, every row is finite and a transition; the snapshot carries what the ring holds; the scalar is
    the host's count"""
    from hirl4ucav_amd import train_all as T

    names, runs, writers = spy(monkeypatch)
    out_dir = T.main(T.parse_args(agent_args(kind, tmp_path) + BRANCH + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    if kind in ("front", "reference"):
        assert ("vector loop: front launch" if kind == "front" else "vector loop: reference order") in out
        assert (names.count("hx_hirl_front") > 0) == (kind == "front")
    run, start, start_succ = runs[0]
    e0 = run.branch.offline_rows
    assert names.count("hx_pilot_branch") == EXPLORE + 2 * 12 == run.branch.call and run.expert is run.branch.ring
    assert run.expert.capacity == e0 + 96 + 10 and len(run.expert) == e0 + 96 == run.expert.fixed_len
    fill = torch.arange(96, device="cuda") % e0
    assert torch.equal(start[e0:e0 + 96], start[fill]) and torch.equal(start_succ[e0:e0 + 96], start_succ[fill])  # the initial fill, labels too
    ring, succ = run.expert.ring, run.expert.success
    assert torch.equal(ring[:e0], start[:e0]) and torch.equal(succ[:e0], start_succ[:e0]) and torch.equal(ring[e0 + 96:], start[e0 + 96:])
    on = ring[e0:e0 + 96]
    assert not bool((on == start[e0:e0 + 96]).all(1).any()) and bool(torch.isfinite(on).all())  # every online row was rewritten (28 calls of 40)
    assert bool((on[:, 16].abs() == 1).all()) and bool((on[:, 13:16].abs() <= 1).all()) and bool(((on[:, 31] == 0) | (on[:, 31] == 1)).all())
    assert bool((on[:, 29] >= 0).all()) and bool((on[:, 30] < 0).all()) and bool((succ[e0:e0 + 96].abs() <= 1).all())
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]["expert_branch"]
    assert snap["call"] == run.branch.call and (snap["online_rows"], snap["per_step"], snap["offline_rows"]) == (96, 40, e0)
    assert torch.equal(bits(snap["online"]), bits(on.cpu())) and torch.equal(snap["success"], succ[e0:e0 + 96].cpu())
    assert [(v, s) for t, v, s in writers[0].rows if t == "Expert/Branch Rows Written"] == [(96.0, 0), (96.0, 1)]


def test_train_all_expert_branch_resume(P, tmp_path, monkeypatch):
    """--separate_launches (one env workgroup: the run is reproducible), together with --expert_online: 1 episode + --resume to 2 equals the
    uninterrupted run bit for bit — networks, moments, replay ring, the branch rows and their labels (the arena but its logged loss slots, sums of
    float atomics: rtol 1e-6 / atol 1e-7, the one tolerance of this file).  --resume under other values of either flag is refused by name."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.agents.engine import HirlEngine

    args = HIRL + BRANCH + ["--separate_launches", "--expert_online", "64", "--expert_online_per_step", "8"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a, b, h = (torch.load(os.path.join(d, "state_rank0.pt"), map_location="cpu", weights_only=False) for d in (whole, rest, half))
    oa, ob, oh = a["driver"]["expert_branch"], b["driver"]["expert_branch"], h["driver"]["expert_branch"]
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and oa["call"] == ob["call"] == EXPLORE + 24 and oh["call"] == EXPLORE + 12
    assert torch.equal(bits(oa["online"]), bits(ob["online"])) and torch.equal(oa["success"], ob["success"]) and not torch.equal(oa["online"], oh["online"])
    assert torch.equal(bits(a["driver"]["expert_online"]["online"]), bits(b["driver"]["expert_online"]["online"]))
    assert a["engine"]["counters"] == b["engine"]["counters"]
    e = HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    print(f"resume: loss slots {x[lo:lo + 8].tolist()} against {y[lo:lo + 8].tolist()}, bit-equal {torch.equal(x[lo:lo + 8].view(torch.int32), y[lo:lo + 8].view(torch.int32))}")
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-6, atol=1e-7)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] and torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32))
    online = ["--expert_online", "64", "--expert_online_per_step", "8"]
    for other, word in ((["--expert_branch", "48", "--expert_branch_per_step", "40"] + online, "--expert_branch 96, --expert_branch 48 given"),
                        (["--expert_branch", "96", "--expert_branch_per_step", "4"] + online, "--expert_branch_per_step 40, --expert_branch_per_step 4 given"),
                        (online, "--expert_branch 96, --expert_branch 0 given")):
        with pytest.raises(SystemExit, match=word):
            T.main(T.parse_args(HIRL + other + ["--separate_launches", "--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))


def test_train_all_switch_off_is_the_parent_path(P, tmp_path, monkeypatch):
    """--expert_branch 0 (the default): run.expert is the ring the parent builds — label_expert's rows stored into a DeviceReplay 10 rows longer —, no
    hx_pilot_branch call is made, nothing of it is logged or stored; switched on, the run makes one launch more per acting launch and nothing else;
    a snapshot written without it is refused under it; each refusal exits with its message"""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    names, runs, writers = spy(monkeypatch)
    cfg = T.parse_args(HIRL + ["--episodes", "1", "--result_dir", str(tmp_path / "a")])
    out_dir = T.main(cfg)
    plain = len(names)  # (before this test's own labelling call)
    run, start, start_succ = runs[0]
    labelled = [T.label_expert(es_k, ea_k, run.device) for es_k, ea_k in T.load_expert_files(cfg)]
    rows, succ = torch.cat([r for r, _ in labelled]), torch.cat([s_ for _, s_ in labelled])
    parent = DeviceReplay(rows.shape[0] + 10, run.device)
    parent.store_rows(rows, succ)
    assert run.branch is None and type(run.expert) is DeviceReplay and run.expert.capacity == parent.capacity and run.expert.fixed_len == parent.fixed_len
    assert torch.equal(bits(run.expert.ring), bits(parent.ring)) and torch.equal(run.expert.success, parent.success) and torch.equal(run.expert.total, parent.total)
    assert torch.equal(bits(start), bits(parent.ring)) and torch.equal(start_succ, parent.success)
    assert names and "hx_pilot_branch" not in names
    assert not [t for t, _, _ in writers[0].rows if t.startswith("Expert/")]
    assert "expert_branch" not in torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]
    del names[:]
    T.main(T.parse_args(HIRL + BRANCH + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    assert names.count("hx_pilot_branch") == EXPLORE + 12 and len(names) - names.count("hx_pilot_branch") == plain
    with pytest.raises(SystemExit, match="--expert_branch 0, --expert_branch 96 given"):
        T.main(T.parse_args(HIRL + BRANCH + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", out_dir]))
    for argv, word in ((["--agent", "TD3"] + COMMON + BRANCH, "TD3 reads no expert ring"), (["--agent", "BC"] + COMMON + BRANCH, "--agent BC reads no expert ring"),
                       (["--agent", "SAC", "--type", "SAC"] + COMMON + BRANCH, "--agent SAC --type SAC reads no expert ring"),
                       (["--agent", "SAC", "--type", "ESAC", "--per"] + COMMON + BRANCH, "--per with --type ESAC"),  # (--per's own refusal stands in front)
                       (HIRL + ["--expert_branch", "96", "--expert_branch_per_step", "65"], "--expert_branch_per_step 65"),
                       (HIRL + ["--expert_branch", "-2"], "--expert_branch -2")):
        ns = T.parser().parse_args(argv + ["--result_dir", str(tmp_path / "e")])
        with pytest.raises(SystemExit, match=word):
            T.main(ns)
