"""GPU tests of expert branches of up to H steps (hx_pilot_branch_steps; utils.pilot.BranchExpert(steps=H); train_all --expert_branch_steps /
--expert_floor) against the CPU model of the conveyor rule, tests/_branch_steps_model.py, against hx_pilot_branch (H = 1) and against the product's own
hx_pilot_act + hx_env_step flown on a clone — bit for bit everywhere but the engines' logged losses (sums of float atomics: rtol 1e-6 / atol 1e-7, as in
tests/test_branch_gpu.py, whose helpers this file uses).  Shapes as there: 1 env, 63, 64, 65, 130 and 300 at a pitch of 320, k from 1 to n, online
regions that are no multiple of k; H = 1, 2 (every second call reseeds), 8 (the cap inside a test's calls) and 400 (never the cap)."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _branch_model as B  # noqa: E402
from tests import _branch_steps_model as S  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _pilot_model as PM  # noqa: E402
from tests import test_branch_gpu as G  # noqa: E402  (helpers only)

STRIDE, GUARD, POISON = G.STRIDE, G.GUARD, G.POISON
dev, bits, inputs, padded_state = G.dev, G.bits, G.inputs, G.padded_state


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import pilot

    return pilot


def steps_call(s, n, o, ring, success, e0, m, k, h, call, work, kpad=None):
    from hirl4ucav_amd import _lib

    _lib.call("hx_pilot_branch_steps", s.data_ptr(), n, STRIDE, o.data_ptr(), ring.data_ptr(), success.data_ptr(), e0, m, k, h, call, work.data_ptr(),
              S.kpad(k) if kpad is None else kpad, _lib.stream_ptr())
    torch.cuda.synchronize()


def start_image(k, zero_ages=True):
    """a workspace of 0xA5 bytes — the guard pattern of columns k..kpad, and what bstate / bobs start as — with the first k ages and counters zeroed"""
    model = S.StepsModel(np.zeros((1, 32), np.float32), np.zeros(1, np.int8), 0, 1, k, 2, work=np.full(S.workspace_bytes(k), 0xA5, np.uint8))
    if zero_ages:
        model.age[:k] = 0
    model.cnt[:, :k] = 0
    return model.image()


class RawSteps:
    """hx_pilot_branch_steps over a ring, success bytes and a workspace with guards behind each, fed from arrays (no env), beside the model"""

    def __init__(self, n, k, m, e0, h, call=0, zero_ages=True):
        self.n, self.k, self.m, self.e0, self.h, self.call = n, k, m, e0, h, call
        off, lab = B.make_offline(e0)
        ring0, succ0 = B.initial_ring(off, lab, m)
        self.image0 = start_image(k, zero_ages)
        self.model = S.StepsModel(ring0, succ0, e0, m, k, h, call, work=self.image0)
        full = np.full((e0 + m + 2, 32), POISON, np.int32)
        full[:e0 + m] = ring0.view(np.int32)
        sfull = np.full(e0 + m + GUARD, 0x5A, np.int8)
        sfull[:e0 + m] = succ0
        wfull = np.full(S.workspace_bytes(k) + 256, 0x5A, np.uint8)
        wfull[:S.workspace_bytes(k)] = self.image0
        self.ring, self.success, self.work, self.off, self.lab = dev(full), dev(sfull), dev(wfull), off, lab

    def push(self, state, obs):
        s, o = padded_state(state), dev(obs)
        s0, o0 = s.clone(), o.clone()
        steps_call(s, self.n, o, self.ring, self.success, self.e0, self.m, self.k, self.h, self.call, self.work)
        assert torch.equal(s, s0) and torch.equal(bits(o), bits(o0)), "state / obs were written"
        self.call += 1
        return self.model.push(state, obs)

    def check(self, what):
        t, b, w, end, nb = self.ring.cpu().numpy(), self.success.cpu().numpy(), self.work.cpu().numpy(), self.e0 + self.m, S.workspace_bytes(self.k)
        assert (t[end:] == POISON).all() and (b[end:] == 0x5A).all() and (w[nb:] == 0x5A).all(), what + ": guard rows / bytes / workspace guard"
        assert np.array_equal(t[:self.e0], self.off.view(np.int32)) and np.array_equal(b[:self.e0], self.lab), what + ": offline rows / labels"
        assert np.array_equal(t[self.e0:end], self.model.ring[self.e0:].view(np.int32)), what + ": online rows"
        assert np.array_equal(b[self.e0:end], self.model.success[self.e0:]), what + ": online success bytes"
        img = self.model.image()
        if not np.array_equal(w[:nb], img):
            kp, at = S.kpad(self.k), int(np.nonzero(w[:nb] != img)[0][0])
            raise AssertionError(f"{what}: workspace differs first at byte {at} (word {at // 4 // kp}, column {at // 4 % kp} of the 32-bit part, kpad {kp})")
        cols = w[:51 * 4 * S.kpad(self.k)].reshape(51, S.kpad(self.k), 4)[:, self.k:]
        assert (cols == 0xA5).all() and (w[51 * 4 * S.kpad(self.k):nb].reshape(3, S.kpad(self.k), 8)[:, self.k:] == 0xA5).all(), what + ": columns k..kpad"


# (n, k, M, E0, H): k from 1 to min(n, M); M no multiple of k wherever k > 1
CASES = [(1, 1, 3, 2, 2), (1, 1, 3, 2, 8), (63, 63, 100, 5, 8), (64, 64, 100, 5, 2), (64, 64, 100, 5, 400), (65, 1, 3, 2, 8), (65, 64, 100, 5, 1), (65, 64, 100, 5, 400),
         (65, 65, 66, 3, 2), (130, 7, 50, 40, 8), (130, 130, 137, 1, 400), (300, 64, 100, 5, 8), (300, 300, 301, 7, 1), (300, 300, 301, 7, 2), (300, 300, 301, 7, 8)]


@pytest.mark.parametrize("n,k,m,e0,h", CASES)
def test_steps_equal_the_model(P, n, k, m, e0, h):
    """12 calls over inputs that change between calls (a reseed reads the state of ITS call); after EVERY call ring, success bytes, the whole workspace,
    the offline part, every guard, state and obs bit for bit"""
    assert k == 1 or m % k
    raw = RawSteps(n, k, m, e0, h)
    raw.check("start")
    for c in range(12):
        raw.push(*inputs(n, c % 3))
        raw.check(f"call {c}")
    ev = raw.model.events
    assert ev["rows"] > 0 and raw.call == 12 and raw.model.counters()[0] == ev["rows"]
    if h > 1:
        assert ev["max_age"] == min(h - 1, 12) and (h > 8 or ev["cap"] > 0) and ev["seeds"] >= k
    if k == n >= 16:
        assert ev["skips"] > 0 and ev["done"] > 0 and ev["kills"] > 0


def test_the_seeded_flights_reach_every_ending(P):
    """make_inputs(16, seed=0, special=True) held static, k = 16, H = 400, M = 64, E0 = 8, 420 calls, compared after every call: kills, done rows,
    non-finite skips, reseeds by the step cap and an age of 399 all occur (tests/test_branch_steps_cpu.py asserts the same of the model alone)"""
    state, obs = B.make_inputs(16, seed=0, special=True)
    raw = RawSteps(16, 16, 64, 8, 400)
    s, o = padded_state(state), dev(obs)
    s0, o0 = s.clone(), o.clone()
    for c in range(420):
        steps_call(s, 16, o, raw.ring, raw.success, 8, 64, 16, 400, c, raw.work)
        raw.model.push(state, obs)
        raw.check(f"call {c}")
    assert torch.equal(s, s0) and torch.equal(bits(o), bits(o0))
    ev = raw.model.events
    print(f"420 calls: {ev}")
    assert ev["kills"] >= 1 and ev["done"] > ev["kills"] and ev["skips"] >= 1 and ev["cap"] >= 1 and ev["max_age"] == 399
    cnt = raw.work[51 * 4 * 64:S.workspace_bytes(16)].cpu().view(torch.int64).reshape(3, 64)[:, :16].sum(1).tolist()
    assert tuple(cnt) == raw.model.counters() == (ev["rows"], ev["done"], ev["kills"])


@pytest.mark.parametrize("call0", [2 ** 32 - 2, 2 ** 40])
@pytest.mark.parametrize("n,k,m,e0", [(65, 64, 100, 5), (300, 7, 50, 40)])
def test_steps_at_large_call_counts(P, n, k, m, e0, call0):
    """call is a 64-bit count: carried across 2^32 (2^32 - 2 .. 2^32 + 1), and 2^40 .. 2^40 + 3"""
    raw = RawSteps(n, k, m, e0, 3, call=call0)
    for c in range(4):
        raw.push(*inputs(n, c % 3))
        raw.check(f"call {call0} + {c}")
    assert raw.call == call0 + 4 and raw.model.events["cap"] > 0


@pytest.mark.parametrize("n,k,m,e0", [(65, 64, 100, 5), (300, 300, 301, 7), (130, 7, 50, 40)])
def test_one_step_is_hx_pilot_branch(P, n, k, m, e0):
    """max_steps = 1 against hx_pilot_branch on the same inputs: the same bits in ring and bytes after every call; the workspace's state, observations
    and ages keep their fill pattern (ages that are NOT zero: they are not read), only the counters move"""
    one, old = RawSteps(n, k, m, e0, 1, zero_ages=False), G.RawBranch(n, k, m, e0)
    for c in range(6):
        state, obs = inputs(n, c % 3)
        one.push(state, obs)
        old.push(state, obs)
        assert torch.equal(one.ring, old.ring) and torch.equal(one.success, old.success), c
        one.check(f"call {c}")
        old.check(f"call {c}")
    w, kp = one.work.cpu().numpy(), S.kpad(k)
    assert (w[:51 * 4 * kp] == 0xA5).all() and one.model.counters()[0] > 0
    assert np.array_equal(w[51 * 4 * kp:S.workspace_bytes(k)].view(np.uint64).reshape(3, kp)[:, :k], one.model.cnt[:, :k])


def test_a_flight_equals_the_products_own_steps(P):
    """k = n = 300 over static inputs, H = 8, M = 8 * 300: at call t lane j that has been resident since call 0 wrote the t-th step of env j.  A clone
    of the population flown 8 steps by hx_pilot_act + hx_env_step (no auto-reset, no time limit) gives the same rows and success bytes, bit for bit"""
    from hirl4ucav_amd import _lib

    n, e0, h = 300, 4, 8
    m = h * n
    state, obs = inputs(n, 0)
    s, o = padded_state(state), dev(obs)
    ring = torch.full((e0 + m + 1, 32), POISON, dtype=torch.int32, device="cuda")
    success = torch.full((e0 + m + 1,), 0x5A, dtype=torch.int8, device="cuda")
    work = torch.zeros(S.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for c in range(h):
        steps_call(s, n, o, ring, success, e0, m, n, h, c, work)
    sc, oc = s.view(torch.float32).clone(), o.clone()
    act = torch.zeros((n, 4), device="cuda")
    reward, done, succ = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int8, device="cuda")
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    compared = []
    for t in range(h):
        prev = oc.clone()
        _lib.call("hx_pilot_act", sc.data_ptr(), n, STRIDE, oc.data_ptr(), None, act.data_ptr(), _lib.stream_ptr())
        _lib.call("hx_env_step", sc.data_ptr(), n, STRIDE, act.data_ptr(), oc.data_ptr(), reward.data_ptr(), done.data_ptr(), succ.data_ptr(), None, _lib.stream_ptr())
        want = torch.cat([bits(prev), bits(act), bits(oc), bits(reward)[:, None], bits(done.float())[:, None]], 1)
        finite = torch.isfinite(want.view(torch.float32)).all(1)
        lo = e0 + t * n  # (call t, k = n: lane j writes slot E0 + t n + j)
        rows, byte = ring[lo:lo + n], success[lo:lo + n]
        here = alive & finite
        assert not bool(((rows != want).any(1) | (byte != succ))[here].any()), t
        assert bool((rows[alive & ~finite] == POISON).all()), t  # a non-finite row was not written
        compared.append(int(here.sum()))
        alive = here & (done == 0)
    print(f"rows compared per step: {compared}")
    assert compared[0] == n - 2 and compared[-1] >= n - 12 and bool((ring[e0 + m:] == POISON).all()) and bool((ring[:e0] == POISON).all())


@pytest.mark.parametrize("scenario", ["straight_line", "serpentine", "circular", "mixed"])
def test_real_envs_are_left_alone_and_reseeds_read_the_current_state(P, scenario):
    """64 real envs stepped between the calls, 16 resident branches of 8 steps: push() changes neither the env state nor obs; a lane that (re)seeds at
    this call writes hx_pilot_act + hx_env_step's row of the CURRENT state of its pick; a resident lane's s is the s' it wrote one call earlier"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    n, k, e0, m, h = 64, 16, 3, 48, 8
    scen = (np.arange(n) % 3).astype(np.int32) if scenario == "mixed" else scenario
    env = BatchedHarfangEnv(n, scenario=scen, seed=7, auto_reset=True, random_reset=True)
    env.reset()
    for _ in range(40):
        env.step(P.device_pilot_actions(env))
    off, lab = B.make_offline(e0)
    be = P.BranchExpert(env, dev(off), dev(lab), m, k, steps=h)
    ages = be.work[50 * 4 * 64:51 * 4 * 64].view(torch.int32)[:k]
    differ, chained, seeded_rows, resident_rows = (torch.zeros((), dtype=torch.int64, device="cuda") for _ in range(4))
    last = None
    for t in range(48):
        state0, obs0 = env.state.clone(), env.obs.clone()
        seeded = ages.clone() == 0
        slots = torch.tensor(PM.slots(be.call, k, m, e0), device="cuda")
        picks = torch.tensor(PM.env_picks(be.call, n, k), device="cuda")
        be.push()
        differ += (bits(env.state) != bits(state0)).sum() + (bits(env.obs) != bits(obs0)).sum()
        act, nobs, reward, done, succ = G.product_step(env.state, n, env.obs)
        rows, byte = be.ring.ring[slots], be.ring.success[slots]
        bad = G.mismatches(rows, byte, env.obs[picks], act[picks], nobs[picks], reward[picks], done[picks], succ[picks])
        differ += bad[seeded].sum()
        if last is not None:
            chained += (bits(rows[:, 0:13]) != bits(last[:, 17:30])).any(1)[~seeded].sum()
        seeded_rows, resident_rows, last = seeded_rows + seeded.sum(), resident_rows + (~seeded).sum(), rows.clone()
        env.step(act)
    got = [int(v) for v in (differ, chained, seeded_rows, resident_rows)]
    print(f"{scenario}: differ {got[0]}, broken chains {got[1]}, seeded rows {got[2]}, resident rows {got[3]}, counters {be.counters()}")
    assert got[0] == 0 and got[1] == 0 and got[2] >= 6 * k and got[3] >= 40 * k - k and be.counters()[0] == 48 * k
    assert torch.equal(be.ring.ring[:e0], dev(off)) and torch.equal(be.ring.success[:e0], dev(lab)) and be.call == 48


def test_steps_refusals(P):
    from hirl4ucav_amd import _lib

    n, k, m, e0, h = 65, 64, 100, 5, 8
    raw = RawSteps(n, k, m, e0, h)
    state, obs = inputs(n, 0)
    s, o, t, b, w = padded_state(state), dev(obs), raw.ring, raw.success, raw.work
    good = (s.data_ptr(), n, STRIDE, o.data_ptr(), t.data_ptr(), b.data_ptr(), e0, m, k, h, 0, w.data_ptr(), 64, _lib.stream_ptr())

    def swap(i, v):
        return good[:i] + (v,) + good[i + 1:]

    for bad in (swap(0, None), swap(1, 0), swap(1, -1), swap(2, n - 1), good[:1] + (1 << 31, 1 << 31) + good[3:], swap(3, None), swap(4, None),
                swap(4, t.data_ptr() + 64), swap(4, t.data_ptr() + 4), swap(5, None), swap(6, -1), swap(6, (1 << 31) - m), swap(7, 0), swap(7, 1 << 31), swap(8, 0),
                swap(8, -3), swap(8, n + 1), good[:7] + (32, 33) + good[9:], good[:7] + (64, 65) + good[9:],
                swap(9, 0), swap(9, -1), swap(9, 65536), swap(11, None), swap(11, w.data_ptr() + 4), swap(11, w.data_ptr() + 8), swap(12, 0), swap(12, 63),
                swap(12, 128), swap(12, -64)):
        with pytest.raises(_lib.HxError, match=r"hx_pilot_branch_steps failed \(-1\)"):
            _lib.call("hx_pilot_branch_steps", *bad)
    torch.cuda.synchronize()
    raw.check("after the refusals")  # nothing was written
    L = _lib.load()
    assert [int(L.hx_branch_workspace_bytes(v)) for v in (-1, 0, 1, 64, 65, 300)] == [0, 0, 64 * 228, 64 * 228, 128 * 228, 320 * 228]
    env = types.SimpleNamespace(n=8, device=torch.device("cuda"))
    off, lab = B.make_offline(5)
    for steps in (0, 65536):
        with pytest.raises(ValueError, match="BranchExpert: steps"):
            P.BranchExpert(env, dev(off), dev(lab), 8, 4, steps=steps)


# ---- engines ---------------------------------------------------------------------------------------------------------------------------------
def live_flights(P, online=1024, per=32, steps=8):
    """tests/test_branch_gpu.live_branches with resident branches"""
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
    be = P.BranchExpert(env, torch.from_numpy(data["expert_rows"]).cuda(), labels.cuda(), online, per, steps=steps)
    return rep, torch.from_numpy(bc).cuda(), env, be


@pytest.mark.parametrize("kind", ["f32", "bf16", "ESAC", "ISAC"])
def test_engines_read_the_live_ring(P, kind):
    """after some pushes through a real env, sample() + learn() with the live ring of resident branches equal the same calls on a copy of it: networks,
    moments and counters bit for bit, the logged losses at rtol 1e-6 / atol 1e-7; the expert rows of the minibatch reach into rewritten rows"""
    rep, bc_table, env, be = live_flights(P)
    start = be.ring.ring.clone()
    hirl = kind in ("f32", "bf16")
    engines = []
    for _ in range(2):
        if hirl:
            from hirl4ucav_amd.agents import engine as E

            params = D.make_params(1)
            eng = E.HirlEngine(batch=128)
            eng.load_params(params["actor"], params["critic"], params["bc_actor"])
            if kind == "bf16":
                eng.set_act_dtype("bf16")
                eng.set_update_dtype("bf16")
        else:
            from hirl4ucav_amd.agents import sac_engine as SE
            from tests.test_isac_gpu import bc_actor_params
            from tests.test_oracle_sac import sac_params

            params = sac_params()
            eng = SE.SacEngine(batch=128)
            eng.load_params(params["policy"], params["q1"], params["q2"])
            if kind == "ISAC":
                eng.set_imitative(bc_actor_params(), slope=0.01)
        engines.append(eng)
    live, ref = engines
    g, hits = torch.Generator(device="cuda").manual_seed(4), 0
    for call in (1, 2, 3):
        G.fly_and_push(P, env, be, call, g)
        copy = G.ring_copy(be.ring)
        for eng, expert in ((live, be.ring), (ref, copy)):
            if hirl:
                eng.sample(rep, expert, bc_table, n_main=40, seed=21, defer=(call != 1))
                eng.learn(bc_weight_now=100 if call == 1 else None)
            else:
                eng.sample(rep, expert if kind == "ESAC" else None, n_main=40, seed=21, defer=(call != 1))
                if kind == "ISAC":
                    eng.sample_expert(expert, seed=21, defer=(call != 1))
                eng.learn()
        torch.cuda.synchronize()
        assert torch.equal(bits(live.rows), bits(ref.rows)), call
        hits += G.reached(live.expert_rows if kind == "ISAC" else live.rows.view(-1, 32)[40:], be, start)
        for name in (G.HIRL_NETS if hirl else G.SAC_STATE):
            assert torch.equal(bits(getattr(live, name)), bits(getattr(ref, name))), (call, name)
        counters = G.HIRL_COUNTERS if hirl else G.SAC_COUNTERS
        assert [getattr(live, c) for c in counters] == [getattr(ref, c) for c in counters]
        G.assert_losses(live, ref, f"{kind} call {call}")
    e0 = D.N_EXPERT_ROWS
    assert hits > 0 and be.call == 15 and be.rows_written() == 480 and be.counters()[0] == 480
    assert torch.equal(be.ring.ring[:e0], start[:e0]) and torch.equal(be.ring.ring[e0 + 480:], start[e0 + 480:]) and bool(torch.isfinite(be.ring.ring).all())
    other = P.BranchExpert(env, start[:e0], be.ring.success[:e0], 1024, 32, steps=8)
    other.load_state_dict(be.state_dict())
    assert other.call == 15 and torch.equal(bits(other.ring.ring), bits(be.ring.ring)) and torch.equal(other.work, be.work) and other.counters() == be.counters()


# ---- train_all -------------------------------------------------------------------------------------------------------------------------------
COMMON, HIRL, BRANCH, EXPLORE = G.COMMON, G.HIRL, G.BRANCH, G.EXPLORE
STEPS = BRANCH + ["--expert_branch_steps", "8"]


def load_snapshot(out_dir):
    return torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)


@pytest.mark.parametrize("kind", ["front", "reference", "ESAC", "ISAC"])
def test_train_all_expert_branch_steps(P, tmp_path, monkeypatch, capsys, kind):
    """2 driver episodes of 12 steps at 64 envs with --expert_branch_steps 8: one hx_pilot_branch_steps launch behind every acting launch, exploration
    included, and no hx_pilot_branch; the online region has left its initial fill and holds finite transitions; the snapshot carries H and the
    workspace; the three scalars are written per driver episode, the two new ones from the device counters"""
    from hirl4ucav_amd import train_all as T

    names, runs, writers = G.spy(monkeypatch)
    out_dir = T.main(T.parse_args(G.agent_args(kind, tmp_path) + STEPS + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    if kind in ("front", "reference"):
        assert ("vector loop: front launch" if kind == "front" else "vector loop: reference order") in out
        assert (names.count("hx_hirl_front") > 0) == (kind == "front")
    run, start, start_succ = runs[0]
    e0 = run.branch.offline_rows
    assert names.count("hx_pilot_branch_steps") == EXPLORE + 2 * 12 == run.branch.call and "hx_pilot_branch" not in names and run.branch.steps == 8
    ring, succ = run.expert.ring, run.expert.success
    assert torch.equal(ring[:e0], start[:e0]) and torch.equal(succ[:e0], start_succ[:e0]) and torch.equal(ring[e0 + 96:], start[e0 + 96:])
    on = ring[e0:e0 + 96]
    assert not bool((on == start[e0:e0 + 96]).all(1).any()) and bool(torch.isfinite(on).all())
    assert bool((on[:, 16].abs() == 1).all()) and bool((on[:, 13:16].abs() <= 1).all()) and bool(((on[:, 31] == 0) | (on[:, 31] == 1)).all())
    snap = load_snapshot(out_dir)["driver"]["expert_branch"]
    assert snap["call"] == run.branch.call and snap["steps"] == 8 and torch.equal(snap["work"], run.branch.work.cpu())
    assert torch.equal(bits(snap["online"]), bits(on.cpu())) and torch.equal(snap["success"], succ[e0:e0 + 96].cpu())
    written, ended, kills = run.branch.counters()
    assert written == 40 * (EXPLORE + 24) and 0 <= kills <= ended <= written
    ages = run.branch.work[50 * 4 * 64:51 * 4 * 64].cpu().view(torch.int32)[:40]
    assert int(ages.max()) <= 7 and int(ages.max()) > 0
    rows = writers[0].rows
    assert [(v, s) for t, v, s in rows if t == "Expert/Branch Rows Written"] == [(96.0, 0), (96.0, 1)]
    assert [(t, s) for t, v, s in rows if t in ("Expert/Branch Episodes Ended", "Expert/Branch Kills")] == [
        ("Expert/Branch Episodes Ended", 0), ("Expert/Branch Kills", 0), ("Expert/Branch Episodes Ended", 1), ("Expert/Branch Kills", 1)]
    assert [v for t, v, s in rows if t == "Expert/Branch Episodes Ended"][-1] == float(ended) and [v for t, v, s in rows if t == "Expert/Branch Kills"][-1] == float(kills)


def test_train_all_expert_branch_steps_resume(P, tmp_path, monkeypatch):
    """--separate_launches (one env workgroup: the run is reproducible), together with --expert_online: 1 episode + --resume to 2 equals the
    uninterrupted run bit for bit — networks, moments, replay ring, the branch rows, their labels and the workspace (the arena but its logged loss
    slots: rtol 1e-6 / atol 1e-7).  --resume under another H, and under another --expert_floor, is refused by name."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.agents.engine import HirlEngine

    args = HIRL + STEPS + ["--separate_launches", "--expert_online", "64", "--expert_online_per_step", "8", "--expert_floor", "32"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a, b, h = (load_snapshot(d) for d in (whole, rest, half))
    oa, ob, oh = a["driver"]["expert_branch"], b["driver"]["expert_branch"], h["driver"]["expert_branch"]
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and oa["call"] == ob["call"] == EXPLORE + 24 and oh["call"] == EXPLORE + 12
    assert a["driver"]["expert_floor"] == b["driver"]["expert_floor"] == 32 and a["driver"]["expert_num"] == b["driver"]["expert_num"]
    assert torch.equal(bits(oa["online"]), bits(ob["online"])) and torch.equal(oa["success"], ob["success"]) and not torch.equal(oa["online"], oh["online"])
    assert torch.equal(oa["work"], ob["work"]) and not torch.equal(oa["work"], oh["work"]) and oa["steps"] == ob["steps"] == 8
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
    online = ["--separate_launches", "--expert_online", "64", "--expert_online_per_step", "8"]
    for other, word in ((BRANCH + ["--expert_branch_steps", "9", "--expert_floor", "32"], "--expert_branch_steps 8, --expert_branch_steps 9 given"),
                        (BRANCH + ["--expert_floor", "32"], "--expert_branch_steps 8, --expert_branch_steps 1 given"),
                        (STEPS + ["--expert_floor", "16"], "--expert_floor 32, --expert_floor 16 given"),
                        (STEPS, "--expert_floor 32, --expert_floor 0 given")):
        with pytest.raises(SystemExit, match=word):
            T.main(T.parse_args(HIRL + other + online + ["--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))


def test_one_step_makes_only_hx_pilot_branch_calls(P, tmp_path, monkeypatch):
    """--expert_branch_steps 1 (the default) is the parent's path: the same library calls as without the flag, none of them hx_pilot_branch_steps, no
    workspace, the parent's snapshot keys, no counter scalars; and each refusal exits with its message"""
    from hirl4ucav_amd import train_all as T

    names, runs, writers = G.spy(monkeypatch)
    T.main(T.parse_args(HIRL + BRANCH + ["--episodes", "1", "--result_dir", str(tmp_path / "a")]))
    plain = list(names)
    del names[:]
    out_dir = T.main(T.parse_args(HIRL + BRANCH + ["--expert_branch_steps", "1", "--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    assert names == plain and names.count("hx_pilot_branch") == EXPLORE + 12 and "hx_pilot_branch_steps" not in names
    run = runs[1][0]
    assert run.branch.steps == 1 and run.branch.work is None
    assert set(load_snapshot(out_dir)["driver"]["expert_branch"]) == {"online", "success", "call", "online_rows", "per_step", "offline_rows"}
    assert "expert_floor" not in load_snapshot(out_dir)["driver"]
    assert sorted({t for t, _, _ in writers[1].rows if t.startswith("Expert/")}) == ["Expert/Branch Rows Written"]
    for argv, word in ((HIRL + ["--expert_branch_steps", "8"], "--expert_branch_steps 8 goes with --expert_branch"),
                       (HIRL + BRANCH + ["--expert_branch_steps", "0"], "--expert_branch_steps 0"),
                       (HIRL + BRANCH + ["--expert_branch_steps", "65536"], "--expert_branch_steps 65536"),
                       (["--agent", "TD3"] + COMMON + ["--expert_floor", "32"], "--expert_floor goes with --agent HIRL"),
                       (["--agent", "BC"] + COMMON + ["--expert_floor", "32"], "--expert_floor goes with --agent HIRL"),
                       (["--agent", "SAC", "--type", "SAC"] + COMMON + ["--expert_floor", "32"], "--agent SAC --type SAC mixes no expert rows"),
                       (HIRL + ["--expert_floor", "129"], "--expert_floor 129")):
        ns = T.parser().parse_args(argv + ["--result_dir", str(tmp_path / "e")])
        with pytest.raises(SystemExit, match=word):
            T.main(ns)


@pytest.mark.parametrize("loop", ["front", "reference"])
def test_expert_floor_keeps_the_reader(P, tmp_path, monkeypatch, loop):
    """10 driver episodes of 130 steps: expert_num loses 13 rows per episode and would reach 0 at step 100 of the tenth.  With --expert_floor 32 it stops at
    32: n_main is 96 from then on, in every update, and the branch launch is made behind every acting launch to the end; without the floor the same run
    ends at n_main 128 and stops launching"""
    from hirl4ucav_amd import train_all as T

    names, runs, writers = G.spy(monkeypatch)
    seen, real_load = [], T.load_expert_tables

    def load(run):
        real_load(run)
        eng, n_main = run.eng, []
        seen.append(n_main)
        for fn in ("step_learn", "sample"):
            real = getattr(eng, fn)
            setattr(eng, fn, (lambda real: lambda *a, **kw: n_main.append(kw["n_main"]) or real(*a, **kw))(real))

    monkeypatch.setattr(T, "load_expert_tables", load)
    common = [v if v != "12" else "130" for v in HIRL] + ["--loop", loop, "--snapshot_every", "0", "--episodes", "10"] + STEPS
    explore = -(-20 * 130 // 64)
    T.main(T.parse_args(common + ["--expert_floor", "32", "--result_dir", str(tmp_path / "a")]))
    with_floor, floor_calls = seen[0], names.count("hx_pilot_branch_steps")
    del names[:]
    T.main(T.parse_args(common + ["--result_dir", str(tmp_path / "b")]))
    without, plain_calls = seen[1], names.count("hx_pilot_branch_steps")
    assert len(with_floor) == len(without) == 10 * 129  # (an episode's last step only acts)
    at = 7 * 129 + 40  # the 96th row is lost at step 40 of the eighth episode (13 per episode; 129 updates per episode)
    assert with_floor[:at] == without[:at] and with_floor[0] == 1 and with_floor[at - 1] == 95 and set(with_floor[at:]) == {96} and without[at + 10] == 97
    assert without[-1] == 128 and min(without) == 1
    assert floor_calls == explore + 1300 and plain_calls < floor_calls and runs[0][0].expert_num == 32 and runs[1][0].expert_num == 0
