"""GPU tests of the pilot kernels (hx_pilot_act, hx_pilot_refresh; utils.pilot) and of train_all --expert_online, against the numpy model of the
rule, tests/_pilot_model.py — bit for bit (fp32 without contraction, correctly rounded divide and square root; tests/test_pilot_cpu.py holds the
model to the torch pilot and to float64).  Smallest shapes that can still go wrong: 1 env, 63, one full workgroup (64), one env more (65: a second
workgroup with one lane), 130 and 300 (ragged tails); the state at a pitch (320) that is not the number of envs."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402
from tests import _pilot_model as M  # noqa: E402

STRIDE, GUARD, POISON = 320, 64, 0x7FC0DEAD


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import pilot

    return pilot


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded_state(state):
    """[37, n] -> a device tensor [37, STRIDE] whose columns behind n are poison"""
    full = np.full((37, STRIDE), POISON, np.int32)
    full[:, :state.shape[1]] = state.view(np.int32)
    return dev(full)


def assert_actions(got, want, what):
    """bit for bit where the model's row is finite; a non-finite row is only required to come out non-finite, with the model's fire value"""
    finite = np.isfinite(want).all(1)
    assert np.array_equal(got[finite].view(np.uint32), want[finite].view(np.uint32)), what
    assert not np.isfinite(got[~finite]).all(1).any() and np.array_equal(got[~finite, 3], want[~finite, 3]), what + ": non-finite rows"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 300])
def test_act_equals_the_model(P, n):
    from hirl4ucav_amd import _lib

    state, obs, noise = M.make_inputs(n)
    d_state, d_obs, d_noise = padded_state(state), dev(obs), dev(noise)
    for nz, d_nz in ((None, None), (noise, d_noise)):
        out = torch.full((n * 4 + GUARD,), POISON, dtype=torch.int32, device="cuda")
        _lib.call("hx_pilot_act", d_state.data_ptr(), n, STRIDE, d_obs.data_ptr(), _lib.ptr(d_nz), out.data_ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[n * 4:] == POISON).all(), "guard words"
        assert_actions(got[:n * 4].view(np.float32).reshape(n, 4), M.actions(state, obs, nz), f"{n} envs, noise {nz is not None}")
    if n > M.SPECIAL["coincide"]:
        assert (got[:n * 4].view(np.float32).reshape(n, 4)[M.SPECIAL["coincide"], :3] == M.clamp(noise[M.SPECIAL["coincide"]])).all()  # 0 / 1e-6 + noise


def test_act_refusals(P):
    from hirl4ucav_amd import _lib

    state, obs, _ = M.make_inputs(64)
    s, o = padded_state(state), dev(obs)
    out = torch.full((64 * 4 + 4,), POISON, dtype=torch.int32, device="cuda")
    good = (s.data_ptr(), 64, STRIDE, o.data_ptr(), None, out.data_ptr(), _lib.stream_ptr())
    for bad in ((None,) + good[1:], good[:1] + (0,) + good[2:], good[:2] + (63,) + good[3:], good[:3] + (None,) + good[4:], good[:5] + (None,) + good[6:],
                good[:5] + (out.data_ptr() + 4,) + good[6:], good[:1] + (1 << 31, 1 << 31) + good[3:]):
        with pytest.raises(_lib.HxError, match=r"hx_pilot_act failed \(-1\)"):
            _lib.call("hx_pilot_act", *bad)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()  # nothing was launched
    env = types.SimpleNamespace(n=64, pitch=STRIDE, state=s.view(torch.float32), obs=o, device=o.device)
    with pytest.raises(ValueError, match="noise"):
        P.device_pilot_actions(env, noise=torch.zeros((64, 4), device="cuda"))
    with pytest.raises(ValueError, match="out"):
        P.device_pilot_actions(env, out=torch.zeros((63, 4), device="cuda"))
    a = P.device_pilot_actions(env)
    assert_actions(a.cpu().numpy(), M.actions(state, obs), "device_pilot_actions")


@pytest.mark.parametrize("scenario", ["straight_line", "serpentine", "circular"])
def test_act_through_a_real_env(P, scenario):
    """65 envs flown for 200 steps by the kernel's own actions: after every step the kernel's output equals the model's on the pulled state, bit
    for bit.  (The flights start with the opponent ahead of the nose, so the levels stay unclamped here: the clamp edges, nrm < 1e-6 and the
    non-finite rows are test_act_equals_the_model's.)"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    n = 65
    env = BatchedHarfangEnv(n, scenario=scenario, seed=7, auto_reset=True, random_reset=True)
    env.reset()
    out = torch.empty((n, 4), device="cuda")
    fires, clamped, free = set(), 0, 0
    for t in range(200):
        a = P.device_pilot_actions(env, out=out)
        assert a is out
        got, state, obs = a.cpu().numpy(), env.state.cpu().numpy(), env.obs.cpu().numpy()
        want = M.actions(state, obs)
        assert np.isfinite(want).all() and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (scenario, t)
        fires.update(np.unique(got[:, 3]).tolist())
        clamped += int((np.abs(got[:, :3]) == 1).sum())
        free += int((np.abs(got[:, :3]) < 1).sum())
        env.step(a)
    print(f"{scenario}: fire values {sorted(fires)}, clamped levels {clamped}, unclamped {free}")
    assert fires <= {-1.0, 1.0} and clamped + free == 200 * n * 3 and free > 0


class RawRefresh:
    """hx_pilot_refresh over a table with guard rows behind it, fed from arrays (no env)"""

    def __init__(self, n, k, m, e0, call=0):
        self.n, self.k, self.m, self.e0, self.call = n, k, m, e0, call
        start = M.initial_table(M.make_offline(e0), m)
        self.model = M.RefreshModel(start, e0, m, k, call)
        full = np.full((e0 + m + 2, 32), POISON, np.int32)
        full[:e0 + m] = start.view(np.int32)
        self.table = dev(full)
        self.offline = start[:e0].copy()

    def push(self, state, obs):
        from hirl4ucav_amd import _lib

        s, o = padded_state(state), dev(obs)
        _lib.call("hx_pilot_refresh", s.data_ptr(), self.n, STRIDE, o.data_ptr(), self.table.data_ptr(), self.e0, self.m, self.k, self.call, _lib.stream_ptr())
        torch.cuda.synchronize()
        self.call += 1
        return self.model.push(state, obs)

    def rows(self):
        return self.table.cpu().numpy()

    def check(self, what):
        t = self.rows()
        assert (t[self.e0 + self.m:] == POISON).all(), what + ": guard rows"
        assert np.array_equal(t[:self.e0], self.offline.view(np.int32)), what + ": offline rows"
        assert np.array_equal(t[self.e0:self.e0 + self.m], self.model.table[self.e0:].view(np.int32)), what + ": online rows"
        assert (t[self.e0:self.e0 + self.m, 17:] == 0).all(), what + ": words 17..31"


CASES = [(1, 1, 1, 3), (65, 64, 100, 5), (300, 7, 50, 40), (300, 130, 130, 1)]


@pytest.mark.parametrize("n,k,m,e0", CASES)
def test_refresh_equals_the_model(P, n, k, m, e0):
    """enough calls to wrap the online region twice; after every call the whole table equals the model's, the offline rows and the guard rows behind
    the table stand.  On every third call the first pick's observation is made non-finite: its slot keeps what it had."""
    raw = RawRefresh(n, k, m, e0)
    raw.check("start")
    calls = 2 * -(-m // k) + 2
    skipped = 0
    for c in range(calls):
        state, obs, _ = M.make_inputs(n, seed=c)
        if c % 3 == 1:
            obs[M.env_picks(c, n, k)[0], c % 13] = (np.nan, np.inf, -np.inf)[(c // 3) % 3]
            slot = M.slots(c, k, m, e0)[0]
            before = raw.rows()[slot].copy()
        wrote = raw.push(state, obs)
        raw.check(f"call {c}")
        if c % 3 == 1:
            assert slot not in wrote and np.array_equal(raw.rows()[slot], before), f"call {c}: a non-finite row left its slot"
            skipped += 1
        assert len(wrote) <= k
    assert skipped >= 1 and raw.call == calls
    assert not np.array_equal(raw.model.table[e0:], M.initial_table(M.make_offline(e0), m)[e0:])  # (the region was rewritten)


@pytest.mark.parametrize("call0", [2 ** 32 - 1, 2 ** 40])
@pytest.mark.parametrize("n,k,m,e0", CASES[1:3])
def test_refresh_at_large_call_counts(P, n, k, m, e0, call0):
    """call is a 64-bit count: 2^32 - 1 -> 2^32 -> 2^32 + 1, and 2^40 .. 2^40 + 2"""
    raw = RawRefresh(n, k, m, e0, call=call0)
    for c in range(3):
        state, obs, _ = M.make_inputs(n, seed=c)
        raw.push(state, obs)
        raw.check(f"call {call0} + {c}")


def test_refresh_refusals(P):
    from hirl4ucav_amd import _lib

    n, k, m, e0 = 65, 64, 100, 5
    raw = RawRefresh(n, k, m, e0)
    state, obs, _ = M.make_inputs(n)
    s, o, t = padded_state(state), dev(obs), raw.table
    good = (s.data_ptr(), n, STRIDE, o.data_ptr(), t.data_ptr(), e0, m, k, 0, _lib.stream_ptr())

    def swap(i, v):
        return good[:i] + (v,) + good[i + 1:]

    for bad in (swap(0, None), swap(1, 0), swap(2, n - 1), swap(3, None), swap(4, None), swap(4, t.data_ptr() + 64), swap(4, t.data_ptr() + 4), swap(5, -1),
                swap(6, 0), swap(7, 0), swap(7, -3), swap(7, n + 1), good[:6] + (32, 33) + good[8:], good[:6] + (64, 65) + good[8:]):
        with pytest.raises(_lib.HxError, match=r"hx_pilot_refresh failed \(-1\)"):
            _lib.call("hx_pilot_refresh", *bad)
    raw.check("after the refusals")  # nothing was written
    env = types.SimpleNamespace(n=8, device=torch.device("cuda"))
    for rows, per in ((0, 1), (4, 5), (16, 9), (4, 0)):
        with pytest.raises(ValueError, match="OnlineExpert"):
            P.OnlineExpert(env, dev(M.make_offline(5)), rows, per)


NETS = ("actor", "target_actor", "bc_actor", "critic", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic", "wstate", "soft_count")
COUNTERS = ("critic_step", "actor_step", "update_count", "sample_calls", "upsample_calls", "actor_trainable")


@pytest.mark.parametrize("dtype,fire", [("f32", False), ("bf16", False), ("f32", True)])
def test_engine_reads_the_live_table(P, dtype, fire):
    """after some refreshes through a real env, sample() + learn() on the live table equal the same calls on a caller-made copy of it: networks,
    moments, soft weight and counters bit for bit; the logged losses (sums of float atomics) at the bar identical launches are held to elsewhere in
    the suite.  The BC minibatch reaches into the online region, and the region has left its initial fill."""
    from hirl4ucav_amd.agents import engine as E
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay, fire_rows

    params, data = D.make_params(1), D.make_data(2)
    rep = DeviceReplay(D.N_REPLAY)
    rep.store_rows(torch.from_numpy(data["replay"]))
    expert = DeviceReplay(D.N_EXPERT_ROWS + 10)
    expert.store_rows(torch.from_numpy(data["expert_rows"]))
    bc = np.zeros((D.N_EXPERT, 32), np.float32)
    bc[:, 0:13], bc[:, 13:17] = data["expert_s"], data["expert_a"]
    offline = torch.from_numpy(bc).cuda()
    env = BatchedHarfangEnv(96, scenario="straight_line", seed=5, auto_reset=True, random_reset=True, max_step=40)
    env.reset()
    on = P.OnlineExpert(env, offline, 1024, 32)
    start = on.table.clone()
    assert on.table.data_ptr() % 128 == 0 and torch.equal(start[D.N_EXPERT:], offline[torch.arange(1024, device="cuda") % D.N_EXPERT])
    engines = []
    for _ in range(2):
        eng = E.HirlEngine(batch=128)
        eng.load_params(params["actor"], params["critic"], params["bc_actor"])
        if dtype == "bf16":
            eng.set_act_dtype("bf16")
            eng.set_update_dtype("bf16")
        if fire:
            eng.set_upsample(None, fire_rows(offline))  # (taken from the offline rows, as train_all does: valid in the extended table)
        engines.append(eng)
    live, ref = engines
    g = torch.Generator(device="cuda").manual_seed(4)
    reached = 0
    for call in (1, 2, 3):
        for _ in range(5):
            env.step(P.device_pilot_actions(env) if call == 2 else torch.rand((96, 4), device="cuda", generator=g) * 2 - 1)
            on.push()
        copy = on.table.clone()
        for eng, table in ((live, on.table), (ref, copy)):
            eng.sample(rep, expert, table, n_main=100, seed=21, defer=(call != 1))
            eng.learn(bc_weight_now=100 if call == 1 else None)
        torch.cuda.synchronize()
        assert torch.equal(live._idx_bc, ref._idx_bc) and torch.equal(live.bc_rows.view(torch.int32), ref.bc_rows.view(torch.int32))
        assert torch.equal(live.bc_rows.view(-1, 32).view(torch.int32), copy[live._idx_bc.long()].view(torch.int32))
        reached += int((live._idx_bc >= D.N_EXPERT).sum())
        for name in NETS:
            assert torch.equal(getattr(live, name).view(torch.int32), getattr(ref, name).view(torch.int32)), (call, name)
        assert [getattr(live, c) for c in COUNTERS] == [getattr(ref, c) for c in COUNTERS]
        la, lb = np.asarray(live.losses_host(), np.float32), np.asarray(ref.losses_host(), np.float32)
        print(f"{dtype} call {call}: losses bit-equal {np.array_equal(la.view(np.uint32), lb.view(np.uint32))}, max |diff| {np.abs(la - lb).max():.3g}")
        np.testing.assert_allclose(la, lb, rtol=1e-6, atol=1e-7)
    assert reached > 0 and on.call == 15 and on.rows_written() == 480
    assert torch.equal(on.table[:D.N_EXPERT], offline) and not torch.equal(on.table[D.N_EXPERT:D.N_EXPERT + 480], start[D.N_EXPERT:D.N_EXPERT + 480])
    assert torch.equal(on.table[D.N_EXPERT + 480:], start[D.N_EXPERT + 480:]) and bool(torch.isfinite(on.table).all())
    st = on.state_dict()
    other = P.OnlineExpert(env, offline, 1024, 32)
    other.load_state_dict(st)
    assert other.call == 15 and torch.equal(other.table.view(torch.int32), on.table.view(torch.int32))


ARGS = ["--agent", "HIRL", "--type", "soft", "--env", "straight_line", "--random", "--seed", "3", "--num_envs", "32", "--buffer_size", "4096", "--max_step", "12",
        "--checkpoint_rate", "1000", "--snapshot_every", "1", "--synthetic_expert"]
ONLINE = ["--expert_online", "64", "--expert_online_per_step", "8"]
EXPLORE = 8  # ceil(20 * 12 / 32) exploration steps


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
    """-> (names of every library call, the runs' states as load_expert_tables left them, the writers)"""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd import train_all as T

    names, runs, writers, real_call, real_load = [], [], [], _lib.call, T.load_expert_tables

    def load(run):
        real_load(run)
        runs.append((run, run.bc_table.clone()))

    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real_call(name, *a))
    monkeypatch.setattr(T, "load_expert_tables", load)
    monkeypatch.setattr(T, "make_writer", lambda d: writers.append(Recorder()) or writers[-1])
    return names, runs, writers


@pytest.mark.parametrize("loop", ["front", "reference"])
def test_train_all_expert_online(P, tmp_path, monkeypatch, capsys, loop):
    """2 driver episodes of 12 steps at 32 envs in either loop form: one refresh behind every acting launch, exploration included; the online region
    has left its initial fill, the offline rows stand, every row is finite; the snapshot carries the region; the scalar is the host's count"""
    from hirl4ucav_amd import train_all as T

    names, runs, writers = spy(monkeypatch)
    out_dir = T.main(T.parse_args(ARGS + ONLINE + ["--loop", loop, "--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert ("vector loop: front launch" if loop == "front" else "vector loop: reference order") in out
    run, start = runs[0]
    e0 = start.shape[0] - 64
    assert names.count("hx_pilot_refresh") == EXPLORE + 2 * 12 == run.online.call and run.bc_table is run.online.table
    assert (names.count("hx_hirl_front") > 0) == (loop == "front")
    assert torch.equal(start[e0:], start[torch.arange(64, device="cuda") % e0])  # the initial fill
    table = run.online.table
    assert torch.equal(table[:e0], start[:e0]) and not torch.equal(table[e0:], start[e0:]) and bool(torch.isfinite(table).all())
    assert bool((table[e0:, 17:] == 0).all()) and bool((table[e0:, 16].abs() == 1).all()) and bool((table[e0:, 13:16].abs() <= 1).all())
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]["expert_online"]
    assert snap["call"] == run.online.call and (snap["online_rows"], snap["per_step"], snap["offline_rows"]) == (64, 8, e0)
    assert torch.equal(snap["online"], table[e0:].cpu())
    assert [(v, s) for t, v, s in writers[0].rows if t == "Expert/Online Rows Written"] == [(64.0, 0), (64.0, 1)]


def test_train_all_expert_online_resume(P, tmp_path, monkeypatch):
    """--separate_launches (one env workgroup: the run is reproducible): 1 episode + --resume to 2 equals the uninterrupted run bit for bit — networks,
    moments, ring and the expert table (the arena but its logged loss slots, sums of float atomics: rtol 1e-4 as in tests/test_epstat_gpu.py).
    --resume under other values of either flag is refused by name."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.agents.engine import HirlEngine

    args = ARGS + ONLINE + ["--separate_launches"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a = torch.load(os.path.join(whole, "state_rank0.pt"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(rest, "state_rank0.pt"), map_location="cpu", weights_only=False)
    h = torch.load(os.path.join(half, "state_rank0.pt"), map_location="cpu", weights_only=False)
    oa, ob, oh = a["driver"]["expert_online"], b["driver"]["expert_online"], h["driver"]["expert_online"]
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and oa["call"] == ob["call"] == EXPLORE + 24 and oh["call"] == EXPLORE + 12
    assert torch.equal(oa["online"].view(torch.int32), ob["online"].view(torch.int32)) and not torch.equal(oa["online"], oh["online"])
    assert a["engine"]["counters"] == b["engine"]["counters"]
    e = HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-4, atol=1e-6)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] and torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32))
    for other, word in ((["--expert_online", "32", "--expert_online_per_step", "8"], "--expert_online 64, --expert_online 32 given"),
                        (["--expert_online", "64", "--expert_online_per_step", "4"], "--expert_online_per_step 8, --expert_online_per_step 4 given"),
                        ([], "--expert_online 64, --expert_online 0 given")):
        with pytest.raises(SystemExit, match=word):
            T.main(T.parse_args(ARGS + other + ["--separate_launches", "--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))


def test_train_all_switch_off_is_the_parent_path(P, tmp_path, monkeypatch):
    """--expert_online 0 (the default): bc_table is the table read from the expert file, no hx_pilot_* call is made, nothing of it is logged or
    stored; a snapshot written so is refused under --expert_online"""
    from hirl4ucav_amd import train_all as T

    names, runs, writers = spy(monkeypatch)
    out_dir = T.main(T.parse_args(ARGS + ["--episodes", "1", "--result_dir", str(tmp_path / "a")]))
    run, start = runs[0]
    assert run.online is None and run.bc_table.shape == start.shape and torch.equal(run.bc_table, start)
    assert names and not [k for k in names if k.startswith("hx_pilot")]
    assert not [t for t, _, _ in writers[0].rows if t.startswith("Expert/")]
    assert "expert_online" not in torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]
    plain = len(names)
    del names[:]
    T.main(T.parse_args(ARGS + ONLINE + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    assert names.count("hx_pilot_refresh") == EXPLORE + 12 and len(names) - names.count("hx_pilot_refresh") == plain  # one launch more per acting launch, nothing else
    with pytest.raises(SystemExit, match="--expert_online 0, --expert_online 64 given"):
        T.main(T.parse_args(ARGS + ONLINE + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", out_dir]))


def test_ai_data_col_device_pilot(P, tmp_path, capsys):
    """--pilot device: the collector flies the kernel; the CSV loads through read_data and the fire rule holds row by row"""
    from hirl4ucav_amd.data import ai_data_col as C
    from hirl4ucav_amd.utils.data_processor import read_data

    out = C.main(["--env", "straight_line", "--random", "--episodes", "6", "--seed", "4", "--noise", "0.05", "--pilot", "device", "--out", str(tmp_path / "expert.csv")])
    assert "Finish" in capsys.readouterr().out
    s, a = read_data(out)
    assert s.shape[1] == 13 and a.shape == (s.shape[0], 4) and s.shape[0] > 600
    assert np.array_equal(a[:, 3] == 1, (s[:, 7] > 0) & (s[:, 8] > 0)) and set(np.unique(a[:, 3])) == {-1.0, 1.0}
    assert (np.abs(a[:, :3]) <= 1).all() and (np.abs(a[:, :3]) < 1).any()
    with pytest.raises(ValueError, match="pilot"):
        C.collect("straight_line", 2, True, pilot="cpu")
