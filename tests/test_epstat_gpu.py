"""GPU tests of the episode statistics by scenario (hx_epstat_push through utils.epstat.EpisodeStats) and of `--env mixed` in both drivers, against
the numpy model of the rule, tests/_epstat_model.py — bit for bit: fp32 without contraction per env, float64 in one fixed lane order per workgroup.
Smallest shapes that can still go wrong: 1 env, 63, one full workgroup (64), one env more (65: a second workgroup with one lane), 130 and 300 (ragged
tails); the state at a pitch (320) that is not the number of envs."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _epstat_model as M  # noqa: E402
from tests import _hirl_data as D  # noqa: E402

STRIDE, GUARD, POISON = 320, 64, 0x7FC0DEAD


@pytest.fixture(scope="module")
def EP():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import epstat

    return epstat


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class RawStats:
    """hx_epstat_* over a workspace with guard words behind it, fed from arrays (no env)"""

    def __init__(self, EP, n):
        import ctypes

        from hirl4ucav_amd import _lib

        self._lib, self._ct, self.n = _lib, ctypes, n
        self.off, self.words, self.groups = EP.workspace_layout(n)
        assert int(_lib.load().hx_epstat_workspace_words(n)) == self.words
        self.ws = torch.full((self.words + GUARD,), POISON, dtype=torch.int32, device="cuda")
        self.es = EP.epstat_struct(self.ws, n)
        self.state = torch.full((37, STRIDE), POISON, dtype=torch.int32, device="cuda")

    def reset(self, ctr):
        self._lib.call("hx_epstat_reset", self._ct.byref(self.es), dev(ctr.astype(np.int32)).data_ptr(), self._lib.stream_ptr())

    def clear(self):
        self._lib.call("hx_epstat_clear", self._ct.byref(self.es), self._lib.stream_ptr())

    def push(self, flags, reward, done, success, ctr):
        self.state[35, :self.n] = dev(flags.view(np.int32))
        r, d, s, c = dev(reward), dev(done), dev(success), dev(ctr.view(np.int32))
        self._lib.call("hx_epstat_push", self._ct.byref(self.es), self.state.data_ptr(), self.n, STRIDE, r.data_ptr(), d.data_ptr(), s.data_ptr(), c.data_ptr(),
                       self._lib.stream_ptr())
        torch.cuda.synchronize()

    def check(self, model, what):
        w = self.ws.cpu().numpy()
        o, n = self.off, self.n
        assert (w[self.words:] == POISON).all(), what + ": guard words"
        assert np.array_equal(w[:o["acc"]].view(np.uint64).reshape(self.groups, M.SLOT), model.part_words()), what + ": partials"
        assert np.array_equal(w[o["acc"]:o["acc"] + n].view(np.uint32), model.acc.view(np.uint32)), what + ": acc"
        assert np.array_equal(w[o["len"]:o["len"] + n].view(np.uint32), model.len), what + ": len"
        assert np.array_equal(w[o["last_ctr"]:o["last_ctr"] + n].view(np.uint32), model.last_ctr), what + ": last_ctr"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 300])
def test_push_equals_the_model(EP, n):
    """40 calls of the seeded stream (tests/test_epstat_cpu.py::test_stream_covers_the_cases); after every call the per-env words and every partial
    equal the model's, bit for bit, and the guard words behind the workspace stand.  clear after call 19, reset after call 29 (reset leaves nothing of
    the poison the workspace was filled with)."""
    ctr0, stream = M.make_stream(n)
    raw, model = RawStats(EP, n), M.EpStatModel(n)
    raw.reset(ctr0)
    model.reset(ctr0)
    raw.check(model, f"{n} envs, reset")
    for c, (flags, reward, done, success, ctr, _) in enumerate(stream):
        raw.push(flags, reward, done, success, ctr)
        model.push(flags, reward, done, success, ctr)
        raw.check(model, f"{n} envs, call {c}")
        if c == 19:
            raw.clear()
            model.clear()
            raw.check(model, f"{n} envs, clear")
        if c == 29:
            raw.reset(ctr)
            model.reset(ctr)
            raw.check(model, f"{n} envs, second reset")
    sums, mn, mx = EP.combine_partials(raw.ws[:raw.off["acc"]].cpu().numpy())
    ts, tmn, tmx = model.totals()
    assert np.array_equal(sums.view(np.uint64), ts.view(np.uint64)) and np.array_equal(mn, tmn) and np.array_equal(mx, tmx)
    assert (sums[3] == 0).all() and sums[:, M.COUNT].sum() > 0


def test_refusals(EP):
    import ctypes

    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    with pytest.raises(ValueError, match="auto_reset=False"):
        EP.EpisodeStats(BatchedHarfangEnv(8, auto_reset=False))
    raw = RawStats(EP, 64)
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    args = (raw.state.data_ptr(), 64, STRIDE, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), _lib.stream_ptr())
    for bad in ((raw.state.data_ptr(), 65, STRIDE) + args[3:], (raw.state.data_ptr(), 64, 63) + args[3:], (None,) + args[1:], args[:6] + (None,) + args[7:]):
        with pytest.raises(_lib.HxError, match="hx_epstat_push"):
            _lib.call("hx_epstat_push", ctypes.byref(raw.es), *bad)
    odd = _lib.HxEpStat(raw.ws.data_ptr() + 4, raw.es.acc, raw.es.len, raw.es.last_ctr, 64)
    with pytest.raises(_lib.HxError, match="8-byte aligned"):
        _lib.call("hx_epstat_clear", ctypes.byref(odd), _lib.stream_ptr())
    with pytest.raises(_lib.HxError, match="episode_ctr"):
        _lib.call("hx_epstat_reset", ctypes.byref(raw.es), None, _lib.stream_ptr())
    L = _lib.load()
    assert L.hx_epstat_workspace_words(0) == 0 and L.hx_epstat_workspace_words(65) == 2 * 72 + 3 * 65 and L.hx_epstat_sizeof() == ctypes.sizeof(_lib.HxEpStat)
    torch.cuda.synchronize()
    assert (raw.ws.cpu().numpy() == POISON).all()  # nothing was launched


def test_through_a_real_env(EP):
    """96 mixed envs, max_step 30, uniform actions for 90 steps: summed over the bins, the episodes that left, those that left by the time limit and
    the good fires equal the deltas of the env's own counters (HxStepOpts.stats) — an independent count that already exists.  state() / load_state()
    carry the workspace."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    n = 96
    env = BatchedHarfangEnv(n, scenario=T.mixed_scenarios(n).astype(np.int32), seed=11, max_step=30, auto_reset=True, random_reset=True)
    env.reset()
    st = EP.EpisodeStats(env)
    before = env.stats_dict()
    g = torch.Generator(device="cuda").manual_seed(4)
    for _ in range(90):
        env.step(torch.rand((n, 4), device="cuda", generator=g) * 2 - 1)
        st.push()
    after = env.stats_dict()
    saved = st.state()
    out = st.read_and_clear()
    assert list(out) == ["straight_line", "serpentine", "circular"]
    assert sum(v["count"] for v in out.values()) == after["episodes"] - before["episodes"] >= 2 * n
    assert sum(v["time_limit"] for v in out.values()) == after["time_limit"] - before["time_limit"] > 0
    assert sum(v["fire_good"] for v in out.values()) == after["good_fires"] - before["good_fires"]
    for v in out.values():
        assert v["count"] == v["done"] + v["time_limit"] >= 32 and 1 <= v["mean_len"] <= 29 and v["min"] <= v["mean"] <= v["max"] and np.isfinite(v["std"])
    assert all(v["count"] == 0 and v["min"] == np.inf for v in st.read().values())  # cleared; the running episodes stay
    assert torch.equal(st.ws[st._off["acc"]:].cpu(), saved["ws"][st._off["acc"]:])
    st.load_state(saved)
    assert st.read() == out
    with pytest.raises(ValueError, match="96 envs"):
        EP.EpisodeStats(BatchedHarfangEnv(64)).load_state(saved)


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


def test_validate_all_mixed(EP, tmp_path, capsys):
    """--scenario mixed on a saved checkpoint: a line per scenario and the pooled line per round; each scenario's numbers are those of a run with
    --scenario <that one> and the same seed, the pooled ones their mean."""
    from hirl4ucav_amd import validate_all as V

    params = D.make_params(D.PARAM_SEED)
    model = tmp_path / "model"
    os.makedirs(model)
    torch.save({k: torch.as_tensor(v) for k, v in params["actor"].items()}, os.path.join(model, "Agent7_100_5_Actor_Harfang_GYM"))
    common = ["--agent", "HIRL", "--model_dir", str(model), "--model_name", "Agent7_100_5_", "--random", "--seed", "3", "--episodes", "8", "--validation_step", "60"]
    single = {name: V.main(V.parse_args(common + ["--scenario", name])) for name in V.SCENARIO_NAMES}
    capsys.readouterr()
    ret, succ, _ = V.main(V.parse_args(common + ["--scenario", "mixed"]))
    out = capsys.readouterr().out
    for k in range(2):
        assert ret[k] == np.mean([single[name][0][k] for name in V.SCENARIO_NAMES]) and succ[k] == np.mean([single[name][1][k] for name in V.SCENARIO_NAMES])
        for name in V.SCENARIO_NAMES:
            assert f"round {k + 1} {name}: avg reward {single[name][0][k]:.2f} fire success {single[name][1][k]:.2f}" in out
        assert f"round {k + 1}: avg reward {ret[k]:.2f}" in out
    with pytest.raises(SystemExit, match="--infinite"):
        V.main(V.parser().parse_args(common + ["--scenario", "mixed", "--infinite"]))


MIXED_ARGS = ["--env", "mixed", "--random", "--seed", "3", "--num_envs", "96", "--buffer_size", "8192", "--max_step", "30", "--synthetic_expert",
              "--checkpoint_rate", "2", "--snapshot_every", "1"]
AGENTS = {"hirl_front": ["--agent", "HIRL", "--type", "soft", "--loop", "front"],
          "hirl_reference": ["--agent", "HIRL", "--type", "soft", "--loop", "reference"],
          "sac": ["--agent", "SAC", "--type", "SAC"],
          # ... and the two forms in which a run is reproducible at all (see test_train_all_mixed): the resumed run is compared bit for bit there
          "hirl_separate": ["--agent", "HIRL", "--type", "soft", "--separate_launches"],
          "sac_separate": ["--agent", "SAC", "--type", "SAC", "--separate_launches"]}


def load_checkpoint(run, sac):
    from hirl4ucav_amd import validate_all as V

    files = sorted(os.listdir(os.path.join(run, "model")))
    assert files, "a checkpoint was written"
    tag = re.search(r"Agent\d+_-?\d+_-?\d+_", files[0]).group(0)  # checkpoint_tag: Agent<k>_<rate>_<score>_
    cfg = V.parser().parse_args(["--agent", "SAC" if sac else "HIRL", "--model_dir", os.path.join(run, "model"), "--model_name", tag])
    return V.load_agent(cfg, torch.device("cuda"))[0], tag


@pytest.mark.parametrize("which", list(AGENTS))
def test_train_all_mixed(EP, tmp_path, monkeypatch, capsys, which):
    """train_all --env mixed, 96 envs, 2 driver episodes of 30 steps: the run completes; the per-scenario Training/* and Validation/* tags are written;
    every per-scenario validation tuple is what validate() gives on the saved checkpoint; --resume under another --env is refused by name.
    1 episode + --resume: the resumed run carries the first episode's (sum, count) pair of the last-100 window over, bit for bit, and completes.  With
    --separate_launches it gives the networks and the statistics of the uninterrupted run, bit for bit (the arena but its logged loss slots, which are
    float-atomic sums: rtol 1e-4 as in tests/test_facade_gpu.py).  Without it that comparison has no meaning: with acting and env step in one launch
    the order in which a step's rows enter the ring depends on the workgroup schedule (train_all --separate_launches says so), and two IDENTICAL
    uninterrupted runs already differ — measured on the MI355X at 96 and at 64 envs, front / reference / SAC alike: about 3.0 of 4.6 million arena
    words, the ring, the env state and 12 to 80 statistics words; under --separate_launches: the loss slots only (2 to 4 words), everything else equal.
    The front loop has no separate-launch form, so its resumed run is held to what the snapshot carries."""
    from hirl4ucav_amd import train_all as T

    writers = []
    monkeypatch.setattr(T, "make_writer", lambda d: writers.append(Recorder()) or writers[-1])
    args, sac, bitwise = AGENTS[which] + MIXED_ARGS, which.startswith("sac"), which.endswith("_separate")
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert "Episode 2:" in out and "Validation 1:" in out and "  circular: avg reward" in out
    rows = writers[0].rows
    tags = {t for t, _, _ in rows}
    for name in ("straight_line", "serpentine", "circular"):
        for t in ("Episode Reward", "Episode Reward Std", "Episode Length", "Average Step Reward", "Ended By Done", "Ended By Time Limit"):
            assert f"Training/{name}/{t}" in tags, (name, t)
        for t in ("Avg Reward", "Std Reward", "Success Rate", "Fire Success Rate"):
            assert f"Validation/{name}/{t}" in tags, (name, t)
    assert {"Training/Last 100 Episode Average Reward", "Validation/Avg Reward", "Validation/Std Reward", "Validation/Success Rate",
            "Validation/Fire Success Rate"} <= tags
    val = {t: v for t, v, _ in rows if t.startswith("Validation/")}
    lens = [v for t, v, _ in rows if t.endswith("/Episode Length")]
    assert all(1 <= v <= 29 for v in lens)
    # the per-scenario validation tuples against validate() on the saved checkpoint; the pooled tags from them
    eng, tag = load_checkpoint(whole, sac)
    direct = {name: T.validate(eng, name, 50, T.MAX_STEP[name], True, 3 + 12345, torch.device("cuda"), sac) for name in ("straight_line", "serpentine", "circular")}
    for name, (mean, std, succ, fire) in direct.items():
        assert (val[f"Validation/{name}/Avg Reward"], val[f"Validation/{name}/Std Reward"], val[f"Validation/{name}/Success Rate"],
                val[f"Validation/{name}/Fire Success Rate"]) == (mean, std, succ / 50, fire / 50), name
    pooled = T.pool_validation(list(direct.values()))
    assert (val["Validation/Avg Reward"], val["Validation/Std Reward"], val["Validation/Success Rate"]) == (pooled[0], pooled[1], pooled[2] / 150)
    assert tag == T.checkpoint_tag(1, pooled[2], 150, pooled[0])
    # resume
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a = torch.load(os.path.join(whole, "state_rank0.pt"), map_location="cpu", weights_only=False)
    b = torch.load(os.path.join(rest, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and a["driver"]["env"] == "mixed"
    sa, sb = a["driver"]["episode_stats"], b["driver"]["episode_stats"]
    h = torch.load(os.path.join(half, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]["episode_stats"]
    assert len(sa["last100"]) == len(sb["last100"]) == 2 and len(h["last100"]) == 1 and sb["last100"][0] == h["last100"][0] and h["last100"][0][1] >= 96
    assert sa["device"]["ws"].shape == sb["device"]["ws"].shape == h["device"]["ws"].shape
    with pytest.raises(SystemExit, match="--env"):
        T.main(T.parse_args(AGENTS[which] + ["--env", "serpentine"] + MIXED_ARGS[2:] + ["--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))
    if not bitwise:
        return
    assert torch.equal(sa["device"]["ws"], sb["device"]["ws"]) and sa["last100"] == sb["last100"]
    assert [r for r in writers[0].rows if r[2] == 1 and r[0].startswith("Training/") and "/" in r[0][9:]] == \
        [r for r in writers[2].rows if r[2] == 1 and r[0].startswith("Training/") and "/" in r[0][9:]]
    if sac:
        from hirl4ucav_amd.agents.sac_engine import SacEngine as Eng
    else:
        from hirl4ucav_amd.agents.engine import HirlEngine as Eng
    e = Eng()
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-4, atol=1e-6)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"


def test_train_bc_mixed_validates_per_scenario(EP, tmp_path, monkeypatch, capsys):
    """--agent BC --env mixed: the validation runs per scenario and pooled, the actor checkpoint carries the pooled tag, --plot writes one file set
    per scenario with the tag <arttir>_<scenario>; two expert files are read one by one"""
    from hirl4ucav_amd import train_all as T

    rng = np.random.default_rng(2)
    real, seen = T.read_data, []
    tables = {"a.csv": (rng.uniform(-1, 1, (40, 13)), rng.uniform(-1, 1, (40, 4))), "b.csv": (rng.uniform(-1, 1, (25, 13)), rng.uniform(-1, 1, (25, 4)))}
    monkeypatch.setattr(T, "read_data", lambda p: seen.append(os.path.basename(p)) or tables[os.path.basename(p)])
    for name in tables:
        open(tmp_path / name, "w").close()
    writers = []
    monkeypatch.setattr(T, "make_writer", lambda d: writers.append(Recorder()) or writers[-1])
    run = T.main(T.parse_args(["--agent", "BC", "--env", "mixed", "--random", "--seed", "3", "--max_step", "5", "--episodes", "1", "--checkpoint_rate", "1",
                               "--bc_validate_from", "1", "--expert_csv", f"{tmp_path / 'a.csv'},{tmp_path / 'b.csv'}", "--plot", "--result_dir", str(tmp_path / "r")]))
    assert seen == ["a.csv", "b.csv"] and real is not None
    val = {t: v for t, v, _ in writers[0].rows if t.startswith("Validation/")}
    per = [(val[f"Validation/{k}/Avg Reward"], val[f"Validation/{k}/Std Reward"], round(val[f"Validation/{k}/Success Rate"] * 50),
            round(val[f"Validation/{k}/Fire Success Rate"] * 50)) for k in ("straight_line", "serpentine", "circular")]
    pooled = T.pool_validation(per)
    assert (val["Validation/Avg Reward"], val["Validation/Std Reward"]) == pooled[:2]
    assert os.listdir(os.path.join(run, "model")) == [T.checkpoint_tag(1, pooled[2], 150, pooled[0]) + "Actor_Harfang_GYM"]
    assert sorted(f for f in os.listdir(os.path.join(run, "plot", "csv")) if f.startswith("distance")) == \
        ["distance1_circular.csv", "distance1_serpentine.csv", "distance1_straight_line.csv"]


def test_single_scenario_issues_no_statistics_call(EP, tmp_path, monkeypatch):
    """without --episode_stats a single-scenario run makes no hx_epstat_* call and writes no per-scenario tag; with it, it does both"""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd import train_all as T

    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    writers = []
    monkeypatch.setattr(T, "make_writer", lambda d: writers.append(Recorder()) or writers[-1])
    args = ["--agent", "SAC", "--type", "SAC", "--env", "serpentine", "--random", "--seed", "3", "--num_envs", "96", "--buffer_size", "8192", "--max_step", "30",
            "--checkpoint_rate", "1000", "--snapshot_every", "0", "--episodes", "1"]
    T.main(T.parse_args(args + ["--result_dir", str(tmp_path / "a")]))
    assert names and not [k for k in names if k.startswith("hx_epstat")]
    assert not [t for t, _, _ in writers[0].rows if t.startswith("Training/serpentine/") or t == "Training/Last 100 Episode Average Reward"]
    plain = len(names)
    del names[:]
    T.main(T.parse_args(args + ["--episode_stats", "--result_dir", str(tmp_path / "b")]))
    ep = [k for k in names if k.startswith("hx_epstat")]
    assert ep.count("hx_epstat_push") == 7 + 30 and ep.count("hx_epstat_reset") == 2 and ep.count("hx_epstat_clear") == 1  # 7 exploration steps; reset: the constructor's and the driver's
    assert len(names) - len(ep) == plain
    tags = {t for t, _, _ in writers[1].rows}
    assert "Training/serpentine/Episode Reward" in tags and "Training/Last 100 Episode Average Reward" in tags and not [t for t in tags if "circular" in t]
