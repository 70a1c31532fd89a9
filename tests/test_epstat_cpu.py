"""Episode statistics by scenario and `--env mixed`, the host side: the numpy model of hx_epstat_push (tests/_epstat_model.py) against a per-env
loop written like the reference's training loop; what the seeded stream covers; mixed_scenarios, pool_validation, the expert list, the flags and
the last-100 window.  No GPU."""
import math

import numpy as np
import pytest

from tests import _epstat_model as M

SIZES = (1, 63, 64, 65, 130, 300)


def run_model(n, calls=40):
    ctr0, stream = M.make_stream(n, calls)
    m = M.EpStatModel(n)
    m.reset(ctr0)
    for flags, reward, done, success, ctr, _ in stream:
        m.push(flags, reward, done, success, ctr)
    return m, stream


@pytest.mark.parametrize("n", SIZES)
def test_model_equals_the_reference_style_loop(n):
    """counts, lengths and fires equal (min and max: see below); the sums to rtol 1e-6: the model adds at most 40 rewards in fp32 where the loop adds in float64
    (each add rounds to 2^-24 relative to a partial sum; the returns here are sums of rewards of either sign, hence the atol of the same size
    relative to the largest |partial sum| an episode can reach, 40 * 3 * 5 sigma)"""
    m, stream = run_model(n)
    sums, mn, mx = m.totals()
    eps, fires = M.reference_loop(n, stream)
    for b in range(M.BINS):
        e = eps[b]
        assert sums[b, M.COUNT] == len(e["ret"]) and sums[b, M.N_DONE] == e["done"] and sums[b, M.N_TIME_LIMIT] == e["time_limit"]
        assert sums[b, M.SUM_LEN] == sum(e["len"])
        assert sums[b, M.FIRE_GOOD] == fires[b, 0] and sums[b, M.FIRE_BAD] == fires[b, 1]
        if e["ret"]:
            # min / max are fp32 returns, the loop's are float64: the same episode's return, to the bound of the sums (they are EQUAL to the
            # fp32 returns formed in step order: test_model_min_max_are_those_of_the_fp32_returns)
            scale = max(abs(x) for x in e["ret"])
            np.testing.assert_allclose(mn[b], min(e["ret"]), rtol=1e-6, atol=1e-6 * scale)
            np.testing.assert_allclose(mx[b], max(e["ret"]), rtol=1e-6, atol=1e-6 * scale)
            np.testing.assert_allclose(sums[b, M.SUM_RET], sum(e["ret"]), rtol=1e-6, atol=1e-6 * sum(abs(x) for x in e["ret"]))
            np.testing.assert_allclose(sums[b, M.SUM_RET_SQ], sum(x * x for x in e["ret"]), rtol=1e-6)
        else:
            assert mn[b] == np.inf and mx[b] == -np.inf and sums[b, M.SUM_RET] == 0


def test_model_min_max_are_those_of_the_fp32_returns():
    """min and max exactly: the per-episode fp32 returns, formed in step order, are what the model holds"""
    n = 130
    ctr0, stream = M.make_stream(n)
    bins = M.scenario_bins(n)
    rets = {b: [] for b in range(M.BINS)}
    for i in range(n):
        acc = np.float32(0)
        for flags, reward, done, success, ctr, tl in stream:
            if tl[i] and not done[i]:
                rets[int(bins[i])].append(acc)
                acc = np.float32(0)
                continue
            acc = np.float32(acc + reward[i])
            if done[i]:
                rets[int(bins[i])].append(acc)
                acc = np.float32(0)
    m, _ = run_model(n)
    _, mn, mx = m.totals()
    for b in range(3):
        assert mn[b] == min(rets[b]) and mx[b] == max(rets[b])


def test_stream_covers_the_cases():
    n = 64  # one workgroup
    ctr0, stream = M.make_stream(n)
    bins = M.scenario_bins(n)
    assert set(bins.tolist()) == {0, 1, 2}, "a workgroup holding all three scenarios, bin 3 never used"
    for k in SIZES:
        assert int(M.scenario_bins(k).max()) <= 2
        assert all(((f >> 8) & 3).max() <= 2 for f, *_ in M.make_stream(k)[1])
    assert set(M.scenario_bins(300)[:64].tolist()) == {0, 1, 2}
    done = np.stack([s[2] for s in stream]).astype(bool)
    tl = np.stack([s[5] for s in stream])
    ctr = np.stack([s[4] for s in stream]).astype(np.int64)
    moved = np.diff(np.concatenate([ctr0[None].astype(np.int64), ctr]), axis=0) != 0
    assert np.array_equal(moved, done | tl), "episode_ctr moves exactly where an episode ends"
    assert done.any(), "an episode ended by done"
    assert (tl & ~done).any(), "an episode ended by the time limit"
    assert (tl & done).any(), "a done on the time-limit step"
    assert done[2, 0] and done[3, 0] and done[4, 0], "two one-step episodes in a row in env 0"
    ended = done | tl
    assert any(ended[c].any() and not ended[c][bins == 2].any() for c in range(len(stream))), "a call in which one bin ends nothing while another ends"
    m, _ = run_model(n)
    sums, _, _ = m.totals()
    assert (sums[3] == 0).all() and (sums[:3, M.COUNT] > 0).all() and (sums[:3, M.N_TIME_LIMIT] > 0).all()


def test_clear_keeps_the_running_episodes():
    n = 65
    ctr0, stream = M.make_stream(n)
    a, b = M.EpStatModel(n), M.EpStatModel(n)
    a.reset(ctr0)
    b.reset(ctr0)
    for k, (flags, reward, done, success, ctr, _) in enumerate(stream):
        a.push(flags, reward, done, success, ctr)
        b.push(flags, reward, done, success, ctr)
        if k == 19:
            first = b.totals()[0].copy()
            b.clear()
            assert (b.sums == 0).all() and np.isinf(b.min).all()
    assert np.array_equal(a.acc, b.acc) and np.array_equal(a.len, b.len)
    np.testing.assert_array_equal(a.totals()[0][:, :4], (first + b.totals()[0])[:, :4])  # the integer fields split exactly at the clear


def test_host_helpers_of_the_binding():
    from hirl4ucav_amd.utils import epstat as EP

    m, _ = run_model(130)
    sums, mn, mx = EP.combine_partials(m.part_words().view(np.int32).reshape(-1))
    ts, tmn, tmx = m.totals()
    assert np.array_equal(sums.view(np.uint64), ts.view(np.uint64)) and np.array_equal(mn, tmn) and np.array_equal(mx, tmx)
    out = EP.summarize(sums, mn, mx)
    assert list(out) == ["straight_line", "serpentine", "circular"]
    for b, name in enumerate(out):
        s = out[name]
        assert s["count"] == ts[b, M.COUNT] == s["done"] + s["time_limit"]
        assert s["mean"] == ts[b, M.SUM_RET] / ts[b, M.COUNT] and s["mean_len"] == ts[b, M.SUM_LEN] / ts[b, M.COUNT]
        assert s["min"] <= s["mean"] <= s["max"] and s["std"] >= 0
    empty = EP.summarize(np.zeros((4, 8)), np.full(4, np.inf, np.float32), np.full(4, -np.inf, np.float32))
    assert empty["serpentine"]["count"] == 0 and math.isnan(empty["serpentine"]["mean"])
    off, words, groups = EP.workspace_layout(130)
    assert groups == 3 and words == 3 * 72 + 3 * 130 and off == {"part": 0, "acc": 216, "len": 346, "last_ctr": 476}


@pytest.mark.parametrize("n", [3, 64, 100])
def test_mixed_scenarios(n):
    from hirl4ucav_amd import train_all as T

    for rank in range(3):
        s = T.mixed_scenarios(n, rank * n)
        assert s.shape == (n,) and (np.diff(s) >= 0).all() and set(s.tolist()) == {0, 1, 2}
        counts = np.bincount(s, minlength=3)
        assert counts.max() - counts.min() <= 1
        assert np.array_equal(s, np.sort((np.arange(n) + rank * n) % 3))  # bench.py --scenario mixed
    assert T.scenarios_of("mixed") == ["straight_line", "serpentine", "circular"] and T.scenarios_of("circular") == ["circular"]
    assert T.default_max_step("mixed") == 1900 and T.default_max_step("serpentine") == 1500
    assert T.MAX_STEP == {"straight_line": 1500, "serpentine": 1500, "circular": 1900}


def test_pool_validation_equals_numpy_on_the_concatenated_scores():
    from hirl4ucav_amd import train_all as T

    rng = np.random.default_rng(5)
    scores = [rng.normal(mu, sd, 50) for mu, sd in ((-300, 40), (-120, 5), (15, 90))]
    kills, fires = [7, 0, 31], [9, 2, 40]
    mean, std, k, f = T.pool_validation([(float(s.mean()), float(s.std()), kk, ff) for s, kk, ff in zip(scores, kills, fires)])
    every = np.concatenate(scores)
    np.testing.assert_allclose(mean, every.mean(), rtol=1e-12)
    np.testing.assert_allclose(std, every.std(), rtol=1e-10)
    assert (k, f) == (38, 51)
    one = T.pool_validation([(-3.5, 2.0, 4, 5)])
    assert one[0] == -3.5 and abs(one[1] - 2.0) < 1e-12 and one[2:] == (4, 5)


def test_expert_list(tmp_path):
    from hirl4ucav_amd import train_all as T

    assert T.expert_paths(None) == [] and T.expert_paths("a.csv") == ["a.csv"] and T.expert_paths("a.csv, b.csv,c.csv") == ["a.csv", "b.csv", "c.csv"]
    with pytest.raises(ValueError, match="empty item"):
        T.expert_paths("a.csv,,b.csv")
    with pytest.raises(FileNotFoundError, match="nope.csv"):
        T.load_expert_files(T.parser().parse_args(["--expert_csv", f"{tmp_path / 'nope.csv'},{tmp_path / 'other.csv'}"]))
    tables = T.load_expert_files(T.parser().parse_args(["--synthetic_expert"]))
    es, ea = T.load_expert(T.parser().parse_args(["--synthetic_expert"]))
    assert len(tables) == 1 and np.array_equal(tables[0][0], es) and np.array_equal(tables[0][1], ea)


def test_flags():
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd import validate_all as V

    cfg = T.parse_args(["--env", "mixed", "--episode_stats", "--num_envs", "96"])
    assert cfg.env == "mixed" and cfg.episode_stats
    assert not T.parse_args(["--env", "circular"]).episode_stats
    with pytest.raises(SystemExit):
        T.parse_args(["--env", "mixed", "--num_envs", "2"])
    assert "at least 3" in T.mixed_refusal(T.parser().parse_args(["--env", "mixed", "--num_envs", "2"]))
    assert T.mixed_refusal(T.parser().parse_args(["--env", "serpentine", "--num_envs", "2"])) is None
    assert V.parse_args(["--model_name", "x", "--model_dir", "y", "--scenario", "mixed"]).scenario == "mixed"
    with pytest.raises(SystemExit):
        V.parse_args(["--model_name", "x", "--model_dir", "y", "--scenario", "mixed", "--infinite"])
    assert "--infinite" in V.mixed_refusal(V.parser().parse_args(["--model_name", "x", "--model_dir", "y", "--scenario", "mixed", "--infinite"]))


def test_last_100_window_and_scalars():
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.epstat import Last100

    w = Last100()
    assert math.isnan(w.mean())
    for k in range(100):
        w.add(10.0 * (k + 1), k + 1)
    assert w.mean() == 10.0
    w.add(0.0, 100)  # the 101st pair pushes the first one (10, 1) out
    assert len(w.pairs) == 100 and w.mean() == (10.0 * 5050 - 10.0) / (5050 - 1 + 100)
    again = Last100(w.state())
    assert again.mean() == w.mean() and again.state() == w.state()

    class W:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, v, step):
            self.rows.append((tag, v, step))

    stats = {"straight_line": dict(count=2, done=1, time_limit=1, mean=3.0, std=1.0, min=2.0, max=4.0, mean_len=5.0, sum_ret=6.0, sum_len=10.0, fire_good=0, fire_bad=0),
             "serpentine": dict(count=0, done=0, time_limit=0, mean=math.nan, std=math.nan, min=math.inf, max=-math.inf, mean_len=math.nan, sum_ret=0.0, sum_len=0.0,
                                fire_good=0, fire_bad=0)}
    wr, last = W(), Last100()
    T.log_episode_stats(wr, 4, stats, last)
    tags = {t: v for t, v, s in wr.rows}
    assert tags == {"Training/straight_line/Episode Reward": 3.0, "Training/straight_line/Episode Reward Std": 1.0, "Training/straight_line/Episode Length": 5.0,
                    "Training/straight_line/Average Step Reward": 0.6, "Training/straight_line/Ended By Done": 1, "Training/straight_line/Ended By Time Limit": 1,
                    "Training/Last 100 Episode Average Reward": 3.0}
    assert all(s == 4 for _, _, s in wr.rows) and last.state() == [[6.0, 2]]
