"""CPU tests of the correlated exploration noise (include/hirl4ucav.h "Exploration noise"): the numpy model of the rule (tests/_noise_model.py) held to what
the header promises — unit variance, the analytic autocorrelation, a 1 / f spectrum for the octave bank — the host recipes of utils/noise.py against the
model's, the sigma ladder, train_all's flags with every refusal by name, the loop line and the resume rule.  The kernel is held to the model, bit for bit,
by tests/test_noise_gpu.py."""
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _noise_model as M  # noqa: E402

RECIPES = [("white", {}), ("ou", {"tau": 16.0}), ("ou", {"tau": 2.5}), ("ou", {"tau": 400.0})] + [("pink", {"octaves": k}) for k in range(1, 9)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the recipes -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", RECIPES)
def test_recipes_have_unit_variance(kind, kw):
    """sum w^2 = 1 and a^2 + b^2 = 1 to fp32 rounding (each stored value is within half an fp32 ulp, 2^-24 relative, of its float64 value: K + 1 of
    them meet in the sum of squares, two in a^2 + b^2), 0 <= a < 1; utils/noise.py's recipe is the model's, bit for bit as fp32"""
    from hirl4ucav_amd.utils import noise as N

    a, b, w = M.recipe(kind, **kw)
    K = len(a)
    assert a.dtype == b.dtype == w.dtype == np.float32 and K == (kw.get("octaves", 1) if kind == "pink" else 1)
    a64, b64, w64 = (v.astype(np.float64) for v in (a, b, w))
    assert abs((w64 * w64).sum() - 1.0) <= 2 * (K + 1) * 2.0 ** -24
    assert (np.abs(a64 * a64 + b64 * b64 - 1.0) <= 4 * 2.0 ** -24).all() and (a >= 0).all() and (a < 1).all()
    got = [np.array(v, np.float64).astype(np.float32) for v in N.coefficients(kind, **kw)]
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, (a, b, w)))
    assert N.lag_autocorr(*[N.coefficients(kind, **kw)[i] for i in (0, 2)], lag=1) == pytest.approx(M.autocorr(a, w, 1), rel=1e-6)
    if kind == "ou":
        assert a[0] == np.float32(np.exp(-1.0 / kw["tau"]))
    if kind == "pink":
        assert np.array_equal(a, np.exp(-(2.0 ** -np.arange(K))).astype(np.float32)) and (w == np.float32(1 / np.sqrt(K))).all()


def test_recipe_refusals():
    from hirl4ucav_amd.utils import noise as N

    for call, words in ((lambda: N.coefficients("brown"), "kind 'brown'"), (lambda: N.coefficients("ou", tau=0.0), "tau 0"),
                        (lambda: N.coefficients("ou", tau=float("nan")), "tau nan"), (lambda: N.coefficients("pink", octaves=0), "octaves 0"),
                        (lambda: N.coefficients("pink", octaves=9), "octaves 9"), (lambda: N.sigma_ladder(4, 0.0, 0.4), "sigma 0"),
                        (lambda: N.sigma_ladder(4, 0.2, 0.1), "sigma_max 0.1")):
        with pytest.raises(ValueError, match=words):
            call()


def test_white_is_sigma_times_eps_bit_for_bit():
    a, b, w = M.recipe("white")
    assert a[0] == 0 and b[0] == 1 and w[0] == 1
    rng = np.random.default_rng(0)
    eps = rng.standard_normal((7, 1, 65, 4)).astype(np.float32)
    z = rng.standard_normal((1, 4, 65)).astype(np.float32)  # (whatever the state held: a = 0 forgets it)
    out = M.fill(z, a, b, w, eps, 0.1)
    assert np.array_equal(bits(out), bits(np.float32(0.1) * eps[:, 0]))
    assert np.array_equal(bits(z[0]), bits(eps[-1, 0].T))
    sig = M.ladder(65, 0.1, 0.4)
    assert np.array_equal(bits(M.fill(z, a, b, w, eps, sig)), bits(sig[None, :, None] * eps[:, 0]))


# ---- what the process is ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def samples():
    """per recipe: x [64, 4096, 4], 64 steps after a stationary start (z ~ N(0, 1)), sigma = 1"""
    out = {}
    for j, (kind, kw) in enumerate((("white", {}), ("ou", {"tau": 16.0}), ("pink", {"octaves": 6}), ("pink", {"octaves": 8}))):
        rng = np.random.default_rng(100 + j)
        a, b, w = M.recipe(kind, **kw)
        z = rng.standard_normal((len(a), 4, 4096)).astype(np.float32)
        eps = rng.standard_normal((64, len(a), 4096, 4)).astype(np.float32)
        out[(kind, tuple(kw.items()))] = ((a, b, w), M.fill(z, a, b, w, eps, 1.0))
    return out


@pytest.mark.parametrize("lag", [1, 4, 16])
def test_autocorrelation_of_a_sample(samples, lag):
    """the lag-l autocorrelation of the model's output is the analytic sum w^2 a^l within 6 sqrt(2 / N): the estimate is the mean of N = 16,384
    independent products x_t x_(t + l) (one per env and component, t = 0), each of variance <= 2 for a unit-variance Gaussian pair"""
    N = 4096 * 4
    for key, ((a, b, w), x) in samples.items():
        est = float((x[0].astype(np.float64) * x[lag].astype(np.float64)).mean())
        assert abs(est - M.autocorr(a, w, lag)) <= 6 * np.sqrt(2.0 / N), (key, lag, est, M.autocorr(a, w, lag))
        var = float((x[63].astype(np.float64) ** 2).mean())  # (lag 0: the marginal variance after 64 steps is still 1)
        assert abs(var - 1.0) <= 6 * np.sqrt(2.0 / N), (key, var)


def test_pink_has_a_one_over_f_spectrum():
    """fitted log-log slope of the analytic spectrum over 64 log-spaced frequencies of the bank's band: within [-1.1, -0.9] for octaves 4, 6, 8
    (-0.956, -0.975, -0.984); ou (a Lorentzian: flat, then 1 / f^2) and white (flat) lie outside over the same bands"""
    for octaves, about in ((4, -0.956), (6, -0.975), (8, -0.984)):
        lo, hi = M.band(octaves)
        assert lo == pytest.approx(1 / (2 * np.pi * 2 ** (octaves - 1))) and hi == pytest.approx(1 / (2 * np.pi))
        a, b, w = M.recipe("pink", octaves=octaves)
        slope = M.loglog_slope(a, w, lo, hi)
        assert -1.1 <= slope <= -0.9 and slope == pytest.approx(about, abs=5e-4), (octaves, slope)
        for kind in ("ou", "white"):
            a, b, w = M.recipe(kind)
            other = M.loglog_slope(a, w, lo, hi)
            assert not -1.1 <= other <= -0.9, (kind, octaves, other)


def test_spectrum_integrates_to_the_variance():
    """the two-sided spectrum of a unit-variance process integrates to 1 over one period (midpoint rule on 2^16 points: the integrand is smooth and periodic)"""
    f = (np.arange(65536) + 0.5) / 65536 - 0.5
    for kind, kw in (("white", {}), ("ou", {"tau": 16.0}), ("pink", {"octaves": 8})):
        a, b, w = M.recipe(kind, **kw)
        assert M.spectrum(a, w, f).mean() == pytest.approx(1.0, abs=1e-6)


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------------------------
def test_ladder():
    """deterministic, within [sigma, sigma_max], the same whichever way the envs are split over ranks, spread over the whole range, and uncorrelated with the
    env's position in the population (--env mixed sorts its scenarios into thirds)"""
    from hirl4ucav_amd.utils import noise as N

    whole = M.ladder(4096, 0.1, 0.4)
    assert whole.dtype == np.float32 and np.array_equal(whole, M.ladder(4096, 0.1, 0.4))
    assert whole.min() >= np.float32(0.1) and whole.max() <= np.float32(0.4) and whole[0] == np.float32(0.1)
    for ranks in (2, 4, 8):
        n = 4096 // ranks
        assert np.array_equal(np.concatenate([M.ladder(n, 0.1, 0.4, env_id0=r * n) for r in range(ranks)]), whole)
    assert np.array_equal(bits(np.array(N.sigma_ladder(300, 0.1, 0.4, env_id0=77), np.float64).astype(np.float32)), bits(M.ladder(300, 0.1, 0.4, env_id0=77)))
    u = np.log(whole.astype(np.float64) / 0.1) / np.log(4.0)
    for third in np.split(u[:4095], 3):  # every third of the population sees the whole ladder: mean 1/2 within 6 / sqrt(12 * 1365)
        assert abs(third.mean() - 0.5) < 6 / np.sqrt(12 * 1365) and third.min() < 0.01 and third.max() > 0.99
    assert np.array_equal(M.ladder(8, 0.3, 0.3), np.full(8, 0.3, np.float32))
    assert M.ladder(1, 0.1, 0.4, env_id0=2 ** 32 - 1)[0] >= np.float32(0.1)  # (the last env id a Philox counter word holds)


def test_philox_counters():
    """the fourth counter word tells a step's draw from the starting draw and both from the acting kernels' draws (0 there); the step is 64-bit"""
    assert M.step_counter(5, 2 ** 32 + 3, 7) == (5, 3, 1, 0x4E4F4907) and M.step_counter(2 ** 32 + 1, 0, 0) == (1, 0, 0, 0x4E4F4900)
    words = {M.TAG_STEP | k for k in range(8)} | {M.TAG_INIT | k for k in range(8)}
    assert len(words) == 16 and 0 not in words
    x, y = M.normal4(M.step_counter(0, 3, 0), 9), M.normal4(M.step_counter(0, 2 ** 32 + 3, 0), 9)
    assert x != y and all(np.isfinite(x)) and M.normal4(M.step_counter(0, 3, 0), 9) == x


# ---- train_all: flags, refusals, the loop line, the resume rule ------------------------------------------------------------------------------------------------
HIRL = ["--agent", "HIRL", "--type", "soft"]
SAC = ["--agent", "SAC", "--type", "SAC"]


def test_parser_defaults_and_values():
    from hirl4ucav_amd import train_all as T

    cfg = T.parse_args(HIRL)
    assert (cfg.explore_noise, cfg.explore_tau, cfg.explore_octaves, cfg.explore_sigma, cfg.explore_sigma_max, cfg.explore_chunk) == ("white", 16.0, 6, 0.1, None, 16)
    assert T.explore_settings(cfg) == dict(T.EXPLORE_FLAGS) and not T.explore_uses_generator(cfg) and T.explore_refusal(cfg) is None
    assert T.explore_settings(types.SimpleNamespace()) == dict(T.EXPLORE_FLAGS)  # (a namespace from before the flags)
    for argv, gen in ((["--explore_sigma", "0.3"], False), (["--explore_sigma", "0"], False), (["--explore_noise", "ou", "--explore_tau", "40"], True),
                      (["--explore_noise", "pink", "--explore_octaves", "8", "--explore_chunk", "64"], True), (["--explore_sigma_max", "0.4"], True),
                      (["--explore_noise", "pink", "--explore_sigma", "0.05", "--explore_sigma_max", "0.4", "--explore_chunk", "1"], True)):
        for agent in (HIRL, ["--agent", "TD3"]):
            for more in ([], ["--loop", "reference"], ["--dtype", "bf16"], ["--gpus", "2"], ["--num_envs", "100"]):
                assert T.explore_uses_generator(T.parse_args(agent + argv + more)) is gen
    for kind in ("SAC", "ESAC", "ISAC"):
        cfg = T.parse_args(["--agent", "SAC", "--type", kind, "--explore_noise", "pink", "--explore_octaves", "4"] + (["--bc_actor", "x", "--synthetic_expert"] if kind == "ISAC" else []))
        assert T.explore_uses_generator(cfg)


def test_refusals_word_for_word(capsys):
    from hirl4ucav_amd import train_all as T

    for argv, words in (
            (["--agent", "BC", "--explore_noise", "pink"], "--explore_noise goes with --agent HIRL, TD3 or SAC, not --agent BC (behaviour cloning never acts while it trains)"),
            (["--agent", "BC", "--explore_sigma", "0.2"], "--explore_sigma goes with --agent HIRL, TD3 or SAC, not --agent BC"),
            (["--agent", "BC", "--explore_chunk", "4"], "--explore_chunk goes with --agent HIRL, TD3 or SAC, not --agent BC"),
            (HIRL + ["--explore_noise", "ou", "--explore_tau", "0"], "--explore_tau 0: the OU process's correlation time in vector steps, > 0"),
            (HIRL + ["--explore_noise", "ou", "--explore_tau", "nan"], "--explore_tau nan:"),
            (HIRL + ["--explore_noise", "pink", "--explore_octaves", "0"], "--explore_octaves 0: the poles of the 1 / f bank, 1..8"),
            (HIRL + ["--explore_noise", "pink", "--explore_octaves", "9"], "--explore_octaves 9: the poles of the 1 / f bank, 1..8"),
            (HIRL + ["--explore_noise", "pink", "--explore_chunk", "0"], "--explore_chunk 0: the vector steps of one generator launch, 1..64"),
            (HIRL + ["--explore_noise", "pink", "--explore_chunk", "65"], "--explore_chunk 65: the vector steps of one generator launch, 1..64"),
            (HIRL + ["--explore_tau", "8"], "--explore_tau goes with --explore_noise ou"),
            (HIRL + ["--explore_noise", "pink", "--explore_tau", "8"], "--explore_tau goes with --explore_noise ou"),
            (HIRL + ["--explore_noise", "ou", "--explore_octaves", "4"], "--explore_octaves goes with --explore_noise pink"),
            (HIRL + ["--explore_chunk", "8"], "--explore_chunk goes with --explore_noise ou or pink, or --explore_sigma_max"),
            (HIRL + ["--explore_sigma", "-0.1"], "--explore_sigma -0.1: the action noise's standard deviation, >= 0"),
            (HIRL + ["--explore_sigma", "inf"], "--explore_sigma inf:"),
            (HIRL + ["--explore_sigma_max", "0.05"], "--explore_sigma_max 0.05 with --explore_sigma 0.1: the ladder runs from --explore_sigma > 0 up to --explore_sigma_max >= it"),
            (HIRL + ["--explore_sigma", "0", "--explore_sigma_max", "0.4"], "--explore_sigma_max 0.4 with --explore_sigma 0:"),
            (HIRL + ["--explore_sigma_max", "nan"], "--explore_sigma_max nan"),
            (SAC + ["--explore_sigma", "0.2"], "--explore_sigma / --explore_sigma_max go with --agent HIRL or TD3: SAC's noise scale is the policy's own log-std"),
            (SAC + ["--explore_noise", "pink", "--explore_sigma_max", "0.4"], "--explore_sigma / --explore_sigma_max go with --agent HIRL or TD3"),
            (["--agent", "SAC", "--type", "ESAC", "--explore_sigma_max", "0.4"], "--explore_sigma / --explore_sigma_max go with --agent HIRL or TD3"),
            (HIRL + ["--explore_noise", "brown"], "invalid choice: 'brown'")):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
        assert words in " ".join(capsys.readouterr().err.split()), argv


def _run(agent, explore=None, loop="front"):
    cfg = types.SimpleNamespace(loop=loop, separate_launches=False, updates_per_step=1, dtype="f32", log_rewards=False, status_check_every=0, resume=None,
                                on_front_trip="exit", snapshot_every=0)
    gen = None if explore is None else types.SimpleNamespace(params={"kind": explore})
    return types.SimpleNamespace(config=cfg, world=1, rank=0, sac=agent == "SAC", n=64, device=torch.device("cpu"), batch=128, per=False, hirl_per=False,
                                 grad_clip=None, inserter=None, multi_step=1, hirl_multi_step=1, buffer_upsample=False, expert_upsample=False, episode0=0, explore=gen)


def test_loop_line(capsys, monkeypatch):
    """HIRL and TD3 keep the front launch under coloured noise and the line is the parent's; SAC takes the reference's order and the line names the flag;
    without a generator SAC's line is the parent's too"""
    from hirl4ucav_amd import train_all as T

    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    front = "vector loop: front launch (env step + first launches of learn() in one launch; draw before the insert)"
    for agent in ("HIRL", "TD3"):
        for explore in (None, "pink", "ou"):
            run = _run(agent, explore)
            T.choose_loop(run)
            assert run.front and capsys.readouterr().out.strip() == front
    run = _run("SAC")
    T.choose_loop(run)
    assert run.front_sac and capsys.readouterr().out.strip() == front
    for explore in ("pink", "ou"):
        run = _run("SAC", explore)
        T.choose_loop(run)
        assert not run.front_sac and capsys.readouterr().out.strip() == (
            f"vector loop: reference order (--explore_noise {explore}: the coloured draws are the Gaussian head's eps, which act_step takes and the front launch "
            "does not)")


class Gen:
    def __init__(self, log):
        self.log, self.calls = log, 0

    def next(self):
        self.calls += 1
        self.log.append(("gen.next", self.calls))
        return f"noise{self.calls}"


def test_the_steps_hand_the_generators_slice_to_the_acting_call():
    """step_front_hirl: act_noise=; step_reference: noise= (HIRL / TD3), eps= (SAC), in one launch and under --separate_launches; one next() per vector step.
    (Without a generator the calls are the parent's, word for word: tests/test_train_loop_cpu.py.)"""
    from hirl4ucav_amd import train_all as T

    log = []

    class Eng:
        def __getattr__(self, name):
            return lambda *a, **kw: log.append((name, kw))

    def make(sac, separate):
        env = types.SimpleNamespace(obs="obs", env_id0=0, step=lambda a: log.append(("env.step", a)), reward=0)
        cfg = types.SimpleNamespace(separate_launches=separate, updates_per_step=1)
        return types.SimpleNamespace(config=cfg, eng=Eng(), env=env, seed=7, rank=0, sac=sac, esac=False, isac=False, hirl=not sac, actions="actions", explore=Gen(log),
                                     act_sigma=0.3, inserter=None, estats=None, per=False, ret=None, max_step=3, batch=128, expert_num=0, expert=None, bc_table=None,
                                     replay="replay", writer=None, log_rate=300, expert_floor=0, warm_up_rate=10)

    run = make(False, False)
    T.step_front_hirl(run, 0, None, 0.0)
    assert log[0] == ("gen.next", 1) and log[1][0] == "step_learn" and log[1][1]["act_noise"] == "noise1" and log[1][1]["act_sigma"] == 0.3
    del log[:]
    T.step_reference(run, 2, None, 0.0)  # (an episode's last step only acts)
    assert log == [("gen.next", 2), ("act_step", dict(noise="noise2", sigma=0.3, seed=8, out="actions"))]
    for sac, separate, name, key in ((False, True, "act", "noise"), (True, False, "act_step", "eps"), (True, True, "act", "eps")):
        del log[:]
        T.step_reference(make(sac, separate), 2, None, 0.0)
        assert log[0] == ("gen.next", 1) and log[1][0] == name and log[1][1][key] == "noise1" and ("sigma" in log[1][1]) == (not sac), (sac, separate, log)


def test_resume_refuses_another_value_by_the_flags_name():
    from hirl4ucav_amd import train_all as T

    ns = types.SimpleNamespace
    pink = {"explore": {"flags": {"explore_noise": "pink", "explore_sigma_max": 0.4}, "generator": {}}}
    now = dict(agent="HIRL", explore_noise="pink", explore_sigma_max=0.4)
    assert T.explore_resume_refusal(ns(**now), None) is None and T.explore_resume_refusal(ns(**now), pink) is None
    assert T.explore_resume_refusal(ns(agent="HIRL"), {}) is None  # (a snapshot from before the flags, a run without them)
    for other, words in ((dict(now, explore_noise="ou"), "was run with --explore_noise pink, --explore_noise ou given"),
                         (dict(now, explore_sigma_max=0.5), "was run with --explore_sigma_max 0.4, --explore_sigma_max 0.5 given"),
                         (dict(now, explore_sigma_max=None), "was run with --explore_sigma_max 0.4, --explore_sigma_max None given"),
                         (dict(now, explore_chunk=8), "was run with --explore_chunk 16, --explore_chunk 8 given"),
                         (dict(now, explore_octaves=4), "was run with --explore_octaves 6, --explore_octaves 4 given"),
                         (dict(now, explore_sigma=0.2), "was run with --explore_sigma 0.1, --explore_sigma 0.2 given"),
                         (dict(agent="HIRL"), "was run with --explore_noise pink, --explore_noise white given")):
        assert T.explore_resume_refusal(ns(**other), pink) == words + ": resume with the flag the run was started with"
    assert T.explore_resume_refusal(ns(**now), {}) == ("was run with --explore_noise white, --explore_noise pink given: resume with the flag the run was "
                                                       "started with")
    assert T.explore_resume_refusal(ns(agent="HIRL", explore_noise="ou", explore_tau=8.0), {"explore": {"flags": {"explore_noise": "ou"}}}) == (
        "was run with --explore_tau 16.0, --explore_tau 8.0 given: resume with the flag the run was started with")
    run = ns(config=ns(resume="/somewhere", **other), snap={"driver": pink})
    with pytest.raises(ValueError, match=re.escape("train_all: --resume /somewhere was run with --explore_noise pink, --explore_noise white given")):
        T.build_explore(run)


def test_the_snapshot_record_carries_flags_and_generator():
    """no --explore_* flag: no key (a snapshot of such a run is what it was); a scale alone: the flag, no generator; a generator: its state"""
    from hirl4ucav_amd import train_all as T

    ns = types.SimpleNamespace
    base = dict(env_type="straight_line", estats=None)
    assert "explore" not in T.stats_record(ns(config=ns(), **base)) and "explore" not in T.stats_record(ns(**base))
    rec = T.stats_record(ns(config=ns(explore_sigma=0.3), explore=None, **base))
    assert rec["explore"] == {"flags": {"explore_sigma": 0.3}, "generator": None}
    gen = ns(state_dict=lambda: {"step": 5}, load_state_dict=lambda st: loaded.append(st))
    loaded = []
    run = ns(config=ns(explore_noise="pink"), explore=gen, **base)
    rec = T.stats_record(run)
    assert rec["explore"] == {"flags": {"explore_noise": "pink"}, "generator": {"step": 5}}
    T.restore_stats(run, rec)
    assert loaded == [{"step": 5}]


def test_abi_version_names_the_change_and_the_unit_is_built_without_contraction():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hirl4ucav.h")).read()
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 134 and "134: correlated exploration noise" in hdr and "Exploration noise (hx_noise.hip)" in hdr
    mk = open(os.path.join(root, "hirl4ucav_amd", "csrc", "Makefile")).read()
    for target in ("hx_noise.o", "stamps_hx_noise.o", "asanhost_hx_noise.o"):
        rule = re.search(rf"^{re.escape(target)}: hx_noise\.hip[^\n]*\n\t([^\n]*)", mk, re.M)
        assert rule and "$(ENVFLAGS)" in rule.group(1), target
    assert " hx_noise.o " in re.search(r"^OBJS = (.*)$", mk, re.M).group(1)
    from hirl4ucav_amd import _abi

    fns = _abi.abi().functions
    assert {"hx_noise_workspace_floats", "hx_noise_init", "hx_noise_fill"} <= set(fns) and len(fns["hx_noise_fill"][1]) == 14
    assert _abi.abi().defines["HX_NOISE_MAX_POLES"] == 8 and _abi.abi().defines["HX_NOISE_MAX_STEPS"] == 64
