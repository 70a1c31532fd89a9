"""GPU tests of the correlated exploration noise (include/hirl4ucav.h "Exploration noise"): hx_noise_fill against the numpy model (tests/_noise_model.py)
bit for bit with injected draws, its Philox draws against a host float64 Philox + Box-Muller, invariance to the chunking of steps and to the split of
the envs over shards, the 64-bit step counter, every argument error, and ColoredNoise through HirlEngine.act_step and train_all.  Smallest shapes that can
still go wrong: one lane, one wave less one, one wave, one wave and a lane, several waves with a ragged tail; one pole, two, the maximum."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402
from tests import _noise_model as M  # noqa: E402
from tests import _sharded_lockstep as LS  # noqa: E402

GUARD = 64  # words in front of and behind every buffer the kernel writes (256 bytes: the payload stays 16-byte aligned)
SENTINEL = 0x7FC0BEEF


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd import _lib

    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """a device buffer of `words` fp32 words between two guard zones"""

    def __init__(self, words, init=None):
        self.words = words
        self.buf = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.body = self.buf[GUARD:GUARD + words].view(torch.float32)
        if init is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def ptr(self):
        return self.body.data_ptr()

    def host(self, shape):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + self.words:] == SENTINEL).all(), "guard words were written"
        return h[GUARD:GUARD + self.words].view(np.float32).reshape(shape).copy()

    def untouched(self):
        return bool((self.buf.cpu().numpy() == SENTINEL).all())


def coef_host(a, b, w):
    c = np.zeros((3, M.MAX_POLES), np.float32)
    for r, row in enumerate((a, b, w)):
        c[r, :len(row)] = row
    return c


def call_fill(L, z, n, poles, coef, out, steps, sigma=0.1, sigma_env=None, seed=7, row0=0, step0=0, eps_in=None, eps_out=None):
    p = lambda t: None if t is None else (t.ptr() if isinstance(t, Guarded) else t.data_ptr())  # noqa: E731
    from hirl4ucav_amd import _lib

    return L.hx_noise_fill(p(z), p(sigma_env), n, poles, sigma, coef.ctypes.data, seed, row0, step0, steps, p(out), p(eps_in), p(eps_out), _lib.stream_ptr())


def bank(poles):
    """coefficients of the tests' banks: the octave recipe at `poles` poles"""
    return M.recipe("pink", octaves=poles)


# ---- (a) the rule, with injected draws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poles", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_fill_equals_the_model_bit_for_bit(L, n, poles):
    a, b, w = bank(poles)
    rng = np.random.default_rng(1000 * n + poles)
    ladder = M.ladder(n, 0.1, 0.4, env_id0=5)
    for steps in (1, 2, 16):
        for sigma_env in (None, ladder):
            z0 = rng.standard_normal((poles, 4, n)).astype(np.float32)
            eps = rng.standard_normal((steps, poles, n, 4)).astype(np.float32)
            z, out, eps_out = Guarded(z0.size, z0), Guarded(steps * n * 4), Guarded(eps.size)
            rc = call_fill(L, z, n, poles, coef_host(a, b, w), out, steps, sigma=0.25, sigma_env=None if sigma_env is None else dev(sigma_env), eps_in=dev(eps),
                           eps_out=eps_out)
            assert rc == 0, L.hx_last_error()
            zm = z0.copy()
            want = M.fill(zm, a, b, w, eps, 0.25 if sigma_env is None else sigma_env)
            what = (n, poles, steps, sigma_env is not None)
            assert np.array_equal(bits(out.host((steps, n, 4))), bits(want)), what
            assert np.array_equal(bits(z.host((poles, 4, n))), bits(zm)), what
            assert np.array_equal(bits(eps_out.host(eps.shape)), bits(eps)), what


def test_one_pole_at_zero_is_sigma_times_eps(L):
    a, b, w = M.recipe("white")
    n, steps = 65, 3
    eps = np.random.default_rng(2).standard_normal((steps, 1, n, 4)).astype(np.float32)
    z, out = Guarded(4 * n, np.ones((1, 4, n), np.float32)), Guarded(steps * n * 4)
    assert call_fill(L, z, n, 1, coef_host(a, b, w), out, steps, sigma=0.1, eps_in=dev(eps)) == 0
    assert np.array_equal(bits(out.host((steps, n, 4))), bits(np.float32(0.1) * eps[:, 0]))


# ---- (b) the Philox path -----------------------------------------------------------------------------------------------------------------------------
def philox_fill(L, n, poles, steps, seed, row0=0, step0=0, z0=None, sigma=0.1):
    a, b, w = bank(poles)
    z0 = np.zeros((poles, 4, n), np.float32) if z0 is None else z0
    z, out, eps_out = Guarded(z0.size, z0), Guarded(steps * n * 4), Guarded(steps * poles * n * 4)
    assert call_fill(L, z, n, poles, coef_host(a, b, w), out, steps, sigma=sigma, seed=seed, row0=row0, step0=step0, eps_out=eps_out) == 0, L.hx_last_error()
    return z.host((poles, 4, n)), out.host((steps, n, 4)), eps_out.host((steps, poles, n, 4))


@pytest.mark.parametrize("n,poles,steps,row0", [(65, 2, 3, 0), (7, 8, 2, 1000)])
def test_philox_draws(L, n, poles, steps, row0):
    """eps_out is the host's float64 Philox + Box-Muller at the tolerance tests/test_per_score_gpu.py holds the same device logf / sinf / cosf draws to;
    out and z are the model run on eps_out, bit for bit; another seed gives other draws"""
    a, b, w = bank(poles)
    seed = 0x1234567800000007
    z0 = np.random.default_rng(3).standard_normal((poles, 4, n)).astype(np.float32)
    z, out, eps = philox_fill(L, n, poles, steps, seed, row0=row0, step0=5, z0=z0)
    np.testing.assert_allclose(eps, M.philox_eps(seed, row0, n, poles, 5, steps), rtol=1e-3, atol=1e-3)
    zm = z0.copy()
    want = M.fill(zm, a, b, w, eps, 0.1)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(z), bits(zm))
    _, _, other = philox_fill(L, n, poles, steps, seed + 1, row0=row0, step0=5, z0=z0)
    assert not np.array_equal(bits(other), bits(eps))
    _, _, low = philox_fill(L, n, poles, steps, seed & 0xFFFFFFFF, row0=row0, step0=5, z0=z0)  # the key's high word counts
    assert not np.array_equal(bits(low), bits(eps))


@pytest.mark.parametrize("n,poles,row0", [(65, 2, 0), (7, 8, 0xFFFFFFFC)])
def test_init_is_the_stationary_draw(L, n, poles, row0):
    """hx_noise_init: z <- N(0, 1) from its own counters (the env id wraps at 2^32 like every Philox counter word); two seeds differ"""
    from hirl4ucav_amd import _lib

    out = []
    for seed in (11, 12):
        z = Guarded(4 * poles * n)
        assert L.hx_noise_init(z.ptr(), n, poles, seed, row0, _lib.stream_ptr()) == 0, L.hx_last_error()
        out.append(z.host((poles, 4, n)))
        np.testing.assert_allclose(out[-1], M.philox_init(seed, row0, n, poles), rtol=1e-3, atol=1e-3)
    assert not np.array_equal(bits(out[0]), bits(out[1]))


def test_chunk_invariance(L):
    """one fill of 16 steps == 16 fills of 1 step == fills of 5 + 11, bit for bit, in out and in z"""
    n, poles, seed = 130, 3, 21
    z0 = np.random.default_rng(4).standard_normal((poles, 4, n)).astype(np.float32)
    a, b, w = bank(poles)
    c = coef_host(a, b, w)
    want_z, want, _ = philox_fill(L, n, poles, 16, seed, step0=40, z0=z0)
    for split in ([1] * 16, [5, 11]):
        z, got, at = Guarded(z0.size, z0), [], 40
        for steps in split:
            out = Guarded(steps * n * 4)
            assert call_fill(L, z, n, poles, c, out, steps, seed=seed, step0=at) == 0
            got.append(out.host((steps, n, 4)))
            at += steps
        assert np.array_equal(bits(np.concatenate(got)), bits(want)), split
        assert np.array_equal(bits(z.host((poles, 4, n))), bits(want_z)), split


def test_shard_invariance(L):
    """row0 = 0 and row0 = 64 over 64 envs each == one generator over 128 envs (init and fill)"""
    from hirl4ucav_amd import _lib

    poles, seed, steps = 6, 33, 4

    def run(n, row0):
        z = Guarded(4 * poles * n)
        assert L.hx_noise_init(z.ptr(), n, poles, seed, row0, _lib.stream_ptr()) == 0
        return philox_fill(L, n, poles, steps, seed, row0=row0, step0=9, z0=z.host((poles, 4, n)))

    (z_lo, out_lo, _), (z_hi, out_hi, _), (z_all, out_all, _) = run(64, 0), run(64, 64), run(128, 0)
    assert np.array_equal(bits(np.concatenate([out_lo, out_hi], axis=1)), bits(out_all))
    assert np.array_equal(bits(np.concatenate([z_lo, z_hi], axis=2)), bits(z_all))


def test_the_step_counter_is_64_bit(L):
    """step0 = 2^32 - 3, 8 steps: the draws follow the model across the wrap of the low word, and differ from the same low words under high word 0"""
    n, poles, seed, step0 = 5, 2, 77, 2 ** 32 - 3
    _, out, eps = philox_fill(L, n, poles, 8, seed, step0=step0)
    np.testing.assert_allclose(eps, M.philox_eps(seed, 0, n, poles, step0, 8), rtol=1e-3, atol=1e-3)
    a, b, w = bank(poles)
    assert np.array_equal(bits(out), bits(M.fill(np.zeros((poles, 4, n), np.float32), a, b, w, eps, 0.1)))
    _, _, before = philox_fill(L, n, poles, 3, seed, step0=step0)
    _, _, after = philox_fill(L, n, poles, 5, seed, step0=0)  # steps 2^32 .. 2^32 + 4 have the low words 0 .. 4
    assert np.array_equal(bits(eps[:3]), bits(before)) and not np.array_equal(bits(eps[3:]), bits(after))


# ---- (c) refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(L):
    """every refusal returns HX_ERR_ARG, names what is wrong, and launches nothing (z, out and eps_out keep their sentinel words)"""
    from hirl4ucav_amd import _lib

    ERR = _lib.DEFINES["HX_ERR_ARG"]
    n, poles, steps = 64, 2, 4
    a, b, w = bank(poles)
    good = coef_host(a, b, w)
    z, out, eps_out = Guarded(4 * poles * n), Guarded(steps * n * 4), Guarded(steps * poles * n * 4)
    eps_in = torch.zeros(steps * poles * n * 4 + 4, device="cuda")
    st = _lib.stream_ptr()

    def coef(row, k, v):
        c = good.copy()
        c[row, k] = v
        return c

    def fill(z_=z.ptr(), n_=n, poles_=poles, sigma=0.1, c=good, steps_=steps, out_=out.ptr(), eps_in_=None, eps_out_=eps_out.ptr()):
        return L.hx_noise_fill(z_, None, n_, poles_, sigma, None if c is None else c.ctypes.data, 1, 0, 0, steps_, out_, eps_in_, eps_out_, st)

    cases = [
        (lambda: fill(poles_=0), "poles is 1..8"), (lambda: fill(poles_=9), "poles is 1..8"),
        (lambda: fill(steps_=0), "steps is 1..64"), (lambda: fill(steps_=65), "steps is 1..64"),
        (lambda: fill(n_=0), "0 < n_envs < 2\\^31"), (lambda: fill(n_=-1), "0 < n_envs < 2\\^31"), (lambda: fill(n_=2 ** 31), "0 < n_envs < 2\\^31"),
        (lambda: fill(z_=None), "hx_noise_fill: z "), (lambda: fill(out_=None), "hx_noise_fill: out "), (lambda: fill(c=None), "coef "),
        (lambda: fill(out_=out.ptr() + 4), "out is 16-byte aligned"), (lambda: fill(eps_in_=eps_in.data_ptr() + 4), "eps_in is 16-byte aligned"),
        (lambda: fill(eps_out_=eps_out.ptr() + 8), "eps_out is 16-byte aligned"),
        (lambda: fill(c=coef(0, 0, 1.0)), "a\\[0\\] = 1"), (lambda: fill(c=coef(0, 1, -0.25)), "a\\[1\\] = -0.25"), (lambda: fill(c=coef(0, 1, np.nan)), "a\\[1\\]"),
        (lambda: fill(c=coef(0, 0, np.inf)), "a\\[0\\]"), (lambda: fill(c=coef(1, 1, np.inf)), "b\\[1\\] and w\\[1\\] are finite"),
        (lambda: fill(c=coef(2, 0, np.nan)), "b\\[0\\] and w\\[0\\] are finite"), (lambda: fill(sigma=float("nan")), "sigma is finite"),
        (lambda: fill(sigma=float("inf")), "sigma is finite"),
        (lambda: L.hx_noise_init(None, n, poles, 1, 0, st), "hx_noise_init: z "), (lambda: L.hx_noise_init(z.ptr(), 0, poles, 1, 0, st), "0 < n_envs"),
        (lambda: L.hx_noise_init(z.ptr(), n, 9, 1, 0, st), "poles is 1..8"),
    ]
    for call, words in cases:
        assert call() == ERR, words
        assert re.search(words, L.hx_last_error().decode()), (words, L.hx_last_error())
    torch.cuda.synchronize()
    assert z.untouched() and out.untouched() and eps_out.untouched(), "a refused call launched something"
    zeros = Guarded(4 * poles * n, np.zeros(4 * poles * n, np.float32))  # (a state of sentinel NaNs would stay one)
    assert fill(z_=zeros.ptr(), c=coef(0, 2, 7.0)) == 0  # (a coefficient beyond `poles` is not read); the same out and eps_out, now written
    torch.cuda.synchronize()
    assert not zeros.untouched() and not out.untouched() and not eps_out.untouched()
    assert L.hx_noise_workspace_floats(n, 9) == 0 and L.hx_noise_workspace_floats(n, 0) == 0
    assert L.hx_noise_workspace_floats(n, poles) == 4 * poles * n and L.hx_noise_workspace_floats(0, 1) == 0 and L.hx_noise_workspace_floats(2 ** 31, 1) == 0


# ---- (d) ColoredNoise ----------------------------------------------------------------------------------------------------------------------------------
def test_colored_noise_next_and_state(L):
    """next() walks the chunk and refills it every `chunk` calls; the sequence does not depend on the chunk; a state round trip continues it bit for bit;
    the ladder is the model's"""
    from hirl4ucav_amd.utils.noise import ColoredNoise

    def make(chunk, **kw):
        return ColoredNoise(130, "pink", octaves=4, sigma=0.1, sigma_max=0.4, seed=5, env_id0=64, chunk=chunk, device="cuda", **kw)

    g5, g16 = make(5), make(16)
    seq5 = [g5.next().clone() for _ in range(23)]
    seq16 = [g16.next().clone() for _ in range(23)]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(seq5, seq16)) and seq5[0].shape == (130, 4)
    assert np.array_equal(bits(g5.sigma_env.cpu().numpy()), bits(M.ladder(130, 0.1, 0.4, env_id0=64))) and g5.step == 23 and g5.cursor == 3
    st = g5.state_dict()
    h = make(5)
    h.load_state_dict(st)
    for _ in range(9):
        assert torch.equal(h.next().view(torch.int32), g16.next().view(torch.int32))
    with pytest.raises(ValueError, match="chunk 5; this generator has chunk 16"):
        make(16).load_state_dict(st)
    # the scale: out / ladder is the unit-variance x.  Over the 520 independent (env, component) series the mean of x at one step has standard deviation
    # 1 / sqrt(520) = 0.044 and the mean of x^2 sqrt(2 / 520) = 0.062: six of those
    x = seq5[-1].cpu().numpy().astype(np.float64) / M.ladder(130, 0.1, 0.4, env_id0=64)[:, None]
    assert abs(x.mean()) < 6 / np.sqrt(520) and abs((x * x).mean() - 1.0) < 6 * np.sqrt(2 / 520)


def test_act_step_with_generated_noise_equals_act_then_step(L):
    """HirlEngine.act_step(env, noise=gen.next()) == act(obs, noise=...) followed by env.step, bit for bit, over an auto-reset"""
    from hirl4ucav_amd.agents import engine as E
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.noise import ColoredNoise

    params = D.make_params(31)
    e = LS.make_engine(E, 128, params)
    envs = [BatchedHarfangEnv(65, scenario="straight_line", seed=5, max_step=6, replay=None) for _ in range(2)]
    for env in envs:
        env.reset()
    gen = ColoredNoise(65, "ou", tau=8.0, sigma=0.2, seed=9, chunk=4, device="cuda")
    for step in range(9):
        nz, obs_before = gen.next(), envs[1].obs.clone()
        a1, o1, r1, d1, s1 = e.act_step(envs[0], noise=nz)
        a2 = e.act(envs[1].obs, noise=nz)
        o2, r2, d2, s2 = envs[1].step(a2)
        for x, y in ((a1, a2), (o1, o2), (r1, r2)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), step
        assert torch.equal(d1, d2) and torch.equal(s1, s2)
    assert not torch.equal(a2, e.act(obs_before)), "the noise reached the actions"


# ---- (e) the driver --------------------------------------------------------------------------------------------------------------------------------------
PINK = ["--explore_noise", "pink", "--explore_sigma_max", "0.4", "--explore_chunk", "5"]
NOISE_CALLS = {"hx_noise_init", "hx_noise_fill"}


@pytest.mark.parametrize("kind", ["front", "reference", "td3", "sac"])
def test_train_all_pink(L, tmp_path, monkeypatch, capsys, kind):
    """2 driver episodes of 12 steps at 64 envs with pink noise over a ladder of scales — HIRL in both loop forms, TD3, and SAC (whose sigma flags are
    refused: pink alone; the reference's order, and the loop line says why): one fill per 5 vector steps, the three scalars once, the generator in the
    snapshot; the same command line without the flags issues the same library calls but the generator's, name for name"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import COMMON, HIRL
    from tests.test_hirl_nstep_gpu import spy

    sac = kind == "sac"
    args = {"front": HIRL + ["--loop", "front"], "reference": HIRL + ["--loop", "reference"], "td3": ["--agent", "TD3"] + COMMON,
            "sac": ["--agent", "SAC", "--type", "SAC"] + COMMON}[kind]
    flags = ["--explore_noise", "pink", "--explore_chunk", "5"] if sac else PINK
    names, runs, writers = spy(monkeypatch)
    out_dir = T.main(T.parse_args(args + flags + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    pink_names = list(names)
    assert names.count("hx_noise_init") == 1 and names.count("hx_noise_fill") == -(-24 // 5), "one fill per 5 vector steps"
    if kind in ("front", "td3"):
        assert "vector loop: front launch" in out and names.count("hx_hirl_front") == 2 * 11
    elif sac:
        assert ("vector loop: reference order (--explore_noise pink: the coloured draws are the Gaussian head's eps, which act_step takes and the front launch "
                "does not)") in out and "hx_sac_front" not in names
    else:
        assert "vector loop: reference order" in out and "hx_hirl_front" not in names
    rows = {tag: v for tag, v, _ in writers[0].rows if tag.startswith("Explore/")}
    a, b, w = M.recipe("pink", octaves=6)
    lo, hi = (1.0, 1.0) if sac else (float(M.ladder(64, 0.1, 0.4).min()), float(M.ladder(64, 0.1, 0.4).max()))
    assert set(rows) == {"Explore/Sigma Min", "Explore/Sigma Max", "Explore/Lag1 Autocorr"} and sum(t.startswith("Explore/") for t, _, _ in writers[0].rows) == 3
    assert rows["Explore/Sigma Min"] == pytest.approx(lo, rel=1e-6) and rows["Explore/Sigma Max"] == pytest.approx(hi, rel=1e-6)
    assert rows["Explore/Lag1 Autocorr"] == pytest.approx(M.autocorr(a, w, 1), rel=1e-6)
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)
    rec = snap["driver"]["explore"]
    assert rec["flags"] == ({"explore_noise": "pink", "explore_chunk": 5} if sac else {"explore_noise": "pink", "explore_sigma_max": 0.4, "explore_chunk": 5})
    assert rec["generator"]["step"] == 24 and rec["generator"]["cursor"] == 4 and torch.isfinite(rec["generator"]["z"]).all()
    assert torch.isfinite(snap["replay"]["ring"][:min(snap["replay"]["total"], 4096)]).all()
    if sac:
        return
    del names[:]
    plain_dir = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "b")]))
    assert names and not NOISE_CALLS & set(names) and [x for x in pink_names if x not in NOISE_CALLS] == names
    assert "explore" not in torch.load(os.path.join(plain_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)["driver"]
    white = list(names)
    del names[:]
    T.main(T.parse_args(args + ["--explore_noise", "white", "--explore_sigma", "0.1", "--episodes", "2", "--result_dir", str(tmp_path / "c")]))
    assert names == white, "white at the default scale is the run without the flags, call for call"


def test_train_all_pink_resume(L, tmp_path):
    """--separate_launches (one env workgroup: the run is reproducible): 1 episode + --resume to 2 equals the uninterrupted run bit for bit — the arena but
    its logged loss slots (rtol 1e-6 / atol 1e-7), the replay ring and the generator's state; --resume under another value of a flag is a ValueError that
    names the flag"""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.agents import engine as E
    from tests.test_branch_gpu import HIRL

    args = HIRL + PINK + ["--separate_launches"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a, b = (torch.load(os.path.join(d, "state_rank0.pt"), map_location="cpu", weights_only=False) for d in (whole, rest))
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and a["engine"]["counters"] == b["engine"]["counters"]
    e = E.HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-6, atol=1e-7)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] and torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32))
    ga, gb = a["driver"]["explore"]["generator"], b["driver"]["explore"]["generator"]
    assert ga["step"] == gb["step"] == 24 and ga["cursor"] == gb["cursor"] and ga["params"] == gb["params"]
    assert torch.equal(ga["z"].view(torch.int32), gb["z"].view(torch.int32)) and torch.equal(ga["out"].view(torch.int32), gb["out"].view(torch.int32))
    for other, words in ((["--explore_noise", "ou", "--explore_sigma_max", "0.4", "--explore_chunk", "5"], "was run with --explore_noise pink, --explore_noise ou given"),
                         (["--explore_noise", "pink", "--explore_sigma_max", "0.4"], "was run with --explore_chunk 5, --explore_chunk 16 given"),
                         ([], "was run with --explore_noise pink, --explore_noise white given")):
        with pytest.raises(ValueError, match=words):
            T.main(T.parse_args(HIRL + other + ["--separate_launches", "--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))
