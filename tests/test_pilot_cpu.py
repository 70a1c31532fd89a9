"""Host-side tests of the pilot kernels' rule and of --expert_online (no GPU): the numpy model of tests/_pilot_model.py against the torch pilot and
against its own float64 form, the conditions the shared seeded inputs must meet, the refresh rule's env picks / slots / initial fill, the parser's
flags with every refusal by name, and OnlineExpert's state round trip."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hirl4ucav_amd import train_all as T  # noqa: E402
from hirl4ucav_amd.data.expert_pilot import pursuit_actions  # noqa: E402
from hirl4ucav_amd.utils import pilot as P  # noqa: E402
from tests import _pilot_model as M  # noqa: E402

N_BIG = 200_000
ULP_AT_ONE = float(np.spacing(np.float32(1.0)))  # 2^-23 = 1.19e-7


@pytest.fixture(scope="module")
def big():
    state, obs, noise = M.make_inputs(N_BIG, seed=5, special=False)
    return state, obs, noise, M.actions(state, obs)


def test_fp32_model_against_the_torch_pilot(big):
    """the fire column is equal; the levels are within one fp32 ulp at 1.0 of torch's (its norm sums the squares in another order: some rows differ
    in a bit, which is why the GPU tests compare against the model and not against torch)"""
    state, obs, _, mine = big
    ref = pursuit_actions(torch.from_numpy(state), torch.from_numpy(obs)).numpy()
    assert np.array_equal(mine[:, 3], ref[:, 3])
    diff = np.abs(mine[:, :3].astype(np.float64) - ref[:, :3].astype(np.float64))
    differ = (mine[:, :3].view(np.uint32) != ref[:, :3].view(np.uint32)).any(1).mean()
    print(f"fp32 model against torch on {N_BIG} states: max |diff| {diff.max():.3g}, rows that differ in some bit {100 * differ:.2f} %")
    assert diff.max() <= ULP_AT_ONE


def test_fp32_model_against_the_fp64_model(big):
    """the fp32 rounding error of the rule itself, against the same rule in float64 on the same (fp32) inputs.  Measured on these inputs: see the
    printed figure (DESIGN.md section 5 records it); the bound is the 6.2e-7 measured when the rule was specified, doubled."""
    state, obs, noise, mine = big
    ref = M.actions(state, obs, dtype=np.float64)
    assert ref.dtype == np.float64 and np.array_equal(mine[:, 3], ref[:, 3])
    err = np.abs(mine[:, :3].astype(np.float64) - ref[:, :3]).max()
    noisy = np.abs(M.actions(state, obs, noise)[:, :3].astype(np.float64) - M.actions(state, obs, noise, dtype=np.float64)[:, :3]).max()
    print(f"fp32 model against the fp64 model on {N_BIG} states: max |diff| {err:.3g} (with noise {noisy:.3g})")
    assert err <= 2 * 6.2e-7 and noisy <= 2 * 6.2e-7


@pytest.mark.parametrize("n", [300])
def test_seeded_inputs_cover_the_cases(n):
    """the inputs the GPU tests run on cannot pass vacuously: each level clamped at +1 and at -1 somewhere and unclamped in at least a third of the
    rows, both fire values, a row with nrm < 1e-6, a non-finite row"""
    state, obs, noise = M.make_inputs(n)
    for nz in (None, noise):
        a = M.actions(state, obs, nz)
        finite = np.isfinite(a).all(1)
        for c in range(3):
            assert (a[finite, c] == 1).any() and (a[finite, c] == -1).any(), c
            assert (np.abs(a[finite, c]) < 1).sum() * 3 >= n, (c, (np.abs(a[finite, c]) < 1).sum())
        assert (a[:, 3] == 1).any() and (a[:, 3] == -1).any() and set(np.unique(a[:, 3])) == {-1.0, 1.0}
        assert not finite.all() and finite.sum() >= n - 2
    nrm = M.norm_of(state)
    assert (nrm < 1e-6).any() and nrm[M.SPECIAL["coincide"]] == 0
    a = M.actions(state, obs)
    assert (a[M.SPECIAL["coincide"], :3] == 0).all()  # 0 / 1e-6
    assert not np.isfinite(a[M.SPECIAL["nan_state"], :3]).all() and not np.isfinite(a[M.SPECIAL["inf_state"], :3]).all()


def test_clamp_keeps_a_nan():
    v = np.array([np.nan, -3.0, 3.0, 0.25, -np.inf, np.inf], np.float32)
    out = M.clamp(v)
    assert np.isnan(out[0]) and list(out[1:]) == [-1.0, 1.0, 0.25, -1.0, 1.0]


@pytest.mark.parametrize("n,k", [(1, 1), (65, 64), (300, 7), (300, 130)])
def test_env_picks(n, k):
    """distinct within a call; every env is picked within n calls (pick 0 alone walks the population); the window moves by one env per call"""
    seen = set()
    for call in range(n):
        picks = M.env_picks(call, n, k)
        assert len(picks) == k == len(set(picks)) and all(0 <= e < n for e in picks)
        assert picks == [(e + 1) % n for e in M.env_picks(call - 1, n, k)] if call else True
        seen.update(picks)
    assert seen == set(range(n))
    for call in (2 ** 32 - 1, 2 ** 32, 2 ** 40):
        picks = M.env_picks(call, n, k)
        assert len(set(picks)) == k and picks[0] == call % n


@pytest.mark.parametrize("k,m,e0", [(1, 1, 3), (64, 100, 5), (7, 50, 40), (130, 130, 1)])
def test_slots_wrap_fifo(k, m, e0):
    """the slots of consecutive calls continue each other around the online region, at small calls and across 2^32 and 2^40"""
    for call0 in (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40):
        run = [s for c in range(call0, call0 + 2 * (m // k + 2)) for s in M.slots(c, k, m, e0)]
        assert all(e0 <= s < e0 + m for s in run)
        assert all((b - e0) == (a - e0 + 1) % m for a, b in zip(run, run[1:]))
        assert run[0] == e0 + (call0 * k) % m
        for c in range(call0, call0 + 3):
            assert len(set(M.slots(c, k, m, e0))) == k
    assert P.rows_written(0, k, m) == 0 and P.rows_written(1, k, m) == min(k, m) and P.rows_written(2 ** 40, k, m) == m


def test_initial_fill():
    off = M.make_offline(5)
    t = M.initial_table(off, 12)
    assert t.shape == (17, 32) and np.array_equal(t[:5], off)
    for i in range(12):
        assert np.array_equal(t[5 + i], off[i % 5])
    assert P.initial_fill_index(5, 12) == [i % 5 for i in range(12)]
    env = types.SimpleNamespace(n=8, device=torch.device("cpu"))
    on = P.OnlineExpert(env, torch.from_numpy(off), 12, 4)
    assert np.array_equal(on.table.numpy(), t) and on.call == 0 and on.rows_written() == 0
    with pytest.raises(Exception, match="GPU only"):
        on.push()


def test_refresh_model_skips_non_finite_rows():
    n, k, m, e0 = 65, 64, 100, 5
    state, obs, _ = M.make_inputs(n)
    model = M.RefreshModel(M.initial_table(M.make_offline(e0), m), e0, m, k)
    before = model.table.copy()
    wrote = model.push(state, obs)
    picks, slots = M.env_picks(0, n, k), M.slots(0, k, m, e0)
    bad = [s for e, s in zip(picks, slots) if e in (M.SPECIAL["nan_state"], M.SPECIAL["inf_state"])]
    assert len(bad) == 2 and not set(bad) & set(wrote) and len(wrote) == k - 2
    assert all(np.array_equal(model.table[s], before[s]) for s in bad) and np.array_equal(model.table[:e0], before[:e0])
    assert (model.table[wrote, 17:] == 0).all() and np.isfinite(model.table).all() and model.call == 1


BASE = ["--agent", "HIRL", "--type", "soft", "--num_envs", "32"]


def test_parser_flags_and_refusals():
    cfg = T.parse_args(BASE)
    assert cfg.expert_online == 0 and cfg.expert_online_per_step == 64 and T.expert_online_refusal(cfg) is None
    cfg = T.parse_args(BASE + ["--expert_online", "64", "--expert_online_per_step", "8"])
    assert (cfg.expert_online, cfg.expert_online_per_step) == (64, 8) and T.expert_online_refusal(cfg) is None
    for extra in (["--type", "linear"], ["--type", "fixed"], ["--dtype", "bf16"], ["--loop", "reference"], ["--separate_launches"], ["--expert_upsample"],
                  ["--buffer_upsample"], ["--env", "mixed"]):
        assert T.expert_online_refusal(T.parse_args(BASE + ["--expert_online", "64", "--expert_online_per_step", "8"] + extra)) is None, extra
    on = ["--num_envs", "32", "--expert_online", "64", "--expert_online_per_step", "8"]
    cases = [(["--agent", "TD3"] + on, "--expert_online goes with --agent HIRL .TD3"),
             (["--agent", "BC"] + on, "--expert_online goes with --agent HIRL .--agent BC has no rollouts"),
             (["--agent", "SAC", "--type", "SAC"] + on, "--expert_online goes with --agent HIRL .SAC / ESAC / ISAC"),
             (["--agent", "SAC", "--type", "ESAC", "--synthetic_expert"] + on, "--expert_online goes with --agent HIRL .SAC / ESAC / ISAC"),
             (["--agent", "SAC", "--type", "ISAC", "--synthetic_expert", "--bc_actor", "x"] + on, "--expert_online goes with --agent HIRL .SAC / ESAC / ISAC"),
             (BASE + ["--gpus", "2", "--expert_online", "64", "--expert_online_per_step", "8"], "--expert_online runs on one GPU"),
             (BASE + ["--expert_online", "-1"], "--expert_online -1"),
             (BASE + ["--expert_online", "64", "--expert_online_per_step", "0"], "--expert_online_per_step 0"),
             (BASE + ["--expert_online", "16", "--expert_online_per_step", "17"], "--expert_online_per_step 17"),
             (BASE + ["--expert_online", "64", "--expert_online_per_step", "33"], "--expert_online_per_step 33")]
    for argv, why in cases:
        got = T.expert_online_refusal(T.parser().parse_args(argv))
        assert got is not None and __import__("re").search(why, got), (argv, got)
        with pytest.raises(SystemExit):
            T.parse_args(argv)
    assert "--gpus" in T.expert_online_refusal(T.parser().parse_args(BASE + ["--expert_online", "64", "--expert_online_per_step", "8"]), world=2)


def test_state_round_trip_and_resume_refusal():
    env = types.SimpleNamespace(n=8, device=torch.device("cpu"))
    off = torch.from_numpy(M.make_offline(5))
    a = P.OnlineExpert(env, off, 12, 4)
    a.table[5:] = torch.arange(12 * 32, dtype=torch.float32).view(12, 32)
    a.call = 2 ** 33 + 7
    st = a.state_dict()
    assert set(st) == {"online", "call", "online_rows", "per_step", "offline_rows"} and not st["online"].is_cuda
    a.table[5:] = 0  # (the snapshot is a copy)
    b = P.OnlineExpert(env, off, 12, 4)
    b.load_state_dict(st)
    assert b.call == 2 ** 33 + 7 and torch.equal(b.table[5:], torch.arange(12 * 32, dtype=torch.float32).view(12, 32)) and torch.equal(b.table[:5], off)
    with pytest.raises(ValueError, match="--expert_online 12 --expert_online_per_step 4"):
        P.OnlineExpert(env, off, 12, 3).load_state_dict(st)
    with pytest.raises(ValueError, match="--expert_online 12"):
        P.OnlineExpert(env, off, 16, 4).load_state_dict(st)
    with pytest.raises(ValueError, match="offline expert rows"):
        P.OnlineExpert(env, torch.from_numpy(M.make_offline(6)), 12, 4).load_state_dict(st)
    for bad in ((8, 5, 0, 1), (8, 0, 4, 1), (8, 5, 4, 0), (8, 5, 4, 5), (3, 5, 12, 4)):
        assert P.online_args_refusal(*bad) is not None, bad
    assert P.online_args_refusal(8, 5, 12, 8) is None
    # --resume under other values of either flag: refused by the flag's name
    driver = {"episode": 1, "expert_online": st}
    cfg = lambda *a_: T.parser().parse_args(BASE + list(a_))  # noqa: E731
    assert T.expert_online_resume_refusal(cfg("--expert_online", "12", "--expert_online_per_step", "4"), driver) is None
    assert T.expert_online_resume_refusal(cfg("--expert_online", "12", "--expert_online_per_step", "4"), None) is None
    assert "--expert_online 12, --expert_online 16 given" in T.expert_online_resume_refusal(cfg("--expert_online", "16", "--expert_online_per_step", "4"), driver)
    assert "--expert_online_per_step 4, --expert_online_per_step 2 given" in T.expert_online_resume_refusal(cfg("--expert_online", "12", "--expert_online_per_step", "2"), driver)
    assert "--expert_online 12, --expert_online 0 given" in T.expert_online_resume_refusal(cfg(), driver)
    assert "--expert_online 0, --expert_online 12 given" in T.expert_online_resume_refusal(cfg("--expert_online", "12", "--expert_online_per_step", "4"), {"episode": 1})
    assert T.expert_online_resume_refusal(cfg(), {"episode": 1}) is None
