"""GPU tests of the episode record (hx_trace_reset / hx_trace_push through utils/trace.py, train_all.validate, validate_all.validate_round and
the two drivers' --plot) against the numpy model of the rule, tests/_trace_model.py — bit for bit: the log is copied words and the score is one
fp32 add per step without contraction.  Smallest shapes that can still go wrong: 1 tracked env, 63 / 64 / 65 (a partial wave, a full one, a
second workgroup with one lane), 130 (three workgroups, ragged tail); 300 envs at a stride of 320; all envs in order and a shuffled id list."""
import ctypes
import glob
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402
from tests import _trace_model as M  # noqa: E402

N, STRIDE, STEPS, GUARD, POISON = 300, 320, 24, 64, 0x5EADBEEF


@pytest.fixture(scope="module")
def TR():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.utils import trace

    return trace


@pytest.fixture(scope="module")
def stream_dev():
    """the CPU test's stream, once, on the device (left unchanged)"""
    s = M.stream(N, STRIDE, STEPS)
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return s, {"state": up(s["state"].view(np.int32)), "reward": up(s["reward"]), "done": up(s["done"]), "success": up(s["success"])}


def raw_push(tr, d, ids, t):
    from hirl4ucav_amd import _lib

    _lib.call("hx_trace_push", ctypes.byref(tr), d["state"][t].data_ptr(), N, STRIDE, d["reward"][t].data_ptr(), d["done"][t].data_ptr(),
              d["success"][t].data_ptr(), _lib.ptr(ids), t, _lib.stream_ptr())


def model_words(model):
    sm = model.summaries()
    return np.concatenate([model.log.ravel()] + [np.ascontiguousarray(sm[name]).view(np.uint32) for name in sm] + [np.array([model.alive], np.uint32)])


def guarded_workspace(TR, k):
    _, words = TR.workspace_layout(k, STEPS)
    ws = torch.zeros(words + GUARD, dtype=torch.int32, device="cuda")
    ws[words:] = POISON
    return ws, words


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 130])
def test_push_equals_the_model(TR, stream_dev, k, gather):
    """24 calls; after every call the whole log, every summary array and the alive word against the model as bits; the guard words behind the
    workspace untouched; reset() + replay writes the same bits again"""
    from hirl4ucav_amd import _lib

    s, d = stream_dev
    ids = np.random.default_rng(100 + k).permutation(N)[:k].astype(np.int32) if gather else None
    ids_dev = torch.from_numpy(ids).cuda() if gather else None
    ws, words = guarded_workspace(TR, k)
    assert words == int(_lib.load().hx_trace_workspace_words(k, STEPS))
    tr = TR.trace_struct(ws, k, STEPS)
    model = M.TraceModel(k, STEPS, ids)
    for rnd in range(2):
        _lib.call("hx_trace_reset", ctypes.byref(tr), _lib.stream_ptr())
        model.reset()
        got = ws.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:words], model_words(model)), f"round {rnd}: after reset"
        for t in range(STEPS):
            raw_push(tr, d, ids_dev, t)
            model.push(s["state"][t], s["reward"][t], s["done"][t], s["success"][t], t)
            got = ws.cpu().numpy().view(np.uint32)
            want = model_words(model)
            bad = np.nonzero(got[:words] != want)[0]
            assert bad.size == 0, f"round {rnd}, step {t}: {bad.size} words differ, first at {bad[:4]}"
            assert (got[words:] == POISON).all(), f"round {rnd}, step {t}: guard words"
    assert 0 <= model.alive <= k and (k < 63 or (model.end_step >= 0).any())


def test_range_errors_launch_nothing(TR, stream_dev):
    from hirl4ucav_amd import _lib

    _, d = stream_dev
    ws, words = guarded_workspace(TR, 65)
    tr = TR.trace_struct(ws, 65, STEPS)
    _lib.call("hx_trace_reset", ctypes.byref(tr), _lib.stream_ptr())
    raw_push(tr, d, None, 0)
    before = ws.cpu().numpy().copy()
    for t in (STEPS, -1):
        with pytest.raises(_lib.HxError, match="hx_trace_push: step"):
            _lib.call("hx_trace_push", ctypes.byref(tr), d["state"][0].data_ptr(), N, STRIDE, d["reward"][0].data_ptr(), d["done"][0].data_ptr(),
                      d["success"][0].data_ptr(), None, t, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(ws.cpu().numpy(), before)


def test_recorder_checks_its_arguments(TR):
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    env = BatchedHarfangEnv(5, scenario="serpentine", seed=1, auto_reset=False, collect_stats=False)
    env.reset()
    for bad in ([5], [0, 0], []):
        with pytest.raises(ValueError):
            TR.EpisodeRecorder(env, bad, max_steps=4)
    with pytest.raises(_lib.HxError, match="GPU only"):
        TR.EpisodeRecorder(env, None, max_steps=4, device="cpu")
    rec = TR.EpisodeRecorder(env, [4, 1], max_steps=2)
    assert rec.alive() == 2 and rec.summary()["end_step"].tolist() == [-1, -1]
    a = torch.zeros(5, 4, device="cuda")
    for _ in range(2):
        env.step(a)
        rec.push()
    with pytest.raises(_lib.HxError, match="hx_trace_push: step 2"):
        rec.push()
    assert rec.t == 2 and rec.summary()["nrec"].tolist() == [2, 2] and rec.episode(1)["self_pos"].shape == (2, 3)
    rec.reset()
    assert rec.t == 0 and rec.summary()["nrec"].tolist() == [0, 0]


EPISODES, EP_STEPS, EP_SEED = 5, 260, 11
FIRE_STEPS = (3, 61, 70, 125, 190, 241)
OUT_OF_BAND, LIFT_AT = 2, 100  # before this step, this episode is put above the altitude band of _get_termination (HarfangEnv_GYM.py:163-164), on both sides


def scripted_actions():
    t = np.arange(EP_STEPS, dtype=np.float64)[:, None, None]
    phase = np.random.default_rng(4).uniform(0, 6.28, (1, EPISODES, 4))
    a = (0.4 * np.sin(0.03 * t + phase)).astype(np.float32)
    a[:, :, 3] = -1.0
    a[list(FIRE_STEPS), :, 3] = 1.0
    return a


def test_a_real_env_against_the_single_env_classes(TR):
    """5 serpentine episodes, random reset, scripted actions and fire steps, 260 steps, all tracked: episode(j) is what the reference's loop
    (train_all.py:28-57) collects from a fresh single-env class stepped with step_test — positions and distance exactly, lists equal"""
    import hirl4ucav_amd.environments.HarfangEnv_GYM as G
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    acts = scripted_actions()
    benv = BatchedHarfangEnv(EPISODES, scenario="serpentine", seed=EP_SEED, auto_reset=False, random_reset=True, collect_stats=False)
    benv.episode_ctr += 1  # (the single-env classes count the episode before they reset: the same Philox counter on both sides)
    benv.reset()
    rec = TR.EpisodeRecorder(benv, None, max_steps=EP_STEPS)
    acts_dev = torch.from_numpy(acts).cuda()
    for t in range(EP_STEPS):
        if t == LIFT_AT:
            benv.state[1, OUT_OF_BAND] = 10050.0
        benv.step(acts_dev[t])
        rec.push()
    sm = rec.summary()
    assert rec.alive() == int((sm["end_step"] < 0).sum())
    assert LIFT_AT <= sm["end_step"][OUT_OF_BAND] < EP_STEPS - 1 and sm["nrec"][OUT_OF_BAND] == sm["end_step"][OUT_OF_BAND] + 1
    for e in range(EPISODES):
        env = G.HarfangSerpentineEnv()
        env._env = BatchedHarfangEnv(1, scenario="serpentine", seed=EP_SEED, auto_reset=False, random_reset=True, env_id0=e, collect_stats=False)
        env.random_reset()
        self_pos, oppo_pos, distance, fire, lock, missile, total, done = [], [], [], [], [], [], 0.0, False
        for step in range(EP_STEPS):
            if done:
                break
            if e == OUT_OF_BAND and step == LIFT_AT:
                env._env.state[1, 0] = 10050.0
            _, reward, done, _, iffire, beforeaction, _, locked, _ = env.step_test(acts[step, e])
            total += reward
            distance.append(env.loc_diff)
            if iffire:
                fire.append(step)
            if locked:
                lock.append(step)
            if beforeaction:
                missile.append(step)
            self_pos.append(env.get_pos())
            oppo_pos.append(env.get_oppo_pos())
        ep = rec.episode(e)
        T = len(distance)
        assert sm["nrec"][e] == T and sm["end_step"][e] == (T - 1 if done else -1), e
        assert np.array_equal(ep["self_pos"], np.array(self_pos)) and np.array_equal(ep["oppo_pos"], np.array(oppo_pos)), e
        assert np.array_equal(ep["distance"], np.array(distance)), e
        assert (ep["fire"], ep["lock"], ep["missile"]) == (fire, lock, missile), e
        assert fire and missile, e
        assert bool(sm["kill"][e]) == (done and env.episode_success) and bool(sm["fire_success"][e]) == (done and env.fire_success), e
        assert abs(float(sm["total"][e]) - total) <= 1e-4 * max(1.0, abs(total)), e  # (fp32 adds against the loop's float64 adds)


class _ScriptedFire:
    """the engine's policy with the launch decision scripted (tests/test_facade_gpu.py: a random-init actor never locks or fires)"""

    def __init__(self, eng, fire_steps):
        self.eng, self.fire_steps, self.t, self.act_calls = eng, set(fire_steps), 0, 0

    def act(self, obs):
        a = self.eng.act(obs).clone()
        a[:, 3] = 1.0 if self.t in self.fire_steps else -1.0
        self.t += 1
        return a


@pytest.fixture(scope="module")
def engine():
    from hirl4ucav_amd.agents import engine as E

    params = D.make_params(D.PARAM_SEED)
    eng = E.HirlEngine(batch=128)
    eng.load_params(params["actor"], params["critic"], params["bc_actor"])
    return eng


def val_env(episodes, seed):
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    env = BatchedHarfangEnv(episodes, scenario="serpentine", seed=seed, auto_reset=False, random_reset=True, collect_stats=False)
    env.reset()
    env.state[1, 3] = 10050.0  # one episode ends at once
    return env


def test_summary_equals_validate(TR, engine):
    from hirl4ucav_amd import train_all as T

    episodes, steps, seed, dev = 8, 200, 21, torch.device("cuda")
    plain = T.validate(_ScriptedFire(engine, FIRE_STEPS), "serpentine", episodes, steps, True, seed, dev, env=val_env(episodes, seed))
    env = val_env(episodes, seed)
    rec = TR.EpisodeRecorder(env, None, max_steps=steps)
    got = T.validate(_ScriptedFire(engine, FIRE_STEPS), "serpentine", episodes, steps, True, seed, dev, env=env, recorder=rec)
    assert got == plain
    sm = rec.summary()
    assert (float(sm["total"].mean()), float(sm["total"].std()), int(sm["kill"].sum()), int(sm["fire_success"].sum())) == got
    assert sm["end_step"][3] >= 0 and sm["end_step"][3] < steps - 1 and rec.alive() == int((sm["end_step"] < 0).sum()) and rec.t == steps


@pytest.mark.parametrize("infinite", [False, True])
def test_summary_equals_validate_round(TR, engine, infinite):
    from hirl4ucav_amd import validate_all as V

    episodes, steps, seed, dev = 8, 200, 22, torch.device("cuda")
    plain = V.validate_round(_ScriptedFire(engine, FIRE_STEPS), episodes, steps, True, seed, dev, infinite=infinite, env=val_env(episodes, seed))
    env = val_env(episodes, seed)
    rec = TR.EpisodeRecorder(env, None, max_steps=steps)
    got = V.validate_round(_ScriptedFire(engine, FIRE_STEPS), episodes, steps, True, seed, dev, infinite=infinite, env=env, recorder=rec)
    assert got == plain
    sm = rec.summary()
    mean = float(torch.from_numpy(sm["total"]).cuda().mean())  # (validate_round's own reduction, on the recorder's scores)
    seen = (sm["end_step"] >= 0) & (sm["end_step"] < steps - 1)  # `done` raised by the last allowed step is never looked at (validate_all.py:59-60)
    launches, hits = int(sm["launches"].sum()), int(sm["hits"].sum())
    rate = hits / launches if (infinite and launches > 0) else 0.0
    assert (mean, int((sm["fire_success"] & seen).sum()) / episodes, rate) == got
    assert launches >= episodes - 1 and (not infinite or launches > episodes)  # missiles DID leave the rail; re-armed ones too


SAC_ARGS = ["--agent", "SAC", "--type", "SAC", "--env", "serpentine", "--random", "--seed", "3", "--num_envs", "64", "--buffer_size", "4096", "--max_step", "12",
            "--checkpoint_rate", "1", "--snapshot_every", "0", "--episodes", "1"]


def test_train_all_plot_writes_the_references_files(TR, tmp_path):
    from hirl4ucav_amd import train_all as T

    run = T.main(T.parse_args(SAC_ARGS + ["--plot", "--result_dir", str(tmp_path / "a")]))
    rows = {}
    for name in ("self_pos", "oppo_pos", "distance", "fire", "lock"):
        f = os.path.join(run, "plot", "csv", f"{name}1.csv")
        assert os.path.exists(f), f
        rows[name] = len(open(f).read().splitlines())
    assert sorted(os.listdir(os.path.join(run, "plot", "csv"))) == sorted(f"{n}1.csv" for n in rows)
    assert 1 <= rows["self_pos"] == rows["oppo_pos"] == rows["distance"] <= 12
    plain = T.main(T.parse_args(SAC_ARGS + ["--result_dir", str(tmp_path / "b")]))
    assert not os.path.exists(os.path.join(plain, "plot", "csv"))
    assert os.listdir(os.path.join(plain, "model")) and os.listdir(os.path.join(run, "model"))  # both validated and saved a checkpoint


def test_validate_all_plot_writes_every_round(TR, tmp_path, capsys):
    from hirl4ucav_amd import validate_all as V

    params = D.make_params(D.PARAM_SEED)
    model = tmp_path / "model"
    os.makedirs(model)
    torch.save({k: torch.as_tensor(v) for k, v in params["actor"].items()}, os.path.join(model, "Agent7_100_5_Actor_Harfang_GYM"))
    common = ["--agent", "HIRL", "--model_dir", str(model), "--model_name", "Agent7_100_5_", "--random", "--seed", "3", "--episodes", "8", "--validation_step", "100"]
    plain = V.main(V.parser().parse_args(common))
    assert not os.path.exists(tmp_path / "plot")
    got = V.main(V.parser().parse_args(common + ["--plot", "--plot_dir", str(tmp_path / "p")]))
    assert got == plain
    for k in (1, 2):
        assert sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "p" / "csv" / f"*round{k}.csv"))) == \
            [f"{n}round{k}.csv" for n in ("distance", "fire", "lock", "oppo_pos", "self_pos")]
    rows = [len(open(tmp_path / "p" / "csv" / f"{n}round2.csv").read().splitlines()) for n in ("distance", "self_pos", "oppo_pos")]
    assert 1 <= rows[0] <= 100 and rows[0] == rows[1] == rows[2]
    V.main(V.parser().parse_args(common + ["--plot"]))  # the default: `plot` beside the checkpoint directory
    assert os.path.exists(tmp_path / "plot" / "csv" / "self_posround1.csv")
