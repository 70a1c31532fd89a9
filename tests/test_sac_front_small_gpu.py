"""The SAC front launch up to 8,192 envs (hx_sac_front's per-tile acting role, act_sac_front_kernel: the workgroups of hx_sac_act_step from the fp32 / bf16 image and the
first forward launch of SacAgent.learn as ONE launch; SacEngine.step_learn; train_all's default loop for SAC / E-SAC).

Parity statement, as for the role beyond 8,192 envs (tests/test_front_gpu.py): one step_learn == act_step, then learn() on a minibatch drawn with
HxSample.total read before the env step and HxSample.guard = n — bit for bit in everything both leave behind (replay rows as a multiset: ring slots are
handed out by an atomic), logged loss sums to 1e-6 (accumulated with atomics)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_front_gpu import allowed_slots, sorted_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state")


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


def make_side(SE, n, cap, dtype, batch=128):
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay
    from tests.test_oracle_sac import sac_params
    from tests.test_sac_bf16_gpu import engine

    if dtype == "bf16":
        assert batch == 128
        e = engine(SE, "bf16", "bf16")
    else:
        p = sac_params()
        e = SE.SacEngine(batch=batch)
        e.load_params(p["policy"], p["q1"], p["q2"])
    rep = DeviceReplay(cap)
    env = BatchedHarfangEnv(n, scenario=(np.arange(n) % 3).astype(np.int32), seed=5, max_step=6, auto_reset=True, random_reset=True, replay=rep)
    env.reset()
    return e, env, rep


def expert_memory(seed):
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    exp = DeviceReplay(64)
    exp.store_rows(torch.from_numpy(np.random.default_rng(seed).normal(size=(40, 32)).astype(np.float32)))
    return exp


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


@pytest.mark.parametrize("n,cap,esac,dtype,batch", [
    pytest.param(200, 512, False, "f32", 128, id="200-512-False-f32"),        # a half-filled last 16-row tile (cap 512: the smallest ring the library takes)
    pytest.param(256, 640, False, "bf16", 128, id="256-640-False-bf16"),      # the driver tests' size
    pytest.param(1000, 2400, True, "f32", 128, id="1000-2400-True-f32"),      # E-SAC's mixed batch (n_main = 96), ragged tail
    pytest.param(4096, 10000, False, "f32", 128, id="4096-10000-False-f32"),  # one full round of 16-row workgroups
    pytest.param(4097, 10000, True, "bf16", 128, id="4097-10000-True-bf16"),  # where the stand-alone bf16 kernel changes its tiling
    pytest.param(8192, 20000, False, "f32", 128, id="8192-20000-False-f32"),  # the last size of the per-tile role
    pytest.param(8192, 20000, False, "bf16", 128, id="8192-20000-False-bf16"),
    pytest.param(200, 512, False, "f32", 48, id="200-512-False-f32-batch48"),    # an odd number of 16-row tiles in the minibatch
    pytest.param(200, 512, False, "f32", 256, id="200-512-False-f32-batch256")])  # kFusedBatchMax: the largest minibatch the front launch takes
def test_sac_small_front_launch_equals_act_step_then_guarded_learn(SE, n, cap, esac, dtype, batch):
    """8 steps from shared states with max_step = 6 (episodes reset; the ring fills and wraps): step_learn on side a, the separate launches with the
    guarded draw on side b.  Every shape leaves the guarded draw at least `batch` slots (cap - n once the ring is full; before that the rows of the
    env steps taken ahead of the first draw: one step, two for 256 rows out of 200 envs); the smallest ring is 512 rows because the library takes none
    below that (check_step_args)."""
    exp = expert_memory(n) if esac else None
    (a, env_a, rep_a), (b, env_b, rep_b) = make_side(SE, n, cap, dtype, batch), make_side(SE, n, cap, dtype, batch)
    state = STATE + (("images",) if dtype == "bf16" else ())
    n_main = batch - 32
    assert cap - n >= batch
    for _ in range(-(-batch // n)):
        a.act_step(env_a, seed=3)  # at least `batch` rows in the ring before the first draw
    snap = torch.zeros(1, dtype=torch.int64, device="cuda")
    for k in range(8):
        b.arena.copy_(a.arena)
        if dtype == "bf16":
            b.images.copy_(a.images)
        for name in ("learning_steps", "sample_calls", "act_calls"):
            setattr(b, name, getattr(a, name))
        env_b._state_store.copy_(env_a._state_store)
        for name in ("obs", "reward", "done", "success", "episode_ctr"):
            getattr(env_b, name).copy_(getattr(env_a, name))
        rep_b.ring.copy_(rep_a.ring); rep_b.success.copy_(rep_a.success); rep_b.total.copy_(rep_a.total)  # noqa: E702
        tot0 = int(rep_a.total.item())
        out_a = a.step_learn(env_a, exp, n_main=n_main, act_seed=3, sample_seed=11)
        snap.copy_(rep_b.total)
        out_b = b.act_step(env_b, seed=3)
        b.sample(rep_b, exp, n_main=n_main, seed=11, defer=True)
        b._pending[0].total, b._pending[0].guard = snap.data_ptr(), n
        b.learn()
        for x, y, name in zip(out_a, out_b, ("actions", "obs", "reward", "done", "success")):
            assert torch.equal(x, y), (k, name)
        assert torch.equal(env_a._state_store, env_b._state_store) and torch.equal(rep_a.total, rep_b.total), k
        np.testing.assert_array_equal(sorted_rows(rep_a), sorted_rows(rep_b), err_msg=f"step {k}: replay rows")
        assert torch.equal(a._idx, b._idx) and torch.equal(a.rows, b.rows), k
        np.testing.assert_allclose(a.losses_host(), b.losses_host(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
        for name in state:
            assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), (k, name)
        i = a._idx.cpu().numpy()
        m = n_main if esac else batch
        assert len(set(i[:m])) == m and np.isin(i[:m], allowed_slots(tot0, cap, n)).all(), (k, tot0)
    assert int(rep_a.total.item()) > cap


ENV_FIELDS = ("obs", "reward", "done", "success", "episode_ctr")
COUNTERS = ("learning_steps", "sample_calls", "act_calls")


def six_steps(SE, record=None, n=1000, cap=2400):
    """Six step_learn calls (fp32, n = 1,000).  record=None: a free run from a fixed start, which returns what every step started from and what it left
    (networks and moments, actions, the sorted ring rows).  record given: the same six calls, each from the recorded starting state, compared bit for bit
    with what the recorded run left.  (Two FREE runs cannot be compared beyond their first step: ring slots are handed out by an atomic per acting
    workgroup, so where a row lands, and with it the next minibatch, follows the workgroup schedule.  Hence every step starts from the recorded state,
    and draws its minibatch at once instead of taking the tile the previous step drew from this run's own ring.)"""
    e, env, rep = make_side(SE, n, cap, "f32")
    e.act_step(env, seed=3)
    rec = {}
    for k in range(6):
        start = {"arena": e.arena, "state_store": env._state_store, "ring": rep.ring, "ring_success": rep.success, "total": rep.total}
        start.update({name: getattr(env, name) for name in ENV_FIELDS})
        if record is None:
            rec.update({f"{k}/start/{name}": t.cpu().numpy() for name, t in start.items()})
            rec[f"{k}/start/counters"] = np.array([getattr(e, name) for name in COUNTERS], dtype=np.int64)
        else:
            for name, t in start.items():
                t.copy_(torch.from_numpy(record[f"{k}/start/{name}"]))
            for name, v in zip(COUNTERS, record[f"{k}/start/counters"]):
                setattr(e, name, int(v))
            e._front_drawn = None
        out = e.step_learn(env, None, act_seed=3, sample_seed=11)
        left = {name: getattr(e, name).cpu().numpy() for name in STATE}
        left["actions"], left["sorted_ring"] = out[0].cpu().numpy(), sorted_rows(rep)
        for name, v in left.items():
            if record is None:
                rec[f"{k}/left/{name}"] = v
            else:
                np.testing.assert_array_equal(v, record[f"{k}/left/{name}"], err_msg=f"step {k}: {name}")
    return rec


CHILD = ("import sys; sys.path.insert(0, %r)\n"
         "import numpy as np\n"
         "from hirl4ucav_amd.agents import sac_engine\n"
         "from tests import test_sac_front_small_gpu as T\n"
         "T.six_steps(sac_engine, record=np.load(sys.argv[1]))\n"
         "print('tiling ok')\n") % ROOT


@pytest.fixture(scope="module")
def default_run(SE, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sac_front_small") / "default_run.npz")
    np.savez(path, **six_steps(SE))
    return path


@pytest.mark.parametrize("rows_per_workgroup,knob", [(16, "1000000000"), (32, "1")])
def test_sac_small_front_tilings_agree_bit_for_bit(default_run, rows_per_workgroup, knob):
    """HX_SAC_FRONT_F32_NRT2_ROWS (read once per process: hence the child) forces 16-row, then 32-row acting workgroups at n = 1,000: a row's action does
    not depend on the tiling, so the same six step_learn calls leave the same networks, actions and ring rows as this process's default run."""
    env = dict(os.environ, HX_SAC_FRONT_F32_NRT2_ROWS=knob, HX_SAC_FRONT_BF16_NRT2_ROWS=knob)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, default_run], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "tiling ok" in r.stdout, (rows_per_workgroup, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _bc_file(tmp_path):
    from tests.test_isac_gpu import bc_actor_params

    f = tmp_path / "bc_actor.pth"
    torch.save({k: torch.from_numpy(v) for k, v in bc_actor_params().items()}, f)
    return str(f)


def test_sac_small_front_drivers(SE, tmp_path, monkeypatch, capsys):
    """train_all --agent SAC at 256 envs takes the front form by default (SAC and E-SAC), --loop reference keeps the reference's order, and --type ISAC
    runs step_learn's reference-order branch and logs its gate."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.scalars import JsonlWriter

    monkeypatch.setattr(T, "make_writer", JsonlWriter)
    monkeypatch.setitem(T.MAX_STEP, "serpentine", 30)
    common = ["--agent", "SAC", "--env", "serpentine", "--random", "--seed", "2", "--num_envs", "256", "--buffer_size", "32768", "--episodes", "1",
              "--checkpoint_rate", "1000", "--snapshot_every", "0"]

    def alpha_of(out):
        return float(re.search(r"Episode 1: .* alpha (\S+)", out).group(1))

    T.main(T.parse_args(common + ["--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert "vector loop: front launch" in out and np.isfinite(alpha_of(out)) and alpha_of(out) > 0.0
    T.main(T.parse_args(common + ["--loop", "reference", "--result_dir", str(tmp_path / "b")]))
    out = capsys.readouterr().out
    assert "vector loop: reference order" in out and np.isfinite(alpha_of(out))
    T.main(T.parse_args(common + ["--type", "ESAC", "--synthetic_expert", "--result_dir", str(tmp_path / "c")]))
    out = capsys.readouterr().out
    assert "vector loop: front launch" in out and np.isfinite(alpha_of(out))
    run = T.main(T.parse_args(common + ["--type", "ISAC", "--synthetic_expert", "--bc_actor", _bc_file(tmp_path), "--result_dir", str(tmp_path / "d")]))
    assert "Episode 1:" in capsys.readouterr().out
    sc = [json.loads(ln) for ln in open(os.path.join(run, "summary", "scalars.jsonl"))]
    w = [s["value"] for s in sc if s["tag"] == "loss/bc_weight"]
    assert w and all(0.0 <= v <= 1.0 for v in w), w


def test_sac_small_front_refusals_remain(SE):
    """what step_learn refused before it still refuses at these sizes: more than one rank, the staged policy half, the critics' Adam as a call of its own,
    a deferred draw still pending"""
    from hirl4ucav_amd import _lib

    e, env, rep = make_side(SE, 256, 640, "f32")
    e.act_step(env, seed=3)
    for attr, value, back in (("world", 2, 1), ("staged_policy", True, False), ("separate_critic_adam", True, False)):
        assert getattr(e, attr) == back
        setattr(e, attr, value)
        with pytest.raises(_lib.HxError, match="one GPU, the one-call learn"):
            e.step_learn(env, None, act_seed=3, sample_seed=11)
        setattr(e, attr, back)
    e.sample(rep, None, seed=11, defer=True)
    with pytest.raises(_lib.HxError, match="still pending"):
        e.step_learn(env, None, act_seed=3, sample_seed=11)
    e._pending = None
    e.step_learn(env, None, act_seed=3, sample_seed=11)  # ... and nothing else is refused
    assert np.isfinite(e.losses_host()).all()
