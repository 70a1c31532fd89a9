"""GPU tests of SAC's imitative branch (hx_sac_policy_grads_imitative / hx_sac_learn_imitative through SacEngine, SacAgent and train_all)
against the CPU restatement tests/_isac_check.py and the golden vectors recorded from the reference's SacAgent.learn(imitative=True)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sac_oracle as S  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _isac_check as C  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402
from tests.test_sac_gpu import grad_bad, sync  # noqa: E402

STATE = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i")


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


def bc_actor_params(seed=5):
    from oracle import hirl_oracle as H

    return H.init_actor(np.random.default_rng(seed))


def make_rings(seed=5):
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    rng = np.random.default_rng(seed)
    rep = DeviceReplay(4096)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(4096, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += 4096
    exp = DeviceReplay(512)
    rows = rng.normal(size=(400, 32)).astype(np.float32)
    rows[:, 13:17] = rng.uniform(-1, 1, (400, 4))
    exp.store_rows(torch.from_numpy(rows))
    return rep, exp


def test_isac_learn_matches_restatement_and_reference(SE, golden_dir):
    """The structure of test_sac_learn_matches_oracle_and_reference on the STAGED imitative sequence (hx_sac_critic_step +
    hx_sac_policy_grads_imitative + hx_sac_adam(1)): per call the restatement is synced to the engine; every gradient entry by grad_bad's rule
    (a miss must be explained by a ReLU kink), the eight outputs against the restatement at rtol 2e-5 (atol 5e-6 for the six existing ones
    only) and against the golden at rtol 5e-5 (absolute floors for the existing outputs as in the existing test; relative only for bc_loss
    and policy_loss, which carries bc_loss * w), the gate's count equal to the golden's."""
    from tests.test_hirl_gpu import oracle_checked

    g = np.load(os.path.join(golden_dir, "isac_learn.npz"))
    params, data = C.isac_params(int(g["seed"])), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"])
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    table = torch.from_numpy(data["expert_rows"]).cuda().contiguous()
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_imitative(params["bc_actor"], slope=0.01)
    e.staged_policy = True
    o = C.IsacCheck(params["policy"], params["q1"], params["q2"], params["bc_actor"])
    worst_o, worst_g = np.zeros(8), np.zeros(8)
    for k in range(g["out"].shape[0]):
        sync(o, e, SE)
        e.assemble(ring, torch.from_numpy(g["idx"][k].astype(np.int32)).cuda())
        e.assemble_expert(table, torch.from_numpy(g["idx_expert"][k].astype(np.int32)).cuda())
        e.learn(torch.from_numpy(g["eps"][k, 0]).cuda(), torch.from_numpy(g["eps"][k, 1]).cuda())
        got = np.asarray(e.losses_host() + e.imitative_losses_host())
        count = int(e.bc_count.item())
        rows, er = data["replay"][g["idx"][k]], data["expert_rows"][g["idx_expert"][k]]
        gq, gp = e.grad_critic.cpu().numpy(), e.grad_policy.cpu()

        def all_grads(oo):
            bad = []
            for h, name in ((0, "q1"), (1, "q2")):
                u = SE.unpack_mlp(torch.from_numpy(gq[h * SE.Q_SIZE:(h + 1) * SE.Q_SIZE]), SE.Q_BLOCK, 17, 1)
                for key in S.MLP_KEYS:
                    bad += grad_bad(u[key].numpy(), oo.last_grads[name][key].numpy(), f"call {k} {name} {key}")
            u = SE.unpack_mlp(gp, SE.POLICY_BLOCK, 13, 8)
            for key in S.MLP_KEYS:
                bad += grad_bad(u[key].numpy(), oo.last_grads["policy"][key].numpy(), f"call {k} policy {key}")
            return bad

        ref = np.asarray(oracle_checked(o, lambda oo: oo.learn((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), g["eps"][k, 0],
                                                               g["eps"][k, 1], (er[:, 0:13], er[:, 13:17])),
                                        [(None, None, all_grads)], f"isac call {k} gradients", module=S))
        gold = np.asarray(g["out"][k])
        rel = lambda x, y: np.abs(x - y) / np.maximum(np.abs(y), 1e-30)  # noqa: E731
        worst_o, worst_g = np.maximum(worst_o, rel(got, ref)), np.maximum(worst_g, rel(got, gold))
        print(f"isac call {k}: count {count} (golden {round(gold[7] * 128)}); relative difference per output vs restatement {rel(got, ref)}, vs golden {rel(got, gold)}")
        assert count == round(gold[7] * 128) == round(ref[7] * 128), (k, count, gold[7], ref[7])
        assert got[7] == count / 128
        np.testing.assert_allclose(got[:6], ref[:6], rtol=2e-5, atol=5e-6, err_msg=f"isac call {k} vs restatement")
        np.testing.assert_allclose(got[6:], ref[6:], rtol=2e-5, atol=0, err_msg=f"isac call {k} bc_loss / bc_weight vs restatement")
        others = [0, 1, 3, 4, 5]
        np.testing.assert_allclose(got[others], gold[others], rtol=5e-5, atol=2e-5, err_msg=f"isac call {k} vs reference golden")
        np.testing.assert_allclose(got[[2, 6]], gold[[2, 6]], rtol=5e-5, atol=0, err_msg=f"isac call {k} policy_loss / bc_loss vs reference golden")
        sd = e.state_dicts()
        for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
            d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-4 and d.max() <= 2.1e-3, f"call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
    print("isac observed maxima (relative) per output [q1, q2, policy, entropy_loss, H, alpha, bc_loss, bc_weight]: vs restatement", worst_o, "vs golden", worst_g)
    assert e.learning_steps == 8


def test_isac_one_call_is_bit_identical_to_staged(SE):
    """hx_sac_learn_imitative against hx_sac_critic_step + hx_sac_policy_grads_imitative + hx_sac_adam(1), against the same with the critic half as
    hx_sac_critic_grads + hx_sac_adam(0) (separate_critic_adam), and expert rows drawn inside the call
    (sample_expert(defer=True)) against the same rows injected by index: after 8 calls networks, moments, alpha state and W2 image equal bit
    for bit; so are losses[3..7].  losses[0..2] are sums of float atomics over workgroups in the launches every SAC call shares (logged only,
    order-dependent in the last bit even between two identical runs, as tests/test_sac_gpu.py notes): compared at rtol 1e-6."""
    params = sac_params()
    rep, exp = make_rings()
    a, b, c, d = (SE.SacEngine(batch=128) for _ in range(4))
    b.staged_policy = True
    d.separate_critic_adam = True
    for e in (a, b, c, d):
        e.load_params(params["policy"], params["q1"], params["q2"])
        e.set_imitative(bc_actor_params(), slope=0.01)
    weights = []
    for k in range(8):
        c.sample(rep, None, seed=11)
        c.sample_expert(exp, seed=11, defer=True)
        c.learn()
        for e in (a, b, d):
            e.sample(rep, None, seed=11)
            e.assemble_expert(exp.ring, c._expert_idx)
            e.learn()
        assert torch.equal(a.expert_rows, c.expert_rows) and torch.equal(a.rows, c.rows), k
        assert len(set(c._expert_idx.cpu().tolist())) == 128 and int(c._expert_idx.max()) < 400  # without replacement, inside the live rows
        weights.append(a.imitative_losses_host()[1])
        for other in (b, c, d):
            assert torch.equal(a.losses[3:8], other.losses[3:8]), (k, a.losses.tolist(), other.losses.tolist())
            np.testing.assert_allclose(a.losses[:3].cpu().numpy(), other.losses[:3].cpu().numpy(), rtol=1e-6)
            assert torch.equal(a.bc_count, other.bc_count)
    for other in (b, c, d):
        for name in STATE:
            assert torch.equal(getattr(a, name), getattr(other, name)), name
    assert any(0 < w < 1 for w in weights), weights  # the mixed case ran


def _gate_engine(SE, sign):
    """critics for which Q(s, a) = a[0] + 2 (one positive path from input column 13), a bc_actor whose output bias saturates a_bc[0] at sign"""
    params = sac_params()
    q = {k: np.zeros_like(v) for k, v in params["q1"].items()}
    q["0.weight"][0, 13], q["0.bias"][0], q["2.weight"][0, 0], q["4.weight"][0, 0] = 1.0, 2.0, 1.0, 1.0
    bc = bc_actor_params()
    bc["final.weight"][:] = 0
    bc["final.bias"][:] = 0
    bc["final.bias"][0] = 20.0 * sign
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], q, q)
    e.set_imitative(bc, slope=0.01)
    return e, params


def _policy_half(SE, e, rows, expert_rows, eps_next, eps_cur, imitative):
    """hx_sac_critic_grads (gradients only: the critics stay as loaded) + the staged policy half -> grad_policy"""
    from hirl4ucav_amd import _lib

    e.rows.copy_(rows.reshape(-1))
    e.expert_rows.copy_(expert_rows.reshape(-1))
    e.eps_next.copy_(eps_next.reshape(-1))
    e.eps_cur.copy_(eps_cur.reshape(-1))
    batch = SE.HxSacBatch(e.rows.data_ptr(), e.batch, e.eps_next.data_ptr(), e.eps_cur.data_ptr(), 0, 0)
    nets, hyper, st = ctypes.byref(e.nets), ctypes.byref(e.hyper), _lib.stream_ptr()
    _lib.call("hx_sac_critic_grads", nets, ctypes.byref(batch), hyper, 0, st)
    if imitative:
        _lib.call("hx_sac_policy_grads_imitative", nets, ctypes.byref(batch), hyper, ctypes.byref(e.imit), st)
    else:
        _lib.call("hx_sac_policy_grads", nets, ctypes.byref(batch), hyper, st)
    torch.cuda.synchronize()
    return e.grad_policy.clone()


def _gate_inputs():
    rng = np.random.default_rng(9)
    data = D.make_data(D.DATA_SEED)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()  # noqa: E731
    return (t(data["replay"][:128]), t(data["expert_rows"][:128]), t(rng.normal(0, 1, (128, 4))), t(rng.normal(0, 1, (128, 4))),
            t(rng.normal(0, 1, (128, 4))), data)


def test_isac_gate_limits(SE):
    """bc_weight == 1: the policy gradient is the pure BC gradient, slot 0 (the RL loss) contributing exactly 0 — it does not change by a bit
    when the sampled actions do; bc_weight == 0: bit-identical to hx_sac_policy_grads on the same inputs."""
    rows, er, e1, e2, e2b, data = _gate_inputs()
    e, params = _gate_engine(SE, +1.0)
    g1 = _policy_half(SE, e, rows, er, e1, e2, True)
    assert e.imitative_losses_host()[1] == 1.0 and int(e.bc_count.item()) == 128
    g1b = _policy_half(SE, e, rows, er, e1, e2b, True)  # other draws for a~: another RL gradient, scaled by exactly 0
    assert torch.equal(g1, g1b)
    p = S.to_t(params["policy"], True)
    se, ae = torch.from_numpy(data["expert_rows"][:128, 0:13]), torch.from_numpy(data["expert_rows"][:128, 13:17])
    bc_loss = torch.nn.functional.mse_loss(ae, torch.tanh(S.policy_forward(p, se)[0])) * 10000
    ref = dict(zip(S.MLP_KEYS, torch.autograd.grad(bc_loss, [p[k] for k in S.MLP_KEYS])))
    u = SE.unpack_mlp(g1.cpu(), SE.POLICY_BLOCK, 13, 8)
    bad = []
    for key in S.MLP_KEYS:
        bad += grad_bad(u[key].numpy(), ref[key].numpy(), f"pure BC gradient {key}")
    assert not bad, bad
    np.testing.assert_allclose(e.imitative_losses_host()[0], bc_loss.item(), rtol=2e-5)
    np.testing.assert_allclose(e.losses_host()[2], bc_loss.item(), rtol=2e-5)  # the combined loss at w = 1
    e, _ = _gate_engine(SE, -1.0)
    g0 = _policy_half(SE, e, rows, er, e1, e2, True)
    assert e.imitative_losses_host()[1] == 0.0 and int(e.bc_count.item()) == 0
    plain = _policy_half(SE, e, rows, er, e1, e2, False)
    assert torch.equal(g0, plain)
    assert float(g0.abs().max()) > 0


def test_isac_log_std_rows_get_no_bc_gradient(SE):
    """bc_weight == 1: the BC loss sees only the mean half of the policy head — 4.weight[4:8] and 4.bias[4:8] get exactly zero"""
    rows, er, e1, e2, _, _ = _gate_inputs()
    e, _ = _gate_engine(SE, +1.0)
    u = SE.unpack_mlp(_policy_half(SE, e, rows, er, e1, e2, True), SE.POLICY_BLOCK, 13, 8)
    assert e.imitative_losses_host()[1] == 1.0
    assert torch.all(u["4.weight"][4:8] == 0) and torch.all(u["4.bias"][4:8] == 0)
    assert float(u["4.weight"][0:4].abs().max()) > 0 and float(u["4.bias"][0:4].abs().max()) > 0


def test_plain_sac_is_untouched(SE):
    """an engine that never called set_imitative, and one whose imitative state was set up but which is driven through hx_sac_learn:
    bit-identical state after 8 calls on the same inputs"""
    params = sac_params()
    rep, _ = make_rings()
    a, b = (SE.SacEngine(batch=128) for _ in range(2))
    for e in (a, b):
        e.load_params(params["policy"], params["q1"], params["q2"])
    b.set_imitative(bc_actor_params(), slope=0.01)
    b.imitative = False  # learn() -> hx_sac_learn
    for k in range(8):
        for e in (a, b):
            e.sample(rep, None, seed=11, defer=bool(k & 1))
            e.learn()
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.losses[3:6], b.losses[3:6]) and torch.all(a.losses[6:8] == 0) and torch.all(b.losses[6:8] == 0)


def test_isac_refusals(SE):
    from hirl4ucav_amd import _lib

    params = sac_params()
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_imitative(bc_actor_params())
    with pytest.raises(ValueError, match="fp32 only"):
        e.set_act_dtype("bf16")
    with pytest.raises(ValueError, match="fp32 only"):
        e.set_update_dtype("bf16")
    f = SE.SacEngine(batch=128)
    f.load_params(params["policy"], params["q1"], params["q2"])
    f.set_act_dtype("bf16")
    with pytest.raises(ValueError, match="fp32 only"):
        f.set_imitative(bc_actor_params())
    f.set_update_dtype("bf16")
    batch = SE.HxSacBatch(f.rows.data_ptr(), 128, None, None, 0, 1)
    for name, args in (("hx_sac_policy_grads_imitative", (ctypes.byref(e.imit), _lib.stream_ptr())),
                       ("hx_sac_learn_imitative", (None, ctypes.byref(e.imit), None, 0, 1, -4.0, _lib.stream_ptr()))):
        with pytest.raises(_lib.HxError, match=name + ".*fp32 only"):
            _lib.call(name, ctypes.byref(f.nets), ctypes.byref(batch), ctypes.byref(f.hyper), *args)
    g = SE.SacEngine(batch=128)
    with pytest.raises(_lib.HxError, match="set_imitative"):
        g.sample_expert(make_rings()[1])
    e.world = 2
    with pytest.raises(_lib.HxError, match="one GPU"):
        e.learn()


def test_isac_facade_learns_and_logs(SE, tmp_path):
    """SacAgent(imitative=True) + load_bc_actor + expert_memory: learn() runs the imitative branch and writes loss/bc, loss/bc_weight"""
    from hirl4ucav_amd.agents.SAC.agent import DeviceMemory, SacAgent

    box = lambda n: types.SimpleNamespace(shape=(n,), sample=lambda: np.zeros(n, np.float32))  # noqa: E731
    ag = SacAgent(box(13), box(4), str(tmp_path / "log"), batch_size=128, lr=1e-3, hidden_units=[256, 512], memory_size=4096, imitative=True,
                  log_interval=2, start_steps=0)
    logged = []
    ag.writer = types.SimpleNamespace(add_scalar=lambda tag, v, step: logged.append((tag, float(v), step)))
    rng = np.random.default_rng(2)
    for mem, n in ((ag.memory, 300), (DeviceMemory(1024), 200)):
        for _ in range(n):
            mem.append(rng.uniform(-1, 1, 13), rng.uniform(-1, 1, 4), float(rng.uniform(-5, 0)), rng.uniform(-1, 1, 13), False)
        last = mem
    with pytest.raises(RuntimeError, match="load_bc_actor"):
        ag.learn(False)
    path = tmp_path / "bc" / "Agent1_Harfang_GYM"
    os.makedirs(path.parent)
    torch.save({k: torch.from_numpy(v) for k, v in bc_actor_params().items()}, path)
    with pytest.raises(FileNotFoundError):
        ag.load_bc_actor(str(tmp_path / "nothing"))
    ag.load_bc_actor("Agent1_", str(path.parent))  # the reference's two-argument call
    with pytest.raises(RuntimeError, match="expert_memory"):
        ag.learn(False)
    ag.expert_memory = last
    before = ag.eng.policy.clone()
    for _ in range(4):
        ag.learn(False)
    tags = [t for t, _, _ in logged]
    assert tags.count("loss/bc") == 2 and tags.count("loss/bc_weight") == 2 and tags.count("loss/policy") == 2
    w = [v for t, v, _ in logged if t == "loss/bc_weight"]
    assert all(0.0 <= x <= 1.0 for x in w) and all(np.isfinite(v) for _, v, _ in logged)
    assert not torch.equal(before, ag.eng.policy)


def _bc_file(tmp_path):
    f = tmp_path / "bc_actor.pth"
    torch.save({k: torch.from_numpy(v) for k, v in bc_actor_params().items()}, f)
    return str(f)


def test_train_all_isac_runs_at_16384_envs(SE, tmp_path, monkeypatch, capsys):
    """--agent SAC --type ISAC at configs[2]'s size for a handful of vector steps (SacEngine.step_learn's imitative order), the two scalars
    through the driver's writer; a missing --bc_actor file is a FileNotFoundError"""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.scalars import JsonlWriter

    monkeypatch.setattr(T, "make_writer", JsonlWriter)
    monkeypatch.setitem(T.MAX_STEP, "serpentine", 6)
    common = ["--agent", "SAC", "--type", "ISAC", "--env", "serpentine", "--random", "--seed", "3", "--num_envs", "16384", "--synthetic_expert",
              "--checkpoint_rate", "1000", "--snapshot_every", "0", "--episodes", "2"]
    with pytest.raises(FileNotFoundError):
        T.main(T.parse_args(common + ["--bc_actor", str(tmp_path / "missing.pth"), "--result_dir", str(tmp_path / "x")]))
    run = T.main(T.parse_args(common + ["--bc_actor", _bc_file(tmp_path), "--result_dir", str(tmp_path / "a")]))
    assert "Episode 2:" in capsys.readouterr().out
    sc =[json.loads(ln) for ln in open(os.path.join(run, "summary", "scalars.jsonl"))]
    for tag in ("loss/bc", "loss/bc_weight"):
        v = [s["value"] for s in sc if s["tag"] == tag]
        assert len(v) == 2 and all(np.isfinite(v)), (tag, v)
    assert all(0.0 <= s["value"] <= 1.0 for s in sc if s["tag"] == "loss/bc_weight")


def test_train_all_isac_resumed_run_continues_bit_identically(SE, tmp_path, monkeypatch):
    """tests/test_facade_gpu.py::test_resumed_run_continues_bit_identically for --type ISAC: 3 episodes straight == 2 episodes, stop, --resume,
    1 more.  At that test's size (256 envs, --separate_launches: one env workgroup, so the replay insert order — and with it the run — is
    reproducible; 16,384 envs insert in workgroup-schedule order and no two runs are equal).  The snapshot carries the frozen bc_actor and
    the expert-draw counter."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.agents.sac_engine import SacEngine

    monkeypatch.setitem(T.MAX_STEP, "serpentine", 48)
    common = ["--agent", "SAC", "--type", "ISAC", "--env", "serpentine", "--random", "--seed", "3", "--num_envs", "256", "--buffer_size", "32768",
              "--checkpoint_rate", "2", "--synthetic_expert", "--separate_launches", "--bc_actor", _bc_file(tmp_path)]
    a = T.main(T.parse_args(common + ["--episodes", "3", "--snapshot_every", "3", "--result_dir", str(tmp_path / "a")]))
    b1 = T.main(T.parse_args(common + ["--episodes", "2", "--snapshot_every", "2", "--result_dir", str(tmp_path / "b")]))
    b2 = T.main(T.parse_args(common + ["--episodes", "3", "--snapshot_every", "3", "--result_dir", str(tmp_path / "c"), "--resume", b1]))
    sa = torch.load(os.path.join(a, "state_rank0.pt"), weights_only=False)
    sb = torch.load(os.path.join(b2, "state_rank0.pt"), weights_only=False)
    assert sa["driver"] == sb["driver"] and sa["driver"]["episode"] == 3
    assert sa["engine"]["counters"] == sb["engine"]["counters"]
    assert sa["engine"]["imitative"]["expert_calls"] == sb["engine"]["imitative"]["expert_calls"] == sa["engine"]["counters"]["learning_steps"] > 0
    assert torch.equal(sa["engine"]["imitative"]["bc_actor"], sb["engine"]["imitative"]["bc_actor"])
    eng = SacEngine()
    lo = (eng.losses.data_ptr() - eng.arena.data_ptr()) // 4
    la, lb = sa["engine"]["arena"][lo:lo + 8].clone(), sb["engine"]["arena"][lo:lo + 8].clone()
    np.testing.assert_allclose(la.numpy(), lb.numpy(), rtol=1e-4, atol=1e-6)  # (the logged sums of float atomics: closely; all else exactly)
    sa["engine"]["arena"][lo:lo + 8] = 0
    sb["engine"]["arena"][lo:lo + 8] = 0
    for part, keys in (("engine", ["arena"]), ("env", ["state", "obs", "episode_ctr", "stats"]), ("replay", ["ring", "success"])):
        for k in keys:
            assert torch.equal(sa[part][k].view(torch.uint8), sb[part][k].view(torch.uint8)), (part, k)
    assert sa["replay"]["total"] == sb["replay"]["total"] > 0
    # a plain SAC engine refuses the imitative snapshot (and the other way round): the branch is part of the run's state
    from hirl4ucav_amd.utils import checkpoint as CK

    with pytest.raises(ValueError, match="ISAC"):
        CK.load_engine_state(eng, sa["engine"])
