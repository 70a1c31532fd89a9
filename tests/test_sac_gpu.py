"""GPU parity tests of the SAC path (hx_sac_* through the C ABI) against the SAC oracle (pinned to the reference's loss math)
and the golden vectors recorded from the reference's SacAgent.learn.  Tolerances as for HIRL (tests/test_hirl_gpu.py)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sac_oracle as S  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


def sync(o, e, SE):
    sd = e.state_dicts()
    for name, dst in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
        for k in dst:
            dst[k].data.copy_(sd[name][k].cpu())
    for opt, m, v, blk, dims in ((o.opt_pi, e.m_policy, e.v_policy, SE.POLICY_BLOCK, (13, 8)), (o.opt_q1, e.m_critic[:SE.Q_SIZE], e.v_critic[:SE.Q_SIZE], SE.Q_BLOCK, (17, 1)),
                                 (o.opt_q2, e.m_critic[SE.Q_SIZE:], e.v_critic[SE.Q_SIZE:], SE.Q_BLOCK, (17, 1))):
        mm, vv = SE.unpack_mlp(m, blk, *dims), SE.unpack_mlp(v, blk, *dims)
        for k in opt.m:
            opt.m[k].copy_(mm[k].cpu())
            opt.v[k].copy_(vv[k].cpu())
        opt.t = e.learning_steps
    a = e.alpha_state.tolist()
    o.log_alpha.data.fill_(a[0])
    o.opt_alpha.m["a"].fill_(a[1]); o.opt_alpha.v["a"].fill_(a[2]); o.opt_alpha.t = e.learning_steps  # noqa: E702
    o.alpha = torch.tensor([a[3]], dtype=o.log_alpha.dtype)  # (an fp64 oracle, tests/test_sac_edges_gpu.py, keeps its dtype)
    o.learning_steps = e.learning_steps


def grad_bad(got, ref, what):
    """-> [] or [(what, n_bad, worst)]: EVERY entry must satisfy |dg| <= 1e-4 |g| + 2e-5 max|g| (no blanket allowance; entries that miss
    must be explained by a ReLU kink: tests/test_hirl_gpu.py::oracle_checked)"""
    g, x = ref.ravel(), got.ravel()
    tol = 1e-4 * np.abs(g) + 2e-5 * max(np.abs(g).max(), 1e-30)
    bad = np.abs(x - g) > tol
    return [(what, int(bad.sum()), float(np.abs(x - g).max()))] if bad.any() else []


def test_sac_act_matches_oracle(SE):
    params = sac_params()
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], params["q1"], params["q2"])
    o = S.SacOracle(params["policy"], params["q1"], params["q2"])
    rng = np.random.default_rng(0)
    for n in (1, 7, 300):
        obs = rng.uniform(-1, 1, (n, 13)).astype(np.float32)
        eps = rng.normal(0, 1, (n, 4)).astype(np.float32)
        np.testing.assert_allclose(e.act(torch.from_numpy(obs).cuda(), explore=False).cpu().numpy(), o.exploit(obs), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(e.act(torch.from_numpy(obs).cuda(), eps=torch.from_numpy(eps).cuda()).cpu().numpy(), o.explore(obs, eps), rtol=1e-5, atol=2e-6)
    a = e.act(torch.zeros((5000, 13), device="cuda")).cpu().numpy()  # Philox sampling
    assert np.all(np.abs(a) <= 1) and a.std() > 0.05
    # from 8,192 rows on the kernel runs 32 rows per workgroup: same arithmetic per row, so bit-identical to the 16-row tiling
    n = 8192 + 21
    obs = torch.from_numpy(rng.uniform(-1, 1, (n, 13)).astype(np.float32)).cuda()
    eps = torch.from_numpy(rng.normal(0, 1, (n, 4)).astype(np.float32)).cuda()
    for kw in ({"explore": False}, {"eps": eps}):
        big = e.act(obs, **kw)
        parts = [e.act(obs[i:i + 4096], **({"eps": eps[i:i + 4096]} if "eps" in kw else kw)) for i in range(0, n, 4096)]
        assert torch.equal(big, torch.cat(parts))
    np.testing.assert_allclose(e.act(obs, eps=eps)[-300:].cpu().numpy(), o.explore(obs[-300:].cpu().numpy(), eps[-300:].cpu().numpy()), rtol=1e-5, atol=2e-6)


def test_sac_learn_matches_oracle_and_reference(SE, golden_dir):
    g = np.load(os.path.join(golden_dir, "sac_learn.npz"))
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"])
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], params["q1"], params["q2"])
    o = S.SacOracle(params["policy"], params["q1"], params["q2"])
    for k in range(g["out"].shape[0]):
        sync(o, e, SE)
        e.assemble(ring, torch.from_numpy(g["idx"][k].astype(np.int32)).cuda())
        e.learn(torch.from_numpy(g["eps"][k, 0]).cuda(), torch.from_numpy(g["eps"][k, 1]).cuda())
        got = e.losses_host()
        rows = data["replay"][g["idx"][k]]
        gq = e.grad_critic.cpu().numpy()
        gp = e.grad_policy.cpu()

        def all_grads(oo):  # every gradient tensor of the three networks against the oracle evaluation `oo`
            bad = []
            for h, name in ((0, "q1"), (1, "q2")):
                u = SE.unpack_mlp(torch.from_numpy(gq[h * SE.Q_SIZE:(h + 1) * SE.Q_SIZE]), SE.Q_BLOCK, 17, 1)
                for key in S.MLP_KEYS:
                    bad += grad_bad(u[key].numpy(), oo.last_grads[name][key].numpy(), f"call {k} {name} {key}")
            u = SE.unpack_mlp(gp, SE.POLICY_BLOCK, 13, 8)
            for key in S.MLP_KEYS:
                bad += grad_bad(u[key].numpy(), oo.last_grads["policy"][key].numpy(), f"call {k} policy {key}")
            return bad

        from tests.test_hirl_gpu import oracle_checked
        ref = oracle_checked(o, lambda oo: oo.learn((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), g["eps"][k, 0], g["eps"][k, 1]),
                             [(None, None, all_grads)], f"sac call {k} gradients", module=S)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=f"sac call {k} vs oracle")
        # free-running vs the reference's recorded run: policy_loss = mean(-min Q) - alpha mean(H) is a difference of O(1)
        # terms that crosses zero around call 5, so it is compared with an absolute tolerance at the terms' scale
        # (entry 2 only; the other five outputs keep rtol 5e-5 with an absolute floor of 2e-5)
        others = [0, 1, 3, 4, 5]
        np.testing.assert_allclose(np.asarray(got)[others], np.asarray(g["out"][k])[others], rtol=5e-5, atol=2e-5, err_msg=f"sac call {k} vs reference golden")
        np.testing.assert_allclose(got[2], g["out"][k][2], rtol=5e-5, atol=1e-4, err_msg=f"sac call {k} policy_loss vs reference golden")
        sd = e.state_dicts()
        for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
            d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-4 and d.max() <= 2.1e-3, f"call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
        # LayerNorm slots of the shared layout stay (1, 0)
        off, n = SE.POLICY_BLOCK["g2"]
        assert torch.all(e.policy[off:off + n] == 1) and torch.all(e.policy[SE.POLICY_BLOCK["be2"][0]:SE.POLICY_BLOCK["be2"][0] + n] == 0)
    assert e.learning_steps == 8


# (the ids of the batch-128 cases are the ones these tests had before they took a batch size)
@pytest.mark.parametrize("esac,batch", [pytest.param(False, 128, id="False"), pytest.param(True, 128, id="True"), pytest.param(False, 48, id="False-batch48"),
                                        pytest.param(True, 48, id="True-batch48"), pytest.param(False, 272, id="False-batch272"), pytest.param(True, 272, id="True-batch272")])
def test_sac_deferred_draw_is_bit_identical_to_the_sampling_launch(SE, esac, batch):
    """sample(defer=True) + learn() (hx_sac_critic_grads_sampled: memory.sample inside the first forward launch; beyond 256 rows a sampling launch
    that the call issues itself) against sample() + learn(): the same indices, row tile and — after 8 calls — the same networks, moments and alpha,
    bit for bit (SAC and E-SAC's expert mix; batch 48: an odd number of 16-row tiles, 272: beyond the in-launch draw).  The ring holds a few more rows
    than the minibatch at the start (150 for the batches up to 128), so that the draw without replacement has a population to draw from."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = sac_params()
    rng = np.random.default_rng(3)
    rep = DeviceReplay(5000)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(5000, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += max(150, batch + 22)
    exp = DeviceReplay(64)
    exp.store_rows(torch.from_numpy(rng.normal(size=(50, 32)).astype(np.float32)))
    a, b = (SE.SacEngine(batch=batch) for _ in range(2))
    for e in (a, b):
        e.load_params(params["policy"], params["q1"], params["q2"])
    for k in range(8):
        if k == 4:
            rep.total += 100000
        outs = []
        for e, defer in ((a, False), (b, True)):
            e.sample(rep, exp if esac else None, n_main=batch - 28, seed=7, defer=defer)
            e.learn()
            outs.append((e._idx.clone(), e.rows.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), k
    for name in ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("defer,batch", [pytest.param(False, 128, id="False"), pytest.param(True, 128, id="True"), pytest.param(False, 48, id="False-batch48"),
                                         pytest.param(True, 48, id="True-batch48"), pytest.param(False, 272, id="False-batch272"), pytest.param(True, 272, id="True-batch272")])
def test_sac_learn_in_one_call_is_bit_identical_to_the_staged_sequence(SE, defer, batch):
    """hx_sac_learn (one GPU, 9 launches: the soft_update and policy.sample(s) in the launch of policy.sample(s'), the min(Q1, Q2) selection and the
    policy head gradient in the backward prologues, q1 / q2 / policy optimizer
    steps and the log-alpha step inside their weight-gradient launches) against BOTH staged sequences — hx_sac_critic_step +
    hx_sac_policy_grads + hx_sac_adam(1) and the fully separate hx_sac_critic_grads[_sampled] + hx_sac_adam(0) + ... (14 launches): after 7
    calls (two of them with the Polyak step of the targets first) the same networks, moments, targets, alpha and W2 image, bit for bit."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = sac_params()
    rng = np.random.default_rng(5)
    rep = DeviceReplay(4096)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(4096, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += 4096
    a, b, c = (SE.SacEngine(batch=batch) for _ in range(3))
    b.staged_policy = True          # hx_sac_critic_step + hx_sac_policy_grads + hx_sac_adam(1)
    c.separate_critic_adam = True   # every stage a call of its own
    for e in (a, b, c):
        e.load_params(params["policy"], params["q1"], params["q2"])
    for k in range(7):
        for e in (a, b, c):
            e.sample(rep, None, seed=11, defer=defer)
            e.learn()
    for other in (b, c):
        for name in ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i"):
            assert torch.equal(getattr(a, name), getattr(other, name)), name
        np.testing.assert_allclose(a.losses.cpu().numpy(), other.losses.cpu().numpy(), rtol=1e-6)  # (atomic accumulation order)


@pytest.mark.parametrize("defer", [False, True])
def test_sac_critic_step_in_the_wgrad_launch_is_bit_identical(SE, defer):
    """hx_sac_critic_step (one GPU: q1_optim / q2_optim step inside the weight-gradient launch) against hx_sac_critic_grads[_sampled] +
    hx_sac_adam(0): after 6 calls (two of them with the Polyak step of the targets first) the same networks, moments, targets and alpha."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = sac_params()
    rng = np.random.default_rng(5)
    rep = DeviceReplay(4096)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(4096, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += 4096
    a, b = (SE.SacEngine(batch=128) for _ in range(2))
    a.staged_policy = True
    b.separate_critic_adam = True
    for e in (a, b):
        e.load_params(params["policy"], params["q1"], params["q2"])
    for k in range(6):
        for e in (a, b):
            e.sample(rep, None, seed=11, defer=defer)
            e.learn()
    for name in ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    np.testing.assert_allclose(a.losses.cpu().numpy(), b.losses.cpu().numpy(), rtol=1e-6)  # (atomic accumulation order)


@pytest.mark.parametrize("n", [7, 4096, 16384])
def test_sac_image_path_is_bit_identical_and_follows_adam(SE, n):
    """hx_sac_act with w2_f32i (the policy's W2 from its re-ordered fp32 image, what SacEngine.act uses) equals hx_sac_act without an image (row-major W2 streamed
    through LDS) BIT FOR BIT — exploit and Philox-sampled explore, 16- and 32-row workgroups — before and after policy Adam steps, and
    the image is the permuted W2."""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = sac_params()
    e = SE.SacEngine(batch=128)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.x9_rows = None  # the fp32 image at every size (from 16,384 rows on the engine's default is the exact 9-term split: tests/test_actp_gpu.py)
    rng = np.random.default_rng(n)
    obs = torch.from_numpy(rng.uniform(-1, 1, (n, 13)).astype(np.float32)).cuda()
    rep = DeviceReplay(4096)
    rep.store_rows(torch.from_numpy(rng.normal(size=(2000, 32)).astype(np.float32)))

    def image_of(policy_flat):
        w2 = SE.unpack_mlp(policy_flat, SE.POLICY_BLOCK, 13, 8)
        w2 = w2[[k for k in w2 if w2[k].shape == (512, 256)][0]]
        return w2.reshape(32, 16, 16, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1).to(e.w2_f32i.device)

    def plain(mode, call):
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        _lib.call("hx_sac_act", e.policy.data_ptr(), None, None, None, obs.data_ptr(), n, out.data_ptr(), mode, None, 3, 0, call, _lib.stream_ptr())
        return out

    for round_ in range(2):
        assert torch.equal(e.w2_f32i, image_of(e.policy))
        assert torch.equal(e.act(obs, explore=False), plain(0, e.act_calls))
        assert torch.equal(e.act(obs, explore=True, seed=3), plain(2, e.act_calls))
        for _ in range(3):
            e.sample(rep, seed=1)
            e.learn()


@pytest.mark.parametrize("n", [4096 + 17, 8192, 16384])  # 16-row / 32-row workgroups with the env tail; 16,384: the persistent kernel (hx_actp.hip)
def test_sac_act_step_in_one_launch_equals_act_then_step(SE, n):
    """hx_sac_act_step = hx_sac_act followed by hx_env_step (explore with given draws, with Philox, and exploit).  16,384 serpentine
    envs is BASELINE.json configs[2] at its own size: beyond 8,192 envs the entry point issues the two launches itself, and the
    dynamics of the last step are checked against the oracle on a 2,000-env sample from the actions the policy produced."""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = sac_params()
    engs, envs, reps = [], [], []
    for _ in range(2):
        e = SE.SacEngine(batch=128)
        e.load_params(params["policy"], params["q1"], params["q2"])
        rep = DeviceReplay(1 << 19)
        env = BatchedHarfangEnv(n, scenario="serpentine", seed=1, max_step=7, auto_reset=True, random_reset=True, replay=rep)
        env.reset()
        engs.append(e); envs.append(env); reps.append(rep)
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.zeros((n, 4), device="cuda")
    for k in range(12):
        kw = [{"explore": False}, {"eps": torch.randn((n, 4), device="cuda", generator=g)}, {"seed": 4}][k % 3]
        prev = (envs[0].state.clone(), envs[0].obs.clone(), envs[0].episode_ctr.clone()) if (k == 11 and n == 16384) else None
        engs[0].act(envs[0].obs, out=acts, **kw)
        envs[0].step(acts)
        a2 = engs[1].act_step(envs[1], **kw)[0]
        assert torch.equal(acts, a2), f"actions, step {k}"
        for name in ("state", "obs", "reward", "done", "success", "episode_ctr"):
            assert torch.equal(getattr(envs[0], name).view(torch.uint8), getattr(envs[1], name).view(torch.uint8)), f"{name}, step {k}"
        assert torch.equal(envs[0].stats.sum(0), envs[1].stats.sum(0)), f"stats, step {k}"  # (kept per way = workgroup % 32: the two launch shapes spread them differently)
    tot = int(reps[0].total.item())
    assert tot == int(reps[1].total.item()) and 0 < tot <= reps[0].capacity
    if n == 16384:
        from tests import _oracle as ox

        sample = np.linspace(0, n - 1, 2000).astype(np.int64)
        st = np.ascontiguousarray(prev[0].cpu().numpy().T[sample])
        o_obs = np.ascontiguousarray(prev[1].cpu().numpy()[sample])
        epi = np.ascontiguousarray(prev[2].cpu().numpy()[sample].astype(np.uint32))
        a = acts.cpu().numpy()[sample]
        for j, i in enumerate(sample):  # per-env ids key the Philox reset offsets: step each sampled env with its own id
            ro, do, so = ox.step_batch(st[j:j + 1], a[j:j + 1], o_obs[j:j + 1], max_step=7, auto_reset=1, randomize=1, seed=1, env_id0=int(i), episode_ctr=epi[j:j + 1])
            assert (int(do[0]), int(so[0])) == (int(envs[0].done[i]), int(envs[0].success[i])), i
            assert ro.view(np.uint32)[0] == envs[0].reward[i:i + 1].cpu().numpy().view(np.uint32)[0], i
        np.testing.assert_array_equal(envs[0].state.cpu().numpy().T[sample].view(np.uint32), st.view(np.uint32))
        np.testing.assert_array_equal(envs[0].obs.cpu().numpy()[sample].view(np.uint32), o_obs.view(np.uint32))
    rows = [r.ring[:tot].cpu().numpy() for r in reps]
    rows = [x[np.lexsort(x.T[::-1])] for x in rows]
    np.testing.assert_array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))
