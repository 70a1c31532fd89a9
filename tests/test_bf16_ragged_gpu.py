"""The bf16 update away from B = 128: HIRL (soft weight with warm-up, expert rows mixed in), TD3, BC pre-training, the staged path and SAC at the
batch sizes where hx_wgrad.hip's bf16 weight-gradient product leaves its full 64-row chunks (tests/_bf16_ragged.BATCHES: 16, 48, 144, 272 — the last
also crosses the 256-row staging chunk of the layer-1 and head jobs).

Reference, bars and method are those of tests/test_bf16_update_gpu.py (and, for SAC, tests/test_sac_bf16_gpu.py), unchanged: the rounded-operand
oracle (HirlOracle inside Bf16Layer2, the kernel's subgradient within KINK of a kink), call by call from identical states; losses rtol 1e-4 /
atol 2e-5; gradients TIGHT for >= 99.8 % of a tensor's entries and LOOSE for all; check_params; every bf16 image bit for bit after every call.
tests/test_bf16_ragged_cpu.py shows on the same inputs that fp32 accumulation in the kernels' grouping passes these bars, and that they reject a
weight gradient whose last 8 batch rows are missing or doubled.  Inputs: tests/_bf16_ragged.py, tests/_sac_edges.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as H  # noqa: E402
from oracle import sac_oracle as S  # noqa: E402
from tests import _bf16_ragged as R  # noqa: E402
from tests import _sac_edges as X  # noqa: E402
from tests import test_bf16_update_gpu as U  # noqa: E402
from tests.test_hirl_gpu import device_tables, sync_oracle  # noqa: E402


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


class Worst:
    """the figures a case prints: losses' largest relative difference, largest TIGHT-miss share and multiple of LOOSE over the tensors, kink units"""

    def __init__(self):
        self.loss = self.tight = self.loose = 0.0
        self.kinks = 0

    def losses(self, got, ref):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        self.loss = max(self.loss, float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30))[np.abs(got - ref) > 0].max(initial=0.0)))

    def grads(self, stats):
        self.tight = max([self.tight] + [s[1] for s in stats])
        self.loose = max([self.loose] + [s[2] for s in stats])

    def __str__(self):
        return (f"losses differ by at most {self.loss:.2e} relative, largest TIGHT-miss share {self.tight:.5f}, largest multiple of LOOSE "
                f"{self.loose:.3f}, {self.kinks} units took the kernel's subgradient")


def new_engine(E_, case, B, staged=False):
    p = R.params()
    if case == "td3":
        e = E_.HirlEngine(batch=B, slope=0.01, use_bc=False)
        e.load_params(p["actor"], p["critic"])
    else:
        e = E_.HirlEngine(batch=B, slope=0.01) if case == "bc" else E_.HirlEngine(batch=B)
        e.load_params(p["actor"], p["critic"], p["bc_actor"])
    e.staged = staged
    e.set_update_dtype("bf16")
    U.assert_images_current(e, E_, "after set_update_dtype")
    return e


def run_learn_case(E_, case, B, staged=False, check=True):
    """N_CALLS[case] learn() calls at batch B; check=False only runs the engine (the staged comparison).  -> engine, losses per call, Worst"""
    ring, exp, bc = device_tables(R.data())
    e, o, worst, all_losses = new_engine(E_, case, B, staged), R.new_oracle(case), Worst(), []
    use_bc, nm = case != "td3", R.n_main(case, B)
    for k, (idx, ibc, noise) in enumerate(R.calls(case, B)):
        batch = R.batch_of(case, B, idx)
        assert batch[4][0] == 1 and batch[4][1] == 0  # a done row and a live row in every minibatch
        was_actor = e.actor_trainable
        sync_oracle(o, e, E_)
        pre = (e.actor.clone(), e.critic.clone())
        if use_bc:
            e.assemble(ring, torch.from_numpy(idx).cuda(), expert_ring=exp, n_main=nm, bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
            e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=R.SOFT, bc_warm_up_weight=R.WARM)
        else:
            e.assemble(ring, torch.from_numpy(idx).cuda())
            e.learn(noise=torch.from_numpy(noise).cuda())
        got = e.losses_host()
        all_losses.append(got)
        what = f"bf16 {case} B={B} call {k}"
        if check:
            with H.Bf16Layer2(), U.KernelKinks(U.learn_masks(e, E_, pre, was_actor, soft=use_bc, use_bc=use_bc, B=B)) as kk:
                ref = o.learn(batch, R.bc_batch_of(ibc) if use_bc else None, noise, *((R.SOFT, R.WARM) if use_bc else ()))
            worst.kinks += kk.taken
            n = 6 if use_bc else 2
            worst.losses(got[:n], ref[:n])
            sc = U.grad_stats(e.grad_critic, o.last_grads["critic"], E_.CRITIC_LAYOUT)
            sa = U.grad_stats(e.grad_actor, o.last_grads["actor"], E_.ACTOR_LAYOUT) if was_actor else []
            worst.grads(sc + sa)
            print(f"\n[bf16 ragged] {what}: losses {np.asarray(got[:n])} oracle {np.asarray(ref[:n])}; so far {worst}")
            np.testing.assert_allclose(got[:n], ref[:n], rtol=U.LOSS_RTOL, atol=U.LOSS_ATOL, err_msg=what + " losses vs the rounded-operand oracle")
            U.check_grads(e.grad_critic, o.last_grads["critic"], E_.CRITIC_LAYOUT, what + " critic gradient")
            if was_actor:
                U.check_grads(e.grad_actor, o.last_grads["actor"], E_.ACTOR_LAYOUT, what + " actor gradient")
            U.check_params(e, o, E_, what + " parameters", was_actor)
        U.assert_images_current(e, E_, what)
    assert e.critic_step == 4 and e.actor_step == 2
    return e, all_losses, worst


@pytest.mark.parametrize("B", R.BATCHES)
def test_bf16_hirl_soft_with_warm_up_at_ragged_batches(E, B):
    """bc_weight_now = 100, warm-up 0.1, four calls (two actor calls: the two-slot actor job with the BC weight on the per-slot fp32 sums, the
    critic's two heads, the soft-estimate slots)"""
    print(f"\n[bf16 ragged] soft B={B}: {run_learn_case(E, 'soft', B)[2]}")


@pytest.mark.parametrize("B", [48, 144])
def test_bf16_hirl_with_expert_rows_at_ragged_batches(E, B):
    """the last 16 of 48 / 64 of 144 minibatch rows come from the expert ring"""
    assert R.n_main("expert", B) == {48: 32, 144: 80}[B]
    print(f"\n[bf16 ragged] expert B={B}: {run_learn_case(E, 'expert', B)[2]}")


@pytest.mark.parametrize("B", [48, 272])
def test_bf16_td3_at_ragged_batches(E, B):
    """the LeakyReLU (slope 0.01), no-BC instantiations"""
    print(f"\n[bf16 ragged] td3 B={B}: {run_learn_case(E, 'td3', B)[2]}")


@pytest.mark.parametrize("B", [16, 144])
def test_bf16_bc_train_actor_at_ragged_batches(E, B):
    """hx_bc_train_actor (BC.py:160-185), three steps"""
    ring, exp, bc = device_tables(R.data())
    e, o, worst = new_engine(E, "bc", B), R.new_oracle("bc"), Worst()
    for k, (idx, ibc, noise) in enumerate(R.calls("bc", B)):
        sync_oracle(o, e, E)
        o.opt_actor.t = e.actor_step
        pre_actor = E.unpack(e.actor.clone(), E.ACTOR_LAYOUT)
        e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
        e.bc_train_actor()
        got = e.losses_host()[2]
        m0, m1 = U.kernel_masks(e, "ABC", pre_actor["layernorm2.weight"].cpu(), pre_actor["layernorm2.bias"].cpu(), B)
        with H.Bf16Layer2(), U.KernelKinks({0: m0, 1: m1}) as kk:
            loss = H.bc_train_actor(o, R.bc_batch_of(ibc))
        worst.kinks += kk.taken
        worst.losses([got], [loss])
        worst.grads(U.grad_stats(e.grad_actor, o.last_grads["actor"], E.ACTOR_LAYOUT))
        print(f"\n[bf16 ragged] bc B={B} step {k}: loss {got} oracle {loss}; so far {worst}")
        np.testing.assert_allclose(got, loss, rtol=U.LOSS_RTOL, err_msg=f"bc B={B} step {k}")
        U.check_grads(e.grad_actor, o.last_grads["actor"], E.ACTOR_LAYOUT, f"bc B={B} step {k}")
        # the stepped actor: check_params' rule for one network (the critic and the targets do not move)
        f = e.actor.cpu().numpy()
        for key, off, shp in E.ACTOR_LAYOUT:
            r, g = o.actor[key].detach().numpy().ravel(), np.abs(o.last_grads["actor"][key].numpy().ravel())
            tol = U.LOOSE[0] * g + U.LOOSE[1] * max(g.max(), 1e-30)
            bound = 2e-6 + 2.1e-3 * np.minimum(1.0, 8.0 * tol / np.maximum(g, 1e-30))
            d = np.abs(f[off:off + r.size] - r)
            assert not (d > bound).any(), f"bc B={B} step {k} {key}: {int((d > bound).sum())} entries beyond their bound, worst {d.max():.2e}"
        U.assert_images_current(e, E, f"bc B={B} step {k}")
    print(f"\n[bf16 ragged] bc B={B}: {worst}")


@pytest.mark.parametrize("B", R.STAGED_BATCHES)
def test_bf16_staged_path_is_bit_identical_at_ragged_batches(E, B):
    """hx_hirl_critic_grads + hx_adam + hx_hirl_actor_backward + hx_hirl_actor_wgrad + hx_adam == hx_hirl_learn on the inputs of ("soft", B): every
    network, moment and image bit for bit (loss sums are float atomics: order-dependent in the last bit, hence rtol 1e-6 — see
    tests/test_bf16_update_gpu.py::test_bf16_staged_path_is_bit_identical_to_the_one_call_path)"""
    a, la, _ = run_learn_case(E, "soft", B, staged=False, check=False)
    b, lb, _ = run_learn_case(E, "soft", B, staged=True, check=False)
    np.testing.assert_allclose(la, lb, rtol=1e-6, atol=1e-7)
    for name in ("actor", "critic", "target_actor", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.images.view(torch.int16), b.images.view(torch.int16))


@pytest.mark.parametrize("B", R.SAC_BATCHES)
def test_sac_bf16_learn_at_ragged_batches(SE, B):
    """the SAC bf16 update on the inputs of tests/_sac_edges.py case "ragged", three calls (the third takes the Polyak step first), with the bars of
    tests/test_sac_bf16_gpu.py::test_sac_bf16_learn_against_the_rounded_operand_oracle"""
    from tests import test_sac_bf16_gpu as B16
    from tests.test_sac_gpu import sync

    params = X.case_params("ragged")
    ring = torch.from_numpy(X.replay()).cuda().contiguous()
    e = SE.SacEngine(batch=B)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_act_dtype("bf16")
    e.set_update_dtype("bf16")
    o = S.SacOracle(params["policy"], params["q1"], params["q2"])
    worst = Worst()
    for k, (idx, e1, e2) in enumerate(X.calls("ragged", B)):
        done = X.replay()[idx, 31]
        assert done[0] == 1 and done[1] == 0
        sync(o, e, SE)
        e.assemble(ring, torch.from_numpy(idx).cuda())
        e.learn(torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda())
        got = e.losses_host()
        with B16.RoundedSac(B16.kernel_masks(e, B=B)) as rs:
            ref = o.learn(X.batch_of(idx), e1, e2)
        worst.kinks += rs.taken
        worst.losses(got, ref)
        gq, gp = e.grad_critic.cpu(), e.grad_policy.cpu()
        checks = []
        for name, flat, blk, dims in (("q1", gq[:SE.Q_SIZE], SE.Q_BLOCK, (17, 1)), ("q2", gq[SE.Q_SIZE:], SE.Q_BLOCK, (17, 1)), ("policy", gp, SE.POLICY_BLOCK, (13, 8))):
            u = SE.unpack_mlp(flat, blk, *dims)
            for key in S.MLP_KEYS:
                x, r = u[key].numpy().ravel(), o.last_grads[name][key].numpy().ravel()
                scale = max(np.abs(r).max(), 1e-30)
                tight = np.abs(x - r) <= B16.TIGHT[0] * np.abs(r) + B16.TIGHT[1] * scale
                loose = float((np.abs(x - r) / (B16.LOOSE[0] * np.abs(r) + B16.LOOSE[1] * scale)).max())
                checks.append((f"{name} {key}", float((~tight).mean()), loose))
        worst.grads(checks)
        print(f"\n[sac bf16 ragged] B={B} call {k}: losses {np.asarray(got)} oracle {np.asarray(ref)}; so far {worst}")
        np.testing.assert_allclose(got, ref, rtol=B16.LOSS_RTOL, atol=B16.LOSS_ATOL, err_msg=f"B={B} call {k} losses")
        for what, miss, loose in checks:
            assert miss <= 0.002, f"B={B} call {k} {what}: {miss:.4f} of the entries beyond TIGHT"
            assert loose <= 1.0, f"B={B} call {k} {what}: beyond LOOSE ({loose:.2f} x)"
        sd = e.state_dicts()
        for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
            d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-3 and d.max() <= 2.1e-3, f"B={B} call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
        np.testing.assert_allclose(e.alpha_state.cpu().numpy()[3], float(o.alpha.reshape(-1)[0]), rtol=1e-5, err_msg=f"B={B} call {k} alpha")
        B16.check_images(SE, e, f"B={B} call {k}")
    assert e.learning_steps == X.CALLS == 3
    print(f"\n[sac bf16 ragged] B={B}: {worst}")
