"""GPU tests of the SAC bf16 path (include/hirl4ucav.h "SAC bf16 path"): bf16 acting with the fp32 Gaussian head (per-tile kernel up to 8,192 rows,
the streaming persistent kernel's MODE 2 beyond), the bf16 update (forward, input-gradient and weight-gradient products of the 256 <-> 512 layer of
the policy, both critics and both target critics on bf16 MFMA), the images that follow every optimizer / Polyak step, the bf16 front launch and the
drivers' --dtype bf16 for SAC.

The reference for the update is the SAC oracle with its "2.weight" layer run through hirl_oracle._RoundedLinear2 (bf16 operands, exact products,
fp64 sums) and, at hidden units whose pre-activation sits within KINK of zero, the kernel's subgradient (its masks read back from the workspace):
the approach of tests/test_bf16_update_gpu.py."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as HO  # noqa: E402
from oracle import sac_oracle as S  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402
from tests.test_sac_gpu import sync  # noqa: E402

H1, H2 = 256, 512
LOSS_RTOL, LOSS_ATOL = 1e-4, 2e-5
TIGHT = (2e-3, 2e-4)   # |dg| <= a |g| + b max|g| for >= 99.8 % of a tensor's entries
LOOSE = (2e-2, 2e-3)   # ... and for every entry
KINK = 5e-3
IM_ACTOR, IM_C1, IM_C2, IM_TA, IM_TC1, IM_TC2, IM_BC, IM_ACTOR_T, IM_C1_T, IM_C2_T = range(10)


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


def engine(SE, act="bf16", update="f32", params=None):
    p = params or sac_params()
    e = SE.SacEngine(batch=128)
    e.load_params(p["policy"], p["q1"], p["q2"])
    e.set_act_dtype(act)
    e.set_update_dtype(update)
    return e


class per_tile_kernel:
    """HX_ACT_PERSIST=0 for the calls inside: the per-tile acting kernel at every size (the library reads the variable per call)"""

    def __enter__(self):
        os.environ["HX_ACT_PERSIST"] = "0"

    def __exit__(self, *exc):
        os.environ.pop("HX_ACT_PERSIST", None)


def image(w2):
    """w2_image_index order of a [512][256] W2 (hx_update.h): (column tile, k slab, k group, column in tile, k in group), as bf16"""
    return w2.to(torch.bfloat16).reshape(32, 16, 8, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def image_t(w2):
    """w2t_image_index order (the transposed image: B[n][k1] = W2[n][k1], tiles of 16 k1, slabs of 32 n)"""
    return w2.t().to(torch.bfloat16).reshape(16, 16, 16, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def w2_of(SE, flat, block):
    off, n = block["W2"]
    return flat[off:off + n].reshape(H2, H1)


def rounded_policy(p, obs):
    """the Gaussian head's pre-activations with bf16(h1) bf16(W2)^T (exact products, fp64 sums), everything else fp32"""
    t = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in p.items()}
    h = torch.relu(torch.as_tensor(obs) @ t["0.weight"].t() + t["0.bias"])
    z = (h.to(torch.bfloat16).double() @ t["2.weight"].to(torch.bfloat16).double().t()).float() + t["2.bias"]
    out = torch.relu(z) @ t["4.weight"].t() + t["4.bias"]
    mean, log_std = out[:, :4], out[:, 4:].clamp(-20.0, 2.0)
    return mean, log_std


def philox_eps(n, seed, call, row0=0):
    """the Gaussian head's Philox draws (hx_act.h philox_normal, tag "SAC1"): counter (row0 + row, call, tag, 0), key = seed; components 0 .. 3 =
    Box-Muller cos / sin of the (u0, u1) and (u2, u3) pairs, u = ((x >> 8) + 0.5) / 2^24 — here in float64 (the device's logf / sinf / cosf differ in
    the last bits, far below the bars)"""
    from tests import _oracle as ox

    L = ox.lib()
    key, out = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32), np.zeros(4, np.uint32)
    eps = np.zeros((n, 4), np.float64)
    for r in range(n):
        ctr = np.array([row0 + r, call, 0x53414331, 0], np.uint32)
        L.ox_philox4x32_10(ox.p(ctr), ox.p(key), ox.p(out))
        u = ((out >> 8).astype(np.float64) + 0.5) / 16777216.0
        for j in range(4):
            p = j & 2
            rad, ang = np.sqrt(-2.0 * np.log(u[p])), 2.0 * np.pi * u[p + 1]
            eps[r, j] = rad * (np.sin(ang) if j & 1 else np.cos(ang))
    return eps.astype(np.float32)


def check_actions(got, ref, full, what):
    d = np.abs(got - ref)
    assert (d <= 1e-4).mean() >= 0.99 and d.max() <= 2e-3, f"{what}: vs rounded operands {(d > 1e-4).mean():.4f} beyond 1e-4, max {d.max():.2e}"
    df = np.abs(got - full)
    assert df.max() <= 2e-2 and df.mean() <= 2e-3, f"{what}: vs the fp32 policy max {df.max():.2e} mean {df.mean():.2e}"


@pytest.mark.parametrize("n", [1, 300, 4096, 8213, 16384])
def test_sac_bf16_acting_against_rounded_operands(SE, n):
    """hx_sac_act from the bf16 image against an fp32 evaluation on the same rounded operands and against the fp32 policy: exploit, injected eps, Philox."""
    p = sac_params()
    e, f = engine(SE), engine(SE, act="f32")
    rng = np.random.default_rng(n)
    obs = rng.uniform(-1, 1, (n, 13)).astype(np.float32)
    eps = rng.normal(0, 1, (n, 4)).astype(np.float32)
    go, ge = torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda()
    mean, log_std = rounded_policy(p["policy"], obs)
    ref_x = torch.tanh(mean).numpy()
    ref_e = torch.tanh(mean + log_std.exp() * torch.from_numpy(eps)).numpy()
    check_actions(e.act(go, explore=False).cpu().numpy(), ref_x, f.act(go, explore=False).cpu().numpy(), f"exploit n={n}")
    check_actions(e.act(go, eps=ge).cpu().numpy(), ref_e, f.act(go, eps=ge).cpu().numpy(), f"eps n={n}")
    # Philox: the kernel draws eps itself (seed 9, row, call 8); the reference draws the same numbers on the host
    e.act_calls = f.act_calls = 7
    ref_p = torch.tanh(mean + log_std.exp() * torch.from_numpy(philox_eps(n, 9, 8))).numpy()
    check_actions(e.act(go, seed=9).cpu().numpy(), ref_p, f.act(go, seed=9).cpu().numpy(), f"philox n={n}")


def test_sac_bf16_launch_shapes_agree_bit_for_bit(SE):
    """MODE 2 of the streaming persistent kernel == the per-tile Gaussian bf16 kernel; 8,213 rows in one call == 4,096-row chunks."""
    e = engine(SE)
    rng = np.random.default_rng(3)
    for n in (8213, 16384, 40000 + 5):
        obs = torch.from_numpy(rng.uniform(-1, 1, (n, 13)).astype(np.float32)).cuda()
        eps = torch.from_numpy(rng.normal(0, 1, (n, 4)).astype(np.float32)).cuda()
        for kw in ({"explore": False}, {"eps": eps}, {"seed": 5}):
            e.act_calls = 3
            big = e.act(obs, **kw)
            with per_tile_kernel():
                e.act_calls = 3
                tile = e.act(obs, **kw)
            assert torch.equal(big, tile), (n, list(kw))
            if n == 8213 and "seed" not in kw:
                parts = [e.act(obs[i:i + 4096], **({"eps": eps[i:i + 4096]} if "eps" in kw else kw)) for i in range(0, n, 4096)]
                assert torch.equal(big, torch.cat(parts)), list(kw)


@pytest.mark.parametrize("n", [4096 + 17, 16384])
def test_sac_bf16_act_step_equals_act_then_step(SE, n):
    """hx_sac_act_step from the bf16 image (per-tile with the env tail / the streaming kernel with env tail and replay insert) == act_bf16 then env.step."""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    side = []
    for _ in range(2):
        e = engine(SE)
        rep = DeviceReplay(1 << 17)
        env = BatchedHarfangEnv(n, scenario="serpentine", seed=1, max_step=7, auto_reset=True, random_reset=True, replay=rep)
        env.reset()
        side.append((e, env, rep))
    (a, env_a, rep_a), (b, env_b, rep_b) = side
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = torch.zeros((n, 4), device="cuda")
    for k in range(9):
        kw = [{"explore": False}, {"eps": torch.randn((n, 4), device="cuda", generator=g)}, {"seed": 4}][k % 3]
        a.act(env_a.obs, out=acts, **kw)
        env_a.step(acts)
        a2 = b.act_step(env_b, **kw)[0]
        assert torch.equal(acts, a2), f"actions, step {k}"
        for name in ("state", "obs", "reward", "done", "success", "episode_ctr"):
            assert torch.equal(getattr(env_a, name).view(torch.uint8), getattr(env_b, name).view(torch.uint8)), f"{name}, step {k}"
    assert int(rep_a.total.item()) == int(rep_b.total.item()) > 0


def slot(e, k, B=128):
    """workspace slot k of SAC (hx_sac.hip SS_*: 0 policy(s'), 1 policy(s), 2/3 Q1/Q2(s, a), 4/5 targets, 6/7 Q1/Q2(s, a~))"""
    from tests.test_bf16_update_gpu import SLOT_FIELDS

    per_row = sum(n for _, n in SLOT_FIELDS)
    ws = e.ws[k * per_row * B:(k + 1) * per_row * B].cpu()
    out, o = {}, 0
    for name, n in SLOT_FIELDS:
        out[name] = ws[o:o + B * n].reshape(B, n)
        o += B * n
    return out


class RoundedSac:
    """sac_oracle with the "2.weight" layer through _RoundedLinear2 and, near kinks, the kernel's ReLU masks (activation calls of the oracle's
    learn(), two per network: policy(s') 0, 1; target Q1, Q2 (s', a') 2 .. 5; Q1, Q2 (s, a) 6 .. 9; policy(s) 10, 11; Q1, Q2 (s, a~) 12 .. 15)"""

    def __init__(self, masks):
        self.masks, self.calls, self.taken = masks, 0, 0

    def __enter__(self):
        self._mlp, self._act = S.mlp, S._act
        outer = self

        class Masked(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, mask):
                ctx.mask = mask
                return torch.where(mask, x, torch.zeros_like(x))

            @staticmethod
            def backward(ctx, g):
                return g * ctx.mask, None

        def act(x, slope=0.0):
            c = outer.calls
            outer.calls += 1
            m = outer.masks.get(c)
            if m is None:
                return outer._act(x, slope)
            own = (x > 0).detach()
            differ = own != m
            if not differ.any():
                return outer._act(x, slope)
            far = differ & (x.detach().abs() > KINK)
            assert not far.any(), f"activation call {c}: the kernel's mask differs at |pre-activation| {float(x.detach().abs()[far].max()):.3e} > {KINK}"
            outer.taken += int(differ.sum())
            return Masked.apply(x, torch.where(differ, m, own))

        def mlp(p, x):
            h = S._act(torch.nn.functional.linear(x, p["0.weight"], p["0.bias"]))
            h = S._act(HO._RoundedLinear2.apply(h, p["2.weight"], p["2.bias"]))
            return torch.nn.functional.linear(h, p["4.weight"], p["4.bias"])

        S.mlp, S._act = mlp, act
        return self

    def __exit__(self, *exc):
        S.mlp, S._act = self._mlp, self._act


def kernel_masks(e, B=128):
    """per activation call of the oracle's learn(): the kernel's masks (layer 1: h1 > 0 where the forward saved it — not for policy(s') and the
    targets, which nothing differentiates; layer 2: z2 > 0, z2 with its bias, the LayerNorm slots being (1, 0))"""
    order = [0, 4, 5, 2, 3, 1, 6, 7]  # slots in the oracle's evaluation order (see RoundedSac)
    masks = {}
    for i, k in enumerate(order):
        f = slot(e, k, B=B)
        if k not in (0, 4, 5):
            masks[2 * i] = f["h1"] > 0
        masks[2 * i + 1] = f["z2"] > 0
    return masks


def test_sac_bf16_learn_against_the_rounded_operand_oracle(SE, golden_dir):
    """The 8 golden learn() calls (Polyak at calls 3 and 6) in bf16: losses, every gradient (TIGHT for 99.8 %, LOOSE for all), parameters after Adam,
    alpha — against the rounded-operand oracle; and after every call every image equals bf16 of its fp32 master, bit for bit."""
    g = np.load(os.path.join(golden_dir, "sac_learn.npz"))
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e = engine(SE, "bf16", "bf16", params)
    o = S.SacOracle(params["policy"], params["q1"], params["q2"])
    for k in range(g["out"].shape[0]):
        sync(o, e, SE)
        e.assemble(ring, torch.from_numpy(g["idx"][k].astype(np.int32)).cuda())
        e.learn(torch.from_numpy(g["eps"][k, 0]).cuda(), torch.from_numpy(g["eps"][k, 1]).cuda())
        got = e.losses_host()
        rows = data["replay"][g["idx"][k]]
        with RoundedSac(kernel_masks(e)):
            ref = o.learn((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), g["eps"][k, 0], g["eps"][k, 1])
        np.testing.assert_allclose(got, ref, rtol=LOSS_RTOL, atol=LOSS_ATOL, err_msg=f"call {k} losses")
        gq, gp = e.grad_critic.cpu(), e.grad_policy.cpu()
        for name, flat, blk, dims in (("q1", gq[:SE.Q_SIZE], SE.Q_BLOCK, (17, 1)), ("q2", gq[SE.Q_SIZE:], SE.Q_BLOCK, (17, 1)),
                                      ("policy", gp, SE.POLICY_BLOCK, (13, 8))):
            u = SE.unpack_mlp(flat, blk, *dims)
            for key in S.MLP_KEYS:
                x, r = u[key].numpy().ravel(), o.last_grads[name][key].numpy().ravel()
                scale = max(np.abs(r).max(), 1e-30)
                tight = np.abs(x - r) <= TIGHT[0] * np.abs(r) + TIGHT[1] * scale
                assert tight.mean() >= 0.998, f"call {k} {name} {key}: {(~tight).sum()} entries beyond TIGHT"
                assert np.all(np.abs(x - r) <= LOOSE[0] * np.abs(r) + LOOSE[1] * scale), f"call {k} {name} {key}: beyond LOOSE"
        sd = e.state_dicts()
        for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
            d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-3 and d.max() <= 2.1e-3, f"call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
        np.testing.assert_allclose(e.alpha_state.cpu().numpy()[3], float(o.alpha.reshape(-1)[0]), rtol=1e-5, err_msg=f"call {k} alpha")
        check_images(SE, e, f"call {k}")


def check_images(SE, e, what):
    im = e.images.view(10, H2 * H1)
    pairs = [(IM_ACTOR, image(w2_of(SE, e.policy, SE.POLICY_BLOCK))), (IM_ACTOR_T, image_t(w2_of(SE, e.policy, SE.POLICY_BLOCK)))]
    for h in range(2):
        c = w2_of(SE, e.critic[h * SE.Q_SIZE:(h + 1) * SE.Q_SIZE], SE.Q_BLOCK)
        pairs += [(IM_C1 + h, image(c)), (IM_C1_T + h, image_t(c)), (IM_TC1 + h, image(w2_of(SE, e.target_critic[h * SE.Q_SIZE:(h + 1) * SE.Q_SIZE], SE.Q_BLOCK)))]
    for i, ref in pairs:
        assert torch.equal(im[i].view(torch.int16), ref.view(torch.int16)), f"{what}: image {i}"


def test_sac_bf16_policy_image_follows_the_fp32_update(SE):
    """bf16_policy (bf16 acting beside the fp32 update): policy_w2_bf16 equals bf16 of the policy's W2 after every Adam step."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    e = engine(SE, "bf16", "f32")
    rng = np.random.default_rng(2)
    rep = DeviceReplay(4096)
    rep.store_rows(torch.from_numpy(rng.normal(size=(2000, 32)).astype(np.float32)))
    for k in range(4):
        assert torch.equal(e.w2_bf16.view(torch.int16), image(w2_of(SE, e.policy, SE.POLICY_BLOCK)).view(torch.int16)), k
        e.sample(rep, seed=1)
        e.learn()


@pytest.mark.parametrize("defer", [False, True])
def test_sac_bf16_learn_in_one_call_is_bit_identical_to_the_staged_sequence(SE, defer):
    """hx_sac_learn in bf16 == hx_sac_critic_step + hx_sac_policy_grads + hx_sac_adam(1) == every stage a call of its own (staged Polyak + image
    repack, hx_sac_adam's image refresh): after 7 calls the same networks, moments, targets, alpha and images, bit for bit."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    rng = np.random.default_rng(5)
    rep = DeviceReplay(4096)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(4096, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += 4096
    a, b, c = (engine(SE, "bf16", "bf16") for _ in range(3))
    b.staged_policy = True
    c.separate_critic_adam = True
    for k in range(7):
        for e in (a, b, c):
            e.sample(rep, None, seed=11, defer=defer)
            e.learn()
    for other in (b, c):
        for name in ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "images"):
            assert torch.equal(getattr(a, name).view(torch.int16), getattr(other, name).view(torch.int16)), name
        np.testing.assert_allclose(a.losses.cpu().numpy(), other.losses.cpu().numpy(), rtol=1e-6)
    check_images(SE, a, "after 7 calls")


def test_staged_bf16_update_gives_the_parents_bits(SE, golden_dir):
    """the staged bf16 update (hx_sac_critic_grads + hx_sac_adam(0) + hx_sac_policy_grads + hx_sac_adam(1): adam_kernel with segment images) at
    B = 48, four calls from a fixed start: networks, moments, alpha state and the whole image block carry the bits of the recording made with the
    library of the commit before adam_kernel's float4 step became shared code (tests/golden/sac_fold_bits.npz, tests/_sac_fold_bits.py)"""
    from tests import _sac_fold_bits

    _sac_fold_bits.assert_replays(SE, sac_params(), np.load(os.path.join(golden_dir, "sac_fold_bits.npz")), ("staged_bf16",))


@pytest.mark.parametrize("n,cap,esac", [(16384, 40000, False), (9000, 20000, True)])
def test_sac_bf16_front_launch_equals_act_step_then_guarded_learn(SE, n, cap, esac):
    """step_learn in bf16 (actps_sac_front_kernel<2>: MODE 2 acting + the bf16 first launch of learn()) == act_step_bf16, then learn() on a minibatch
    drawn with HxSample.total read before the step and guard = n — bit for bit, step by step; SAC and E-SAC."""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay
    from tests.test_front_gpu import allowed_slots, sorted_rows

    rng = np.random.default_rng(n)
    exp = None
    if esac:
        exp = DeviceReplay(64)
        exp.store_rows(torch.from_numpy(rng.normal(size=(40, 32)).astype(np.float32)))
    scen = (np.arange(n) % 3).astype(np.int32)
    side = []
    for _ in range(2):
        e = engine(SE, "bf16", "bf16")
        rep = DeviceReplay(cap)
        env = BatchedHarfangEnv(n, scenario=scen, seed=5, max_step=6, auto_reset=True, random_reset=True, replay=rep)
        env.reset()
        side.append((e, env, rep))
    (a, env_a, rep_a), (b, env_b, rep_b) = side
    a.act_step(env_a, seed=3)
    snap = torch.zeros(1, dtype=torch.int64, device="cuda")
    for k in range(6):
        b.arena.copy_(a.arena)
        b.images.copy_(a.images)
        for name in ("learning_steps", "sample_calls", "act_calls"):
            setattr(b, name, getattr(a, name))
        env_b._state_store.copy_(env_a._state_store)
        for name in ("obs", "reward", "done", "success", "episode_ctr"):
            getattr(env_b, name).copy_(getattr(env_a, name))
        rep_b.ring.copy_(rep_a.ring); rep_b.success.copy_(rep_a.success); rep_b.total.copy_(rep_a.total)  # noqa: E702
        tot0 = int(rep_a.total.item())
        out_a = a.step_learn(env_a, exp, n_main=96, act_seed=3, sample_seed=11)
        snap.copy_(rep_b.total)
        out_b = b.act_step(env_b, seed=3)
        b.sample(rep_b, exp, n_main=96, seed=11, defer=True)
        b._pending[0].total, b._pending[0].guard = snap.data_ptr(), n
        b.learn()
        for x, y, name in zip(out_a, out_b, ("actions", "obs", "reward", "done", "success")):
            assert torch.equal(x, y), (k, name)
        assert torch.equal(env_a._state_store, env_b._state_store) and torch.equal(rep_a.total, rep_b.total), k
        np.testing.assert_array_equal(sorted_rows(rep_a), sorted_rows(rep_b), err_msg=f"step {k}: replay rows")
        assert torch.equal(a._idx, b._idx) and torch.equal(a.rows, b.rows), k
        np.testing.assert_allclose(a.losses_host(), b.losses_host(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
        for name in ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "images"):
            assert torch.equal(getattr(a, name).view(torch.int16), getattr(b, name).view(torch.int16)), (k, name)
        i = a._idx.cpu().numpy()
        m = 96 if esac else 128
        assert len(set(i[:m])) == m and np.isin(i[:m], allowed_slots(tot0, cap, n)).all(), (k, tot0)


def test_sac_bf16_drivers(SE, tmp_path, capsys):
    """train_all --agent SAC --dtype bf16: no warning, finite losses, the snapshot records bf16 and resumes; --dtype f32 on it is refused; an unmarked
    SAC snapshot (before SAC had bf16) resumed with --dtype bf16 runs fp32 with the warning.  validate_all --agent SAC --dtype bf16 completes a round."""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd import validate_all as V

    common = ["--agent", "SAC", "--env", "serpentine", "--random", "--seed", "2", "--num_envs", "256", "--buffer_size", "32768", "--snapshot_every", "1"]
    T.MAX_STEP["serpentine"] = 30
    try:
        run = T.main(T.parser().parse_args(common + ["--episodes", "1", "--dtype", "bf16", "--result_dir", str(tmp_path / "a")]))
        out = capsys.readouterr().out
        assert "WARNING: --dtype" not in out and "nan" not in out.lower() and "alpha" in out
        st = torch.load(os.path.join(run, "state_rank0.pt"), weights_only=False)
        assert st["driver"]["dtype"] == "bf16" and st["driver"]["dtype_honoured"]
        T.main(T.parser().parse_args(common + ["--episodes", "2", "--dtype", "bf16", "--result_dir", str(tmp_path / "b"), "--resume", run]))
        assert "WARNING: --dtype" not in capsys.readouterr().out
        with pytest.raises(SystemExit, match="--dtype bf16"):
            T.main(T.parser().parse_args(common + ["--episodes", "2", "--dtype", "f32", "--result_dir", str(tmp_path / "c"), "--resume", run]))
        # an unmarked snapshot: what a SAC run given --dtype bf16 stored before (dtype "f32", no mark)
        old = os.path.join(str(tmp_path), "old")
        os.makedirs(old)
        st["driver"]["dtype"] = "f32"
        del st["driver"]["dtype_honoured"]
        torch.save(st, os.path.join(old, "state_rank0.pt"))
        d = T.main(T.parser().parse_args(common + ["--episodes", "2", "--dtype", "bf16", "--result_dir", str(tmp_path / "d"), "--resume", old]))
        assert "WARNING: --dtype bf16 has no effect" in capsys.readouterr().out
        sd = torch.load(os.path.join(d, "state_rank0.pt"), weights_only=False)["driver"]
        assert sd["dtype"] == "f32" and "dtype_honoured" not in sd and sd["episode"] == 2  # the legacy run's snapshots stay unmarked ...
        T.main(T.parser().parse_args(common + ["--episodes", "3", "--dtype", "bf16", "--result_dir", str(tmp_path / "e"), "--resume", d]))
        assert "WARNING: --dtype bf16 has no effect" in capsys.readouterr().out  # ... so its second resume, same command line, runs fp32 again
    finally:
        T.MAX_STEP["serpentine"] = 1500
    model = os.path.join(run, "model")
    tags = sorted({f[len("policy_"):-len(".pth")] for f in os.listdir(model) if f.startswith("policy_")})
    if not tags:  # no checkpoint in so short a run: write one
        e = engine(SE, "bf16")
        e.save_models(model, "Agent1_0_0_")
        tags = ["Agent1_0_0_"]
    vr, vs, _ = V.main(V.parser().parse_args(["--agent", "SAC", "--model_dir", model, "--model_name", tags[0], "--random", "--seed", "5", "--episodes", "4",
                                              "--validation_step", "60", "--nums", "1", "--dtype", "bf16"]))
    assert len(vr) == 1 and np.isfinite(vr[0]) and "WARNING: --dtype" not in capsys.readouterr().out
