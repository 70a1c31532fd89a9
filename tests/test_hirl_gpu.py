"""GPU parity tests of the actor/critic path (hx_actor_act, hx_hirl_*, hx_adam, hx_polyak through the C ABI) against
the update oracle (oracle/hirl_oracle.py, itself pinned to the reference) and against the golden vectors recorded from
the reference's own Agent.learn (tests/golden/hirl_learn_*.npz, td3_learn.npz, hirl_choose_action.npz).

Tolerances (fp32 everywhere; the GPU sums in MFMA k-order, the reference in MKL/oneDNN order):
  returned losses            rtol 2e-5 (north_star: HIRL loss parity)
  gradients vs the oracle    |diff| <= 1e-4 |g| + 2e-5 max|g| per tensor (entries that are sums of cancelling terms
                             carry fp32 summation-order noise relative to the tensor's scale, not to themselves)
  parameters after k steps   atol 2e-6 + rtol 1e-5 on the probes (Adam turns last-bit gradient differences of
                             near-zero entries into visible fractions of lr = 1e-3; bounded by the probe check)"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_data as D  # noqa: E402

MODES = ["soft_e0", "soft_e64", "fixed_e32", "linear_e0"]


@pytest.fixture(scope="module")
def eng_mod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


def device_tables(data):
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    exp = torch.from_numpy(data["expert_rows"]).cuda().contiguous()
    bc = np.zeros((data["expert_s"].shape[0], 32), np.float32)
    bc[:, 0:13], bc[:, 13:17] = data["expert_s"], data["expert_a"]
    return ring, exp, torch.from_numpy(bc).cuda().contiguous()


GRAD_RTOL, GRAD_ATOL_OF_MAX = 1e-4, 2e-5   # |dg| <= 1e-4 |g| + 2e-5 max|g| per tensor, EVERY entry
FRAGILE = 4e-6                              # |pre-activation| below this: the unit's ReLU derivative is a coin toss in fp32


def grad_mismatch(got_flat, oracle_grads, layout):
    """-> list of (key, n_bad, worst, max|g|) for tensors with ANY entry outside |dg| <= 1e-4 |g| + 2e-5 max|g|"""
    got = got_flat.cpu().numpy()
    out = []
    for k, off, shp in layout:
        g = oracle_grads[k].numpy().ravel()
        x = got[off:off + g.size]
        tol = GRAD_RTOL * np.abs(g) + GRAD_ATOL_OF_MAX * max(np.abs(g).max(), 1e-30)
        bad = np.abs(x - g) > tol
        if bad.any():
            out.append((k, int(bad.sum()), float(np.abs(x - g).max()), float(np.abs(g).max())))
    return out


class ActProbe:
    """Patches the oracle's activation: records every pre-activation tensor of a learn() call and, on request, evaluates the
    backward pass with the ReLU / LeakyReLU derivative of chosen (call, row, unit) positions FLIPPED.  The forward value is untouched
    (the activation is continuous); only the subgradient picked at a kink changes."""

    def __init__(self, flips=(), module=None):
        self.mod = module if module is not None else H
        self.flips = {}
        for c, r, u in flips:
            self.flips.setdefault(c, []).append((r, u))
        self.pre = []

    def __enter__(self):
        self._orig = self.mod._act

        class Flipped(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, slope, mask):
                ctx.slope, ctx.mask = slope, mask
                return torch.where(x > 0, x, x * slope)

            @staticmethod
            def backward(ctx, g):
                return g * torch.where(ctx.mask, torch.ones_like(g), torch.full_like(g, ctx.slope)), None, None

        def act(x, slope=0.0):
            c = len(self.pre)
            self.pre.append(x.detach())
            if c not in self.flips:
                return self._orig(x, slope)
            mask = (x > 0).detach().clone()
            for r, u in self.flips[c]:
                mask[r, u] = ~mask[r, u]
            return Flipped.apply(x, slope, mask)

        self.mod._act = act
        return self

    def __exit__(self, *exc):
        self.mod._act = self._orig

    def fragile(self):
        out = []
        for c, x in enumerate(self.pre):
            if x.dim() == 2:
                for r, u in (x.abs() < FRAGILE).nonzero().tolist():
                    out.append((c, r, u))
        return out


def oracle_checked(o, run, pairs, what, module=None):
    """ref = run(o) advances the oracle `o` by one call; `pairs` = [(engine gradient buffer, key of o.last_grads, layout)].  The engine's
    gradients are compared under the STRICT elementwise tolerance — no entry may miss.  If some do, the only accepted explanation is a
    hidden unit whose pre-activation sits within fp32 rounding of zero for some row (its ReLU derivative is then 0 on one side and
    1 on the other): the oracle's backward pass is re-evaluated with those derivatives flipped (every subset of the fragile
    positions, at most 2^6), and the engine's gradients must match ONE of these valid subgradients in every entry.  Returns ref;
    `o` ends in the state of the matching evaluation."""
    import copy
    import itertools

    before = copy.deepcopy(o)
    with ActProbe(module=module) as probe:
        ref = run(o)

    def mismatches(oo):
        m = []
        for flat, key, layout in pairs:
            m += layout(oo) if callable(layout) else grad_mismatch(flat, oo.last_grads[key], layout)
        return m

    first = mismatches(o)
    if not first:
        return ref
    frag = probe.fragile()
    assert frag, f"{what}: gradient entries outside the tolerance and NO pre-activation within {FRAGILE} of zero: {first}"
    assert len(frag) <= 6, f"{what}: {len(frag)} fragile positions"
    for k in range(1, len(frag) + 1):
        for subset in itertools.combinations(frag, k):
            alt = copy.deepcopy(before)
            with ActProbe(subset, module=module):
                ref_alt = run(alt)
            if not mismatches(alt):
                o.__dict__.update(alt.__dict__)
                return ref_alt
    raise AssertionError(f"{what}: no choice of subgradients at the {len(frag)} fragile positions {frag} reproduces the engine's gradients: {first}")


def oracle_learn_checked(eng_mod, e, o, args, was_actor_call, what):
    pairs = [(e.grad_critic, "critic", eng_mod.CRITIC_LAYOUT)] + ([(e.grad_actor, "actor", eng_mod.ACTOR_LAYOUT)] if was_actor_call else [])
    return oracle_checked(o, lambda oo: oo.learn(*args), pairs, what)


def probes_of(e, eng_mod):
    """same flattening as the golden probes: exact (unpadded) state_dict order"""
    out = []
    for flat, layout in ((e.actor, eng_mod.ACTOR_LAYOUT), (e.critic, eng_mod.CRITIC_LAYOUT), (e.target_actor, eng_mod.ACTOR_LAYOUT),
                         (e.target_critic, eng_mod.CRITIC_LAYOUT)):
        f = flat.cpu().numpy()
        out.append(D.net_probe(np.concatenate([f[off:off + int(np.prod(shp))] for k, off, shp in layout])))
    return out


def test_act_row_tilings_agree_bit_for_bit(eng_mod):
    """hx_actor_act runs 16 rows per workgroup below 8,192 rows and 32 from there on (every W2 chunk multiplied against two row
    tiles): the per-row arithmetic is the same, so the outputs must be identical, ragged tail included."""
    params = D.make_params(D.PARAM_SEED)
    e = eng_mod.HirlEngine(batch=128)
    e.x9_rows = None  # the fp32-MFMA family at every size (the engine's default takes the exact-split format from 4,096 rows on: tests/test_x9_gpu.py, test_actp_gpu.py)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    rng = np.random.default_rng(5)
    n = 8192 + 37
    obs = torch.from_numpy(rng.uniform(-1, 1, (n, 13)).astype(np.float32)).cuda()
    per = torch.from_numpy(rng.normal(0, 0.3, (n, 4)).astype(np.float32)).cuda()
    big = e.act(obs, noise=per)
    parts = [e.act(obs[i:i + 4096], noise=per[i:i + 4096]) for i in range(0, n, 4096)]
    assert torch.equal(big, torch.cat(parts))
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"])
    np.testing.assert_allclose(big[-200:].cpu().numpy(), o.choose_action(obs[-200:].cpu().numpy(), per[-200:].cpu().numpy()), rtol=1e-5, atol=1e-6)
    # Philox exploration noise is keyed by the global row: the tiling does not change the draw
    a1 = e.act(obs, sigma=0.1, seed=9)
    e.act_calls -= 1
    a2 = torch.cat([e.act(obs[:4096], sigma=0.1, seed=9, row0=0)] + [None] * 0)
    assert torch.equal(a1[:4096], a2)


def test_actor_act_matches_oracle_and_reference(eng_mod, golden_dir):
    params = D.make_params(D.PARAM_SEED)
    e = eng_mod.HirlEngine(batch=128)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"])
    rng = np.random.default_rng(0)
    for n in (1, 5, 16, 1000):
        obs = rng.uniform(-1, 1, (n, 13)).astype(np.float32)
        a = e.act(torch.from_numpy(obs).cuda()).cpu().numpy()
        np.testing.assert_allclose(a, o.choose_action(obs), rtol=1e-5, atol=1e-6)
        shared = (rng.normal(0, 0.5, 4)).astype(np.float32)
        a = e.act(torch.from_numpy(obs).cuda(), noise=torch.from_numpy(shared).cuda()).cpu().numpy()
        np.testing.assert_allclose(a, o.choose_action(obs, shared), rtol=1e-5, atol=1e-6)
        per = rng.normal(0, 0.5, (n, 4)).astype(np.float32)
        a = e.act(torch.from_numpy(obs).cuda(), noise=torch.from_numpy(per).cuda()).cpu().numpy()
        np.testing.assert_allclose(a, o.choose_action(obs, per), rtol=1e-5, atol=1e-6)
    # golden: the reference's chooseAction / SmallNoise / NoNoise with its recorded noise draws
    g = np.load(os.path.join(golden_dir, "hirl_choose_action.npz"))
    st = torch.from_numpy(g["states"]).cuda()
    np.testing.assert_allclose(e.act(st).cpu().numpy(), g["action_clean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e.act(st, noise=torch.from_numpy(g["noise"]).cuda()).cpu().numpy(), g["action"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e.act(st, noise=torch.from_numpy(g["small_noise"]).cuda()).cpu().numpy(), g["action_small"], rtol=1e-5, atol=1e-6)
    # Philox exploration noise: deterministic per (seed, row, call), right scale, independent per row
    obs = torch.zeros((20000, 13), device="cuda")
    clean = e.act(obs)
    e.act_calls = 10
    n1 = (e.act(obs, sigma=0.1, seed=5) - clean).cpu().numpy()
    e.act_calls = 10
    n2 = (e.act(obs, sigma=0.1, seed=5) - clean).cpu().numpy()
    n3 = (e.act(obs, sigma=0.1, seed=5) - clean).cpu().numpy()
    assert np.array_equal(n1, n2) and not np.array_equal(n1, n3)
    inner = np.abs(clean.cpu().numpy()) < 0.5  # away from the clamp
    assert inner.any()
    z = n1[inner] / 0.1
    assert abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03 and abs(np.corrcoef(n1[:, 0], n1[:, 1])[0, 1]) < 0.03


def sync_oracle(o, e, E):
    """Copy the engine's whole state (5 nets, Adam moments and step counts, alternation counters) into the oracle, so
    that one call is compared from IDENTICAL states.  Free-running fp32 trajectories separate chaotically as soon as
    one ReLU unit sits within rounding of zero; per-call comparison keeps the check about the kernels."""
    sd = e.state_dicts()
    for name, dst in (("actor", o.actor), ("critic", o.critic), ("targetActor", o.target_actor), ("targetCritic", o.target_critic)):
        for k in dst:
            dst[k].data.copy_(sd[name][k].cpu())
    for opt, m, v, layout, t in ((o.opt_actor, e.m_actor, e.v_actor, E.ACTOR_LAYOUT, e.actor_step),
                                 (o.opt_critic, e.m_critic, e.v_critic, E.CRITIC_LAYOUT, e.critic_step)):
        mm, vv = E.unpack(m, layout), E.unpack(v, layout)
        for k in opt.m:
            opt.m[k].copy_(mm[k].cpu())
            opt.v[k].copy_(vv[k].cpu())
        opt.t = t
    o.actor_trainable, o.update_count = e.actor_trainable, e.update_count


def assert_losses(got, ref, what):
    # rl_loss is a mean of O(1) Q values of both signs: absolute fp32 noise ~1e-6
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=what)


def check_params(e, o, E, what, was_actor_call=True):
    """After one step from identical states, EVERY parameter obeys |dp| <= 2e-6 + 2.1e-3 min(1, 8 tol_g / |g|), tol_g the
    gradient tolerance above: Adam divides by sqrt(v), so early in training an entry moves by ~lr sign(g) whatever |g| is — an entry
    whose gradient is within the tolerance of zero may legitimately land 2 lr away, one whose gradient is well resolved may not move
    by more than its relative gradient error allows.  Targets (Polyak) inherit tau times that."""
    for flat, layout, ref, grads in ((e.actor, E.ACTOR_LAYOUT, o.actor, o.last_grads.get("actor") if was_actor_call else None),
                                     (e.critic, E.CRITIC_LAYOUT, o.critic, o.last_grads["critic"]),
                                     (e.target_actor, E.ACTOR_LAYOUT, o.target_actor, o.last_grads.get("actor") if was_actor_call else None),
                                     (e.target_critic, E.CRITIC_LAYOUT, o.target_critic, o.last_grads["critic"])):
        f = flat.cpu().numpy()
        for k, off, shp in layout:
            r = ref[k].detach().numpy().ravel()
            d = np.abs(f[off:off + r.size] - r)
            if grads is None:
                bound = np.full_like(d, 2e-6)
            else:
                g = np.abs(grads[k].numpy().ravel())
                tol = GRAD_RTOL * g + GRAD_ATOL_OF_MAX * max(g.max(), 1e-30)
                bound = 2e-6 + 2.1e-3 * np.minimum(1.0, 8.0 * tol / np.maximum(g, 1e-30))
            bad = d > bound
            assert not bad.any(), f"{what} {k}: {int(bad.sum())} entries beyond their gradient-resolved bound, worst {d[bad].max():.2e}"


def check_probes_free_running(e, E, g, k, what):
    """The engine's own trajectory vs the reference's recorded one (no re-sync): 128 probed entries per network.  Adam
    normalises gradients, so fp32 summation-order noise on a near-zero gradient entry becomes a few 1e-6 of parameter
    difference per step; >= 97 % of the probes stay within 2e-6, none may leave 5e-5, and the |x| sums agree to 2e-6."""
    for j, (s, a, v) in enumerate(probes_of(e, E)):
        d = np.abs(v - g["probe_val"][k][j])
        assert (d > 2e-6).mean() <= 0.03 and d.max() < 5e-5, f"{what} net {j}: {(d > 2e-6).sum()} probes off, max {d.max():.2e}"
        np.testing.assert_allclose(a, g["probe_abs"][k][j], rtol=2e-6, err_msg=f"{what} net {j} |sum|")


@pytest.mark.parametrize("mode", MODES)
def test_learn_matches_oracle_and_reference(eng_mod, mode, golden_dir):
    """10 consecutive Agent.learn calls (three "episodes": soft-weight estimate, stale weight, re-estimate; actor every
    2nd call; Polyak at the 6th).  Free-running against the reference's recorded outputs; call by call against the
    oracle from identical states (losses, every gradient tensor, parameters after Adam/Polyak)."""
    g = np.load(os.path.join(golden_dir, f"hirl_learn_{mode}.npz"))
    params, data = D.make_params(D.PARAM_SEED), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"]) and D.checksum(data) == str(g["data_checksum"])
    ring, exp, bc = device_tables(data)
    e = eng_mod.HirlEngine(batch=128)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"])
    ne = int(g["expert_num"])
    for k in range(g["out"].shape[0]):
        idx = np.concatenate([g["idx_buf"][k], g["idx_exp"][k]]).astype(np.int32)
        w_in = 100 if g["bc_w_in"][k] == 100 else float(g["bc_w_in"][k])
        warm = float(g["warm_in"][k])
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, eng_mod)
        e.assemble(ring, torch.from_numpy(idx).cuda(), expert_ring=exp, n_main=128 - ne, bc_table=bc,
                   idx_bc=torch.from_numpy(g["idx_bc"][k].astype(np.int32)).cuda())
        e.learn(noise=torch.from_numpy(g["noise"][k]).cuda(), bc_weight_now=w_in, bc_warm_up_weight=warm)
        got = e.losses_host()
        rows = data["replay"][g["idx_buf"][k]]
        if ne:
            rows = np.concatenate([rows, data["expert_rows"][g["idx_exp"][k]]], 0)
        ob = (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31])
        ref = oracle_learn_checked(eng_mod, e, o, (ob, (data["expert_s"][g["idx_bc"][k]], data["expert_a"][g["idx_bc"][k]]), g["noise"][k], w_in, warm),
                                   was_actor_call, f"{mode} call {k} gradients")
        assert_losses(got, ref, f"{mode} call {k} vs oracle")
        check_params(e, o, eng_mod, f"{mode} call {k} params", was_actor_call)
        # the reference's own recorded run
        assert_losses(got, g["out"][k], f"{mode} call {k} vs reference golden")
        check_probes_free_running(e, eng_mod, g, k, f"{mode} call {k}")
    assert e.critic_step == 10 and e.actor_step == 5 and e.update_count == 5 and e.actor_trainable


def test_learn_without_layernorm_matches_oracle_and_reference(eng_mod, golden_dir):
    """The reference's `layerNorm=False` networks (HIRL.py:70-80,92-97,135-138) through HxHyper.no_layernorm / noise_mode + 16: 10 consecutive
    learn() calls against the oracle (identical states, every gradient entry) and the reference's recorded run, then chooseActionNoNoise."""
    g = np.load(os.path.join(golden_dir, "hirl_learn_soft_noln.npz"))
    params, data = D.plain_layernorm(D.make_params(D.PARAM_SEED)), D.make_data(D.DATA_SEED)
    ring, exp, bc = device_tables(data)
    e = eng_mod.HirlEngine(batch=128, layer_norm=False)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"], layer_norm=False)
    for k in range(g["out"].shape[0]):
        w_in = 100 if g["bc_w_in"][k] == 100 else float(g["bc_w_in"][k])
        warm = float(g["warm_in"][k])
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, eng_mod)
        e.assemble(ring, torch.from_numpy(g["idx_buf"][k].astype(np.int32)).cuda(), bc_table=bc, idx_bc=torch.from_numpy(g["idx_bc"][k].astype(np.int32)).cuda())
        e.learn(noise=torch.from_numpy(g["noise"][k]).cuda(), bc_weight_now=w_in, bc_warm_up_weight=warm)
        got = e.losses_host()
        rows = data["replay"][g["idx_buf"][k]]
        ob = (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31])
        ref = oracle_learn_checked(eng_mod, e, o, (ob, (data["expert_s"][g["idx_bc"][k]], data["expert_a"][g["idx_bc"][k]]), g["noise"][k], w_in, warm),
                                   was_actor_call, f"noln call {k} gradients")
        assert_losses(got, ref, f"noln call {k} vs oracle")
        check_params(e, o, eng_mod, f"noln call {k} params", was_actor_call)
        assert_losses(got, g["out"][k], f"noln call {k} vs reference golden")
        check_probes_free_running(e, eng_mod, g, k, f"noln call {k}")
    a = e.act(torch.from_numpy(g["states"]).cuda()).cpu().numpy()
    np.testing.assert_allclose(a, g["action_clean_after"], rtol=1e-5, atol=3e-5)  # (free-running: five actor steps of fp32 summation-order drift)
    sd = e.state_dicts()
    assert torch.all(sd["actor"]["layernorm1.weight"] == 1) and torch.all(sd["critic"]["layernorm4.bias"] == 0)  # untouched, as in the reference


def test_td3_learn_matches_reference(eng_mod, golden_dir):
    g = np.load(os.path.join(golden_dir, "td3_learn.npz"))
    params, data = D.make_params(D.PARAM_SEED), D.make_data(D.DATA_SEED)
    ring, exp, bc = device_tables(data)
    e = eng_mod.HirlEngine(batch=128, slope=0.01, use_bc=False)
    e.load_params(params["actor"], params["critic"])
    o = H.HirlOracle(params["actor"], params["critic"], None, slope=0.01, use_bc=False)
    for k in range(g["out"].shape[0]):
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, eng_mod)
        e.assemble(ring, torch.from_numpy(g["idx_buf"][k].astype(np.int32)).cuda())
        e.learn(noise=torch.from_numpy(g["noise"][k]).cuda())
        got = e.losses_host()
        rows = data["replay"][g["idx_buf"][k]]
        ref = oracle_learn_checked(eng_mod, e, o, ((rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]), None, g["noise"][k]),
                                   was_actor_call, f"td3 call {k} gradients")
        assert_losses(got[:2], ref[:2], f"td3 call {k} vs oracle")
        assert_losses(got[:2], g["out"][k], f"td3 call {k} vs reference golden")
        check_params(e, o, eng_mod, f"td3 call {k} params", was_actor_call)
        check_probes_free_running(e, eng_mod, g, k, f"td3 call {k}")


def test_learn_ragged_batches_and_outlier_rows(eng_mod):
    """Batch sizes other than 128 (multiples of 16), rows carrying the +600 kill bonus (100x TD errors), soft weight
    with warm-up: losses, gradients and stepped parameters match the oracle call by call."""
    params, data = D.make_params(11), D.make_data(12, outliers=True)
    ring, exp, bc = device_tables(data)
    rng = np.random.default_rng(1)
    for B in (16, 48, 256, 272, 512):
        e = eng_mod.HirlEngine(batch=B)
        e.load_params(params["actor"], params["critic"], params["bc_actor"])
        o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"])
        for k in range(4):
            idx = rng.integers(0, D.N_REPLAY, B).astype(np.int32)
            ibc = rng.integers(0, D.N_EXPERT, B).astype(np.int32)
            noise = rng.normal(0, 0.2, 4).astype(np.float32)
            was_actor_call = e.actor_trainable
            sync_oracle(o, e, eng_mod)
            e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
            e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=100, bc_warm_up_weight=0.1)
            rows = data["replay"][idx]
            ref = oracle_learn_checked(eng_mod, e, o, ((rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]),
                                                       (data["expert_s"][ibc], data["expert_a"][ibc]), noise, 100, 0.1),
                                       was_actor_call, f"B={B} call {k} gradients")
            assert_losses(e.losses_host(), ref, f"B={B} call {k}")
            check_params(e, o, eng_mod, f"B={B} call {k} params", was_actor_call)


T_PAST_2_32 = ((1 << 32) // 700 + 1) * 700 + 620  # the 64-bit counter past 2^32, congruent to 3 * 700 + 620 mod 700


@pytest.mark.parametrize("guard,tot", [(0, 700), (0, 431), (150, 3 * 700 + 620), (150, 400), (150, T_PAST_2_32), (0, T_PAST_2_32)])
def test_device_draw_is_uniform(eng_mod, guard, tot):
    """UniformMemory.sample is random.sample(population, batchSize) (hirl/utils/buffer.py:45): every slot of the population equally likely, no duplicates
    inside a minibatch.  test_device_sampler / test_guarded_draw_covers_its_population prove support and distinctness; this is the FREQUENCY: 4,000 draws
    of 128 from a 700-slot ring (full / part full; unguarded, and the front loop's guarded draw that leaves out the 150 slots behind the ring head).
    A slot's count over K draws is Binomial(K, 128/P) and the counts are exchangeable with sum 128 K, so (P-1)/P * sum (c - K p)^2 / (K p (1-p)) is
    chi-square with P - 1 degrees of freedom; the Philox streams are keyed by (seed, call), so the statistic is the same on every run — no flake.
    Position r of the minibatch must not prefer slots either (the LDS hash set resolves collisions by re-drawing): first and last position checked alone."""
    from scipy import stats

    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    cap, B, K = 700, 128, 4000
    rep = DeviceReplay(cap)
    rep.total.fill_(tot)
    e = eng_mod.HirlEngine(batch=B, use_bc=False)
    live = np.arange(min(tot, cap))
    pop = np.setdiff1d(live, (tot + np.arange(guard)) % cap)
    P = len(pop)
    counts = torch.zeros(cap, dtype=torch.int64, device="cuda")
    first, last = torch.zeros_like(counts), torch.zeros_like(counts)
    for call in range(1, K + 1):
        _lib.call("hx_sample_batch_guarded", rep.total.data_ptr(), cap, rep.ring.data_ptr(), None, 0, None, 0, B, B, 1, 12345, call, 0.2,
                  e._idx.data_ptr(), None, e._noise.data_ptr(), e.rows.data_ptr(), None, guard, _lib.stream_ptr())
        i = e._idx.to(torch.int64)
        counts += torch.bincount(i, minlength=cap)
        first[i[0]] += 1
        last[i[B - 1]] += 1
    c = counts.cpu().numpy()
    assert c.sum() == K * B and c[np.setdiff1d(np.arange(cap), pop)].sum() == 0  # nothing outside the population
    p = B / P
    chi = (P - 1) / P * (((c[pop] - K * p) ** 2).sum() / (K * p * (1 - p)))
    pv = stats.chi2.sf(chi, P - 1)
    assert 1e-3 < pv < 1 - 1e-3, (guard, tot, P, chi, pv)  # not too uneven — and not too even either (a permutation walk would be)
    for name, v in (("first", first), ("last", last)):
        f = v.cpu().numpy()[pop]
        chi1 = ((f - K / P) ** 2).sum() / (K / P)
        pv1 = stats.chi2.sf(chi1, P - 1)
        assert 1e-3 < pv1 < 1 - 1e-3, (name, guard, tot, chi1, pv1)


def test_device_sampler(eng_mod):
    """hx_sample_batch: indices inside the live part of each table, no duplicates inside a group (random.sample /
    np.random.choice(replace=False) semantics), deterministic per (seed, call), ring length read on the device, and the
    compact row tiles hold exactly the selected rows."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    e = eng_mod.HirlEngine(batch=128)
    rng = np.random.default_rng(0)
    rep = DeviceReplay(5000)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(5000, 32)).astype(np.float32)))
    rep.total += 300  # only 300 rows are live
    exp = DeviceReplay(210)
    exp.store_rows(torch.from_numpy(rng.normal(size=(200, 32)).astype(np.float32)))
    bc = torch.from_numpy(rng.normal(size=(150, 32)).astype(np.float32)).cuda()
    seen = []
    for call in range(50):
        idx, idx_bc, noise = e.sample(rep, exp, bc, n_main=96, seed=9)
        i, b, z = idx.cpu().numpy(), idx_bc.cpu().numpy(), noise.cpu().numpy()
        assert i[:96].min() >= 0 and i[:96].max() < 300 and len(set(i[:96])) == 96
        assert i[96:].min() >= 0 and i[96:].max() < 200 and len(set(i[96:])) == 32
        assert b.min() >= 0 and b.max() < 150 and len(set(b)) == 128  # 128 of 150 without replacement
        rows = e.rows.reshape(128, 32).cpu().numpy()
        np.testing.assert_array_equal(rows[:96], rep.ring.cpu().numpy()[i[:96]])
        np.testing.assert_array_equal(rows[96:], exp.ring.cpu().numpy()[i[96:]])
        np.testing.assert_array_equal(e.bc_rows.reshape(128, 32).cpu().numpy(), bc.cpu().numpy()[b])
        seen.append((i.copy(), z.copy()))
    assert not np.array_equal(seen[0][0], seen[1][0])
    zs = np.stack([z for _, z in seen])
    assert abs(zs.mean()) < 0.08 and abs(zs.std() - 0.2) < 0.05
    e2 = eng_mod.HirlEngine(batch=128)
    idx2, _, n2 = e2.sample(rep, exp, bc, n_main=96, seed=9)
    assert np.array_equal(idx2.cpu().numpy(), seen[0][0]) and np.array_equal(n2.cpu().numpy(), seen[0][1])
    rep.total += 100000  # ring wrapped: the whole capacity is live
    idx3, _, _ = e.sample(rep, exp, bc, n_main=128, seed=9)
    assert idx3.max().item() >= 300 and idx3.max().item() < 5000
    # large minibatches (one index stream at a time): 1,024 of 5,000 and 1,024 of 1,500 collide in the first round for certain
    big = eng_mod.HirlEngine(batch=1024)
    bc2 = torch.from_numpy(rng.normal(size=(1500, 32)).astype(np.float32)).cuda()
    for call in range(5):
        idx, idx_bc, _ = big.sample(rep, None, bc2, seed=3)
        i, b = idx.cpu().numpy(), idx_bc.cpu().numpy()
        assert len(set(i)) == 1024 and i.min() >= 0 and i.max() < 5000 and len(set(b)) == 1024 and b.max() < 1500
        np.testing.assert_array_equal(big.rows.reshape(1024, 32).cpu().numpy(), rep.ring.cpu().numpy()[i])


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("use_bc", [True, False])
def test_deferred_draw_is_bit_identical_to_the_sampling_launch(eng_mod, staged, use_bc):
    """sample(defer=True) + learn() (hx_hirl_learn_sampled / hx_hirl_critic_grads_sampled: the draw and the gather run inside the first
    launch of the update) against sample() + learn() (hx_sample_batch, then the update): the same indices, smoothing noise, row tiles,
    losses and — after 14 calls — the same networks and Adam moments, bit for bit.  The main ring has few live rows at first (many
    redraw rounds), then wraps; expert rows are mixed in; HIRL (BC minibatch) and TD3 (none)."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = D.make_params(31)
    rng = np.random.default_rng(7)
    rep = DeviceReplay(6000)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(6000, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()   # done flags
    rep.total += 140                                     # 96 of 140 without replacement: collisions in every round
    exp = DeviceReplay(64)
    exp.store_rows(torch.from_numpy(rng.normal(size=(40, 32)).astype(np.float32)))
    bc = torch.from_numpy(rng.normal(size=(150, 32)).astype(np.float32)).cuda() if use_bc else None
    engines = []
    for _ in range(2):
        e = eng_mod.HirlEngine(batch=128, use_bc=use_bc, slope=0.0 if use_bc else 0.01)
        e.staged = staged
        e.load_params(params["actor"], params["critic"], params["bc_actor"] if use_bc else None)
        engines.append(e)
    a, b = engines
    for k in range(14):
        if k == 7:
            rep.total += 100000  # wrapped: the whole capacity is live
        w = (100 if k % 4 == 0 else None) if use_bc else 0.0
        outs = []
        for e, defer in ((a, False), (b, True)):
            idx, idx_bc, noise = e.sample(rep, exp, bc, n_main=96, seed=11, defer=defer)
            e.learn(bc_weight_now=w, bc_warm_up_weight=0.05)
            outs.append((idx.clone(), idx_bc.clone(), noise.clone(), e.rows.clone(), e.bc_rows.clone(), e.losses_host()))
        for x, y, name in zip(outs[0][:5], outs[1][:5], ("idx", "idx_bc", "noise", "rows", "bc_rows")):
            if use_bc or name not in ("idx_bc", "bc_rows"):
                assert torch.equal(x, y), (k, name)
        np.testing.assert_allclose(outs[0][5], outs[1][5], rtol=1e-6, atol=1e-7, err_msg=f"call {k}")  # (loss sums: atomic order)
        i = outs[1][0].cpu().numpy()
        assert len(set(i[:96])) == 96 and len(set(i[96:])) == 32 and i[:96].max() < (140 if k < 7 else 6000) and i[96:].max() < 40
    for name in ("actor", "critic", "target_actor", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("batch", [256, 512])
def test_deferred_draw_at_other_batch_sizes(eng_mod, batch):
    """hx_hirl_learn_sampled at the largest batch whose draw still runs inside launch A (256) and at one that falls back to the sampling
    launch inside the same call (512): indices, tiles and the updated networks equal sample() + learn() bit for bit."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = D.make_params(33)
    rng = np.random.default_rng(batch)
    rep = DeviceReplay(9000)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(9000, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += 2 * batch
    exp = DeviceReplay(300)
    exp.store_rows(torch.from_numpy(rng.normal(size=(260, 32)).astype(np.float32)))
    bc = torch.from_numpy(rng.normal(size=(2 * batch, 32)).astype(np.float32)).cuda()
    a, b = (eng_mod.HirlEngine(batch=batch) for _ in range(2))
    for e in (a, b):
        e.load_params(params["actor"], params["critic"], params["bc_actor"])
    for k in range(6):
        outs = []
        for e, defer in ((a, False), (b, True)):
            idx, idx_bc, noise = e.sample(rep, exp, bc, n_main=batch - 32, seed=5, defer=defer)
            e.learn(bc_weight_now=100 if k % 2 == 0 else None, bc_warm_up_weight=0.1)
            outs.append((idx.clone(), idx_bc.clone(), noise.clone(), e.rows.clone(), e.bc_rows.clone()))
        for x, y, name in zip(outs[0], outs[1], ("idx", "idx_bc", "noise", "rows", "bc_rows")):
            assert torch.equal(x, y), (k, name)
    for name in ("actor", "critic", "target_actor", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_staged_path_equals_fused_path(eng_mod):
    """The stage-by-stage sequence a sharded run uses (critic_grads -> [all-reduce] -> adam -> actor_backward -> [all-reduce
    count] -> actor_wgrad -> [all-reduce] -> adam -> polyak) and the single-GPU one-call path (actor forwards folded into the
    first launch) are the same arithmetic: identical parameters after 12 calls."""
    params, data = D.make_params(21), D.make_data(22, outliers=True)
    ring, exp, bc = device_tables(data)
    rng = np.random.default_rng(5)
    engines = []
    for staged in (False, True):
        e = eng_mod.HirlEngine(batch=128)
        e.staged = staged
        e.load_params(params["actor"], params["critic"], params["bc_actor"])
        engines.append(e)
    for k in range(12):
        idx = rng.integers(0, D.N_REPLAY, 128).astype(np.int32)
        ibc = rng.integers(0, D.N_EXPERT, 128).astype(np.int32)
        noise = rng.normal(0, 0.2, 4).astype(np.float32)
        w = 100 if k % 4 == 0 else (None if k % 4 < 3 else 0.3)
        outs = []
        for e in engines:
            e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
            e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=w, bc_warm_up_weight=0.05)
            outs.append(e.losses_host())
        np.testing.assert_allclose(outs[0], outs[1], rtol=1e-6, atol=1e-7, err_msg=f"call {k}")
    a, b = engines
    for name in ("actor", "critic", "target_actor", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.update_count == 6 and b.update_count == 6


def test_bc_train_actor_matches_oracle_and_reference(eng_mod, golden_dir):
    """BC.Agent.train_actor through hx_bc_train_actor: loss, gradient and stepped actor call by call vs the oracle (from
    identical states) and the loss / probes vs the reference's recorded run."""
    g = np.load(os.path.join(golden_dir, "bc_train.npz"))
    params, data = D.make_params(D.PARAM_SEED), D.make_data(D.DATA_SEED)
    ring, exp, bc = device_tables(data)
    e = eng_mod.HirlEngine(batch=128, slope=0.01)
    e.load_params(params["actor"], params["critic"])
    o = H.HirlOracle(params["actor"], params["critic"], None, slope=0.01)
    for k in range(g["out"].shape[0]):
        idx = g["idx_bc"][k].astype(np.int32)
        sync_oracle(o, e, eng_mod)
        t = torch.from_numpy(idx).cuda()
        e.assemble(bc, t, bc_table=bc, idx_bc=t)
        e.bc_train_actor()
        got = e.losses_host()[2]
        ref = oracle_checked(o, lambda oo: H.bc_train_actor(oo, (data["expert_s"][idx], data["expert_a"][idx])),
                             [(e.grad_actor, "actor", eng_mod.ACTOR_LAYOUT)], f"bc call {k} actor grad")
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6, err_msg=f"bc call {k} vs oracle")
        np.testing.assert_allclose(got, g["out"][k], rtol=2e-5, atol=1e-6, err_msg=f"bc call {k} vs reference golden")
        f = e.actor.cpu().numpy()
        for kk, off, shp in eng_mod.ACTOR_LAYOUT:  # the stepped actor: every entry within its gradient-resolved bound (check_params)
            gk = np.abs(o.last_grads["actor"][kk].numpy().ravel())
            tol = GRAD_RTOL * gk + GRAD_ATOL_OF_MAX * max(gk.max(), 1e-30)
            d = np.abs(f[off:off + gk.size] - o.actor[kk].detach().numpy().ravel())
            assert (d <= 2e-6 + 2.1e-3 * np.minimum(1.0, 8.0 * tol / np.maximum(gk, 1e-30))).all(), (kk, d.max())
        s_, a_, v_ = D.net_probe(f)
        dv = np.abs(v_ - g["probe_val"][k])
        assert (dv > 2e-6).mean() <= 0.03 and dv.max() < 5e-5


@pytest.mark.parametrize("staged", [False, True])
def test_two_stream_issue_order_is_bit_identical_to_serial(staged):
    """bench.py --overlap issues the next act + env.step beside a critic-only learn() on a second stream
    (utils/pipeline.py).  Same reads and writes as the strict serial order of train_all.py:343-361: networks, Adam moments,
    env state, replay rows must come out bit for bit equal.  256 envs = one workgroup, so the replay insert order is fixed."""
    import bench

    def run(serial):
        # --separate-launches + 256 envs: ONE env workgroup, so the replay insert order is fixed
        args = bench.parse(["--envs", "256", "--separate-launches"] + (["--staged"] if staged else []) + ([] if serial else ["--overlap"]))
        loop = bench.Loop(args, 0, 1, torch.device("cuda", 0))
        assert loop.pipe.overlap == (not serial)
        for _ in range(61):
            loop.step()
        torch.cuda.synchronize()
        lo = (loop.eng.losses.data_ptr() - loop.eng.arena.data_ptr()) // 4
        arena = loop.eng.arena.clone()
        arena[lo:lo + 8] = 0  # logged loss sums: float atomics
        n = int(loop.replay.total.item())
        return arena.cpu(), loop.env.state.cpu().clone(), loop.replay.ring[:min(n, 1 << 16)].cpu().clone(), n, loop.pipe.issued

    a, b = run(True), run(False)
    assert not b[4] and a[3] == b[3] >= 61 * 200  # call 61 is an actor call: nothing of step 62 is in flight
    for x, y, name in zip(a[:3], b[:3], ("arena", "env state", "replay")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


@pytest.mark.parametrize("n", [83, 4096, 8192, 8192 + 40])  # 16-row tail, one round of 16-row / 32-row workgroups, the persistent kernel (hx_actp.hip)
def test_act_step_in_one_launch_equals_act_then_step(eng_mod, n):
    """hx_actor_act_step = hx_actor_act followed by hx_env_step, in the tail of the same kernel (16 or 32 envs per workgroup on
    the lanes of one wave): actions, state words, observations, rewards, masks, statistics and the replay rows must be
    identical — only the ORDER of the rows a step appends to the ring may differ (slots are handed out per workgroup)."""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    params = D.make_params(D.PARAM_SEED)
    engs, envs, reps = [], [], []
    for _ in range(2):
        e = eng_mod.HirlEngine(batch=128)
        e.load_params(params["actor"], params["critic"], params["bc_actor"])
        rep = DeviceReplay(1 << 19)
        env = BatchedHarfangEnv(n, scenario=np.arange(n) % 3, seed=3, max_step=9, auto_reset=True, random_reset=True, env_id0=100, replay=rep)
        env.reset()
        engs.append(e); envs.append(env); reps.append(rep)
    acts = torch.zeros((n, 4), device="cuda")
    for k in range(24):  # crosses the 9-step time limit twice: unstored steps, in-place resets
        engs[0].act(envs[0].obs, sigma=0.3, seed=5, row0=100, out=acts)
        envs[0].step(acts)
        a2 = engs[1].act_step(envs[1], sigma=0.3, seed=5)[0]
        assert torch.equal(acts, a2), f"actions, step {k}"
        for name in ("state", "obs", "reward", "done", "success", "episode_ctr"):
            x, y = getattr(envs[0], name), getattr(envs[1], name)
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{name}, step {k}"
        assert torch.equal(envs[0].stats.sum(0), envs[1].stats.sum(0)), f"stats, step {k}"  # (kept per way = workgroup % 32: the two launch shapes spread them differently)
    tot = int(reps[0].total.item())
    assert tot == int(reps[1].total.item()) == n * 24 - n * 2 and tot <= reps[0].capacity
    rows = [np.concatenate([r.ring[:tot].cpu().numpy(), r.success[:tot].cpu().numpy().astype(np.float32)[:, None]], 1) for r in reps]
    rows = [x[np.lexsort(x.T[::-1])] for x in rows]
    np.testing.assert_array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))
