"""GPU tests of gradient-norm clipping and the fixed entropy coefficient for SAC (hx_sac_grad_norm, hx_sac_adam_clipped, hx_sac_learn_weighted_clipped,
a NaN target entropy = HX_SAC_FIXED_ALPHA, through SacEngine, SacAgent and train_all).

The clip's arithmetic is the reference's (update_params, SAC/utils.py:15-21), restated over the SAC oracle by tests/_sac_clip.py and pinned on the CPU
against the reference's own run (tests/test_sac_clip_cpu.py); here the kernels are held to it at the bars of tests/test_sac_gpu.py.  Smallest shapes
that can still go wrong: minibatches of 16, 48 and 144 rows (one, an odd number of, and more than eight 16-row tiles); the norm kernel's shape does not
depend on the batch (its buffers are the networks')."""
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
from tests import _sac_clip as C  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402
from tests.test_sac_gpu import grad_bad, sync  # noqa: E402

STATE = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state")
NAMES = ("q1", "q2", "policy")


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


@pytest.fixture(scope="module")
def data():
    return D.make_data(D.DATA_SEED)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def new_engine(SE, B, params=None):
    params = sac_params() if params is None else params
    e = SE.SacEngine(batch=B)
    e.load_params(params["policy"], params["q1"], params["q2"])
    return e


def random_ring(seed=5, cap=4096):
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    rng = np.random.default_rng(seed)
    rep = DeviceReplay(cap)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(cap, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += cap
    return rep


def batch_of(rows):
    return rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]


# ---- the norm kernel and the clipped step alone ----------------------------------------------------------------------------------------------------

def live_mask(block, size):
    """the words a norm is taken over: W1, b1, W2, b2, W3, b3 — not the LayerNorm slots, not the padding"""
    m = np.zeros(size, bool)
    for slot in ("W1", "b1", "W2", "b2", "W3", "b3"):
        off, n = block[slot]
        m[off:off + n] = True
    return m


def segments(SE):
    """(name, slice of e.grad, live mask) of Q1, Q2 and the policy"""
    q, p = SE.Q_SIZE, SE.POLICY_SIZE
    return (("q1", slice(0, q), live_mask(SE.Q_BLOCK, q)), ("q2", slice(q, 2 * q), live_mask(SE.Q_BLOCK, q)),
            ("policy", slice(2 * q, 2 * q + p), live_mask(SE.POLICY_BLOCK, p)))


def norm_and_step(e, max_norm, step=1):
    """hx_sac_grad_norm + hx_sac_adam_clipped on whatever e.grad holds, both halves -> clip_ws on the host (norms, coefficients, partial sums)"""
    from hirl4ucav_amd import _lib

    nets, hyper, st, cw = ctypes.byref(e.nets), ctypes.byref(e.hyper), _lib.stream_ptr(), e.clip_ws.data_ptr()
    for which in (0, 1):
        _lib.call("hx_sac_grad_norm", nets, which, cw, st)
        _lib.call("hx_sac_adam_clipped", nets, hyper, which, step, 1.0, e.target_entropy, max_norm, cw, st)
    return e.clip_ws.cpu().numpy().copy()


def summation_depth():
    """roundings on the longest path of one segment's sum of squares, derived from the kernel's constants (hx_sac_clip_shape): the square; the float4's
    two-level tree; the thread's float4s one after the other; the tree over a wave's 64 lanes; the tree over the workgroup's waves; the tree over
    the partials one wave re-adds.  Every term is non-negative, so the computed sum is within depth * 2^-24 (relative) of the exact one — and the norm,
    its square root (half the relative error, plus the root's and the output's own roundings), well inside the same figure."""
    from hirl4ucav_amd import _lib

    shape = (ctypes.c_int32 * 6)()
    assert _lib.load().hx_sac_clip_shape(shape) == 0
    vecs, chunk, max_parts, nq, npi, depth = list(shape)
    threads = chunk // (4 * vecs)
    assert threads * 4 * vecs == chunk and threads % 64 == 0 and max_parts <= 64
    mine = 1 + 2 + (vecs - 1) + 6 + int(np.log2(threads // 64)) + int(np.ceil(np.log2(max_parts)))
    assert mine == depth, (mine, depth)
    return depth, chunk, (nq, npi)


def test_norm_kernel_against_float64_and_its_own_rounding_bound(SE):
    """Random gradients over five decades in the engine's real buffers: the three norms against float64 within depth * 2^-24 (relative), derived from
    the kernel's constants; max_norm = 1e30 gives coefficients of exactly 1; a binding max_norm gives max_norm / (norm + 1e-6)."""
    depth, chunk, (nq, npi) = summation_depth()
    assert nq == -(-SE.Q_SIZE // chunk) and npi == -(-SE.POLICY_SIZE // chunk)  # every word of a segment lies in one of its chunks
    e = new_engine(SE, 16)
    e.set_grad_clip(1e30)
    rng = np.random.default_rng(7)
    g = (rng.normal(size=e.grad.numel()) * 10.0 ** rng.uniform(-4, 1, e.grad.numel())).astype(np.float32)
    e.grad.copy_(torch.from_numpy(g))
    ws = norm_and_step(e, 1e30)
    exact = [np.sqrt((g[sl].astype(np.float64)[m] ** 2).sum()) for _, sl, m in segments(SE)]
    for i, (name, _, _) in enumerate(segments(SE)):
        err = abs(float(ws[i]) - exact[i]) / exact[i]
        print(f"{name}: norm {ws[i]:.6f}, float64 {exact[i]:.6f}, relative error {err:.2e} (bound {depth * 2.0 ** -24:.2e})")
        assert err <= depth * 2.0 ** -24
    assert (ws[3:6] == 1.0).all()
    for name in STATE:
        assert torch.isfinite(getattr(e, name)).all(), name
    c = float(min(exact)) / 2  # every network clips
    e.grad.copy_(torch.from_numpy(g))
    ws2 = norm_and_step(e, c, step=2)
    assert (ws2[:3] == ws[:3]).all()
    want = np.float32(c) / (ws2[:3] + np.float32(1e-6))
    np.testing.assert_allclose(ws2[3:6], want, rtol=2.0 ** -22, atol=0)  # a sum and a quotient in fp32
    assert (ws2[3:6] < 1.0).all()


def test_norm_ignores_layernorm_slots_and_padding_and_is_reproducible(SE):
    """Values planted in the LayerNorm slots the shared layout carries and in the padding behind each block leave norms AND partial sums bit for bit
    what they were; two runs on the same gradients give the same bits; an all-zero gradient gives norm 0, coefficient 1, no NaN and no step."""
    e = new_engine(SE, 16)
    e.set_grad_clip(1e30)
    rng = np.random.default_rng(8)
    g = rng.normal(size=e.grad.numel()).astype(np.float32)
    dead = np.concatenate([~m for _, _, m in segments(SE)])
    assert dead.sum() == 2 * (2 * 256 + 2 * 512 + 3) + (2 * 256 + 2 * 512)  # g1, be1, g2, be2 of three blocks; three padding words per Q block
    g[dead] = 0.0
    e.grad.copy_(torch.from_numpy(g))
    a = norm_and_step(e, 1e30)
    e.grad.copy_(torch.from_numpy(g))
    b = norm_and_step(e, 1e30, step=2)
    assert a.tobytes() == b.tobytes()
    planted = g.copy()
    planted[dead] = 1e3
    e.grad.copy_(torch.from_numpy(planted))
    c = norm_and_step(e, 1e30, step=3)
    assert a.tobytes() == c.tobytes()
    e.grad.zero_()
    z = norm_and_step(e, 0.5, step=4)
    assert (z[:3] == 0.0).all() and (z[3:6] == 1.0).all()
    for name in STATE:
        assert torch.isfinite(getattr(e, name)).all(), name
    # (Adam with g = 0 still moves a parameter by its decaying first moment: only a FRESH engine stands still)
    f = new_engine(SE, 16)
    f.set_grad_clip(0.5)
    p0, c0 = f.policy.clone(), f.critic.clone()
    z = norm_and_step(f, 0.5)
    assert (z[:3] == 0.0).all() and (z[3:6] == 1.0).all() and torch.equal(f.policy, p0) and torch.equal(f.critic, c0)


def format_engine(SE, fmt):
    from tests.test_sac_bf16_gpu import engine

    if fmt == "bf16":
        return engine(SE, "bf16", "bf16"), ("images",)
    if fmt == "bf16_policy":
        return engine(SE, "bf16", "f32"), ("w2_bf16", "w2_f32i")
    e = new_engine(SE, 128)
    if fmt == "x9":  # the exact-split acting images: built by the first large acting call, kept current by every policy step
        e.x9_rows = 16
        e.act(torch.zeros((16, 13), device="cuda"), explore=False)
        assert e.w2_x9 is not None
        return e, ("w2_x9", "w2_f32i")
    return e, ("w2_f32i",)


@pytest.mark.parametrize("fmt", ["f32", "x9", "bf16_policy", "bf16"])
def test_never_binding_clip_gives_hx_sac_adam_bits(SE, fmt):
    """max_norm = 1e30: the clipped sequence (gradients -> norm -> clipped step) against the unclipped staged one (gradients -> hx_sac_adam) after three
    calls — parameters, moments, the alpha state and every live image of W2 (fp32, exact split, bf16 acting, the bf16 update's block), bit for bit."""
    (a, images), (b, _) = format_engine(SE, fmt), format_engine(SE, fmt)
    a.separate_critic_adam = True
    b.set_grad_clip(1e30)
    rep = random_ring()
    for k in range(3):
        for e in (a, b):
            e.sample(rep, None, seed=11)
            e.learn()
    norms, coefs = b.grad_norms_host()
    assert coefs == (1.0, 1.0, 1.0) and all(n > 0 for n in norms)
    for name in STATE + images:
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert torch.equal(a.losses[3:6], b.losses[3:6])


def test_clipped_paths_give_the_parents_bits(SE, golden_dir):
    """hx_sac_learn_weighted_clipped, and the clipped staged sequence (gradients -> hx_sac_grad_norm -> hx_sac_adam_clipped) with entropy tuning and
    with a fixed alpha, from a fixed start (B = 48, four calls, a max_norm that clips 7 of the 8 critic steps and never the policy in the weighted run): the same
    bits as the recording made with the library of the commit before these paths were folded into the shared code
    (tests/golden/sac_fold_bits.npz, tests/_sac_fold_bits.py) — networks, moments, alpha state, acting image, the norms and coefficients of every call"""
    from tests import _sac_fold_bits

    _sac_fold_bits.assert_replays(SE, sac_params(), np.load(os.path.join(golden_dir, "sac_fold_bits.npz")), ("weighted_clipped", "clipped"))


# ---- learn() with a clip against the oracle --------------------------------------------------------------------------------------------------------

def unclipped_norms(SE, e, make_oracle, run):
    """the three norms an UNCLIPPED oracle call from the engine's present state would see (a throw-away oracle, synced to the engine)"""
    p = make_oracle()
    sync(p, e, SE)
    run(p)
    return [C.total_norm(p.last_grads[n]).item() for n in NAMES]


def engine_grads_bad(SE, e, k):
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
    return all_grads


def check_clip_outputs(e, o, k, what):
    norms, coefs = e.grad_norms_host()
    ref_n, ref_c = [o.last_norms[n] for n in NAMES], [o.last_coefs[n] for n in NAMES]
    print(f"{what} call {k}: norms {norms} (oracle {ref_n}), coefficients {coefs} (oracle {ref_c})")
    np.testing.assert_allclose(norms, ref_n, rtol=2e-5, err_msg=f"{what} call {k} norms")
    np.testing.assert_allclose(coefs, ref_c, rtol=2e-5, err_msg=f"{what} call {k} coefficients")
    assert [c == 1.0 for c in coefs] == [c == 1.0 for c in ref_c], (what, k, coefs, ref_c)


def check_params(SE, e, o, k, frac=2e-4):
    sd = e.state_dicts()
    for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
        d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
        assert (d > 2e-6).mean() < frac and d.max() <= 2.1e-3, f"call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"


def pick_max_norm(mode, norms):
    """from the oracle's own (unclipped) norms: under every norm, above every norm, or between the Q networks' and the policy's"""
    if mode == "all":
        return 0.5 * min(norms)
    if mode == "none":
        return 2.0 * max(norms)
    lo, hi = sorted((norms[2], min(norms[:2])))
    return float(np.sqrt(lo * hi))


@pytest.mark.parametrize("mode", ["all", "none", "between"])
@pytest.mark.parametrize("B", [16, 48, 144])
def test_clipped_learn_matches_oracle(SE, data, B, mode):
    """Three calls, the oracle synced before each as tests/test_sac_gpu.py does; max_norm per call from the oracle's own norms on the CPU.  Before the
    comparison the CLIPPED oracle's norms must all be at least 1 % away from max_norm (fp32 rounding cannot flip a decision then) and decide as the mode
    says.  Gradients (before clipping) by the elementwise rule, norms and coefficients at the losses' relative bar, losses and parameters at the bars of
    test_sac_learn_matches_oracle_and_reference.  mode none: bit-identical to the unclipped staged sequence run beside it."""
    from tests.test_hirl_gpu import oracle_checked

    params = sac_params()
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e = new_engine(SE, B, params)
    u = new_engine(SE, B, params)
    u.separate_critic_adam = True
    o = C.install_clip(S.SacOracle(params["policy"], params["q1"], params["q2"]), 1.0)
    rng = np.random.default_rng(100 + B)
    for k in range(3):
        idx = rng.choice(D.N_REPLAY, B, replace=False).astype(np.int32)
        eps = rng.normal(size=(2, B, 4)).astype(np.float32)
        rows = data["replay"][idx]
        run = lambda oo: oo.learn(batch_of(rows), eps[0], eps[1])  # noqa: E731
        sync(o, e, SE)
        c = pick_max_norm(mode, unclipped_norms(SE, e, lambda: S.SacOracle(params["policy"], params["q1"], params["q2"]), run))
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        for eng in (e, u):
            eng.assemble(ring, torch.from_numpy(idx).cuda())
            eng.learn(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda())
        got = e.losses_host()
        ref = oracle_checked(o, run, [(None, None, engine_grads_bad(SE, e, k))], f"clip {mode} B={B} call {k} gradients", module=S)
        for n in NAMES:  # first, on the oracle: no norm within 1 % of max_norm, and the decisions the mode asks for
            assert abs(o.last_norms[n] - c) >= 0.01 * c, (k, n, o.last_norms[n], c)
        clipped = [o.last_coefs[n] < 1.0 for n in NAMES]
        assert clipped == {"all": [True] * 3, "none": [False] * 3}.get(mode, clipped) and (mode != "between" or clipped[0] != clipped[2]), (mode, clipped)
        check_clip_outputs(e, o, k, f"clip {mode} B={B}")
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=f"clip {mode} B={B} call {k} vs oracle")
        check_params(SE, e, o, k)
        if mode == "none":
            for name in STATE + ("w2_f32i",):
                assert torch.equal(getattr(e, name), getattr(u, name)), (k, name)
    assert e.learning_steps == 3


# ---- the clip across the variants, batch 48 ---------------------------------------------------------------------------------------------------------

def test_clipped_bf16_update_matches_the_rounded_operand_oracle(SE, data):
    """bf16 update + clip, two calls at batch 48, every network clipping: the bars of tests/test_sac_bf16_gpu.py's learn() test."""
    from tests import test_sac_bf16_gpu as B16

    B = 48
    params = sac_params()
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e = SE.SacEngine(batch=B)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_act_dtype("bf16")
    e.set_update_dtype("bf16")
    o = C.install_clip(S.SacOracle(params["policy"], params["q1"], params["q2"]), 1.0)
    rng = np.random.default_rng(148)

    def masks():  # tests/test_sac_bf16_gpu.kernel_masks at this batch
        out = {}
        for i, k in enumerate([0, 4, 5, 2, 3, 1, 6, 7]):
            f = B16.slot(e, k, B=B)
            if k not in (0, 4, 5):
                out[2 * i] = f["h1"] > 0
            out[2 * i + 1] = f["z2"] > 0
        return out

    for k in range(2):
        idx = rng.choice(D.N_REPLAY, B, replace=False).astype(np.int32)
        eps = rng.normal(size=(2, B, 4)).astype(np.float32)
        rows = data["replay"][idx]
        run = lambda oo: oo.learn(batch_of(rows), eps[0], eps[1])  # noqa: E731
        sync(o, e, SE)
        c = 0.5 * min(unclipped_norms(SE, e, lambda: S.SacOracle(params["policy"], params["q1"], params["q2"]), run))
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        e.assemble(ring, torch.from_numpy(idx).cuda())
        e.learn(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda())
        got = e.losses_host()
        with B16.RoundedSac(masks()):
            ref = run(o)
        assert all(o.last_norms[n] >= 1.01 * c for n in NAMES), (o.last_norms, c)
        np.testing.assert_allclose(got, ref, rtol=B16.LOSS_RTOL, atol=B16.LOSS_ATOL, err_msg=f"bf16 clip call {k} losses")
        norms, coefs = e.grad_norms_host()
        print(f"bf16 clip call {k}: norms {norms} oracle {[o.last_norms[n] for n in NAMES]}")
        for i, n in enumerate(NAMES):
            # the gradient bar of the bf16 learn() test, |dg| <= a |g| + b max|g| per tensor (TIGHT), carried to the norm by the triangle inequality:
            # | |x| - |g| | <= |x - g| <= a |g| + b sqrt(sum over tensors of N_t max_t^2); the coefficient max_norm / (norm + 1e-6) moves by the same fraction
            gr = o.last_grads[n]
            bound = B16.TIGHT[0] * o.last_norms[n] + B16.TIGHT[1] * float(np.sqrt(sum(v.numel() * float(v.abs().max()) ** 2 for v in gr.values())))
            assert abs(norms[i] - o.last_norms[n]) <= bound, (k, n, norms[i], o.last_norms[n], bound)
            assert abs(coefs[i] - o.last_coefs[n]) <= o.last_coefs[n] * bound / o.last_norms[n] * 1.001 and coefs[i] < 1.0, (k, n, coefs[i], o.last_coefs[n])
        check_params(SE, e, o, k, frac=2e-3)
        B16.check_images(SE, e, f"bf16 clip call {k}")


def test_clipped_isac_matches_restatement(SE, data):
    """the imitative branch + clip (on the combined (1 - w) dL + w dL_bc), two calls at batch 48, against tests/_isac_check.IsacCheck behind the clip"""
    from tests import _isac_check as I
    from tests.test_hirl_gpu import oracle_checked

    B = 48
    params = I.isac_params(I.ISAC_SEED0)
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    table = torch.from_numpy(data["expert_rows"]).cuda().contiguous()
    e = new_engine(SE, B, params)
    e.set_imitative(params["bc_actor"], slope=0.01)
    make = lambda: I.IsacCheck(params["policy"], params["q1"], params["q2"], params["bc_actor"])  # noqa: E731
    o = C.install_clip(make(), 1.0)
    rng = np.random.default_rng(248)
    for k in range(2):
        idx = rng.choice(D.N_REPLAY, B, replace=False).astype(np.int32)
        ide = rng.choice(data["expert_rows"].shape[0], B, replace=False).astype(np.int32)
        eps = rng.normal(size=(2, B, 4)).astype(np.float32)
        rows, er = data["replay"][idx], data["expert_rows"][ide]
        run = lambda oo: oo.learn(batch_of(rows), eps[0], eps[1], (er[:, 0:13], er[:, 13:17]))  # noqa: E731
        sync(o, e, SE)
        c = 0.5 * min(unclipped_norms(SE, e, make, run))
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        e.assemble(ring, torch.from_numpy(idx).cuda())
        e.assemble_expert(table, torch.from_numpy(ide).cuda())
        e.learn(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda())
        got = np.asarray(e.losses_host() + e.imitative_losses_host())
        ref = np.asarray(oracle_checked(o, run, [(None, None, engine_grads_bad(SE, e, k))], f"isac clip call {k} gradients", module=S))
        assert all(o.last_norms[n] >= 1.01 * c for n in NAMES), (o.last_norms, c)
        check_clip_outputs(e, o, k, "isac clip")
        np.testing.assert_allclose(got[:6], ref[:6], rtol=2e-5, atol=5e-6, err_msg=f"isac clip call {k}")
        np.testing.assert_allclose(got[6:], ref[6:], rtol=2e-5, atol=0, err_msg=f"isac clip call {k} bc_loss / bc_weight")
        check_params(SE, e, o, k)


def test_clipped_weighted_learn_matches_checker(SE, data):
    """prioritized replay + clip (hx_sac_learn_weighted_clipped), two calls at batch 48, against tests/_per_check.WeightedSacOracle behind the clip; the
    log-alpha step stays its own launch and is not clipped"""
    from tests import _per_check as P
    from tests.test_hirl_gpu import oracle_checked
    from tests.test_per_gpu import weighted_engine

    B = 48
    params = sac_params()
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e, rep = weighted_engine(SE, params, B)
    make = lambda: P.WeightedSacOracle(params["policy"], params["q1"], params["q2"])  # noqa: E731
    o = C.install_clip(make(), 1.0)
    rng = np.random.default_rng(348)
    for k in range(2):
        idx = rng.choice(min(D.N_REPLAY, rep.capacity), B, replace=False).astype(np.int32)
        w = rng.uniform(0.05, 1.0, B).astype(np.float32)
        w[1], w[B - 2] = 0.0, 1.0
        eps = rng.normal(size=(2, B, 4)).astype(np.float32)
        rows = data["replay"][idx]
        run = lambda oo: oo.learn(batch_of(rows), eps[0], eps[1], w)  # noqa: E731
        sync(o, e, SE)
        c = 0.5 * min(unclipped_norms(SE, e, make, run))
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        e.assemble(ring, torch.from_numpy(idx).cuda())
        e._idx.copy_(torch.from_numpy(idx))
        e.per_weights.copy_(torch.from_numpy(w))
        e.learn(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda())
        got, err = e.losses_host(), e.per_errors.cpu().numpy()
        ref, ref_err = oracle_checked(o, run, [(None, None, engine_grads_bad(SE, e, k))], f"per clip call {k} gradients", module=S)
        assert all(o.last_norms[n] >= 1.01 * c for n in NAMES), (o.last_norms, c)
        check_clip_outputs(e, o, k, "per clip")
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=f"per clip call {k}")
        np.testing.assert_allclose(err, ref_err, rtol=2e-5, atol=5e-6, err_msg=f"per clip call {k} errors")
        check_params(SE, e, o, k)
        np.testing.assert_allclose(rep.prio[torch.from_numpy(idx.astype(np.int64)).cuda()].cpu().numpy(), (err.astype(np.float64) + 1e-4) ** 0.6, rtol=2e-5)


def front_side(SE, n=512, cap=2048, dtype="f32"):
    from tests.test_sac_front_small_gpu import make_side

    e, env, rep = make_side(SE, n, cap, dtype)
    e.act_step(env, seed=3)  # rows in the ring before the first draw
    return e, env, rep


def test_step_learn_with_a_clip_takes_the_reference_order(SE):
    """512 envs: step_learn under a clip == act_step, sample(defer), learn() under the same clip — the reference's order, no front tiles — bit for bit over
    three steps (ring slots are handed out by an atomic, so side b draws from side a's ring once both hold the same rows as a multiset); the minibatch
    sees this step's rows, which the front form's guard forbids; and its first env step leaves the env and the ring where the unclipped front loop's
    leaves them (the policy is the same until then)."""
    from tests.test_front_gpu import sorted_rows

    (a, env_a, rep_a), (b, env_b, rep_b), (c, env_c, rep_c) = front_side(SE), front_side(SE), front_side(SE)
    a.set_grad_clip(1.0)
    b.set_grad_clip(1.0)
    for k in range(3):
        tot0 = int(rep_a.total.item())
        out_a = a.step_learn(env_a, None, act_seed=3, sample_seed=11)
        out_b = b.act_step(env_b, seed=3)
        for x, y, name in zip(out_a, out_b, ("actions", "obs", "reward", "done", "success")):
            assert torch.equal(x, y), (k, name)
        assert torch.equal(env_a._state_store, env_b._state_store) and torch.equal(rep_a.total, rep_b.total), k
        np.testing.assert_array_equal(sorted_rows(rep_a), sorted_rows(rep_b), err_msg=f"step {k}: replay rows")
        rep_b.ring.copy_(rep_a.ring)
        b.sample(rep_b, None, seed=11, defer=True)
        b.learn()
        if k == 0:  # (the ring has not wrapped: slots from tot0 on are this step's rows — 128 draws out of 1,024 rows, half of them new)
            assert int((a._idx >= tot0).sum()) > 0 and int(a._idx.max()) < tot0 + 512
        assert torch.equal(a._idx, b._idx) and torch.equal(a.rows, b.rows), k
        for name in STATE + ("w2_f32i", "clip_ws"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        if k == 0:
            out_c = c.step_learn(env_c, None, act_seed=3, sample_seed=11)
            assert c._front_tiles is not None  # the unclipped engine did take the front form
            assert torch.equal(out_a[0], out_c[0]) and torch.equal(env_a._state_store, env_c._state_store) and torch.equal(rep_a.total, rep_c.total)
            np.testing.assert_array_equal(sorted_rows(rep_a), sorted_rows(rep_c))
            assert int(c._idx.max()) < tot0  # the front form drew before the insert
    assert a._front_tiles is None and a.learning_steps == 3
    norms, coefs = a.grad_norms_host()
    assert all(np.isfinite(norms)) and all(0 < x <= 1 for x in coefs)


# ---- the fixed entropy coefficient -------------------------------------------------------------------------------------------------------------------

def test_fixed_alpha_matches_reference_golden_and_oracle(SE, data, golden_dir):
    """SacAgent(entropy_tuning=False, ent_coef=0.2): the reference's six recorded calls (B = 128, the golden's batch) at the golden bars of
    tests/test_sac_gpu.py, and three calls at batch 48 against the oracle at that test's oracle bars; entropy_loss stays 0, alpha == ent_coef."""
    from tests.test_hirl_gpu import oracle_checked

    g = np.load(os.path.join(golden_dir, "sac_clip_learn.npz"))
    params = sac_params()
    assert D.checksum(params) == str(g["param_checksum"])
    x = float(g["ent_coef"])
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    for B, calls in ((128, g["fixed_out"].shape[0]), (48, 3)):
        e = new_engine(SE, B, params)
        e.set_entropy_tuning(False, x)
        alpha0 = e.alpha_state.clone()
        assert alpha0.tolist() == [0.0, 0.0, 0.0, float(np.float32(x))]
        o = C.install_fixed_alpha(S.SacOracle(params["policy"], params["q1"], params["q2"]), x)
        rng = np.random.default_rng(448)
        for k in range(calls):
            idx = g["fixed_idx"][k].astype(np.int32) if B == 128 else rng.choice(D.N_REPLAY, B, replace=False).astype(np.int32)
            eps = g["fixed_eps"][k] if B == 128 else rng.normal(size=(2, B, 4)).astype(np.float32)
            rows = data["replay"][idx]
            sync(o, e, SE)
            e.assemble(ring, torch.from_numpy(idx).cuda())
            e.learn(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda())
            got = e.losses_host()
            ref = oracle_checked(o, lambda oo: C.fixed_learn(oo, batch_of(rows), eps[0], eps[1]), [(None, None, engine_grads_bad(SE, e, k))],
                                 f"fixed alpha B={B} call {k} gradients", module=S)
            np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=f"fixed alpha B={B} call {k} vs oracle")
            assert got[3] == 0.0 and got[5] == float(np.float32(x)) and torch.equal(e.alpha_state, alpha0), (k, got, e.alpha_state.tolist())
            check_params(SE, e, o, k)
            if B == 128:
                others = [0, 1, 3, 4, 5]
                np.testing.assert_allclose(np.asarray(got)[others], g["fixed_out"][k][others], rtol=5e-5, atol=2e-5, err_msg=f"fixed alpha call {k} vs golden")
                np.testing.assert_allclose(got[2], g["fixed_out"][k][2], rtol=5e-5, atol=1e-4, err_msg=f"fixed alpha call {k} policy_loss vs golden")


def test_fixed_alpha_in_every_form(SE):
    """Three calls each: the one call, both staged forms (bit-identical to it), the clipped sequence, the imitative branch (one call and staged),
    prioritized replay, and the front launch at 512 envs in fp32 and bf16 — the alpha state's bits never change, entropy_loss stays 0 and
    losses[5] == ent_coef."""
    from tests.test_isac_gpu import bc_actor_params, make_rings
    from tests.test_per_gpu import weighted_engine

    x = 0.2
    want = [0.0, 0.0, 0.0, float(np.float32(x))]

    def check(e, what):
        assert e.alpha_state.tolist() == want, (what, e.alpha_state.tolist())
        v = e.losses.tolist()
        assert v[3] == 0.0 and v[5] == want[3], (what, v)
        for name in STATE:
            assert torch.isfinite(getattr(e, name)).all(), (what, name)

    rep, exp = make_rings()
    # plain: one call, staged policy, staged both halves, clipped
    plain = [new_engine(SE, 48) for _ in range(4)]
    plain[1].staged_policy = True
    plain[2].separate_critic_adam = True
    plain[3].set_grad_clip(1e30)
    for e in plain:
        e.set_entropy_tuning(False, x)
    for k in range(3):
        for e in plain:
            e.sample(rep, None, seed=11, defer=(k == 1))
            e.learn()
    for i, e in enumerate(plain):
        check(e, f"plain form {i}")
        for name in STATE + ("w2_f32i",):
            assert torch.equal(getattr(plain[0], name), getattr(e, name)), (i, name)  # one call == staged == never-binding clip, bit for bit
    # the policy moved, and not as under entropy tuning (alpha 0.2 instead of 1)
    tuned = new_engine(SE, 48)
    for k in range(3):
        tuned.sample(rep, None, seed=11, defer=(k == 1))
        tuned.learn()
    assert not torch.equal(tuned.policy, plain[0].policy) and tuned.alpha_state.tolist() != want
    # the imitative branch
    isac = [new_engine(SE, 48) for _ in range(2)]
    isac[1].staged_policy = True
    for e in isac:
        e.set_imitative(bc_actor_params(), slope=0.01)
        e.set_entropy_tuning(False, x)
    for k in range(3):
        for e in isac:
            e.sample(rep, None, seed=11)
            e.sample_expert(exp, seed=11)
            e.learn()
    for i, e in enumerate(isac):
        check(e, f"isac form {i}")
        for name in STATE:
            assert torch.equal(getattr(isac[0], name), getattr(e, name)), (i, name)
    # prioritized replay
    per, prep = weighted_engine(SE, sac_params(), 48)
    per.set_entropy_tuning(False, x)
    for k in range(3):
        per.sample(prep, seed=11)
        per.learn()
    check(per, "per")
    # the front launch, both acting kernels' formats
    for dtype in ("f32", "bf16"):
        e, env, _ = front_side(SE, dtype=dtype)
        e.set_entropy_tuning(False, x)
        for k in range(3):
            e.step_learn(env, None, act_seed=3, sample_seed=11)
        assert e._front_tiles is not None
        check(e, f"front {dtype}")
    # back to entropy tuning: alpha = exp(log_alpha) again, and the log-alpha step runs
    e = plain[0]
    e.set_entropy_tuning(True)
    assert e.alpha_state.tolist() == [0.0, 0.0, 0.0, 1.0]
    e.sample(rep, None, seed=11)
    e.learn()
    assert e.alpha_state[0].item() != 0.0 and e.losses[5].item() == e.alpha_state[3].item()


# ---- façade and driver -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"grad_clip": 1.0}, {"entropy_tuning": False, "ent_coef": 0.2}, {"grad_clip": 1.0, "entropy_tuning": False, "ent_coef": 0.3}],
                         ids=["grad_clip", "fixed_alpha", "both"])
def test_facade_takes_grad_clip_and_fixed_alpha(SE, tmp_path, kw):
    """SacAgent(grad_clip=1.0) and SacAgent(entropy_tuning=False, ent_coef=0.2) construct, learn and log"""
    from hirl4ucav_amd.agents.SAC.agent import SacAgent

    box = lambda n: types.SimpleNamespace(shape=(n,), sample=lambda: np.zeros(n, np.float32))  # noqa: E731
    ag = SacAgent(box(13), box(4), str(tmp_path / "log"), batch_size=16, lr=1e-3, hidden_units=[256, 512], memory_size=1000, log_interval=2, start_steps=0, **kw)
    logged = []
    ag.writer = types.SimpleNamespace(add_scalar=lambda tag, v, step: logged.append((tag, float(v), step)))
    rng = np.random.default_rng(2)
    np.random.seed(5)
    torch.manual_seed(5)
    for i in range(100):
        ag.memory.append(rng.uniform(-1, 1, 13), rng.uniform(-1, 1, 4), float(rng.uniform(-5, 0)), rng.uniform(-1, 1, 13), False, episode_done=False)
    policy0 = ag.eng.policy.clone()
    for _ in range(4):
        ag.learn(False)
    assert not torch.equal(policy0, ag.eng.policy)
    tags = [t for t, _, _ in logged]
    assert tags.count("loss/policy") == 2 and "loss/alpha" not in tags and all(np.isfinite(v) for _, v, _ in logged)
    if "grad_clip" in kw:
        norms, coefs = ag.eng.grad_norms_host()
        assert ag.eng.grad_clip == 1.0 and all(n > 0 for n in norms) and all(0 < c <= 1 for c in coefs)
        assert all(c == min(1.0, c) and abs(c - min(1.0, 1.0 / (n + 1e-6))) <= 1e-6 for n, c in zip(norms, coefs))
    else:
        assert ag.eng.grad_clip is None
    if "ent_coef" in kw:
        assert float(ag.alpha) == float(np.float32(kw["ent_coef"])) and ag.eng.alpha_state.tolist()[:3] == [0.0, 0.0, 0.0]
        assert [v for t, v, _ in logged if t == "stats/alpha"] == [float(np.float32(kw["ent_coef"]))] * 2
    else:
        assert float(ag.alpha) != 1.0 and ag.eng.alpha_state[0].item() != 0.0  # entropy tuning runs on (the log-alpha step is not clipped away)
    assert float(ag.explore(np.zeros(13, np.float32)).max()) <= 1.0


def test_train_all_with_grad_clip_and_fixed_alpha_and_resume(SE, tmp_path, monkeypatch, capsys):
    """--grad_clip 1.0 and --fixed_alpha 0.2 at a small size: each trains, says which loop runs, logs the norms; --resume continues and refuses a changed flag"""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.scalars import JsonlWriter

    monkeypatch.setattr(T, "make_writer", JsonlWriter)
    common = ["--agent", "SAC", "--type", "SAC", "--env", "serpentine", "--random", "--seed", "3", "--num_envs", "64", "--buffer_size", "4096", "--max_step", "24",
              "--checkpoint_rate", "1000", "--snapshot_every", "1"]
    run = T.main(T.parse_args(common + ["--grad_clip", "1.0", "--episodes", "1", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert "vector loop: reference order (--grad_clip" in out and "Episode 1:" in out
    sc = [json.loads(ln) for ln in open(os.path.join(run, "summary", "scalars.jsonl"))]
    for tag in ("stats/grad_norm_q1", "stats/grad_norm_q2", "stats/grad_norm_policy"):
        v = [s["value"] for s in sc if s["tag"] == tag]
        assert len(v) == 1 and np.isfinite(v[0]) and v[0] > 0, (tag, v)
    T.main(T.parse_args(common + ["--grad_clip", "1.0", "--episodes", "2", "--resume", run, "--result_dir", str(tmp_path / "b")]))
    assert "Episode 2:" in capsys.readouterr().out
    for changed in (["--grad_clip", "2.0"], [], ["--grad_clip", "1.0", "--fixed_alpha", "0.2"]):
        with pytest.raises(ValueError, match="--grad_clip|--fixed_alpha"):
            T.main(T.parse_args(common + changed + ["--episodes", "2", "--resume", run, "--result_dir", str(tmp_path / "c")]))
    capsys.readouterr()
    run = T.main(T.parse_args(common + ["--fixed_alpha", "0.2", "--episodes", "1", "--result_dir", str(tmp_path / "d")]))
    out = capsys.readouterr().out
    assert "vector loop: front launch" in out and "alpha 0.2000" in out
    T.main(T.parse_args(common + ["--fixed_alpha", "0.2", "--episodes", "2", "--resume", run, "--result_dir", str(tmp_path / "e")]))
    assert "alpha 0.2000" in capsys.readouterr().out
    with pytest.raises(ValueError, match="--fixed_alpha"):
        T.main(T.parse_args(common + ["--fixed_alpha", "0.3", "--episodes", "2", "--resume", run, "--result_dir", str(tmp_path / "f")]))
