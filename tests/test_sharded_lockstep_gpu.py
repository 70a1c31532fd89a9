"""The actor phase of a sharded HIRL run — hx_hirl_actor_wgrad_split (the merged message [dL_rl | dL_bc | count words]) and hx_adam_mixed (the weight from
the GLOBAL count, the mix, Adam, the target, every W2 image) — on ONE GPU in ONE process: tests/_sharded_lockstep.py holds W engines as virtual ranks
and issues the stages of HirlEngine._learn_staged in lockstep, the exchanges replaced by the exact rank-order fp32 sum or by the real transports in
their one-process form (tests/test_xchg_gpu.py).  The reference is one process (hirl/agents/HIRL.py:52): its counterpart here is ONE engine updating
the global batch, and the update oracle (oracle/hirl_oracle.py) for the two separate actor gradients."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _sharded_lockstep as LS  # noqa: E402
from tests import _xchg_model as X  # noqa: E402

BATCHES, WORLDS = (16, 48, 128), (2, 3, 8)
GRAD_RTOL, GRAD_ATOL_OF_MAX = 1e-4, 2e-5  # this project's gradient bar (tests/test_hirl_gpu.py): |dg| <= 1e-4 |g| + 2e-5 max|g| per tensor, EVERY entry


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


def call(name, *args):
    from hirl4ucav_amd import _lib

    _lib.call(name, *args, _lib.stream_ptr())


def draw(rng, W, B):
    return (rng.integers(0, D.N_REPLAY, (W, B)).astype(np.int32), rng.integers(0, D.N_EXPERT, (W, B)).astype(np.int32),
            rng.normal(0, 0.2, 4).astype(np.float32))


def bar_mismatch(got, ref, layout):
    """float64 [size] vs float64 [size] by tensor of `layout` -> [(key, n_bad, worst, max|g|)] of the tensors with ANY entry outside the gradient bar"""
    out = []
    for k, off, shp in layout:
        n = int(np.prod(shp))
        g, x = ref[off:off + n], got[off:off + n]
        bad = np.abs(x - g) > GRAD_RTOL * np.abs(g) + GRAD_ATOL_OF_MAX * max(np.abs(g).max(), 1e-30)
        if bad.any():
            out.append((k, int(bad.sum()), float(np.abs(x - g).max()), float(np.abs(g).max())))
    return out


# ---- (a) the driver is the product's sequence ---------------------------------------------------------------------------------------------------------
MODES = {"soft": ({}, lambda k: 100 if k == 0 else None, 0.05),        # HIRL soft: the weight estimated in call 0, stored afterwards
         "fixed": ({}, lambda k: 0.3, 0.0),                             # HIRL fixed
         "td3": ({"use_bc": False, "slope": 0.01}, lambda k: 0.0, 0.0),  # TD3.py: LeakyReLU, no BC
         "noln": ({"layer_norm": False}, lambda k: 100 if k == 0 else None, 0.05)}


def actor_loss_evaluations(losses, use_bc):
    """the bit patterns losses[1] may hold given losses[2] (bc), [3] (rl), [5] (w): rl for TD3 (TD3.py:236), else bc w + rl (1 - w) evaluated in fp32 —
    1 - w rounded, then both products rounded, or either one fused into the sum"""
    from fractions import Fraction as Fr

    f32 = np.float32
    if not use_bc:
        return {int(losses[3:4].view(np.uint32)[0])}
    bc, rl, w = f32(losses[2]), f32(losses[3]), f32(losses[5])
    omw = f32(f32(1.0) - w)
    exact = lambda x: Fr(float(x))  # noqa: E731
    forms = (LS.round_f32(exact(bc) * exact(w) + exact(f32(rl * omw))), LS.round_f32(exact(f32(bc * w)) + exact(rl) * exact(omw)),
             f32(f32(bc * w) + f32(rl * omw)))
    return {int(np.asarray([v], np.float32).view(np.uint32)[0]) for v in forms}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_one_virtual_rank_is_the_sharded_sequence_of_learn_in_bits(E, mode, bf16):
    """W = 1 in the driver against ONE engine with sharded_sequence = staged = True calling learn(): six calls, B = 16, 48, 128; after every call all five
    networks, the four moment buffers, wstate, every live W2 image and losses[5] equal in bits, losses[0, 2, 3, 4] at rtol 1e-6.
    losses[1] (the actor loss, bc_loss w + rl_loss (1 - w), HIRL.py:321; rl_loss for TD3) cannot be equal in bits between two runs: its inputs
    losses[2] and losses[3] are sums of float atomics over the workgroups, whose order the hardware picks (hx_bwd_body.h) — two runs of the SAME
    engine differ in their last bit.  What is exact is its relation to the engine's own words: on both engines losses[1] must be, in bits, an fp32
    evaluation of that formula from its own losses[2], losses[3] and losses[5] (fused on either product or on neither), and the two engines agree at
    the rtol of the inputs."""
    kw, weight, warm = MODES[mode]
    params, data = D.make_params(51), D.make_data(52, outliers=True)
    for B in BATCHES:
        ls = LS.Lockstep(E, 1, B, params, data, bf16=bf16, **kw)
        e = LS.make_engine(E, B, params, bf16=bf16, **kw)
        e.staged = e.sharded_sequence = True
        rng = np.random.default_rng([5, B])
        for k in range(6):
            idx, ibc, noise = draw(rng, 1, B)
            if e.use_bc:
                e.assemble(ls.ring, torch.from_numpy(idx[0]).cuda(), bc_table=ls.bc, idx_bc=torch.from_numpy(ibc[0]).cuda())
            else:
                e.assemble(ls.ring, torch.from_numpy(idx[0]).cuda())
            e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=weight(k), bc_warm_up_weight=warm)
            ls.learn([(idx[0], ibc[0])], noise, weight(k), warm)
            what = (mode, bf16, B, "call", k)
            LS.assert_same_state(ls.engines[0], e, what)
            got, ref = ls.engines[0].losses.cpu().numpy(), e.losses.cpu().numpy()
            assert got[5:6].view(np.uint32)[0] == ref[5:6].view(np.uint32)[0], (what, got, ref)
            np.testing.assert_allclose(got[[0, 1, 2, 3, 4]], ref[[0, 1, 2, 3, 4]], rtol=1e-6, err_msg=str(what))
            for v in (got, ref):
                if ls.was_actor_call:
                    assert v[1:2].view(np.uint32)[0] in actor_loss_evaluations(v, e.use_bc), (what, v)
        assert e.critic_step == 6 and e.actor_step == 3 and e.update_count == 3  # (the third actor call moved the targets)
        assert np.all(ls.actor_msgs[:, ls.n:].cpu().numpy() == LS.GUARD_VALUE)


# ---- (b) the split message --------------------------------------------------------------------------------------------------------------------------
def split_oracle_run(data, idx, ibc, noise, use_bc):
    """run(o): one call of the oracle up to the actor's gradients, which it keeps SEPARATE — the critic step, then grad of -Q1(s, pi(s)).mean() ("rl") and of
    mse(pi(s_bc), a_bc) 10000 ("bc") with the updated critic, as tests/test_distributed_cpu._shard_grads forms them"""
    F = torch.nn.functional

    def run(o):
        rows = data["replay"][idx]
        s, a, ns, r, d = (torch.tensor(x) for x in (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]))
        with torch.no_grad():
            na = (H.actor_forward(o.target_actor, ns, o.slope) + torch.tensor(noise).clamp(-0.5, 0.5)).clamp(-1, 1)
            q1t, q2t = H.critic_forward(o.target_critic, ns, na, o.slope)
            y = r.reshape(-1, 1) + 0.99 * torch.min(q1t, q2t) * (1 - d).reshape(-1, 1)
        q1, q2 = H.critic_forward(o.critic, s, a, o.slope)
        keys = list(o.critic)
        grads = dict(zip(keys, H._grads(F.mse_loss(q1, y) + F.mse_loss(q2, y), o.critic, keys)))
        o.last_grads["critic"] = {k: g.clone() for k, g in grads.items()}
        o.opt_critic.step(o.critic, grads)  # the actor phase sees the UPDATED critic (HIRL.py:288 precedes :296)
        akeys = list(o.actor)
        rl_q = H.critic_q1(o.critic, s, H.actor_forward(o.actor, s, o.slope), o.slope)
        o.last_grads["rl"] = dict(zip(akeys, H._grads(-rl_q.mean(), o.actor, akeys)))
        if use_bc:
            bs, ba = torch.tensor(data["expert_s"][ibc]), torch.tensor(data["expert_a"][ibc])
            o.last_grads["bc"] = dict(zip(akeys, H._grads(F.mse_loss(H.actor_forward(o.actor, bs, o.slope), ba) * 10000.0, o.actor, akeys)))

    return run


@pytest.mark.parametrize("B", BATCHES)
def test_split_message_holds_the_two_gradients_and_the_count_words(E, B):
    """One actor call from fresh parameters.  msg[0:P] and msg[P:2P] meet the gradient bar against the oracle's separate gradients (fragile ReLU units by
    tests/test_hirl_gpu.oracle_checked); tail word 0 = float(soft_count), words 1..7 its base-32 digits, words 8..63 zero in a zeroed buffer and NOT
    written (a sentinel survives a second launch); the 64 guard floats and grad_actor — which this launch must not write — keep their sentinels; an
    int32 written into e.soft_count arrives as that float and those digits."""
    from tests.test_hirl_gpu import oracle_checked

    params, data = D.make_params(53), D.make_data(54, outliers=True)
    ls = LS.Lockstep(E, 1, B, params, data)
    e, P = ls.engines[0], (E.ACTOR_SIZE + 3) & ~3
    e.grad_actor.fill_(-5.0)
    idx, ibc, noise = draw(np.random.default_rng([6, B]), 1, B)
    seen = []
    ls.learn([(idx[0], ibc[0])], noise, 100, 0.05, before_message=lambda r, eng: seen.append(int(eng.soft_count.item())))
    assert ls.was_actor_call and len(seen) == 1 and 0 <= seen[0] <= B
    msg = ls.actor_msgs[0].clone()
    o = H.HirlOracle(params["actor"], params["critic"], params["bc_actor"])
    oracle_checked(o, split_oracle_run(data, idx[0], ibc[0], noise, True),
                   [(ls.critic_sum, "critic", E.CRITIC_LAYOUT), (msg[0:P], "rl", E.ACTOR_LAYOUT), (msg[P:2 * P], "bc", E.ACTOR_LAYOUT)], f"B={B} split message")
    host = msg.cpu().numpy()
    assert np.all(host[E.ACTOR_SIZE:P] == 0) and np.all(host[P + E.ACTOR_SIZE:2 * P] == 0)  # (the padding words, if the layout ever has any)
    assert np.array_equal(host[2 * P:2 * P + 8], LS.count_words(seen[0])), (host[2 * P:2 * P + 8], seen[0])
    assert host[2 * P] == float(seen[0]) and np.all(host[2 * P + 8:ls.n] == 0)
    assert np.all(host[ls.n:] == LS.GUARD_VALUE)
    assert torch.all(e.grad_actor == -5.0)
    # an int32 of the caller's choice: it arrives as that float, and as digits that rebuild it; the rest of the tail is not written
    for c in (777, 1023, 0, (1 << 31) - 1):
        e.soft_count[0] = c
        ls.actor_msgs[0, 2 * P + 8:ls.n] = -3.0
        e._stage_actor_message(ls.actor_msgs[0, :ls.n])
        host = ls.actor_msgs[0].cpu().numpy()
        assert host[2 * P] == np.float32(c) and np.array_equal(host[2 * P:2 * P + 8], LS.count_words(c)) and LS.count_from_words(host[2 * P:]) == c
        assert np.all(host[2 * P + 8:ls.n] == -3.0) and np.all(host[ls.n:] == LS.GUARD_VALUE)
    assert torch.all(e.grad_actor == -5.0)


def test_split_message_of_td3_writes_the_rl_half_and_zero_count_words(E):
    """use_bc = 0 (include/hirl4ucav.h, hx_hirl_actor_wgrad_split): dL_rl and the eight count words (all 0) are written; the dL_bc half, the rest of the
    tail, the guard floats and grad_actor keep what they held."""
    from tests.test_hirl_gpu import oracle_checked

    B = 48
    params, data = D.make_params(55), D.make_data(56, outliers=True)
    ls = LS.Lockstep(E, 1, B, params, data, use_bc=False, slope=0.01)
    e, P = ls.engines[0], (E.ACTOR_SIZE + 3) & ~3
    e.grad_actor.fill_(-5.0)
    ls.actor_msgs[0, P:ls.n] = -3.0
    idx, ibc, noise = draw(np.random.default_rng(7), 1, B)
    ls.learn([(idx[0], None)], noise)
    msg = ls.actor_msgs[0].clone()
    o = H.HirlOracle(params["actor"], params["critic"], None, slope=0.01, use_bc=False)
    oracle_checked(o, split_oracle_run(data, idx[0], None, noise, False), [(ls.critic_sum, "critic", E.CRITIC_LAYOUT), (msg[0:P], "rl", E.ACTOR_LAYOUT)],
                   "TD3 split message")
    host = msg.cpu().numpy()
    assert np.all(host[P:2 * P] == -3.0) and np.all(host[2 * P:2 * P + 8] == 0) and np.all(host[2 * P + 8:ls.n] == -3.0)
    assert np.all(host[ls.n:] == LS.GUARD_VALUE) and torch.all(e.grad_actor == -5.0)


# ---- (c) hx_adam_mixed, exact edges -------------------------------------------------------------------------------------------------------------------
CONFIGS = {"f32": {}, "act-bf16": {"act": "bf16"}, "act-x9": {"act": "f32x9"}, "update-bf16": {"bf16": True}, "td3": {"use_bc": False, "slope": 0.01}}


def config_engine(E, params, cfg):
    cfg = dict(cfg)
    act = cfg.pop("act", None)
    e = LS.make_engine(E, 16, params, **cfg)
    if act:
        e.set_act_dtype(act)
    return e


def randomize(engines, seed, wstate):
    """the same random actor, moments (v >= 0), target and loss words into every engine; images rebuilt"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = engines[0].actor.numel()
    p, t, m = (torch.randn(n, generator=g, device="cuda") * s for s in (0.1, 0.1, 1e-3))
    v = (torch.randn(n, generator=g, device="cuda") * 1e-3) ** 2
    losses = torch.randn(8, generator=g, device="cuda")
    for e in engines:
        for dst, src in ((e.actor, p), (e.target_actor, t), (e.m_actor, m), (e.v_actor, v), (e.losses, losses)):
            dst.copy_(src)
        e.wstate.fill_(wstate)
        e.refresh_bf16()


def synthetic_message(n, P, seed, counts):
    """[a | b | the summed count words of per-rank counts `counts`] with random halves -> (device message [n], a, b as device tensors)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    msg = torch.zeros(n, dtype=torch.float32, device="cuda")
    msg[:2 * P] = torch.randn(2 * P, generator=g, device="cuda") * 1e-2
    words = X.rank_order_sum(np.stack([LS.count_words(c) for c in counts]))
    msg[2 * P:2 * P + 8] = torch.from_numpy(words).cuda()
    return msg, msg[:P], msg[P:2 * P]


def split_count(count, W):
    """W per-rank counts that add up to `count`"""
    return [count // W + (1 if r < count % W else 0) for r in range(W)]


EDGES = [  # name, w_kind, w_given, warm, count (of the global batch BW), stored weight, which half IS the gradient
    ("count 0, warm 0: w = 0", 1, 0.0, 0.0, lambda BW: 0, 0.5, "a"),
    ("count = BW: w = 1", 1, 0.0, 0.0, lambda BW: BW, 0.5, "b"),
    ("count = BW - 1, warm 0.05: clipped to 1", 1, 0.0, 0.05, lambda BW: BW - 1, 0.5, "b"),
    ("given 0", 0, 0.0, 0.05, lambda BW: 7, 0.5, "a"),
    ("given 1", 0, 1.0, 0.05, lambda BW: 7, 0.5, "b"),
    ("stored 0", 2, 0.3, 0.05, lambda BW: 7, 0.0, "a"),
    ("stored 1", 2, 0.3, 0.05, lambda BW: 7, 1.0, "b"),
]


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c != "td3"])
def test_adam_mixed_at_weights_0_and_1_equals_adam_on_that_half_in_bits(E, cfg):
    """w = 0 makes the mixed gradient dL_rl exactly, w = 1 dL_bc exactly: hx_adam_mixed must then leave the bits hx_adam(which = 1) leaves on a second engine
    whose grad_actor holds that half — p, m, v, the target (Polyak on and off), every live W2 image (fp32 image; bf16 image; the three exact-split parts;
    the ten images of the bf16 update), wstate, losses[1] and losses[5] — for every B x W of the suite."""
    params = D.make_params(57)
    a_eng, b_eng = config_engine(E, params, CONFIGS[cfg]), config_engine(E, params, CONFIGS[cfg])
    P, n = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL
    case = 0
    for B in BATCHES:
        for W in WORLDS:
            BW = B * W
            for name, w_kind, w_given, warm, count, stored, half in EDGES:
                for polyak in (0, 1):
                    case += 1
                    c = count(BW)
                    randomize([a_eng, b_eng], case, stored)
                    msg, ga, gb = synthetic_message(n, P, 1000 + case, split_count(c, W))
                    call("hx_adam_mixed", ctypes.byref(a_eng.nets), ctypes.byref(a_eng.hyper), polyak, 3, 1.0 / W, w_kind, w_given, warm, BW, msg.data_ptr())
                    b_eng.grad_actor.copy_((ga if half == "a" else gb)[:E.ACTOR_SIZE])
                    b_eng.soft_count[0] = c
                    call("hx_adam", ctypes.byref(b_eng.nets), ctypes.byref(b_eng.hyper), 1 | (16 if polyak else 0), 3, 1.0 / W, w_kind, w_given, warm, BW)
                    what = (cfg, B, W, name, "polyak", polyak)
                    LS.assert_same_state(a_eng, b_eng, what)
                    la, lb = a_eng.losses.cpu().numpy(), b_eng.losses.cpu().numpy()
                    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (what, la, lb)
                    assert la[5] == (0.0 if half == "a" else 1.0) and float(a_eng.wstate.item()) == la[5], (what, la)


def test_adam_mixed_of_td3_steps_on_the_rl_half_and_leaves_wstate(E):
    params = D.make_params(57)
    a_eng, b_eng = config_engine(E, params, CONFIGS["td3"]), config_engine(E, params, CONFIGS["td3"])
    P, n = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL
    for polyak in (0, 1):
        randomize([a_eng, b_eng], 70 + polyak, 0.625)
        msg, ga, _ = synthetic_message(n, P, 80 + polyak, [5, 6])
        msg[P:] = float("nan")  # neither the dL_bc half nor the tail is read
        call("hx_adam_mixed", ctypes.byref(a_eng.nets), ctypes.byref(a_eng.hyper), polyak, 3, 0.5, 1, 0.0, 0.05, 96, msg.data_ptr())
        b_eng.grad_actor.copy_(ga[:E.ACTOR_SIZE])
        call("hx_adam", ctypes.byref(b_eng.nets), ctypes.byref(b_eng.hyper), 1 | (16 if polyak else 0), 3, 0.5, 1, 0.0, 0.05, 96)
        LS.assert_same_state(a_eng, b_eng, ("td3", polyak))
        la, lb = a_eng.losses.cpu().numpy(), b_eng.losses.cpu().numpy()
        assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and la[1] == la[3]  # TD3.py:236
        assert float(a_eng.wstate.item()) == 0.625 and bool(torch.isfinite(a_eng.actor).all())


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_adam_mixed_behind_a_failed_exchange_changes_nothing(E, cfg):
    """HxNets.xchg_status pointing at a non-zero word: no parameter, moment, target, image, wstate or loss word changes"""
    params = D.make_params(57)
    e = config_engine(E, params, CONFIGS[cfg])
    P, n = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL
    randomize([e], 90, 0.25)
    before = {k: t.clone() for k, t in LS.state_tensors(e).items()}
    losses = e.losses.clone()
    word = torch.ones(16, dtype=torch.int32, device="cuda")
    msg, _, _ = synthetic_message(n, P, 91, [40, 41])
    e.nets.xchg_status = word.data_ptr()
    try:
        call("hx_adam_mixed", ctypes.byref(e.nets), ctypes.byref(e.hyper), 1, 3, 0.5, 1, 0.0, 0.05, 96, msg.data_ptr())
        torch.cuda.synchronize()
    finally:
        e.nets.xchg_status = None
    after = LS.state_tensors(e)
    assert not [k for k in before if not LS.bits_equal(before[k], after[k])] and LS.bits_equal(losses, e.losses)
    call("hx_adam_mixed", ctypes.byref(e.nets), ctypes.byref(e.hyper), 1, 3, 0.5, 1, 0.0, 0.05, 96, msg.data_ptr())  # (and with the word gone the same call steps)
    assert not LS.bits_equal(before["actor"], e.actor)


# ---- (d) hx_adam_mixed, interior weights against float64 ---------------------------------------------------------------------------------------------
U = 2.0 ** -24  # unit roundoff of one correctly rounded fp32 operation; the two hardware operations (sqrt, reciprocal) are within 1 ulp <= 2 U relative


def adam_mixed_reference(a, b, p, m, v, w, gs, step, lr=1e-3):
    """float64 (g = (w b + (1 - w) a) gs, then Adam with the host's fp32 step_size and bc2_sqrt) -> (p', m', v') and the bounds (e_p, e_m, e_v) on what
    the fp32 kernel may differ by: see test_adam_mixed_interior_weights_against_float64"""
    a, b, p, m, v = (np.asarray(x, np.float64) for x in (a, b, p, m, v))
    w, gs = float(np.float32(w)), float(np.float32(gs))
    b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
    c1, c2 = float(np.float32(1.0) - np.float32(0.9)), float(np.float32(1.0) - np.float32(0.999))  # exact in fp32 (Sterbenz)
    ss = float(np.float32(lr / (1.0 - 0.9 ** step)))           # set_adam_scalars: formed in double, rounded once
    bc2s = float(np.float32(np.sqrt(1.0 - 0.999 ** step)))
    omw = 1.0 - w
    S = np.abs(w * b) + np.abs(omw * a)
    mix = w * b + omw * a
    e_mix = 3 * U * S * (1 + 3 * U)                            # 1 - w, (1 - w) a, w b, the sum: each term meets at most three roundings
    g = mix * gs
    e_g = gs * e_mix + U * (np.abs(g) + gs * e_mix)            # ... times grad_scale: one rounding
    mb, vb = np.abs(m * b1), np.abs(v * b2)
    m2 = g * c1 + m * b1
    e_m = c1 * e_g + U * mb + U * (np.abs(m2) + c1 * e_g + U * mb)            # RN(m b1), then ONE fma
    gg = g * g
    e_gg = 2 * np.abs(g) * e_g + e_g ** 2
    e_gg = e_gg + U * (gg + e_gg)                                              # RN(g g)
    v2 = gg * c2 + v * b2
    e_v = c2 * e_gg + U * vb + U * (v2 + c2 * e_gg + U * vb)                  # RN(v b2), then ONE fma
    sq = np.sqrt(v2)
    e_sq = (sq - np.sqrt(np.maximum(v2 - e_v, 0.0))) + 2 * U * (2 * sq)        # the input's error through the (concave) root + 1 ulp of the hardware sqrt
    rc = 1.0 / bc2s
    e_rc = 2 * U * rc                                                          # 1 ulp of the hardware reciprocal
    A = sq * rc
    e_A = e_sq * rc + sq * e_rc + e_sq * e_rc
    e_A = e_A + U * (A + e_A)                                                  # RN(sqrt * rcp)
    den = A + eps
    e_den = e_A + U * (den + e_A)                                              # RN(... + eps)
    assert np.all(den > 2 * e_den)
    r = 1.0 / den
    e_r = (1.0 / (den - e_den) - r) + 2 * U / (den - e_den)                    # the input's error + 1 ulp of the hardware reciprocal
    q = m2 * r
    e_q = e_m * r + np.abs(m2) * e_r + e_m * e_r
    e_q = e_q + U * (np.abs(q) + e_q)                                          # RN(m rcp)
    t = ss * q
    e_t = ss * e_q + U * (np.abs(t) + ss * e_q)                                # RN(step_size ...)
    p2 = p - t
    e_p = e_t + U * (np.abs(p2) + e_t)                                         # RN(p - ...)
    return (p2, m2, v2), (e_p, e_m, e_v)


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_mixed_interior_weights_against_float64(E, step):
    """Counts 1, 255, 257, 511, 513, 1023 of a global batch of 1,024 (the counts around the powers of two where a rounded count word would show), grad_scale
    1/2, 1/3, 1/8, warm 0 and 5e-4, Adam steps 1 and 1000: p, m, v against float64, and w — losses[5] — in bits.

    w: the kernels form fma(float32(count), float32(1/1024), warm), ONE rounding (the one-GPU path's count * inv_batch + warm compiles to a fused
    multiply-add, and the sharded path must give the same bits as the one-GPU path); LS.soft_weight_f32 rounds the exact value once.

    The tolerance is TWICE the following bound, U = 2^-24 the unit roundoff of a correctly rounded fp32 operation, first and second order terms kept
    (adam_mixed_reference computes it per element in float64; w itself is exact, see above).
      mix   t = w b + (1 - w) a: at most three roundings on either term (1 - w; the product; the sum — fewer where the compiler fuses):
            e_mix = 3 U (|w b| + |(1 - w) a|)
      g     = RN(mix gs):                          e_g = gs e_mix + U |g|
      m'    = fma(g, 1 - b1, RN(m b1)):            e_m = (1 - b1) e_g + U |m b1| + U |m'|        (1 - b1, 1 - b2 are exact in fp32)
      v'    = fma(RN(g g), 1 - b2, RN(v b2)):      e_v = (1 - b2) (2 |g| e_g + U g^2) + U |v b2| + U v'
      den   = RN(RN(sqrt(v') rcp(bc2_sqrt)) + eps), sqrt and rcp the two hardware operations of 1 ulp (2 U relative):
            e_sq = sqrt(v') - sqrt(v' - e_v) + 2 U sqrt(v'),  e_A = e_sq / bc2_sqrt + (2 U + U) A,  e_den = e_A + U den
      p'    = RN(p - RN(step_size RN(m' rcp(den)))), rcp again within 1 ulp:
            e_r = 1 / (den - e_den) - 1 / den + 2 U / den,  e_q = e_m / den + |m'| e_r + U |q|,  e_p = step_size e_q + U |t| + U |p'|
    step_size and bc2_sqrt are the host's fp32 values (hx_update.h set_adam_scalars: formed in double, rounded once) in the kernel and in the reference."""
    params = D.make_params(58)
    e = config_engine(E, params, CONFIGS["f32"])
    P, n, N, BW = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL, E.ACTOR_SIZE, 1024
    case = 0
    for count in (1, 255, 257, 511, 513, 1023):
        for W in (2, 3, 8):
            for warm in (0.0, 5e-4):
                case += 1
                randomize([e], 100 + case, 0.5)
                p0, m0, v0 = (t.cpu().numpy() for t in (e.actor, e.m_actor, e.v_actor))
                msg, ga, gb = synthetic_message(n, P, 200 + case, split_count(count, W))
                call("hx_adam_mixed", ctypes.byref(e.nets), ctypes.byref(e.hyper), 0, step, 1.0 / W, 1, 0.0, warm, BW, msg.data_ptr())
                what = ("count", count, "W", W, "warm", warm, "step", step)
                w_ref = LS.soft_weight_f32(count, BW, warm)
                w_got = e.losses[5:6].cpu().numpy()
                assert w_got.view(np.uint32)[0] == np.asarray([w_ref], np.float32).view(np.uint32)[0] and 0 < w_ref < 1, (what, w_got, w_ref)
                assert float(e.wstate.item()) == float(w_ref)
                (p_ref, m_ref, v_ref), (e_p, e_m, e_v) = adam_mixed_reference(ga.cpu().numpy()[:N], gb.cpu().numpy()[:N], p0, m0, v0, w_ref, np.float32(1.0 / W), step)
                for name, got, ref, bound in (("m", e.m_actor, m_ref, e_m), ("v", e.v_actor, v_ref, e_v), ("p", e.actor, p_ref, e_p)):
                    d = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                    print(what, name, "worst |d| / bound", float((d / bound).max()))
                    assert np.all(d <= 2 * bound), (what, name, int((d > 2 * bound).sum()), float((d / bound).max()))


# ---- (e) shards against the global batch, at gradient level ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("W", WORLDS)
def test_shards_equal_the_global_batch_at_gradient_level(E, W, B):
    """W lockstep ranks of B rows against ONE engine of B W rows fed the concatenated minibatches, networks and moments synchronised before each of 4
    calls (soft weight estimated in every actor call, warm-up 0.05, outlier rows).  In EVERY entry the summed critic message / W meets the gradient bar
    against the global grad_critic, and so does the mixed actor gradient — recomputed on the host in float64 from the summed message and w — against
    the global grad_actor; the summed count (from the ranks' soft_count words AND as rebuilt from the message's digit words) equals the global
    engine's as integers; losses[5] is equal in bits; the replicas stay bit-identical.  Fixed seeds, no escape clause."""
    params, data = D.make_params(41), D.make_data(42, outliers=True)
    ls = LS.Lockstep(E, W, B, params, data)
    g = LS.make_engine(E, B * W, params)
    P = (E.ACTOR_SIZE + 3) & ~3
    rng = np.random.default_rng([8, W, B])
    for k in range(4):
        LS.copy_state(g, ls.engines[0])
        idx, ibc, noise = draw(rng, W, B)
        g.assemble(ls.ring, torch.from_numpy(idx.reshape(-1)).cuda(), bc_table=ls.bc, idx_bc=torch.from_numpy(ibc.reshape(-1)).cuda())
        g.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=100, bc_warm_up_weight=0.05)
        counts = []
        ls.learn([(idx[r], ibc[r]) for r in range(W)], noise, 100, 0.05, before_message=lambda r, e: counts.append(int(e.soft_count.item())))
        what = ("W", W, "B", B, "call", k)
        for r in range(1, W):
            LS.assert_same_state(ls.engines[r], ls.engines[0], what + ("replica", r))
        bad = bar_mismatch(ls.critic_sum.cpu().numpy().astype(np.float64) / W, g.grad_critic.cpu().numpy().astype(np.float64), E.CRITIC_LAYOUT)
        assert not bad, (what, "critic", bad)
        if not ls.was_actor_call:
            continue
        msg = ls.actor_sum.cpu().numpy()
        assert len(counts) == W and sum(counts) == int(g.soft_count.item()) == LS.count_from_words(msg[2 * P:]), (what, counts, int(g.soft_count.item()))
        w_l, w_g = ls.engines[0].losses[5:6].cpu().numpy(), g.losses[5:6].cpu().numpy()
        assert w_l.view(np.uint32)[0] == w_g.view(np.uint32)[0] and w_l[0] == LS.soft_weight_f32(sum(counts), B * W, 0.05), (what, w_l, w_g)
        w, m64 = float(w_l[0]), msg.astype(np.float64)
        mixed = (w * m64[P:2 * P] + (1.0 - w) * m64[0:P]) / W
        bad = bar_mismatch(mixed, g.grad_actor.cpu().numpy().astype(np.float64), E.ACTOR_LAYOUT)
        assert not bad, (what, "actor", bad)


# ---- (f) real messages through the real transports ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranks():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.test_xchg_gpu import Ranks

    r = Ranks()
    yield r
    r.free()


ODD_COUNTS = {3: (171, 170, 172), 8: (120, 127, 1, 128, 77, 64, 33, 15)}  # sums 513 and 565: odd and above 512 (bf16 keeps 8 bits: steps of 4 there)


@pytest.mark.parametrize("W", [3, 8])
def test_real_actor_messages_through_the_transports_keep_the_count_exact(E, ranks, W):
    """The W ranks' actor messages of one lockstep call (B = 128), their soft_count words set so that the global count is odd and above 512, through
    hx_allreduce_oneshot, twostage and twostage-bf16 in the one-process form of tests/test_xchg_gpu.py: the fp32 transports return the rank-order sum in
    bits, twostage-bf16 its round-to-nearest-even bf16 image (Case.check_dst, every word), and on EVERY rank and variant hx_adam_mixed reads the exact
    global count out of what arrived."""
    from tests.test_xchg_gpu import run_case

    assert sum(ODD_COUNTS[W]) % 2 == 1 and sum(ODD_COUNTS[W]) > 512
    B = 128
    params, data = D.make_params(41), D.make_data(42, outliers=True)
    ls = LS.Lockstep(E, W, B, params, data)
    idx, ibc, noise = draw(np.random.default_rng([9, W]), W, B)

    def set_count(r, e):
        e.soft_count[0] = ODD_COUNTS[W][r]

    ls.learn([(idx[r], ibc[r]) for r in range(W)], noise, 100, 0.0, before_message=set_count)
    host = ls.actor_msgs[:, :ls.n].cpu().numpy()
    P = (E.ACTOR_SIZE + 3) & ~3
    assert LS.count_from_words(ls.actor_sum.cpu().numpy()[2 * P:]) == sum(ODD_COUNTS[W])
    assert float(ls.engines[0].losses[5].item()) == float(LS.soft_weight_f32(sum(ODD_COUNTS[W]), B * W, 0.0))
    reader = ls.engines[0]  # (its actor is stepped by every reading: nothing compares it afterwards)
    for variant in ("oneshot", "twostage", "twostage-bf16"):
        c = run_case(ranks, variant, W, ls.n, None, messages=host)
        for r in range(W):
            got = LS.count_read_by_adam_mixed(reader, c.dst[r, :ls.n])
            assert got == sum(ODD_COUNTS[W]), (variant, "rank", r, "hx_adam_mixed read", got, "the global count is", sum(ODD_COUNTS[W]))


# ---- (g) RcclDirect(bf16=True) at world 1 -------------------------------------------------------------------------------------------------------------
def test_rccl_bf16_keeps_a_count_of_1023_exact(E):
    """A real actor message whose count is 1023 (bf16 rounds that WORD to 1024) through RcclDirect(bf16=True) with one rank: what hx_adam_mixed reads from
    the message afterwards is 1023, and the gradient words are the bf16 images of what was sent.  (Two real devices are beyond a one-GPU box: at world
    > 1 the bf16 sums of the digit words stay exact by tests/test_sharded_lockstep_cpu.py.)"""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents.exchange import RcclDirect

    try:
        RcclDirect.available()
    except _lib.HxError as e:
        print("hx_rccl_available:", e)
        pytest.skip(f"RCCL cannot be bound in this process: {e}")
    B = 128
    params, data = D.make_params(41), D.make_data(42, outliers=True)
    ls = LS.Lockstep(E, 1, B, params, data)
    idx, ibc, noise = draw(np.random.default_rng(10), 1, B)

    def set_count(r, e):
        e.soft_count[0] = 1023

    ls.learn([(idx[0], ibc[0])], noise, 100, 0.0, before_message=set_count)
    sent = ls.actor_msgs[0, :ls.n].cpu().numpy()
    comm = RcclDirect(RcclDirect.make_id(), 1, 0, bf16=True)
    try:
        t = comm.allreduce(ls.actor_msgs[0, :ls.n])
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert X.same(got, X.to_bf16_rne(sent)).all() and np.all(ls.actor_msgs[0, ls.n:].cpu().numpy() == LS.GUARD_VALUE)
        P = (E.ACTOR_SIZE + 3) & ~3
        assert got[2 * P] == 1024.0  # (the count WORD is rounded, which is why nothing computes with it)
        assert LS.count_read_by_adam_mixed(ls.engines[0], t) == 1023
    finally:
        comm.close()
