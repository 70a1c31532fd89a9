"""Gradient-norm clipping for HIRL and TD3 on the GPU (hx_hirl_clip.hip: hx_hirl_grad_norm, hx_adam_clipped; HirlEngine.set_grad_clip; train_all
--hirl_grad_clip): torch.nn.utils.clip_grad_norm_ once per optimizer — both Q heads and their LayerNorms under ONE norm, the whole actor — in front of the
optimizer step of every staged form of the update.  The reference's HIRL.py / TD3.py have no clip; the rule is tests/_hirl_clip's (CPU-pinned against
clip_grad_norm_ itself by tests/test_hirl_clip_cpu.py).

Bounds, none of them taken from what the kernels give (U = 2^-24, the unit roundoff of one fp32 operation):
  norms against float64     |norm - norm64| <= depth U norm64.  The sum of squares is a tree of non-negative terms `depth` operations deep (square, float4
                            tree, the thread's sequence, three reduction trees; + 1 for the critic's head 0 + head 1), each rounding at most U relative: the
                            sum is within depth U (1 + O(U)); the square root halves that and adds its own U — below depth U for depth >= 2.  `depth` is
                            re-derived here from the shape words of hx_hirl_clip_shape and compared with the library's own.
  message form, interior w  the same, plus the mix's two roundings per element — the product w b and the fused multiply-add —, each at most U of
                            |w b| + |(1 - w) a|: the mixed vector is within 2 U M of the exact one in 2-norm, M = || |w b| + |(1 - w) a| ||, and so is its norm.
  against the oracle        tests/test_hirl_gpu.py's bars, unchanged: losses rtol 2e-5, gradients |dg| <= 1e-4 |g| + 2e-5 max|g| (fragile ReLU units by
                            oracle_checked), parameters by check_params.  The norm follows from the gradient bar: | ||x|| - ||g|| | <= ||x - g||.
  bf16                      tests/test_bf16_update_gpu.py's bars against the rounded-operand oracle, unchanged.
  never-binding clip        bit for bit (coef == 1.0f multiplies exactly).  Logged loss words that are sums of float atomics keep rtol 1e-6 / atol 1e-7,
                            the one tolerance tests/test_hirl_gpu.py::test_staged_path_equals_fused_path already has for them."""
import copy
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_clip as C  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _sharded_lockstep as LS  # noqa: E402

U = 2.0 ** -24
NEW_CALLS = ("hx_hirl_grad_norm", "hx_adam_clipped", "hx_hirl_clip_floats", "hx_hirl_clip_shape")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


@pytest.fixture(scope="module")
def shape(E):
    """hx_hirl_clip_shape's eight words, the depth re-derived from the shape: (vecs, chunk, max parts, chunks Q, chunks actor, depth critic, depth actor,
    first partial word)"""
    from hirl4ucav_amd import _lib

    s = (ctypes.c_int32 * 8)()
    _lib.call("hx_hirl_clip_shape", s)
    vecs, chunk, parts, nq, na, dc, da, lo = list(s)
    assert chunk == 4096 and chunk == 256 * 4 * vecs and parts == 64
    assert nq == -(-E.Q_PADDED // chunk) <= parts and na == -(-E.ACTOR_SIZE // chunk) <= parts
    depth = 1 + 2 + (vecs - 1) + 6 + 2 + int(np.log2(parts))  # square, (x + y) + (z + w), the thread's vecs terms, 64 lanes, 4 waves, <= 64 partials
    assert (dc, da) == (depth + 1, depth) and int(_lib.load().hx_hirl_clip_floats()) == lo + 3 * parts
    return list(s)


def call(name, *args):
    from hirl4ucav_amd import _lib

    _lib.call(name, *args, _lib.stream_ptr())


def grad_norm(e, which, w_kind=0, w_given=0.0, warm=0.0, batch=None, msg=None, ws=None):
    call("hx_hirl_grad_norm", ctypes.byref(e.nets), ctypes.byref(e.hyper), which, w_kind, w_given, warm, e.batch if batch is None else batch,
         None if msg is None else msg.data_ptr(), (e.clip_ws if ws is None else ws).data_ptr())


def clipped_step(e, which, max_norm, step=3, scale=1.0, w_kind=0, w_given=0.0, warm=0.0, batch=None, msg=None):
    call("hx_adam_clipped", ctypes.byref(e.nets), ctypes.byref(e.hyper), which, step, scale, w_kind, w_given, warm, e.batch if batch is None else batch,
         None if msg is None else msg.data_ptr(), max_norm, e.clip_ws.data_ptr())


def norm_of(e, which, **kw):
    """the norm as the library forms it: the norm launch, then a clipped step that never binds (it STEPS the network: throwaway engines) -> fp32 norm"""
    grad_norm(e, which, **kw)
    clipped_step(e, which, 1e30, **kw)
    norms, coefs = e.grad_norms_host()
    assert coefs[which] == 1.0
    return norms[which]


def parts_of(e, shape, which):
    """the partial sums of optimizer `which`, bits: the critic's two heads or the actor's"""
    lo, p = shape[7], shape[2]
    ws = e.clip_ws.cpu().numpy().view(np.uint32)
    if which == 0:
        return np.concatenate([ws[lo:lo + shape[3]], ws[lo + p:lo + p + shape[3]]])
    return ws[lo + 2 * p:lo + 2 * p + shape[4]].copy()


def fresh(E, batch=16, grad_clip=1.0, **kw):
    e = LS.make_engine(E, batch, D.make_params(57), **kw)
    if grad_clip is not None:
        e.set_grad_clip(grad_clip)
    return e


def five_decades(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, generator=g, device="cuda") * 10.0 ** (torch.rand(n, generator=g, device="cuda") * 5.0 - 3.0)


# ---- (a) the norms against float64 -----------------------------------------------------------------------------------------------------------------
def test_norms_against_float64(E, shape):
    e = fresh(E)
    e.grad.copy_(five_decades(e.grad.numel(), 1))
    pad = torch.from_numpy(C.padding_words(E)).cuda()
    assert pad.numel() == 6  # three words behind each Q head's 138,241
    e.grad_critic[pad] = 0.0
    got, parts = {}, {}
    for which, layout, depth in ((0, E.CRITIC_LAYOUT, shape[5]), (1, E.ACTOR_LAYOUT, shape[6])):
        flat = (e.grad_critic if which == 0 else e.grad_actor).cpu().numpy()
        live = C.live_words(E, which)
        ref = C.norm64(flat, live)
        got[which] = norm_of(e, which)
        parts[which] = parts_of(e, shape, which)
        print(f"which {which}: norm {got[which]!r} float64 {ref!r} relative error {abs(got[which] - ref) / ref:.3e} bound {depth * U:.3e}")
        assert abs(got[which] - ref) <= depth * U * ref, (which, got[which], ref)
        # the LayerNorm words count: without them the norm is another number altogether
        no_ln = C.norm64(flat, np.setdiff1d(live, C.layernorm_words(layout)))
        assert abs(got[which] - no_ln) > 100 * depth * U * ref, (which, no_ln, ref)
    # padding words never count: 1e3 planted there moves neither the partials nor the norms, in bits
    e.grad_critic[pad] = 1e3
    assert np.float32(norm_of(e, 0)).view(np.uint32) == np.float32(got[0]).view(np.uint32) and np.array_equal(parts_of(e, shape, 0), parts[0])
    # two runs give the same bits (no atomics, one fixed order) — every word of the workspace
    first = e.clip_ws.clone()
    for which in (0, 1):
        norm_of(e, which)
    assert LS.bits_equal(first, e.clip_ws)


def test_zero_gradient_gives_norm_0_coefficient_1_and_a_fresh_engine_stands_still(E):
    e = fresh(E, grad_clip=0.5)
    e.clip_ws.fill_(7.0)
    before = {k: t.clone() for k, t in LS.state_tensors(e).items()}
    for which in (0, 1):
        grad_norm(e, which)
        clipped_step(e, which, 0.5, step=1)
    assert e.grad_norms_host() == ((0.0, 0.0), (1.0, 1.0))
    after = LS.state_tensors(e)
    assert not [k for k in before if k != "wstate" and not LS.bits_equal(before[k], after[k])]  # Adam on g = 0 from zero moments moves nothing


# ---- (b) the message form --------------------------------------------------------------------------------------------------------------------------
def test_message_form_at_weights_0_and_1_is_the_local_form_on_that_half_in_bits(E, shape):
    """w = 0 makes the mixed gradient dL_rl exactly, w = 1 dL_bc exactly: partials, norm, coefficient and the clipped step (a BINDING max_norm) are then
    those of the local form on a second engine whose grad_actor holds that half — every state tensor in bits"""
    from tests.test_sharded_lockstep_gpu import EDGES, randomize, split_count, synthetic_message

    a_eng, b_eng = fresh(E), fresh(E)
    P, n = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL
    for case, (name, w_kind, w_given, warm, count, stored, half) in enumerate(EDGES):
        W, BW, polyak = 2 + case % 2, 16 * (2 + case % 2), case % 2
        c = count(BW)
        randomize([a_eng, b_eng], case, stored)
        msg, ga, gb = synthetic_message(n, P, 1000 + case, split_count(c, W))
        kw = dict(w_kind=w_kind, w_given=w_given, warm=warm, batch=BW)
        grad_norm(a_eng, 1, msg=msg, **kw)
        clipped_step(a_eng, 1 | (16 if polyak else 0), 0.25, scale=1.0 / W, msg=msg, **kw)
        b_eng.grad_actor.copy_((ga if half == "a" else gb)[:E.ACTOR_SIZE])
        b_eng.soft_count[0] = c
        grad_norm(b_eng, 1, **kw)
        clipped_step(b_eng, 1 | (16 if polyak else 0), 0.25, scale=1.0 / W, **kw)
        what = (name, "W", W, "polyak", polyak)
        assert np.array_equal(parts_of(a_eng, shape, 1), parts_of(b_eng, shape, 1)), what
        assert LS.bits_equal(a_eng.clip_ws[:4], b_eng.clip_ws[:4]) and a_eng.grad_norms_host()[1][1] < 1.0, (what, a_eng.grad_norms_host())
        LS.assert_same_state(a_eng, b_eng, what)
        la, lb = a_eng.losses.cpu().numpy(), b_eng.losses.cpu().numpy()
        assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and la[5] == (0.0 if half == "a" else 1.0), (what, la, lb)


@pytest.mark.parametrize("w_kind,w_given,count", [(0, 0.3, 7), (0, 0.75, 7), (1, 0.0, 13), (2, 0.0, 7)])
def test_message_form_interior_weights_against_float64(E, shape, w_kind, w_given, count):
    from tests.test_sharded_lockstep_gpu import randomize, split_count, synthetic_message

    e = fresh(E)
    P, n, W, BW = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL, 2, 32
    randomize([e], 11, 0.625)
    msg, ga, gb = synthetic_message(n, P, 12, split_count(count, W))
    msg[:2 * P] = five_decades(2 * P, 13)
    a, b = ga.cpu().numpy().astype(np.float64), gb.cpu().numpy().astype(np.float64)
    kw = dict(w_kind=w_kind, w_given=w_given, warm=0.05, batch=BW, msg=msg)
    grad_norm(e, 1, **kw)
    clipped_step(e, 1, 1e30, scale=1.0 / W, **kw)
    got = e.grad_norms_host()[0][1]
    w = np.float32(e.losses[5].item())  # the weight the step formed: given, LS.soft_weight_f32 of the summed digits, or the stored one
    assert w == {0: np.float32(w_given), 1: LS.soft_weight_f32(count, BW, 0.05), 2: np.float32(0.625)}[w_kind] and 0.0 < w < 1.0
    omw = np.float32(1.0) - w  # (the kernels' own 1 - w: an fp32 number the reference takes as it is)
    live = C.live_words(E, 1)
    ref = C.norm64(float(w) * b + float(omw) * a, live) / W
    M = C.norm64(np.abs(float(w) * b) + np.abs(float(omw) * a), live) / W
    bound = shape[6] * U * ref + 2 * U * M
    print(f"w {w!r}: norm {got!r} float64 {ref!r} |d| {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound * (1 + 1e-3), (got, ref, bound)


def test_td3_reads_the_rl_half_of_the_message_alone(E, shape):
    from tests.test_sharded_lockstep_gpu import randomize, synthetic_message

    a_eng, b_eng = (fresh(E, use_bc=False, slope=0.01) for _ in range(2))
    P, n = (E.ACTOR_SIZE + 3) & ~3, 2 * ((E.ACTOR_SIZE + 3) & ~3) + LS.TAIL
    randomize([a_eng, b_eng], 70, 0.625)
    msg, ga, _ = synthetic_message(n, P, 80, [5, 6])
    msg[P:] = float("nan")  # neither the dL_bc half nor the tail is read
    kw = dict(w_kind=1, warm=0.05, batch=96)
    grad_norm(a_eng, 1, msg=msg, **kw)
    clipped_step(a_eng, 1 | 16, 0.25, scale=0.5, msg=msg, **kw)
    b_eng.grad_actor.copy_(ga[:E.ACTOR_SIZE])
    grad_norm(b_eng, 1, **kw)
    clipped_step(b_eng, 1 | 16, 0.25, scale=0.5, **kw)
    assert np.array_equal(parts_of(a_eng, shape, 1), parts_of(b_eng, shape, 1)) and LS.bits_equal(a_eng.clip_ws[:4], b_eng.clip_ws[:4])
    norm = a_eng.grad_norms_host()[0][1]
    ref = C.norm64(ga.cpu().numpy(), C.live_words(E, 1)) * 0.5
    assert np.isfinite(norm) and abs(norm - ref) <= shape[6] * U * ref and a_eng.grad_norms_host()[1][1] < 1.0
    LS.assert_same_state(a_eng, b_eng, "td3")
    assert float(a_eng.wstate.item()) == 0.625 and bool(torch.isfinite(a_eng.actor).all())


# ---- (c) a clip that never binds leaves the unclipped bits --------------------------------------------------------------------------------------------
CONFIGS = {"f32": {}, "act-x9": {"act": "f32x9"}, "bf16": {"bf16": True}, "noln": {"layer_norm": False}, "td3": {"use_bc": False, "slope": 0.01}}


def config_engine(E, B, params, cfg):
    cfg = dict(cfg)
    act = cfg.pop("act", None)
    e = LS.make_engine(E, B, params, **cfg)
    if act:
        e.set_act_dtype(act)
    e.target_update_freq = 2  # (the third call's actor step carries the soft_update: + 16)
    return e


def three_calls(E, engines, B, seed):
    data = D.make_data(22, outliers=True)
    ring, bc = LS.tables(data)
    rng = np.random.default_rng(seed)
    for k in range(3):
        idx, ibc = rng.integers(0, D.N_REPLAY, B).astype(np.int32), rng.integers(0, D.N_EXPERT, B).astype(np.int32)
        noise = torch.from_numpy(rng.normal(0, 0.2, 4).astype(np.float32)).cuda()
        outs = []
        for e in engines:
            if e.use_bc:
                e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
            else:
                e.assemble(ring, torch.from_numpy(idx).cuda())
            e.learn(noise=noise, bc_weight_now=(100 if k == 0 else None) if e.use_bc else 0.0, bc_warm_up_weight=0.05)
            outs.append(e.losses.cpu().numpy())
        yield k, outs


@pytest.mark.parametrize("cfg,message", [(c, False) for c in CONFIGS] + [(c, True) for c in ("f32", "bf16", "td3")])
def test_a_clip_that_never_binds_leaves_the_unclipped_bits(E, cfg, message):
    """max_norm 1e30 against the unclipped staged path (message form: against hx_adam_mixed, both engines in the sharded sequence), three calls: parameters,
    moments, targets, wstate and every live W2 image in bits after each; losses[5] in bits, the loss words that are sums of float atomics to 1e-6"""
    params = D.make_params(21)
    a, b = config_engine(E, 48, params, CONFIGS[cfg]), config_engine(E, 48, params, CONFIGS[cfg])
    a.set_grad_clip(1e30)
    b.staged = True
    a.sharded_sequence = b.sharded_sequence = message
    for k, (la, lb) in three_calls(E, [a, b], 48, 5):
        LS.assert_same_state(a, b, (cfg, message, "call", k))
        assert la[5].view(np.uint32) == lb[5].view(np.uint32), (k, la, lb)
        np.testing.assert_allclose(la[:6], lb[:6], rtol=1e-6, atol=1e-7, err_msg=f"call {k}")
    assert a.update_count == 2 and a.grad_norms_host()[1] == (1.0, 1.0) and min(a.grad_norms_host()[0]) > 0.0


# ---- (d) clipped learn() against the oracle ----------------------------------------------------------------------------------------------------------
def norm_bar(grads):
    """what the gradient bar |dg| <= 1e-4 |g| + 2e-5 max|g| (per tensor, every entry) allows the 2-norm to differ by: || tol ||"""
    from tests.test_hirl_gpu import GRAD_ATOL_OF_MAX, GRAD_RTOL

    t2 = 0.0
    for g in grads.values():
        x = np.abs(g.numpy().astype(np.float64)).ravel()
        t2 += ((GRAD_RTOL * x + GRAD_ATOL_OF_MAX * x.max()) ** 2).sum()
    return float(np.sqrt(t2))


@pytest.mark.parametrize("mode", ["all", "none", "between"])
@pytest.mark.parametrize("B", [16, 48, 144])
def test_clipped_learn_matches_the_oracle(E, shape, B, mode):
    """Four calls from synchronised states (HIRL soft with warm-up, outlier rows): max_norm from the oracle's OWN unclipped norms of the call — half the
    smaller (both optimizers clip), four times the larger (none), their geometric mean (one of the two where they lie apart) —, then losses, every
    gradient entry, norms, coefficients and stepped parameters against the clipped oracle under tests/test_hirl_gpu.py's bars"""
    from tests.test_hirl_gpu import assert_losses, check_params, device_tables, oracle_learn_checked, sync_oracle

    params, data = D.make_params(11), D.make_data(12, outliers=True)
    ring, exp, bc = device_tables(data)
    rng = np.random.default_rng([3, B])
    e = E.HirlEngine(batch=B)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    o = C.install_clip(H.HirlOracle(params["actor"], params["critic"], params["bc_actor"]), 1.0)
    one_sided = 0
    for k in range(4):
        idx, ibc = rng.integers(0, D.N_REPLAY, B).astype(np.int32), rng.integers(0, D.N_EXPERT, B).astype(np.int32)
        noise = rng.normal(0, 0.2, 4).astype(np.float32)
        rows = data["replay"][idx]
        args = ((rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]), (data["expert_s"][ibc], data["expert_a"][ibc]), noise, 100, 0.1)
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        probe = copy.deepcopy(o)
        probe.clip["max_norm"] = 1e30
        probe.learn(*args)
        free = [probe.last_norms["critic"]] + ([probe.last_norms["actor"]] if was_actor_call else [])
        c = {"all": 0.5 * min(free), "none": 4.0 * max(free), "between": float(np.sqrt(free[0] * free[-1])) if was_actor_call else 0.5 * free[0]}[mode]
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
        e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=100, bc_warm_up_weight=0.1)
        what = f"B={B} {mode} call {k}"
        ref = oracle_learn_checked(E, e, o, args, was_actor_call, what + " gradients")
        assert_losses(e.losses_host(), ref, what)
        norms, coefs = e.grad_norms_host()
        for which, name in ((0, "critic"),) + (((1, "actor"),) if was_actor_call else ()):
            bar = norm_bar(o.last_grads[name]) + shape[5 + which] * U * o.last_norms[name]
            print(f"{what} {name}: norm {norms[which]!r} oracle {o.last_norms[name]!r} bar {bar:.3e}; coefficient {coefs[which]!r} oracle {o.last_coefs[name]!r}")
            assert abs(norms[which] - o.last_norms[name]) <= bar, (what, name, norms[which], o.last_norms[name], bar)
            mine = C.coef_f32(norms[which], c)  # the coefficient follows from the engine's own norm by one add and one division
            assert abs(coefs[which] - mine) <= 4 * U * mine and (coefs[which] < 1.0) == (o.last_coefs[name] < 1.0), (what, name, coefs[which], mine)
            assert (coefs[which] < 1.0) == {"all": True, "none": False}.get(mode, coefs[which] < 1.0), (what, name, coefs)
        if mode == "between" and was_actor_call and max(free) > 1.5 * min(free):
            assert (coefs[0] < 1.0) != (coefs[1] < 1.0), (what, free, c, coefs)
            one_sided += 1
        check_params(e, o, E, what + " params", was_actor_call)
    print(f"B={B} {mode}: {one_sided} actor calls clipped one optimizer of the two")


def test_clipped_bf16_learn_matches_the_rounded_operand_oracle(E, golden_dir):
    """bf16 acting + update under a clip that binds in both optimizers: the first two calls of tests/test_bf16_update_gpu.py's soft run (an actor call, a
    critic-only call) against the rounded-operand oracle behind the clip — that file's bars, its kernel-kink rule and its image check"""
    from tests import test_bf16_update_gpu as B16
    from tests.test_hirl_gpu import device_tables, sync_oracle

    g = np.load(os.path.join(golden_dir, "hirl_learn_soft_e0.npz"))  # (only the recorded minibatch indices, noise and weights are used)
    params, data = D.make_params(D.PARAM_SEED), D.make_data(D.DATA_SEED)
    ring, exp, bc = device_tables(data)
    e = E.HirlEngine(batch=128)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    e.set_update_dtype("bf16")
    e.set_act_dtype("bf16")
    o = C.install_clip(H.HirlOracle(params["actor"], params["critic"], params["bc_actor"]), 1.0)
    o.split_actor_grads = True
    for k in range(2):
        idx = g["idx_buf"][k].astype(np.int32)
        w_in = 100 if g["bc_w_in"][k] == 100 else float(g["bc_w_in"][k])
        warm = float(g["warm_in"][k])
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        rows = data["replay"][g["idx_buf"][k]]
        args = ((rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31]), (data["expert_s"][g["idx_bc"][k]], data["expert_a"][g["idx_bc"][k]]),
                g["noise"][k], w_in, warm)
        probe = copy.deepcopy(o)
        probe.clip["max_norm"] = 1e30
        with H.Bf16Layer2():
            probe.learn(*args)
        c = 0.5 * min([probe.last_norms["critic"]] + ([probe.last_norms["actor"]] if was_actor_call else []))
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        pre = (e.actor.clone(), e.critic.clone())
        e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(g["idx_bc"][k].astype(np.int32)).cuda())
        e.learn(noise=torch.from_numpy(g["noise"][k]).cuda(), bc_weight_now=w_in, bc_warm_up_weight=warm)
        got = e.losses_host()
        with H.Bf16Layer2(), B16.KernelKinks(B16.learn_masks(e, E, pre, was_actor_call, soft=(w_in == 100))):
            ref = o.learn(*args)
        what = f"clipped bf16 call {k}"
        np.testing.assert_allclose(got, ref, rtol=B16.LOSS_RTOL, atol=B16.LOSS_ATOL, err_msg=what)
        B16.check_grads(e.grad_critic, o.last_grads["critic"], E.CRITIC_LAYOUT, what + " critic gradient")
        if was_actor_call:
            B16.check_grads(e.grad_actor, o.last_grads["actor"], E.ACTOR_LAYOUT, what + " actor gradient")
        coefs = e.grad_norms_host()[1]
        assert coefs[0] < 1.0 and o.last_coefs["critic"] < 1.0 and (not was_actor_call or (coefs[1] < 1.0 and o.last_coefs["actor"] < 1.0)), (what, coefs)
        B16.check_params(e, o, E, what + " parameters", was_actor_call)
        B16.assert_images_current(e, E, what)


# ---- (e) the front loop ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_bc,slope", [(True, 0.0), (False, 0.01)], ids=["hirl", "td3"])
def test_clipped_front_launch_equals_act_step_then_guarded_clipped_learn(E, use_bc, slope):
    """step_learn under a clip (the front launch, hx_hirl_critic_grads_back, the clipped stages) against act_step + the deferred guarded draw + learn()
    under the same clip (hx_hirl_critic_grads_sampled, the clipped stages) from synchronised states, 64 envs = one env workgroup: bit for bit"""
    from hirl4ucav_amd import _lib
    from tests.test_front_gpu import NETS, make_pair, sorted_rows, sync

    L = _lib.load()
    n, cap = 64, 512  # (the smallest ring the acting launch takes)
    side, exp, bc = make_pair(E, n, cap, use_bc, slope, seed=n)
    (a, env_a, rep_a), (b, env_b, rep_b) = side
    for e in (a, b):
        e.set_grad_clip(0.05)
    for _ in range(5):
        a.act_step(env_a, sigma=0.1, seed=3)  # enough rows in the ring for the first draw of 96 behind a guard of 64
    assert int(rep_a.total.item()) >= 96 + n
    snap = torch.zeros(1, dtype=torch.int64, device="cuda")
    names, real = [], _lib.call
    clipped = 0
    for k in range(8):
        sync(side[1], side[0])
        w = ((100 if k % 4 == 0 else (None if k % 4 < 3 else 0.3)) if use_bc else 0.0)
        _lib.call = lambda name, *args: names.append(name) or real(name, *args)
        try:
            out_a = a.step_learn(env_a, exp, bc, n_main=96, act_sigma=0.1, act_seed=3, sample_seed=11, bc_weight_now=w, bc_warm_up_weight=0.05)
        finally:
            _lib.call = real
        snap.copy_(rep_b.total)
        out_b = b.act_step(env_b, sigma=0.1, seed=3)
        b.sample(rep_b, exp, bc, n_main=96, seed=11, defer=True)
        b._pending[0].total, b._pending[0].guard = snap.data_ptr(), n
        L.hx_debug_set_fwd_nt(64, 1, 1)  # launch B in the front launch's tiling (tests/test_front_gpu.py)
        try:
            b.learn(bc_weight_now=w, bc_warm_up_weight=0.05)
        finally:
            L.hx_debug_set_fwd_nt(0, 0, 0)
        a.front_check()
        for x, y, name in zip(out_a, out_b, ("actions", "obs", "reward", "done", "success")):
            assert torch.equal(x, y), (k, name)
        assert torch.equal(env_a._state_store, env_b._state_store) and torch.equal(rep_a.total, rep_b.total), k
        np.testing.assert_array_equal(sorted_rows(rep_a), sorted_rows(rep_b), err_msg=f"step {k}: replay rows")
        for name in ("_idx", "_noise", "rows") + (("_idx_bc", "bc_rows") if use_bc else ()):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        np.testing.assert_allclose(a.losses_host(), b.losses_host(), rtol=1e-6, atol=1e-7, err_msg=f"step {k}")
        for name in NETS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        assert LS.bits_equal(a.clip_ws, b.clip_ws), k
        clipped += sum(c < 1.0 for c in a.grad_norms_host()[1])
    assert "hx_hirl_front" in names and "hx_hirl_critic_grads_back" in names and "hx_hirl_learn_back" not in names
    assert names.count("hx_adam_clipped") == names.count("hx_hirl_grad_norm") == 8 + 4 and "hx_adam" not in names
    assert int(rep_a.total.item()) > cap and clipped > 0, (int(rep_a.total.item()), clipped)


# ---- (f) virtual ranks in lockstep --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 8])
def test_lockstep_ranks_clip_the_global_batchs_gradient(E, shape, W):
    """W virtual ranks of 16 rows (tests/_sharded_lockstep.Lockstep, unchanged: the clip sits in the stage methods it calls) against ONE clipped engine of
    16 W rows fed the concatenated minibatches, synchronised before each of 4 calls: the replicas stay identical in bits and hold ONE norm and ONE
    coefficient per optimizer; that norm is the global batch's within what the gradient bar allows (the bound test_shards_equal_the_global_batch_at_
    gradient_level holds the summed gradients to), and both sides clip"""
    from tests.test_sharded_lockstep_gpu import draw

    B, c = 16, 1e-3
    params, data = D.make_params(41), D.make_data(42, outliers=True)
    ls = LS.Lockstep(E, W, B, params, data)
    g = LS.make_engine(E, B * W, params)
    for e in ls.engines + [g]:
        e.set_grad_clip(c)
    rng = np.random.default_rng([8, W, B])
    for k in range(4):
        LS.copy_state(g, ls.engines[0])
        idx, ibc, noise = draw(rng, W, B)
        g.assemble(ls.ring, torch.from_numpy(idx.reshape(-1)).cuda(), bc_table=ls.bc, idx_bc=torch.from_numpy(ibc.reshape(-1)).cuda())
        g.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=100, bc_warm_up_weight=0.05)
        ls.learn([(idx[r], ibc[r]) for r in range(W)], noise, 100, 0.05)
        what = ("W", W, "call", k)
        for r in range(1, W):
            LS.assert_same_state(ls.engines[r], ls.engines[0], what + ("replica", r))
            assert LS.bits_equal(ls.engines[r].clip_ws, ls.engines[0].clip_ws), what + ("replica", r)
        (norms, coefs), (gn, gc) = ls.engines[0].grad_norms_host(), g.grad_norms_host()
        for which, flat, layout in ((0, g.grad_critic, E.CRITIC_LAYOUT),) + (((1, g.grad_actor, E.ACTOR_LAYOUT),) if ls.was_actor_call else ()):
            grads = {key: t.cpu() for key, t in E.unpack(flat, layout).items()}
            bar = norm_bar(grads) + 2 * shape[5 + which] * U * gn[which]
            print(f"{what} which {which}: ranks {norms[which]!r} global {gn[which]!r} bar {bar:.3e}; coefficients {coefs[which]!r} {gc[which]!r}")
            assert abs(norms[which] - gn[which]) <= bar, (what, which, norms[which], gn[which], bar)
            assert coefs[which] < 1.0 and gc[which] < 1.0 and abs(coefs[which] - C.coef_f32(norms[which], c)) <= 4 * U * coefs[which], (what, coefs, gc)


def test_a_set_exchange_status_word_changes_nothing_under_the_clip(E):
    """HxNets.xchg_status pointing at a non-zero word (a failed exchange): the clipped steps of a lockstep call change no parameter, moment, target, image,
    wstate, norm or coefficient; with the word gone the same call steps"""
    from tests.test_sharded_lockstep_gpu import draw

    W, B = 2, 16
    ls = LS.Lockstep(E, W, B, D.make_params(41), D.make_data(42, outliers=True))
    word = torch.ones(16, dtype=torch.int32, device="cuda")
    for e in ls.engines:
        e.set_grad_clip(1e-3)
        e.clip_ws[:4] = -3.0
    before = [{k: t.clone() for k, t in LS.state_tensors(e).items()} for e in ls.engines]
    rng = np.random.default_rng(9)
    idx, ibc, noise = draw(rng, W, B)
    for e in ls.engines:
        e.nets.xchg_status = word.data_ptr()
    try:
        ls.learn([(idx[r], ibc[r]) for r in range(W)], noise, 100, 0.05)
        torch.cuda.synchronize()
    finally:
        for e in ls.engines:
            e.nets.xchg_status = None
    assert ls.was_actor_call
    for e, was in zip(ls.engines, before):
        now = LS.state_tensors(e)
        assert not [k for k in was if not LS.bits_equal(was[k], now[k])] and e.clip_ws[:4].tolist() == [-3.0] * 4
    ls.learn([(idx[r], ibc[r]) for r in range(W)], noise, 100, 0.05)
    assert not LS.bits_equal(before[0]["critic"], ls.engines[0].critic) and float(ls.engines[0].clip_ws[0].item()) > 0.0  # (a critic-only call)


# ---- (g) argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(E):
    from hirl4ucav_amd import _lib

    e = fresh(E)
    nets, hyper, ws, st = ctypes.byref(e.nets), ctypes.byref(e.hyper), e.clip_ws.data_ptr(), _lib.stream_ptr()
    msg = torch.zeros(int(_lib.load().hx_actor_message_floats()) + 4, dtype=torch.float32, device="cuda")
    before = {k: t.clone() for k, t in LS.state_tensors(e).items()}

    def step(which=0, step_no=1, scale=1.0, m=None, max_norm=1.0, w=ws, n=nets, h=hyper):
        _lib.call("hx_adam_clipped", n, h, which, step_no, scale, 0, 0.0, 0.0, 16, m, max_norm, w, st)

    def norm(which=0, m=None, w=ws, n=nets, h=hyper):
        _lib.call("hx_hirl_grad_norm", n, h, which, 0, 0.0, 0.0, 16, m, w, st)

    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(_lib.HxError, match="max_norm must be positive"):
            step(max_norm=bad)
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(_lib.HxError, match="grad_scale must be positive"):
            step(scale=bad)
    for f in (step, norm):
        with pytest.raises(_lib.HxError, match="clip_ws must be 16-byte aligned"):
            f(w=ws + 4)
        with pytest.raises(_lib.HxError, match="bad arguments"):
            f(w=None)
        with pytest.raises(_lib.HxError, match="bad arguments"):
            f(n=None)
        with pytest.raises(_lib.HxError, match="bad arguments"):
            f(h=None)
        with pytest.raises(_lib.HxError, match="belongs to the actor step"):
            f(which=0, m=msg.data_ptr())
        with pytest.raises(_lib.HxError, match="which is 0 .critic. or 1 .actor."):
            f(which=2)
        with pytest.raises(_lib.HxError, match="which is 0 .critic. or 1 .actor."):
            f(which=3)
        with pytest.raises(_lib.HxError, match="16-byte aligned message"):
            f(which=1, m=msg.data_ptr() + 4)
        own = e.nets.grad_actor
        e.nets.grad_actor = own + 4
        try:
            with pytest.raises(_lib.HxError, match="buffers must be 16-byte aligned"):
                f(which=1)
        finally:
            e.nets.grad_actor = own
    with pytest.raises(_lib.HxError, match="bad arguments"):
        step(step_no=0)
    with pytest.raises(_lib.HxError, match="which is 0"):
        step(which=2 | 16)
    with pytest.raises(_lib.HxError, match="null output"):
        _lib.call("hx_hirl_clip_shape", None)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="positive maximum norm"):
            e.set_grad_clip(bad)
    with pytest.raises(_lib.HxError, match="no clip was ever set"):
        LS.make_engine(E, 16, D.make_params(57)).grad_norms_host()
    torch.cuda.synchronize()
    now = LS.state_tensors(e)
    assert not [k for k in before if not LS.bits_equal(before[k], now[k])]  # a refused call launches nothing


# ---- (h) switched off, the parent's paths call for call ------------------------------------------------------------------------------------------------
def recorded(fn):
    from hirl4ucav_amd import _lib

    names, real = [], _lib.call
    _lib.call = lambda name, *args: names.append(name) or real(name, *args)
    try:
        fn()
    finally:
        _lib.call = real
    return names


@pytest.mark.parametrize("staged", [False, True])
def test_with_no_clip_no_new_entry_point_is_called(E, staged):
    """never clipped, and clipped then set_grad_clip(None): the same library calls, name for name, none of them new; the networks in bits.  Under the clip
    the one call gives way to the stages and hx_adam to the two new launches"""
    params = D.make_params(21)
    plain, back, on = (config_engine(E, 16, params, {}) for _ in range(3))
    back.set_grad_clip(0.5)
    back.set_grad_clip(None)
    on.set_grad_clip(1e-3)
    for e in (plain, back, on):
        e.staged = staged
    seq = [recorded(lambda e=e: [None for _ in three_calls(E, [e], 16, 5)]) for e in (plain, back, on)]
    assert seq[0] == seq[1] and not set(seq[0]) & set(NEW_CALLS)
    assert ("hx_hirl_learn_sampled" in seq[0]) == (not staged) and ("hx_adam" in seq[0]) == staged
    LS.assert_same_state(plain, back, "clip switched off again")
    assert back.grad_clip is None and "hx_hirl_learn_sampled" not in seq[2] and "hx_adam" not in seq[2] and "hx_adam_mixed" not in seq[2]
    assert seq[2].count("hx_hirl_grad_norm") == seq[2].count("hx_adam_clipped") == 3 + 2  # three critic steps, two actor steps
    assert not LS.bits_equal(plain.critic, on.critic)


# ---- (i) the drivers ---------------------------------------------------------------------------------------------------------------------------------
CLIP = ["--hirl_grad_clip", "0.05"]


@pytest.mark.parametrize("kind", ["front", "reference", "td3"])
def test_train_all_grad_clip(E, tmp_path, monkeypatch, capsys, kind):
    """2 driver episodes of 12 steps at 64 envs, HIRL soft in both loop forms and TD3: the clipped stages run (behind the front launch in the front loop),
    the loop line says so, both norms are logged where the losses are, the snapshot carries the value; without the flag no new call is made"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import COMMON, HIRL, spy

    args = (["--agent", "TD3"] + COMMON if kind == "td3" else HIRL + ["--loop", kind])
    real_load = T.load_expert_tables
    names, runs, writers = spy(monkeypatch)
    if kind == "td3":
        monkeypatch.setattr(T, "load_expert_tables", real_load)  # (spy's hook copies the expert ring, which TD3 has not)
    out_dir = T.main(T.parse_args(args + CLIP + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    front = kind != "reference"
    assert ("vector loop: front launch" if front else "vector loop: reference order") in out and "--hirl_grad_clip 0.05: the clipped update runs as stages" in out
    assert ("behind the front launch" in out) == front and (names.count("hx_hirl_front") > 0) == front
    assert names.count("hx_adam_clipped") == names.count("hx_hirl_grad_norm") > 0 and "hx_adam" not in names and "hx_hirl_learn_back" not in names
    assert "hx_hirl_learn_sampled" not in names and "hx_hirl_learn" not in names
    rows = writers[0].rows
    for tag in ("stats/grad_norm_critic", "stats/grad_norm_actor"):
        vals = [v for t, v, _ in rows if t == tag]
        assert len(vals) == len([1 for t, _, _ in rows if t == "Loss/Critic_Loss"]) > 0 and all(np.isfinite(vals)) and max(vals) > 0.0, (tag, vals)
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert snap["engine"]["grad_clip"] == 0.05
    del names[:]
    T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    assert names and not set(names) & set(NEW_CALLS) and not [t for t, _, _ in writers[-1].rows if t.startswith("stats/grad_norm")]


def test_train_all_grad_clip_resume(E, tmp_path):
    """--separate_launches (one env workgroup: the run is reproducible): 1 episode + --resume to 2 equals the uninterrupted clipped run bit for bit —
    the arena but its logged loss slots (sums of float atomics: rtol 1e-6 / atol 1e-7, as tests/test_branch_gpu.py), the replay ring; --resume under
    another value, or none, is refused by the flag's name"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import HIRL

    args = HIRL + CLIP + ["--separate_launches"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a, b = (torch.load(os.path.join(d, "state_rank0.pt"), map_location="cpu", weights_only=False) for d in (whole, rest))
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and a["engine"]["counters"] == b["engine"]["counters"]
    assert a["engine"]["grad_clip"] == b["engine"]["grad_clip"] == 0.05
    e = E.HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-6, atol=1e-7)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] and torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32))
    for other in (["--hirl_grad_clip", "0.5"], []):
        with pytest.raises((ValueError, SystemExit), match="--hirl_grad_clip"):
            T.main(T.parse_args(HIRL + other + ["--separate_launches", "--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))


def test_facade_keyword(E):
    """Agent(..., grad_clip=c) of agents/HIRL.py and agents/TD3.py: the engine clips at c (None, the default: it does not); a TD3 agent learns under it"""
    from hirl4ucav_amd.agents import HIRL, TD3

    rng = np.random.default_rng(2)
    es, ea = rng.uniform(-1, 1, (40, 13)).astype(np.float32), rng.uniform(-1, 1, (40, 4)).astype(np.float32)
    h = HIRL.Agent(1e-3, 1e-3, 13, 4, 256, 512, 0.005, 0.99, 1000, 16, True, "x", es, ea, grad_clip=2.0)
    assert h.grad_clip == 2.0 and h.eng.grad_clip == 2.0
    assert HIRL.Agent(1e-3, 1e-3, 13, 4, 256, 512, 0.005, 0.99, 1000, 16, True, "x", es, ea).eng.grad_clip is None
    t = TD3.Agent(1e-3, 1e-3, 13, 4, 256, 512, 0.005, 0.99, 1000, 16, True, "x", grad_clip=1e-3)
    assert t.eng.grad_clip == 1e-3 and TD3.Agent(1e-3, 1e-3, 13, 4, 256, 512, 0.005, 0.99, 1000, 16, True, "x").eng.grad_clip is None
    for _ in range(40):
        t.store(rng.uniform(-1, 1, 13), rng.uniform(-1, 1, 4), rng.uniform(-1, 1, 13), float(rng.uniform(-9, 0)), False)
    for _ in range(2):
        out = t.learn()
    norms, coefs = t.eng.grad_norms_host()
    assert len(out) == 2 and all(np.isfinite(out)) and min(norms) > 1e-3 and max(coefs) < 1.0, (out, norms, coefs)
