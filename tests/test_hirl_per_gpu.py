"""Prioritized replay for HIRL and TD3 on the GPU (hx_hirl_per.hip: hirl_td_head_weighted_kernel behind hx_hirl_critic_grads_weighted;
HirlEngine.set_prioritized; train_all --hirl_per).  A declared extension (the reference's prioritized branch is dead code): the rule is
include/hirl4ucav.h "Prioritized replay for HIRL / TD3", restated around the oracle by tests/_hirl_per (CPU-pinned against float64 by
tests/test_hirl_per_cpu.py); the store and the draw are tests/_per_check.PerModel's, as for SAC.

Bars, none of them taken from what the kernels give:
  against the restatement   tests/test_hirl_gpu.py's, unchanged: losses rtol 2e-5 / atol 5e-6, gradients |dg| <= 1e-4 |g| + 2e-5 max|g| in EVERY entry (fragile
                            ReLU units by oracle_checked), parameters by check_params
  errors                    rtol 2e-5 / atol 5e-6: the bar tests/test_per_gpu.py holds SAC's errors_out to against its checker
  bf16                      tests/test_bf16_update_gpu.py's bars against the rounded-operand restatement, unchanged
  priorities                rtol 2e-5 against the float64 model (tests/test_per_gpu.py's bar for powf); every untouched slot and block sum in bits
  bit identities            where stated: n_weighted, zero weights, the draw's untouched rows, the switched-off path, resume"""
import ctypes
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hirl_oracle as H  # noqa: E402
from tests import _hirl_clip as C  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _hirl_per as W  # noqa: E402
from tests import _per_check as P  # noqa: E402
from tests import _sharded_lockstep as LS  # noqa: E402

ERR_RTOL, ERR_ATOL = 2e-5, 5e-6
NEW_CALLS = ("hx_hirl_critic_grads_weighted",)
PER_CALLS = ("hx_per_sample", "hx_per_update", "hx_per_mark_new")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import engine

    return engine


@pytest.fixture(scope="module")
def shared():
    """networks, tables (outlier rows: the +600 kill bonus) and their device copies, made once and left unchanged"""
    from tests.test_hirl_gpu import device_tables

    params, data = D.make_params(11), D.make_data(12, outliers=True)
    ring, exp, bc = device_tables(data)
    return types.SimpleNamespace(params=params, data=data, ring=ring, exp=exp, bc=bc)


def replay_of(ring):
    """a PrioritizedReplay that holds `ring`'s rows, every slot marked at pmax"""
    from hirl4ucav_amd.utils.buffer import PrioritizedReplay

    rep = PrioritizedReplay(ring.shape[0])
    rep.store_rows(ring)
    rep.mark_new()
    return rep


def per_engine(E, B, params, rep, **kw):
    e = LS.make_engine(E, B, params, **kw)
    e.set_prioritized(rep)
    return e


def draw_call(rng, B, nm, weights=True):
    idx = np.concatenate([rng.integers(0, D.N_REPLAY, nm), rng.integers(0, D.N_EXPERT_ROWS, B - nm)]).astype(np.int32)
    ibc = rng.integers(0, D.N_EXPERT, B).astype(np.int32)
    noise = rng.normal(0, 0.2, 4).astype(np.float32)
    w = rng.uniform(0.05, 1.0, B).astype(np.float32)
    if nm >= 2:  # spread over [0.05, 1]
        w[0], w[nm - 1] = 0.05, 1.0
    elif nm == 1:
        w[0] = 0.05
    return idx, ibc, noise, w


def oracle_args(data, idx, ibc, noise, nm, use_bc=True, w_now=100, warm=0.1, ring=None):
    rows = np.concatenate([(data["replay"] if ring is None else ring)[idx[:nm]], data["expert_rows"][idx[nm:]]], 0)
    batch = (rows[:, 0:13], rows[:, 13:17], rows[:, 17:30], rows[:, 30], rows[:, 31])
    if not use_bc:
        return batch, None, noise
    return batch, (data["expert_s"][ibc], data["expert_a"][ibc]), noise, w_now, warm


def engine_call(e, sh, idx, ibc, noise, nm, w, ring=None, w_now=100, warm=0.1):
    cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    if e.use_bc:
        e.assemble(sh.ring if ring is None else ring, cuda(idx), expert_ring=sh.exp, n_main=nm, bc_table=sh.bc, idx_bc=cuda(ibc))
    else:
        e.assemble(sh.ring if ring is None else ring, cuda(idx), expert_ring=sh.exp, n_main=nm)
    if e.prioritized is not None:
        e.set_weights(w, nm, idx=idx)
    e.learn(noise=cuda(noise), **(dict(bc_weight_now=w_now, bc_warm_up_weight=warm) if e.use_bc else {}))


def checked(E, e, o, args, w, nm, was_actor_call, what):
    """the restatement's call under tests/test_hirl_gpu.py's oracle_checked -> (the six outputs, errors)"""
    from tests.test_hirl_gpu import oracle_checked

    pairs = [(e.grad_critic, "critic", E.CRITIC_LAYOUT)] + ([(e.grad_actor, "actor", E.ACTOR_LAYOUT)] if was_actor_call else [])
    return oracle_checked(o, lambda oo: W.weighted_learn(oo, *args, weights=w, n_main=nm), pairs, what)


# ---- (a) weighted learn() against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "less5", "one"])
@pytest.mark.parametrize("B", [16, 48, 144])
def test_weighted_learn_matches_the_restatement(E, shared, B, which):
    """three consecutive calls (actor, critic-only, actor) from synchronised states, HIRL soft with warm-up, outlier rows; rows [n_main, B) come from the
    expert ring and weigh 1: losses, every gradient entry, |Q1 - y| of every row, stepped parameters, and the priorities learn() leaves behind"""
    from tests.test_hirl_gpu import assert_losses, check_params, sync_oracle

    sh, nm = shared, {"all": B, "less5": B - 5, "one": 1}[which]
    rep = replay_of(sh.ring)
    e = per_engine(E, B, sh.params, rep)
    o = H.HirlOracle(sh.params["actor"], sh.params["critic"], sh.params["bc_actor"])
    rng = np.random.default_rng([7, B, nm])
    for k in range(3):
        idx, ibc, noise, w = draw_call(rng, B, nm)
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        before = rep.prio.clone()
        engine_call(e, sh, idx, ibc, noise, nm, w)
        what = f"B={B} n_main={nm} call {k}"
        ref, err = checked(E, e, o, oracle_args(sh.data, idx, ibc, noise, nm), w, nm, was_actor_call, what + " gradients")
        assert_losses(e.losses_host(), ref, what)
        got = e._errors.cpu().numpy()
        print(f"{what}: errors max |d| {np.abs(got - err).max():.3e} at max |err| {np.abs(err).max():.3e}")
        np.testing.assert_allclose(got, err, rtol=ERR_RTOL, atol=ERR_ATOL, err_msg=what + " errors")
        check_params(e, o, E, what + " params", was_actor_call)
        m = P.PerModel(D.N_REPLAY)
        m.set(np.arange(D.N_REPLAY), before.cpu().numpy().astype(np.float64))
        m.update(idx[:nm], got[:nm])
        pr = rep.prio.cpu().numpy()
        np.testing.assert_allclose(pr[idx[:nm]], m.prio[idx[:nm]], rtol=2e-5, atol=0, err_msg=what + " priorities")
        rest = np.setdiff1d(np.arange(D.N_REPLAY), idx[:nm])
        assert np.array_equal(pr[rest].view(np.uint32), before.cpu().numpy()[rest].view(np.uint32)), what
    assert e.critic_step == 3 and e.actor_step == 2


# ---- (b) n_weighted -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nm", [(16, 11), (48, 0), (144, 143)])
def test_weights_behind_n_weighted_are_never_read(E, shared, B, nm):
    """NaN planted in weights[n_weighted:] against ones there: gradients, errors and every state tensor in bits (n_weighted = 0: weights NULL too)"""
    sh = shared
    a, b = (per_engine(E, B, sh.params, replay_of(sh.ring)) for _ in range(2))
    idx, ibc, noise, w = draw_call(np.random.default_rng([8, B]), B, nm)
    for e, tail in ((a, float("nan")), (b, 1.0)):
        e._weights.fill_(tail)
        engine_call(e, sh, idx, ibc, noise, nm, w)
    assert bool(a._weights[nm:].isnan().all()) and bool((b._weights[nm:] == 1.0).all()) and (nm == 0 or LS.bits_equal(a._weights[:nm], b._weights[:nm]))
    LS.assert_same_state(a, b, ("n_weighted", nm))
    assert LS.bits_equal(a.grad, b.grad) and LS.bits_equal(a._errors, b._errors) and bool(torch.isfinite(a.grad).all())
    np.testing.assert_allclose(a.losses_host(), b.losses_host(), rtol=1e-6, atol=1e-7)
    assert LS.bits_equal(a.prioritized.prio, b.prioritized.prio)


# ---- (c) teeth: zero weights ----------------------------------------------------------------------------------------------------------------------------
def test_zero_weights_leave_the_critic_where_it_was(E, shared):
    """all weights 0 at n_main = B: the critic's parameters and Adam moments after the first call are bit for bit what they were, the critic loss is 0;
    errors are what a run with other weights gives, in bits (they do not depend on the weights)"""
    sh, B = shared, 48
    a, b = (per_engine(E, B, sh.params, replay_of(sh.ring)) for _ in range(2))
    idx, ibc, noise, w = draw_call(np.random.default_rng(9), B, B)
    before = {k: getattr(a, k).clone() for k in ("critic", "m_critic", "v_critic", "target_critic")}
    engine_call(a, sh, idx, ibc, noise, B, np.zeros(B, np.float32))
    engine_call(b, sh, idx, ibc, noise, B, w)
    for k, t in before.items():
        assert LS.bits_equal(t, getattr(a, k)), k
    assert a.losses_host()[0] == 0.0 and float(a.grad_critic.abs().max()) == 0.0
    assert not LS.bits_equal(before["critic"], b.critic) and b.losses_host()[0] > 0.0
    assert LS.bits_equal(a._errors, b._errors) and float(a._errors.min()) > 0.0
    assert not LS.bits_equal(a.actor, LS.make_engine(E, B, sh.params).actor)  # (an actor call: the unweighted actor half did step)


# ---- (d) teeth: the weights matter ------------------------------------------------------------------------------------------------------------------------
def test_weight_zero_hides_planted_rows_and_weight_one_does_not(E, shared):
    """three rows carry a planted reward of 1e6.  With weight 0 on them the call matches the restatement under the bars of (a); the same call with weight 1
    on them must NOT match that restatement: loss and gradients leave their bars"""
    from tests.test_hirl_gpu import assert_losses, check_params, grad_mismatch, sync_oracle

    sh, B, planted = shared, 48, [3, 17, 40]
    idx, ibc, noise, w = draw_call(np.random.default_rng(10), B, B)
    assert len(set(idx[planted].tolist())) == 3
    ring_np = sh.data["replay"].copy()
    ring_np[idx[planted], 30] = 1e6
    ring = torch.from_numpy(ring_np).cuda()
    w0 = w.copy()
    w0[planted] = 0.0
    w1 = w.copy()
    w1[planted] = 1.0
    args = oracle_args(sh.data, idx, ibc, noise, B, ring=ring_np)
    e = per_engine(E, B, sh.params, replay_of(ring))
    o = H.HirlOracle(sh.params["actor"], sh.params["critic"], sh.params["bc_actor"])
    sync_oracle(o, e, E)
    engine_call(e, sh, idx, ibc, noise, B, w0, ring=ring)
    ref, err = checked(E, e, o, args, w0, B, True, "planted rows at weight 0")
    assert_losses(e.losses_host(), ref, "planted rows at weight 0")
    np.testing.assert_allclose(e._errors.cpu().numpy(), err, rtol=ERR_RTOL, atol=ERR_ATOL)
    assert err[planted].min() > 9e5
    check_params(e, o, E, "planted rows at weight 0", True)
    e1 = per_engine(E, B, sh.params, replay_of(ring))
    engine_call(e1, sh, idx, ibc, noise, B, w1, ring=ring)
    got = e1.losses_host()
    assert abs(got[0] - ref[0]) > 100 * (2e-5 * abs(ref[0]) + 5e-6), (got[0], ref[0])
    assert grad_mismatch(e1.grad_critic, o.last_grads["critic"], E.CRITIC_LAYOUT)
    assert LS.bits_equal(e1._errors, e._errors)


# ---- (e) unit weights against the unweighted staged path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 48, 144])
def test_unit_weights_against_the_unweighted_staged_path(E, shared, B):
    """weights of 1 on every row against the staged unweighted path from the same state, three calls: every parameter within tests/test_hirl_gpu.py's
    check_params bound around the unweighted path's (bit identity is not claimed: the per-row head and bwd_l2<0>'s prologue are two instruction sequences)"""
    from tests.test_hirl_gpu import check_params

    sh = shared
    a, b = per_engine(E, B, sh.params, replay_of(sh.ring)), LS.make_engine(E, B, sh.params)
    b.staged = True
    rng = np.random.default_rng([11, B])
    worst = 0.0
    for k in range(3):
        idx, ibc, noise, _ = draw_call(rng, B, B)
        LS.copy_state(a, b)
        was_actor_call = b.actor_trainable
        for e in (a, b):
            engine_call(e, sh, idx, ibc, noise, B, np.ones(B, np.float32))
        cpu = lambda flat, layout: {key: t.cpu() for key, t in E.unpack(flat, layout).items()}  # noqa: E731
        ref = types.SimpleNamespace(actor=cpu(b.actor, E.ACTOR_LAYOUT), critic=cpu(b.critic, E.CRITIC_LAYOUT), target_actor=cpu(b.target_actor, E.ACTOR_LAYOUT),
                                    target_critic=cpu(b.target_critic, E.CRITIC_LAYOUT),
                                    last_grads={"critic": cpu(b.grad_critic, E.CRITIC_LAYOUT), "actor": cpu(b.grad_actor, E.ACTOR_LAYOUT)})
        check_params(a, ref, E, f"unit weights B={B} call {k}", was_actor_call)
        np.testing.assert_allclose(a.losses_host(), b.losses_host(), rtol=2e-5, atol=5e-6)
        worst = max([worst] + [float((getattr(a, n) - getattr(b, n)).abs().max()) for n in ("actor", "critic", "target_actor", "target_critic")])
    print(f"unit weights B={B}: largest parameter difference against the unweighted staged path over 3 calls {worst:.3e}")


# ---- (f) the draw ---------------------------------------------------------------------------------------------------------------------------------------
def draw_setup(E, params, B=48):
    from hirl4ucav_amd.utils.buffer import DeviceReplay
    from tests.test_per_gpu import CAP, integer_priorities, new_replay

    rep = new_replay()
    pr = integer_priorities()
    rep.set_priorities(np.arange(CAP), pr)
    m = P.PerModel(CAP)
    m.set(np.arange(CAP), pr)
    rng = np.random.default_rng(13)
    expert = DeviceReplay(300)  # (its indices would be valid main slots: a leak into the store would show)
    expert.store_rows(torch.from_numpy(rng.normal(size=(290, 32)).astype(np.float32)))
    bc = torch.from_numpy(rng.normal(size=(200, 32)).astype(np.float32)).cuda()
    return rep, m, pr, expert, bc


@pytest.mark.parametrize("nm", [48, 43, 1, 0])
def test_the_draw(E, shared, nm):
    """injected u: idx[:n_main] is PerModel.draw(u), rows [0, n_main) are ring[idx] and the weights the model's; rows, indices [n_main, B), the BC tile and
    the noise are in bits what an engine WITHOUT prioritized replay drew with the same seed and call; n_main = 0 makes no prioritized call"""
    from hirl4ucav_amd import _lib

    B = 48
    rep, m, pr, expert, bc = draw_setup(E, shared.params)
    a, b = per_engine(E, B, shared.params, rep), LS.make_engine(E, B, shared.params)
    ks = np.random.default_rng(nm).choice(4096, max(nm, 1), replace=False)
    if nm > 2:
        ks[2] = ks[1]  # one target twice: a slot repeats
    u = ((ks + 0.5) / 4096.0).astype(np.float32)
    names, real = [], _lib.call
    _lib.call = lambda name, *args: names.append(name) or real(name, *args)
    try:
        a.sample(rep, expert, bc, n_main=nm, seed=21, u=torch.from_numpy(u).cuda() if nm else None)
    finally:
        _lib.call = real
    b.sample(rep, expert, bc, n_main=nm, seed=21)
    assert names.count("hx_per_sample") == (1 if nm else 0) and names[0] == "hx_sample_batch" and a.per_calls == (1 if nm else 0) and a.sample_calls == 1
    idx = a._idx.cpu().numpy().astype(np.int64)
    if nm:
        want = m.draw(u[:nm].astype(np.float64))
        np.testing.assert_array_equal(idx[:nm], want)
        assert nm < 3 or idx[1] == idx[2]
        assert torch.equal(a.rows.view(-1, 32)[:nm].view(torch.int32), rep.ring[torch.from_numpy(want).cuda()].view(torch.int32))
        np.testing.assert_allclose(a._weights[:nm].cpu().numpy(), m.weights(want, 0.4, 2500), rtol=2e-5, atol=0)
        assert float(a._weights[:nm].max()) == 1.0 and rep.beta == pytest.approx(0.4001)
    for name in ("rows", "_idx"):
        x, y = getattr(a, name).view(B, -1)[nm:], getattr(b, name).view(B, -1)[nm:]
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    for name in ("bc_rows", "_idx_bc", "_noise"):
        assert LS.bits_equal(getattr(a, name), getattr(b, name)), name
    if nm > 2:
        assert not torch.equal(a._idx[:nm], b._idx[:nm])


# ---- (g) priorities after learn() ------------------------------------------------------------------------------------------------------------------------
def test_priorities_after_learn(E, shared):
    """sample(u) then learn(): the drawn slots hold powf(err + 1e-4, alpha), a repeated slot the maximum; every other slot, every block sum no drawn slot
    falls into, in bits; the expert ring's indices (valid main slots, all of them) never reach hx_per_update"""
    B, nm = 48, 37
    rep, m, pr, expert, bc = draw_setup(E, shared.params)
    e = per_engine(E, B, shared.params, rep)
    ks = np.random.default_rng(5).choice(np.arange(0, 1500), nm, replace=False)  # (targets below 1,500 of 4,096: block 0 alone is drawn from)
    ks[5] = ks[4]
    u = ((ks + 0.5) / 4096.0).astype(np.float32)
    e.sample(rep, expert, bc, n_main=nm, seed=3, u=torch.from_numpy(u).cuda())
    idx = e._idx.cpu().numpy().astype(np.int64)
    assert idx[4] == idx[5] and (idx[:nm] < 1024).all()
    before, bsum0, pmax0 = rep.prio.clone().cpu().numpy(), rep.bsum.clone(), rep.pmax
    e.learn(bc_weight_now=100, bc_warm_up_weight=0.1)
    err = e._errors.cpu().numpy()
    assert np.isfinite(err).all() and err[4] == err[5]  # (one slot drawn twice: the same row, the same error)
    m.update(idx[:nm], err[:nm])
    now = rep.prio.cpu().numpy()
    np.testing.assert_allclose(now[idx[:nm]], m.prio[idx[:nm]], rtol=2e-5, atol=0)
    np.testing.assert_allclose(now[idx[4]], (max(err[4], err[5]) + 1e-4) ** 0.6, rtol=2e-5)
    rest = np.setdiff1d(np.arange(rep.capacity), idx[:nm])
    assert np.array_equal(now[rest].view(np.uint32), before[rest].view(np.uint32))
    leaked = np.setdiff1d(idx[nm:], idx[:nm])
    assert leaked.size > 0 and (before[leaked] > 0).any() and np.array_equal(now[leaked], before[leaked])  # expert indices name live main slots; untouched
    assert torch.equal(rep.bsum[1:].view(torch.int32), bsum0[1:].view(torch.int32)) and not torch.equal(rep.bsum[:1], bsum0[:1])
    np.testing.assert_allclose(rep.pmax, max(pmax0, m.prio[idx[:nm]].max()), rtol=2e-5)
    from tests.test_per_gpu import check_sums

    check_sums(rep)


# ---- (h) variants ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [128, 48])
def test_bf16_weighted_learn_matches_the_rounded_operand_restatement(E, B):
    """bf16 acting + update, HIRL soft with expert rows behind n_main, an actor call and a critic-only call: tests/test_bf16_update_gpu.py's bars, its
    kernel-kink rule (which reads the LayerNorm stats the head kernel and bwd_l2<3> leave in st2) and its image check; errors at that file's loss bar
    against the restatement evaluated on the same rounded operands"""
    from tests import _bf16_ragged as R
    from tests import test_bf16_update_gpu as B16
    from tests.test_hirl_gpu import device_tables, sync_oracle

    case = "expert" if B == 48 else "soft"
    nm = R.n_main(case, B) if B == 48 else B - 16
    ring, exp, bc = device_tables(R.data())
    rep = replay_of(ring)
    p = R.params()
    e = LS.make_engine(E, B, p, bf16=True)
    e.set_prioritized(rep)
    o = R.new_oracle(case)
    rng = np.random.default_rng([14, B])
    sh = types.SimpleNamespace(ring=ring, exp=exp, bc=bc)
    for k, (idx, ibc, noise) in enumerate(R.calls(case, B)[:2]):
        if B == 128:  # (R's "soft" case draws every row from the replay: the last 16 from the expert ring here)
            idx = idx.copy()
            idx[nm:] = rng.integers(0, D.N_EXPERT_ROWS, B - nm)
        w = rng.uniform(0.05, 1.0, B).astype(np.float32)
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        pre = (e.actor.clone(), e.critic.clone())
        engine_call(e, sh, idx, ibc, noise, nm, w, w_now=R.SOFT, warm=R.WARM)
        got = e.losses_host()
        d = R.data()
        args = oracle_args(d, idx, ibc, noise, nm, w_now=R.SOFT, warm=R.WARM)
        with H.Bf16Layer2(), B16.KernelKinks(B16.learn_masks(e, E, pre, was_actor_call, soft=True, B=B)):
            ref, err = W.weighted_learn(o, *args, weights=w, n_main=nm)
        what = f"bf16 weighted B={B} call {k}"
        np.testing.assert_allclose(got, ref, rtol=B16.LOSS_RTOL, atol=B16.LOSS_ATOL, err_msg=what)
        B16.check_grads(e.grad_critic, o.last_grads["critic"], E.CRITIC_LAYOUT, what + " critic gradient")
        if was_actor_call:
            B16.check_grads(e.grad_actor, o.last_grads["actor"], E.ACTOR_LAYOUT, what + " actor gradient")
        B16.check_params(e, o, E, what + " parameters", was_actor_call)
        B16.assert_images_current(e, E, what)
        np.testing.assert_allclose(e._errors.cpu().numpy(), err, rtol=B16.LOSS_RTOL, atol=B16.LOSS_ATOL, err_msg=what + " errors")


@pytest.mark.parametrize("kind", ["td3", "noln"])
def test_td3_and_no_layernorm(E, shared, kind):
    """TD3 (use_bc = 0, LeakyReLU 0.01: the head kernel's non-ReLU instantiation) and layer_norm = False (Mlp::no_ln through the head), B = 48, n_main
    = 43, three calls against the restatement under the bars of (a)"""
    from tests.test_hirl_gpu import assert_losses, check_params, sync_oracle

    sh, B, nm = shared, 48, 43
    params = sh.params if kind == "td3" else D.plain_layernorm(sh.params)
    kw = dict(use_bc=False, slope=0.01) if kind == "td3" else dict(layer_norm=False)
    e = per_engine(E, B, params, replay_of(sh.ring), **kw)
    o = H.HirlOracle(params["actor"], params["critic"], None if kind == "td3" else params["bc_actor"], **kw)
    rng = np.random.default_rng([15, kind == "td3"])
    for k in range(3):
        idx, ibc, noise, w = draw_call(rng, B, nm)
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        engine_call(e, sh, idx, ibc, noise, nm, w)
        what = f"{kind} call {k}"
        ref, err = checked(E, e, o, oracle_args(sh.data, idx, ibc, noise, nm, use_bc=kind != "td3"), w, nm, was_actor_call, what + " gradients")
        n = 2 if kind == "td3" else 6
        assert_losses(e.losses_host()[:n], ref[:n], what)
        np.testing.assert_allclose(e._errors.cpu().numpy(), err, rtol=ERR_RTOL, atol=ERR_ATOL, err_msg=what + " errors")
        check_params(e, o, E, what + " params", was_actor_call)


@pytest.mark.parametrize("mode", ["binding", "never"])
def test_with_a_gradient_clip(E, shared, mode):
    """set_grad_clip beside set_prioritized (no code of its own: the clip lives in _adam): max_norm from the restatement's own unclipped norms — half the
    smaller (both optimizers clip) or four times the larger (none) — against the restatement behind tests/_hirl_clip.ClippedAdam, three calls"""
    import copy

    from tests.test_hirl_gpu import assert_losses, check_params, sync_oracle

    sh, B, nm = shared, 48, 43
    e = per_engine(E, B, sh.params, replay_of(sh.ring))
    o = C.install_clip(H.HirlOracle(sh.params["actor"], sh.params["critic"], sh.params["bc_actor"]), 1.0)
    rng = np.random.default_rng(16)
    for k in range(3):
        idx, ibc, noise, w = draw_call(rng, B, nm)
        was_actor_call = e.actor_trainable
        sync_oracle(o, e, E)
        args = oracle_args(sh.data, idx, ibc, noise, nm)
        probe = copy.deepcopy(o)
        probe.clip["max_norm"] = 1e30
        W.weighted_learn(probe, *args, weights=w, n_main=nm)
        free = [probe.last_norms["critic"]] + ([probe.last_norms["actor"]] if was_actor_call else [])
        c = 0.5 * min(free) if mode == "binding" else 4.0 * max(free)
        o.clip["max_norm"] = c
        e.set_grad_clip(c)
        engine_call(e, sh, idx, ibc, noise, nm, w)
        what = f"clip {mode} call {k}"
        ref, err = checked(E, e, o, args, w, nm, was_actor_call, what + " gradients")
        assert_losses(e.losses_host(), ref, what)
        np.testing.assert_allclose(e._errors.cpu().numpy(), err, rtol=ERR_RTOL, atol=ERR_ATOL)
        coefs = e.grad_norms_host()[1]
        for which, name in ((0, "critic"),) + (((1, "actor"),) if was_actor_call else ()):
            assert (coefs[which] < 1.0) == (mode == "binding") == (o.last_coefs[name] < 1.0), (what, name, coefs, o.last_coefs)
        check_params(e, o, E, what + " params", was_actor_call)


# ---- (i) refusals and drivers ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_engine_refusals(E, shared):
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay, PrioritizedReplay, SuccessUpsampler

    sh, B = shared, 16
    rep = replay_of(sh.ring)
    e = per_engine(E, B, sh.params, rep)
    idx, ibc, noise, w = draw_call(np.random.default_rng(17), B, B)
    e.assemble(sh.ring, torch.from_numpy(idx).cuda(), bc_table=sh.bc, idx_bc=torch.from_numpy(ibc).cuda())
    before = {k: t.clone() for k, t in LS.state_tensors(e).items()}
    batch = E.HxBatch(e.rows.data_ptr(), e.bc_rows.data_ptr(), B, e._noise.data_ptr())
    nets, hyper, st = ctypes.byref(e.nets), ctypes.byref(e.hyper), _lib.stream_ptr()
    wp, ep = e._weights.data_ptr(), e._errors.data_ptr()

    def call(n=nets, b=batch, h=hyper, weights=wp, nw=B, errors=ep):
        _lib.call("hx_hirl_critic_grads_weighted", n, None if b is None else ctypes.byref(b), h, weights, nw, errors, 0, st)

    for kw in (dict(n=None), dict(b=None), dict(h=None), dict(b=E.HxBatch(e.rows.data_ptr(), None, 24, e._noise.data_ptr())),
               dict(b=E.HxBatch(e.rows.data_ptr(), None, 0, e._noise.data_ptr()))):
        with pytest.raises(_lib.HxError, match="batch must be a positive multiple of 16"):
            call(**kw)
    for bad in (-1, B + 1):
        with pytest.raises(_lib.HxError, match="is not in 0..batch"):
            call(nw=bad)
    with pytest.raises(_lib.HxError, match="weights may be NULL only with n_weighted == 0"):
        call(weights=None, nw=1)
    with pytest.raises(_lib.HxError, match="errors_out.batch. is required"):
        call(errors=None)
    with pytest.raises(_lib.HxError, match="null rows, workspace or losses"):
        call(b=E.HxBatch(None, None, B, e._noise.data_ptr()))
    torch.cuda.synchronize()
    now = LS.state_tensors(e)
    assert not [k for k in before if not LS.bits_equal(before[k], now[k])]  # a refused call launches nothing
    # the engine's own refusals
    with pytest.raises(TypeError, match="PrioritizedReplay"):
        LS.make_engine(E, B, sh.params).set_prioritized(DeviceReplay(64))
    with pytest.raises(ValueError, match="new_rows='max'"):
        LS.make_engine(E, B, sh.params).set_prioritized(rep, new_rows="td")
    x = LS.make_engine(E, B, sh.params)
    x.sharded_sequence = True
    with pytest.raises(_lib.HxError, match="runs on one GPU"):
        x.set_prioritized(rep)
    x = LS.make_engine(E, B, sh.params)
    x.set_upsample(SuccessUpsampler(rep), None)
    with pytest.raises(_lib.HxError, match="does not go with set_upsample"):
        x.set_prioritized(rep)
    with pytest.raises(_lib.HxError, match="does not go with set_prioritized"):
        e.set_upsample(SuccessUpsampler(rep), None)
    with pytest.raises(_lib.HxError, match="another replay"):
        e.sample(PrioritizedReplay(64), None, sh.bc)
    with pytest.raises(_lib.HxError, match="set_prioritized first"):
        LS.make_engine(E, B, sh.params).sample(rep, None, sh.bc, u=torch.zeros(B, device="cuda"))
    with pytest.raises(_lib.HxError, match="set_weights goes with set_prioritized"):
        LS.make_engine(E, B, sh.params).set_weights(w, B)
    with pytest.raises(ValueError, match="n_main is 0..batch"):
        e.set_weights(w, B + 1)
    env = BatchedHarfangEnv(64, scenario="straight_line", device="cuda", seed=1, max_step=50, auto_reset=True, random_reset=True, replay=rep)
    env.reset()
    calls0 = (e.critic_step, e.sample_calls, e.act_calls)
    with pytest.raises(_lib.HxError, match="step_learn: set_prioritized"):
        e.step_learn(env, None, sh.bc)
    assert (e.critic_step, e.sample_calls, e.act_calls) == calls0
    e.sharded_sequence = True
    with pytest.raises(_lib.HxError, match="learn: prioritized replay runs on one GPU"):
        e.learn()
    e.sharded_sequence = False


def recorded(fn):
    from hirl4ucav_amd import _lib

    names, real = [], _lib.call
    _lib.call = lambda name, *args: names.append(name) or real(name, *args)
    try:
        fn()
    finally:
        _lib.call = real
    return names


@pytest.mark.parametrize("clip", [None, 0.5])
def test_switched_off_the_parents_paths_call_for_call(E, shared, clip):
    """never prioritized, and prioritized then set_prioritized(None): the same library calls name for name over three sample() + learn() rounds, none of
    them new, and the same bits; switched on, the one call gives way to the stages with the weighted entry point in front and the draw and the update
    around them"""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    sh, B = shared, 16
    rep = replay_of(sh.ring)
    expert = DeviceReplay(D.N_EXPERT_ROWS)
    expert.store_rows(sh.exp)
    plain, back, on = (LS.make_engine(E, B, sh.params) for _ in range(3))
    back.set_prioritized(rep)
    back.set_prioritized(None)
    on.set_prioritized(rep)
    for e in (plain, back, on):
        e.set_grad_clip(clip)

    def rounds(e):
        for k in range(3):
            e.sample(rep, expert, sh.bc, n_main=B - 4, seed=9, defer=(k == 1))
            e.learn(bc_weight_now=100 if k == 0 else None, bc_warm_up_weight=0.05)

    seq = [recorded(lambda e=e: rounds(e)) for e in (plain, back, on)]
    assert seq[0] == seq[1] and not set(seq[0]) & set(NEW_CALLS + PER_CALLS)
    LS.assert_same_state(plain, back, "prioritized replay switched off again")
    assert back.prioritized is None and plain.per_calls == back.per_calls == 0
    assert ("hx_hirl_learn_sampled" in seq[0]) == (clip is None)
    assert seq[2].count("hx_hirl_critic_grads_weighted") == seq[2].count("hx_per_sample") == seq[2].count("hx_per_update") == 3 == on.per_calls
    assert not {"hx_hirl_learn_sampled", "hx_hirl_critic_grads", "hx_hirl_critic_grads_sampled"} & set(seq[2])
    assert seq[2].count("hx_adam_clipped" if clip else "hx_adam") == 3 + 2 and ("hx_adam" in seq[2]) == (clip is None)
    at = [i for i, n in enumerate(seq[2]) if n in ("hx_sample_batch", "hx_per_sample", "hx_hirl_critic_grads_weighted", "hx_per_update")]
    assert [seq[2][i] for i in at[:4]] == ["hx_sample_batch", "hx_per_sample", "hx_hirl_critic_grads_weighted", "hx_per_update"]


PER = ["--hirl_per", "--per_beta_annealing", "0.01"]


@pytest.mark.parametrize("kind", ["hirl", "td3", "bf16"])
def test_train_all_hirl_per(E, tmp_path, monkeypatch, capsys, kind):
    """2 driver episodes of 12 steps at 64 envs, HIRL soft (fp32 and --dtype bf16) and TD3: the loop takes the reference's order and names the reason, every
    acting launch is followed by one mark_new, every learn() is a draw, the weighted stage and an update; the snapshot carries the flag, the call word
    and the priorities; without the flag no new call is made"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import COMMON, HIRL, spy

    args = (["--agent", "TD3"] + COMMON if kind == "td3" else HIRL) + (["--dtype", "bf16"] if kind == "bf16" else [])
    real_load = T.load_expert_tables
    names, runs, writers = spy(monkeypatch)
    if kind == "td3":
        monkeypatch.setattr(T, "load_expert_tables", real_load)  # (spy's hook copies the expert ring, which TD3 has not)
    out_dir = T.main(T.parse_args(args + PER + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert "vector loop: reference order (--hirl_per: the front launch draws before the step's insert" in out
    learns = names.count("hx_hirl_critic_grads_weighted")
    assert learns == 2 * 11 and "hx_hirl_front" not in names and "hx_hirl_learn_sampled" not in names and "hx_hirl_critic_grads" not in names
    assert names.count("hx_per_update") == names.count("hx_per_sample") == learns and names.count("hx_actor_act_step") == 2 * 12  # (n_main > 0 from step 0 on)
    assert names.count("hx_per_mark_new") == 2 * 12 + 1  # behind every acting launch, and once behind the exploration steps
    for i, n in enumerate(names):
        if n == "hx_actor_act_step":
            assert "hx_per_mark_new" in names[i + 1:i + 6], names[i:i + 6]
    snap = torch.load(os.path.join(out_dir, "state_rank0.pt"), map_location="cpu", weights_only=False)
    assert snap["engine"]["prioritized"] is True and snap["engine"]["per_calls"] == names.count("hx_per_sample") > 0
    per = snap["replay"]["per"]
    n_live = min(snap["replay"]["total"], 4096)
    assert per["marked"] == snap["replay"]["total"] and (per["prio"][:n_live] > 0).all() and torch.isfinite(per["prio"]).all()
    assert len(torch.unique(per["prio"])) > (20 if kind == "td3" else 5) and per["beta"] == pytest.approx(0.4 + 0.01 * snap["engine"]["per_calls"])
    assert torch.isfinite(snap["engine"]["arena"]).all()
    assert [v for t, v, _ in writers[0].rows if t == "stats/per_beta"]
    del names[:]
    T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    assert names and not set(names) & set(NEW_CALLS + PER_CALLS) and "hx_hirl_front" in names


def test_train_all_hirl_per_resume(E, tmp_path):
    """--separate_launches (one env workgroup: the run is reproducible): 1 episode + --resume to 2 equals the uninterrupted run bit for bit — the arena
    but its logged loss slots (sums of float atomics: rtol 1e-6 / atol 1e-7, as tests/test_hirl_clip_gpu.py), the replay ring, the priorities, pmax,
    marked, beta and the call word; --resume under the other setting is refused by the flag's name, both ways"""
    from hirl4ucav_amd import train_all as T
    from tests.test_branch_gpu import HIRL

    args = HIRL + PER + ["--separate_launches"]
    whole = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    half = T.main(T.parse_args(args + ["--episodes", "1", "--result_dir", str(tmp_path / "b")]))
    rest = T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "c"), "--resume", half]))
    a, b = (torch.load(os.path.join(d, "state_rank0.pt"), map_location="cpu", weights_only=False) for d in (whole, rest))
    assert a["driver"]["episode"] == b["driver"]["episode"] == 2 and a["engine"]["counters"] == b["engine"]["counters"]
    assert a["engine"]["per_calls"] == b["engine"]["per_calls"] > 0
    e = E.HirlEngine(batch=128)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    x, y = a["engine"]["arena"].clone(), b["engine"]["arena"].clone()
    np.testing.assert_allclose(x[lo:lo + 8].numpy(), y[lo:lo + 8].numpy(), rtol=1e-6, atol=1e-7)
    x[lo:lo + 8], y[lo:lo + 8] = 0, 0
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "arena"
    assert a["replay"]["total"] == b["replay"]["total"] and torch.equal(a["replay"]["ring"].view(torch.int32), b["replay"]["ring"].view(torch.int32))
    pa, pb = a["replay"]["per"], b["replay"]["per"]
    assert torch.equal(pa["prio"].view(torch.int32), pb["prio"].view(torch.int32)) and torch.equal(pa["pmax"].view(torch.int32), pb["pmax"].view(torch.int32))
    assert (pa["marked"], pa["beta"]) == (pb["marked"], pb["beta"])
    with pytest.raises(SystemExit, match="was run with --hirl_per"):
        T.main(T.parse_args(HIRL + ["--separate_launches", "--episodes", "2", "--result_dir", str(tmp_path / "d"), "--resume", half]))
    plain = T.main(T.parse_args(HIRL + ["--separate_launches", "--episodes", "1", "--result_dir", str(tmp_path / "e")]))
    with pytest.raises(SystemExit, match="was run without --hirl_per"):
        T.main(T.parse_args(args + ["--episodes", "2", "--result_dir", str(tmp_path / "f"), "--resume", plain]))
