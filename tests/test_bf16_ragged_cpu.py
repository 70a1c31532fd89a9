"""Are the bf16 update's bars (tests/test_bf16_update_gpu.py: TIGHT for >= 99.8 % of a gradient tensor's entries, LOOSE for all, check_params,
the loss tolerances — set at B = 128) honest at the ragged batches of tests/test_bf16_ragged_gpu.py?  Two questions, both answered without a GPU:

  FAIR   the rounded-operand oracle with the kernels' fp32 accumulation (tests/_bf16_ragged.KernelSums: 32-wide slabs; dW2 in 32-row groups per
         half, the halves split at hr) passes every bar against the same oracle with fp64 sums, call by call from identical states, on every
         (case, B) the GPU file runs — so a miss on the GPU is not the rounding of a correct kernel.  A second stand-in, KernelSumsNearMisses,
         also rounds every h1 / dz2 element within an fp32 ulp of a bf16 rounding boundary the other way (the one difference between kernel and
         oracle that tests/test_bf16_update_gpu.py describes): one such element moves its whole row, and at B = 16 a row is 1/16 of the batch.
         A (case, B) on which either stand-in misses a bar gets another seed (tests/_bf16_ragged.REJECTED lists them), never another bar;
  TEETH  the fp64-sum gradient of the 256 -> 512 weight with the LAST 8 BATCH ROWS left out (what a wrong tail would compute), or counted twice
         (what a wrong clamp would compute), is REJECTED by check_grads at every B — so a wrong tail cannot pass."""
import copy
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hirl_oracle as H  # noqa: E402
from oracle import sac_oracle as S  # noqa: E402
from tests import _bf16_ragged as R  # noqa: E402
from tests import _sac_edges as X  # noqa: E402
from tests import test_bf16_update_gpu as U  # noqa: E402  (its bars and helpers; its tests are not collected from here)


@pytest.fixture(scope="module")
def E():
    from hirl4ucav_amd.agents import engine  # (the flat layouts only: nothing here touches a device)

    return engine


def flat(E, tree, layout, size):
    return E.pack(tree, layout, size, "cpu")


def as_engine(E, o):
    """the oracle's four networks as the flat buffers check_params reads from an engine"""
    return types.SimpleNamespace(actor=flat(E, o.actor, E.ACTOR_LAYOUT, E.ACTOR_SIZE), critic=flat(E, o.critic, E.CRITIC_LAYOUT, E.CRITIC_SIZE),
                                 target_actor=flat(E, o.target_actor, E.ACTOR_LAYOUT, E.ACTOR_SIZE),
                                 target_critic=flat(E, o.target_critic, E.CRITIC_LAYOUT, E.CRITIC_SIZE))


def worst(stats):
    return max(s[1] for s in stats), max(s[2] for s in stats)


STAND_INS = [pytest.param(R.KernelSums, id="fp32_sums"), pytest.param(R.KernelSumsNearMisses, id="near_misses")]


@pytest.mark.parametrize("sums", STAND_INS)
@pytest.mark.parametrize("case,B", R.HIRL_CASES)
def test_fp32_accumulation_in_the_kernels_grouping_passes_the_bf16_bars(E, case, B, sums):
    """FAIR, HIRL / TD3 / BC pre-training.  `lead` plays the engine: it runs with the stand-in `sums` and its own ReLU masks; the fp64-sum oracle starts every
    call from lead's state and takes lead's masks at the activation calls for which the GPU test hands over the kernel's (KernelKinks, KINK)."""
    lead = R.new_oracle(case)
    tight = loose = 0.0
    for k, (idx, ibc, noise) in enumerate(R.calls(case, B)):
        ref = copy.deepcopy(lead)
        what = f"{case} B={B} call {k}"
        if case == "bc":
            with R.Swapped(sums), H.Bf16Layer2(), R.RecordedMasks() as masks:
                got = H.bc_train_actor(lead, R.bc_batch_of(ibc))
            with H.Bf16Layer2(), U.KernelKinks({0: masks[0], 1: masks[1]}):
                exp = H.bc_train_actor(ref, R.bc_batch_of(ibc))
            np.testing.assert_allclose(got, exp, rtol=U.LOSS_RTOL, err_msg=what)
            was_actor = True
        else:
            was_actor, soft, use_bc = lead.actor_trainable, case != "td3", case != "td3"
            args = (R.batch_of(case, B, idx), R.bc_batch_of(ibc) if use_bc else None, noise) + ((R.SOFT, R.WARM) if use_bc else ())
            with R.Swapped(sums), H.Bf16Layer2(), R.RecordedMasks() as masks:
                got = lead.learn(*args)
            with H.Bf16Layer2(), U.KernelKinks({c: masks[c] for c in R.learn_mask_calls(was_actor, soft, use_bc)}):
                exp = ref.learn(*args)
            n = 6 if use_bc else 2
            np.testing.assert_allclose(got[:n], exp[:n], rtol=U.LOSS_RTOL, atol=U.LOSS_ATOL, err_msg=what)
            gc = flat(E, lead.last_grads["critic"], E.CRITIC_LAYOUT, E.CRITIC_SIZE)
            t, l = worst(U.grad_stats(gc, ref.last_grads["critic"], E.CRITIC_LAYOUT))
            tight, loose = max(tight, t), max(loose, l)
            U.check_grads(gc, ref.last_grads["critic"], E.CRITIC_LAYOUT, what + " critic gradient")
        if was_actor:
            ga = flat(E, lead.last_grads["actor"], E.ACTOR_LAYOUT, E.ACTOR_SIZE)
            t, l = worst(U.grad_stats(ga, ref.last_grads["actor"], E.ACTOR_LAYOUT))
            tight, loose = max(tight, t), max(loose, l)
            U.check_grads(ga, ref.last_grads["actor"], E.ACTOR_LAYOUT, what + " actor gradient")
        if case != "bc":
            U.check_params(as_engine(E, lead), ref, E, what + " parameters", was_actor)
    print(f"\n[bf16 ragged, {sums.__name__} vs fp64 sums] {case} B={B}: largest TIGHT-miss share {tight:.5f}, largest multiple of LOOSE {loose:.3f}")


@pytest.mark.parametrize("sums", STAND_INS)
@pytest.mark.parametrize("B", R.SAC_BATCHES)
def test_fp32_accumulation_passes_the_sac_bf16_bars(B, sums):
    """FAIR, SAC: the inputs of tests/_sac_edges.py case "ragged", the oracle through tests/test_sac_bf16_gpu.RoundedSac, the bars of
    test_sac_bf16_learn_against_the_rounded_operand_oracle.  The fp64-sum run takes lead's masks where the GPU test has the kernel's (kernel_masks)."""
    from tests import test_sac_bf16_gpu as B16

    p = X.case_params("ragged")
    lead = S.SacOracle(p["policy"], p["q1"], p["q2"])
    given = [c for i, k in enumerate([0, 4, 5, 2, 3, 1, 6, 7]) for c in ((2 * i, 2 * i + 1) if k not in (0, 4, 5) else (2 * i + 1,))]
    tight_worst = loose_worst = 0.0
    for k, (idx, e1, e2) in enumerate(X.calls("ragged", B)):
        ref = copy.deepcopy(lead)
        with R.Swapped(sums), B16.RoundedSac({}), R.RecordedMasks(S) as masks:
            got = lead.learn(X.batch_of(idx), e1, e2)
        with B16.RoundedSac({c: masks[c] for c in given}):
            exp = ref.learn(X.batch_of(idx), e1, e2)
        np.testing.assert_allclose(got, exp, rtol=B16.LOSS_RTOL, atol=B16.LOSS_ATOL, err_msg=f"B={B} call {k} losses")
        for name in ("q1", "q2", "policy"):
            for key in S.MLP_KEYS:
                x, r = lead.last_grads[name][key].numpy().ravel(), ref.last_grads[name][key].numpy().ravel()
                scale = max(np.abs(r).max(), 1e-30)
                tight = np.abs(x - r) <= B16.TIGHT[0] * np.abs(r) + B16.TIGHT[1] * scale
                tight_worst = max(tight_worst, float((~tight).mean()))
                loose_worst = max(loose_worst, float((np.abs(x - r) / (B16.LOOSE[0] * np.abs(r) + B16.LOOSE[1] * scale)).max()))
                assert tight.mean() >= 0.998, f"B={B} call {k} {name} {key}: {(~tight).sum()} entries beyond TIGHT"
                assert np.all(np.abs(x - r) <= B16.LOOSE[0] * np.abs(r) + B16.LOOSE[1] * scale), f"B={B} call {k} {name} {key}: beyond LOOSE"
        for a, b in ((lead.policy, ref.policy), (lead.q1, ref.q1), (lead.q2, ref.q2), (lead.q1_t, ref.q1_t), (lead.q2_t, ref.q2_t)):
            d = np.concatenate([np.abs(a[key].detach().numpy() - b[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-3 and d.max() <= 2.1e-3, f"B={B} call {k}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
    print(f"\n[sac bf16 ragged, {sums.__name__} vs fp64 sums] B={B}: largest TIGHT-miss share {tight_worst:.5f}, largest multiple of LOOSE {loose_worst:.3f}")


def tail(dz, h1, rows=8):
    """the last `rows` batch rows' share of dW2 = dz2^T h1, rounded operands, fp64"""
    return (dz[-rows:].t() @ h1[-rows:]).float()


@pytest.mark.parametrize("B", R.BATCHES)
def test_the_bars_reject_a_wrong_batch_tail(E, B):
    """TEETH: call 0 of ("soft", B) (an actor call).  The critic's full2 / full4 and the actor's full2 weight gradient minus, and plus, the share of
    the last 8 batch rows.  The actor's is the kernel's two-slot sum: w x (last 8 rows of actor(s_bc)) + (1 - w) x (last 8 rows of actor(s))."""
    o = R.new_oracle("soft")
    idx, ibc, noise = R.calls("soft", B)[0]
    with R.Captured() as log, H.Bf16Layer2():
        o.learn(R.batch_of("soft", B, idx), R.bc_batch_of(ibc), noise, R.SOFT, R.WARM)
    by_w = {}
    for ptr, dz, h1 in log:
        by_w.setdefault(ptr, []).append((dz, h1))
        assert dz.shape == (B, 512) and h1.shape == (B, 256)
    c2, c4, a2 = (by_w[t.data_ptr()] for t in (o.critic["full2.weight"], o.critic["full4.weight"], o.actor["full2.weight"]))
    # the critic's own step differentiates each head once (the first backward of that weight; Q1(s, pi) passes through full2 again later);
    # the actor's weight sees the BC loss's backward first, then the RL loss's (HirlOracle._learn, split_actor_grads)
    assert len(c2) == 2 and len(c4) == 1 and len(a2) == 2
    w = float(o.bc_weight)
    assert 0.0 < w < 1.0
    shares = {("critic", "full2.weight"): tail(*c2[0]), ("critic", "full4.weight"): tail(*c4[0]),
              ("actor", "full2.weight"): w * tail(*a2[0]) + (1.0 - w) * tail(*a2[1])}
    # the capture is the gradient: all B rows of the same operands give the oracle's tensor
    np.testing.assert_allclose(tail(*c2[0], rows=B).numpy(), o.last_grads["critic"]["full2.weight"].numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose((w * tail(*a2[0], rows=B) + (1.0 - w) * tail(*a2[1], rows=B)).numpy(), o.last_grads["actor"]["full2.weight"].numpy(), rtol=1e-5, atol=1e-9)
    for (net, key), share in shares.items():
        layout, size = (E.CRITIC_LAYOUT, E.CRITIC_SIZE) if net == "critic" else (E.ACTOR_LAYOUT, E.ACTOR_SIZE)
        U.check_grads(flat(E, o.last_grads[net], layout, size), o.last_grads[net], layout, "unchanged")
        for sign, what in ((-1.0, "left out"), (1.0, "counted twice")):
            wrong = dict(o.last_grads[net])
            wrong[key] = wrong[key] + sign * share
            stats = {s[0]: s for s in U.grad_stats(flat(E, wrong, layout, size), o.last_grads[net], layout)}[key]
            print(f"\n[bf16 ragged teeth] B={B} {net} {key}, last 8 rows {what}: {stats[1]:.4f} of the entries outside TIGHT, worst entry {stats[2]:.1f} x LOOSE")
            with pytest.raises(AssertionError):
                U.check_grads(flat(E, wrong, layout, size), o.last_grads[net], layout, f"B={B} {net} {key} {what}")
