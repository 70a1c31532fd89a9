"""GPU tests of prioritized replay for SAC (hx_per_* and hx_sac_learn_weighted through PrioritizedReplay, SacEngine, SacAgent and train_all).

The draw rule is this project's own, stated by the numpy model tests/_per_check.PerModel; the weighted loss arithmetic is the reference's, held to
the bars of tests/test_sac_gpu.py against tests/_per_check.WeightedSacOracle and the reference's recorded run (tests/golden/sac_per_learn.npz).
Smallest shapes that can still go wrong: a ring of 2,500 slots = three blocks of 1,024 with a ragged last one; batches 16, 48, 128."""
import json
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sac_oracle as S  # noqa: E402
from tests import _hirl_data as D  # noqa: E402
from tests import _per_check as P  # noqa: E402
from tests import _sac_bits  # noqa: E402
from tests import _sac_fold_bits  # noqa: E402
from tests.test_oracle_sac import sac_params  # noqa: E402
from tests.test_sac_gpu import grad_bad, sync  # noqa: E402

CAP = 2500
NETS = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i")


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


def new_replay(cap=CAP, live=None, **kw):
    from hirl4ucav_amd.utils.buffer import PrioritizedReplay

    rep = PrioritizedReplay(cap, **kw)
    rng = np.random.default_rng(cap)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(cap, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
    rep.total += cap if live is None else live
    return rep


def draw(rep, B, u=None, beta=0.4, seed=0, call=0):
    idx = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    w = torch.zeros(B, device="cuda")
    rows = torch.zeros((B, 32), device="cuda")
    rep.sample_into(B, idx, w, rows, u=None if u is None else torch.from_numpy(np.asarray(u, np.float32)).cuda(), seed=seed, call=call, beta=beta)
    assert torch.equal(rows, rep.ring[idx.long()])  # the gathered tile is the drawn rows
    return idx.cpu().numpy().astype(np.int64), w.cpu().numpy()


def check_sums(rep):
    """each block sum equals the float64 sum of its block within rtol 1e-6; the padding behind the capacity holds zeros"""
    pr = rep._prio.cpu().numpy().astype(np.float64)
    assert (pr[rep.capacity:] == 0).all()
    np.testing.assert_allclose(rep.bsum.cpu().numpy(), pr.reshape(-1, 1024).sum(1), rtol=1e-6, atol=0)


def integer_priorities():
    """integer priorities over 2,500 slots with total 2^12: a run of zeros inside block 0, the WHOLE middle block empty, zeros at the tail"""
    rng = np.random.default_rng(4)
    pr = np.zeros(CAP)
    pr[:1024] = rng.integers(0, 4, 1024)
    pr[300:340] = 0
    pr[2048:2400] = rng.integers(0, 6, 352)
    pr[2399] = 3
    pr[0] = 2
    nz = np.flatnonzero(pr > 0)
    q, r = divmod(int(4096 - pr.sum()), nz.size)  # top the live slots up to the total, still integers
    assert q >= 0
    pr[nz] += q
    pr[nz[:r]] += 1
    assert pr.sum() == 4096 and pr[1024:2048].sum() == 0 and pr[2400:].sum() == 0
    return pr


@pytest.mark.parametrize("B", [16, 48, 128])
def test_exact_draw_equals_the_model(SE, B):
    """Integer priorities with S = 2^12 and u = (k + 0.5) / S: every fp32 prefix sum and target is exact, so the slots equal the numpy model's
    EXACTLY — on both sides of every run of zeros and of the empty block.  u = 0 gives the first slot that holds priority; u = 1 - 2^-24 (the
    largest fp32 below 1: its target S - 2^-12 is exact here) the last one.  No draw returns an empty slot or one beyond the live length."""
    pr = integer_priorities()
    rep = new_replay()
    rep.set_priorities(np.arange(CAP), pr)
    check_sums(rep)
    m = P.PerModel(CAP)
    m.set(np.arange(CAP), pr)
    cum = np.cumsum(pr)
    edges = np.unique(np.concatenate([[0, 1, 4095, 4094], cum[[299, 339, 340, 1023, 2047, 2048, 2398]] - 1, cum[[299, 339, 1023, 2048]]]))
    edges = edges[(edges >= 0) & (edges < 4096)]
    rng = np.random.default_rng(B)
    ks = np.concatenate([edges, rng.choice(4096, 64 - edges.size, replace=False)])[:64]
    assert ks.size == 64
    u_all = np.concatenate([[0.0, 1.0 - 2.0 ** -24], (ks + 0.5) / 4096.0]).astype(np.float32)
    for lo in range(0, u_all.size, B):  # every one of the 66 targets, B at a time (the last batch wraps round)
        u = np.resize(u_all[lo:], B) if u_all[lo:].size < B else u_all[lo:lo + B]
        idx, w = draw(rep, B, u)
        np.testing.assert_array_equal(idx, m.draw(u.astype(np.float64)))
        assert (pr[idx] > 0).all() and (idx < CAP).all() and w.max() == 1.0
    idx, _ = draw(rep, 16, np.resize(np.float32([0.0, 1.0 - 2.0 ** -24]), 16))
    assert idx[0] == 0 and idx[1] == 2399
    # u = 1.0f (what a float64 uniform just below 1 rounds to): the target IS S, past every interval — the sampler's "rounded to S" path: the last
    # entry of the scan, then the nearest lower block and slot that hold priority.  With u S = S in every row, and beside ordinary targets.
    idx, w = draw(rep, B, np.ones(B, np.float32))
    assert (idx == 2399).all() and (w == 1.0).all()
    u = np.resize(np.float32([1.0, 0.25, 1.0, 0.75]), B)
    idx, _ = draw(rep, B, u)
    np.testing.assert_array_equal(idx, m.draw(u.astype(np.float64)))
    assert (idx[0::4] == 2399).all() and (idx[2::4] == 2399).all()


def test_philox_draw_is_proportional_and_keyed(SE):
    """Three classes of slots, p = 1, p = 4 and p = 0; 64 calls x 256 rows.  The fraction landing in the p = 4 class is within 5 sqrt(f (1 - f) / n)
    of f = 0.8 (a binomial bound; the seed is fixed, so this is deterministic); the empty class is never drawn; (seed, call) keys the draw."""
    pr = np.zeros(CAP)
    live = np.arange(2400)
    pr[live[live % 3 == 0]], pr[live[live % 3 == 1]] = 1.0, 4.0
    rep = new_replay()
    rep.set_priorities(np.arange(CAP), pr)
    hits = np.concatenate([draw(rep, 256, seed=9, call=c + 1)[0] for c in range(64)])
    assert (pr[hits] > 0).all() and hits.max() < 2400
    n, f = hits.size, 0.8
    got = (pr[hits] == 4.0).mean()
    print(f"p = 4 class: {got:.4f} of {n} draws (expected {f}, bound {5 * np.sqrt(f * (1 - f) / n):.4f})")
    assert abs(got - f) <= 5 * np.sqrt(f * (1 - f) / n)
    assert np.unique(hits).size > 1500  # (with replacement over 1,600 live slots)
    a, b, c = draw(rep, 256, seed=9, call=3)[0], draw(rep, 256, seed=9, call=3)[0], draw(rep, 256, seed=9, call=4)[0]
    assert np.array_equal(a, b) and np.array_equal(a, hits[2 * 256:3 * 256]) and not np.array_equal(a, c)
    assert not np.array_equal(a, draw(rep, 256, seed=10, call=3)[0])


@pytest.mark.parametrize("B", [16, 48, 128])
@pytest.mark.parametrize("beta", [0.4, 1.0])
def test_weights_match_the_model(SE, B, beta):
    """w_r = (n p_r / S)^-beta / max against the float64 model at rtol 2e-5 (the project's HIP-vs-oracle bar); the largest weight is exactly 1"""
    rng = np.random.default_rng(B)
    pr = np.zeros(CAP)
    pr[:2300] = rng.uniform(0.01, 3.0, 2300) ** 2
    rep = new_replay(live=2300)
    rep.set_priorities(np.arange(CAP), pr)
    m = P.PerModel(CAP)
    m.set(np.arange(CAP), pr.astype(np.float32))
    idx, w = draw(rep, B, rng.random(B), beta=beta)
    assert (idx < 2300).all() and w.max() == 1.0 and (w > 0).all()
    np.testing.assert_allclose(w, m.weights(idx, beta, 2300), rtol=2e-5, atol=0)
    if beta == 0.4:  # annealing on the host: beta <- min(1, beta + annealing) per sample call
        rep.beta, rep.beta_annealing = 0.9995, 0.0003
        assert rep.next_beta() == 0.9995 and rep.next_beta() == pytest.approx(0.9998) and rep.next_beta() == 1.0 and rep.next_beta() == 1.0


def live_invariants(rep, model=None):
    total = int(rep.total.item())
    live = min(total, rep.capacity)
    pr = rep.prio.cpu().numpy()
    assert (pr[:live] > 0).all() and (pr[live:] == 0).all(), "prio > 0 exactly on the live slots"
    assert rep.marked == total
    check_sums(rep)
    if model is not None:
        np.testing.assert_allclose(pr, model.prio, rtol=2e-5, atol=0)
    return total, pr


def test_mark_new_through_a_real_env(SE):
    """48 envs, act_step for 60 steps into a 2,500-slot ring (default, unordered slot allocation): the rows wrap the ring.  mark_new after each step;
    an update at step 10 raises pmax, so the slots written afterwards hold another value than the ones before.  Then one mark after MORE than the
    capacity arrived."""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    params = sac_params()
    e = SE.SacEngine(batch=16)
    e.load_params(params["policy"], params["q1"], params["q2"])
    from hirl4ucav_amd.utils.buffer import PrioritizedReplay

    rep = PrioritizedReplay(CAP)
    env = BatchedHarfangEnv(48, scenario="serpentine", seed=1, auto_reset=True, random_reset=True, replay=rep)
    env.reset()
    m = P.PerModel(CAP)
    since = []  # slots written since the update
    for step in range(1, 61):
        before = int(rep.total.item())
        e.act_step(env, seed=4)
        rep.mark_new(48)
        total = int(rep.total.item())
        assert 0 < total - before <= 48
        m.mark_new(total)
        since += [s % CAP for s in range(before, total)]
        if step == 10:
            idx, err = np.arange(0, 32, 2), np.linspace(2.0, 9.0, 16)
            rep.update(idx, err)
            m.update(idx, err)
            m.pmax = float(np.float32(rep.pmax))  # (the running maximum as the device rounded it: the slots marked later hold exactly this)
            since = []
        if step in (1, 52, 53, 60):
            total, pr = live_invariants(rep, m)
            pm = np.float32(rep.pmax)
            assert (pr[np.asarray(since[-CAP:], np.int64)] == pm).all(), "every slot written since the last update holds pmax"
            assert pm == (1.0 if step < 10 else np.float32(pr.max()))
    assert int(rep.total.item()) > CAP  # the ring wrapped (52 steps x 48 rows reach the capacity)
    # more than cap rows between two marks
    rep2 = PrioritizedReplay(CAP)
    env2 = BatchedHarfangEnv(48, scenario="serpentine", seed=1, auto_reset=True, random_reset=True, replay=rep2)
    env2.reset()
    for step in range(10):
        e.act_step(env2, seed=4)
    rep2.mark_new(480)
    rep2.update(np.arange(8), np.full(8, 4.0))
    for step in range(60):
        e.act_step(env2, seed=4)
    assert int(rep2.total.item()) - rep2.marked > CAP
    rep2.mark_new()
    _, pr = live_invariants(rep2)
    assert (pr == np.float32(rep2.pmax)).all() and rep2.pmax > 1.0


def test_update_priorities_duplicates_and_pmax(SE):
    rng = np.random.default_rng(6)
    pr0 = rng.uniform(0.2, 1.5, CAP)
    idx = rng.choice(CAP, 128, replace=False)
    idx[5], idx[77] = idx[20], idx[20]  # one slot three times: it keeps the maximum
    err = rng.normal(0, 2.0, 128)
    err[20], err[5], err[77] = 0.3, -6.5, 2.0
    err[9] = 0.0
    reps = []
    for _ in range(2):
        rep = new_replay()
        rep.set_priorities(np.arange(CAP), pr0)
        p_before = rep.pmax
        rep.update(idx, err)
        reps.append(rep)
        assert rep.pmax >= p_before
    rep = reps[0]
    m = P.PerModel(CAP)
    m.set(np.arange(CAP), pr0.astype(np.float32))
    m.update(idx, err.astype(np.float32))
    pr = rep.prio.cpu().numpy()
    np.testing.assert_allclose(pr[idx], m.prio[idx], rtol=2e-5, atol=0)
    np.testing.assert_allclose(pr[idx[20]], (6.5 + 1e-4) ** 0.6, rtol=2e-5)
    np.testing.assert_allclose(pr[idx[9]], 1e-4 ** 0.6, rtol=2e-5)
    untouched = np.setdiff1d(np.arange(CAP), idx)
    np.testing.assert_array_equal(pr[untouched], pr0.astype(np.float32)[untouched])
    np.testing.assert_allclose(rep.pmax, max(1.0, pr0.max(), m.prio[idx].max()), rtol=2e-5)
    check_sums(rep)
    # pmax never falls; a non-finite error leaves its slot as it was
    top = rep.pmax
    rep.update(idx[:16], np.full(16, 1e-3))
    assert rep.pmax == top
    keep = float(rep.prio[int(idx[40])].item())
    rep.update(idx[40:41], np.float32([np.nan]))
    assert float(rep.prio[int(idx[40])].item()) == keep
    check_sums(rep)
    # two runs of the same update: identical bits
    for name in ("_prio", "bsum", "_header"):
        rep_a, rep_b = new_replay(), new_replay()
        for r in (rep_a, rep_b):
            r.set_priorities(np.arange(CAP), pr0)
            r.update(idx, err)
        assert torch.equal(getattr(rep_a, name), getattr(rep_b, name)), name


def weighted_engine(SE, params, B, cap=CAP):
    rep = new_replay(cap)
    rep.mark_new()
    e = SE.SacEngine(batch=B)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_prioritized(rep)
    return e, rep


def weighted_call(SE, e, o, ring, rows_np, idx, w, eps, k):
    """one weighted learn() on the engine and on the checker (gradients under the strict elementwise rule, tests/test_hirl_gpu.oracle_checked)"""
    from tests.test_hirl_gpu import oracle_checked

    sync(o, e, SE)
    e.assemble(ring, torch.from_numpy(idx.astype(np.int32)).cuda())
    e._idx.copy_(torch.from_numpy(idx.astype(np.int32)))
    e.per_weights.copy_(torch.from_numpy(w))
    e.learn(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda())
    got, err = e.losses_host(), e.per_errors.cpu().numpy()
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

    rows = rows_np[idx]
    ref, ref_err = oracle_checked(o, lambda oo: oo.learn((rows[:, 0:13], rows[:, 13:17], rows[:, 30], rows[:, 17:30], rows[:, 31]), eps[0], eps[1], w),
                                  [(None, None, all_grads)], f"per call {k} gradients", module=S)
    print(f"call {k}: losses rel {np.max(np.abs(np.asarray(got) - ref) / (np.abs(ref) + 1e-12)):.2e}, errors abs {np.max(np.abs(err - ref_err)):.2e}")
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=f"per call {k} vs checker")
    np.testing.assert_allclose(err, ref_err, rtol=2e-5, atol=5e-6, err_msg=f"per call {k} errors vs checker")
    return got, err


def test_weighted_learn_matches_checker_and_reference(SE, golden_dir):
    """B = 128, the six recorded calls of the reference's SacAgent(per=True).learn, at exactly the bars of tests/test_sac_gpu.py (losses rtol 2e-5 /
    atol 5e-6 against the checker; the golden bars of its lines 113-114), errors_out at the checker's bar, the network probes as that test checks
    them; and the priorities the call leaves behind are (errors + 1e-4)^0.6."""
    g = np.load(os.path.join(golden_dir, "sac_per_learn.npz"))
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    assert D.checksum(params) == str(g["param_checksum"])
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e, rep = weighted_engine(SE, params, 128)
    o = P.WeightedSacOracle(params["policy"], params["q1"], params["q2"])
    for k in range(g["out"].shape[0]):
        got, err = weighted_call(SE, e, o, ring, data["replay"], g["idx"][k], g["weights"][k], g["eps"][k], k)
        others = [0, 1, 3, 4, 5]
        np.testing.assert_allclose(np.asarray(got)[others], np.asarray(g["out"][k])[others], rtol=5e-5, atol=2e-5, err_msg=f"per call {k} vs reference golden")
        np.testing.assert_allclose(got[2], g["out"][k][2], rtol=5e-5, atol=1e-4, err_msg=f"per call {k} policy_loss vs reference golden")
        np.testing.assert_allclose(err, g["errors"][k], rtol=5e-5, atol=2e-5, err_msg=f"per call {k} errors vs reference golden")
        sd = e.state_dicts()
        for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
            d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-4 and d.max() <= 2.1e-3, f"call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
        np.testing.assert_allclose(rep.prio[torch.from_numpy(g["idx"][k].astype(np.int64)).cuda()].cpu().numpy(), (err.astype(np.float64) + 1e-4) ** 0.6, rtol=2e-5)
    assert e.learning_steps == 6
    check_sums(rep)


@pytest.mark.parametrize("B", [16, 48])
def test_weighted_learn_at_ragged_batches(SE, B):
    """one and three 16-row tiles, two calls each, against the checker; the weights include an exact 0 and an exact 1"""
    params, data = sac_params(), D.make_data(D.DATA_SEED)
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    e, rep = weighted_engine(SE, params, B)
    o = P.WeightedSacOracle(params["policy"], params["q1"], params["q2"])
    rng = np.random.default_rng(B)
    for k in range(2):
        idx = rng.choice(D.N_REPLAY, B, replace=False)
        w = rng.uniform(0.05, 1.0, B).astype(np.float32)
        w[1], w[B - 2] = 0.0, 1.0
        eps = rng.normal(size=(2, B, 4)).astype(np.float32)
        weighted_call(SE, e, o, ring, data["replay"], idx, w, eps, k)


def test_unit_weights_against_the_plain_call(SE):
    """hx_sac_learn_weighted with w == 1 against hx_sac_learn from the same start, 3 calls at B = 128 (a power of two: mean(w) is exactly 1 and
    w / B exactly 1 / B).  The policy half runs the staged kernels the one call is bit-identical to, and the log-alpha step the same arithmetic on
    the same numbers.  The critics' TD head is a per-row kernel here (head_row) and a backward prologue there (head_regs from an LDS image): two
    instruction sequences for the same formula, which need not round alike (hx_bwd_body.h says so of its own two copies).  So EVERY buffer is held
    to a bar: the networks, the targets and the acting image of the policy's W2 to the checker's bar for parameters (tests/test_sac_gpu.py: entries off
    by more than 2e-6 rarer than 2e-4, none by more than 2.1e-3); the alpha state to rtol 2e-5; the Adam moments to the project's gradient rule — m is a
    linear combination of three gradients, so |dm| <= 1e-4 |m| + 2e-5 max|m| per network (grad_bad's rule), and v one of their squares, so twice the
    relative terms: |dv| <= 2e-4 |v| + 4e-5 max|v|.  Observed on an MI355X: max |diff| 1.5e-8 in policy and critic
    parameters (5,284 of 140,808 and 7,289 of 276,488 entries differ), 3.7e-9 in the targets, one ulp (1.2e-7) in the alpha state."""
    params = sac_params()
    rng = np.random.default_rng(8)
    e, rep = weighted_engine(SE, params, 128)
    p = SE.SacEngine(batch=128)
    p.load_params(params["policy"], params["q1"], params["q2"])
    for k in range(3):
        idx = torch.from_numpy(rng.choice(CAP, 128, replace=False).astype(np.int32)).cuda()
        for eng in (e, p):
            eng.assemble(rep.ring, idx)
            eng._seed = 13
        e._idx.copy_(idx)
        e.per_weights.fill_(1.0)
        e.learn()
        p.learn()
    worst = {}
    for name in NETS:
        a, b = getattr(e, name), getattr(p, name)
        worst[name] = (float((a - b).abs().max()), int((a != b).sum()), a.numel())
    print("unit weights vs hx_sac_learn, max |diff| / entries that differ / entries:", worst)
    np.testing.assert_allclose(e.losses.cpu().numpy()[:6], p.losses.cpu().numpy()[:6], rtol=2e-5, atol=5e-6)
    np.testing.assert_allclose(e.alpha_state.cpu().numpy(), p.alpha_state.cpu().numpy(), rtol=2e-5, atol=0)
    for name in ("policy", "critic", "target_critic", "w2_f32i"):
        d = (getattr(e, name) - getattr(p, name)).abs().cpu().numpy()
        assert (d > 2e-6).mean() < 2e-4 and d.max() <= 2.1e-3, (name, worst[name])
    Q = SE.Q_SIZE
    for name, parts in (("m_policy", [slice(None)]), ("v_policy", [slice(None)]), ("m_critic", [slice(0, Q), slice(Q, 2 * Q)]), ("v_critic", [slice(0, Q), slice(Q, 2 * Q)])):
        f = 2.0 if name[0] == "v" else 1.0
        for part in parts:
            got, ref = getattr(e, name)[part].cpu().numpy().astype(np.float64), getattr(p, name)[part].cpu().numpy().astype(np.float64)
            tol = f * (1e-4 * np.abs(ref) + 2e-5 * np.abs(ref).max())
            used = float((np.abs(got - ref) / tol).max())
            print(f"{name}[{part.start}:{part.stop}]: max |ref| {np.abs(ref).max():.3e}, worst entry uses {used:.3e} of its tolerance")
            assert np.abs(ref).max() > 0 and used <= 1.0, (name, part, used, worst[name])
    assert set(NETS) == {"policy", "critic", "target_critic", "w2_f32i", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state"}  # all of them are held above


def test_unchanged_paths_give_the_parents_bits(SE, golden_dir):
    """hx_sac_learn and the staged sequence ending in hx_sac_adam from a fixed start: the same bits as the recording made with the library of the
    commit before prioritized replay (tests/golden/sac_unchanged_bits.npz, tests/_sac_bits.py)"""
    g = np.load(os.path.join(golden_dir, "sac_unchanged_bits.npz"))
    now = _sac_bits.record(SE, sac_params())
    assert sorted(now) == sorted(g.files) and len(now) == 2 * len(_sac_bits.NAMES)
    for k in g.files:
        np.testing.assert_array_equal(now[k], g[k], err_msg=k)


def test_weighted_paths_give_the_parents_bits(SE, golden_dir):
    """hx_sac_learn_weighted from a fixed start (B = 48, non-unit weights, the Polyak step in call 3 of 4): the same bits as the recording made with
    the library of the commit before the weighted, clipped and scoring paths were folded into the shared code (tests/golden/sac_fold_bits.npz,
    tests/_sac_fold_bits.py) — networks, moments, alpha state, acting image, errors_out, the priorities hx_per_update leaves"""
    _sac_fold_bits.assert_replays(SE, sac_params(), np.load(os.path.join(golden_dir, "sac_fold_bits.npz")), ("weighted",))


def build_loop(SE, annealing=0.001):
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import PrioritizedReplay

    params = sac_params()
    rep = PrioritizedReplay(CAP, ordered_slots=True, beta_annealing=annealing)  # (row-tile order: the same inputs fill the ring in the same order)
    env = BatchedHarfangEnv(48, scenario="serpentine", seed=2, auto_reset=True, random_reset=True, replay=rep)
    env.reset()
    e = SE.SacEngine(batch=16)
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_prioritized(rep)
    return e, env, rep


def test_engine_loop_and_resume(SE, tmp_path):
    """SacEngine.step_learn with a prioritized replay (act_step -> mark_new -> sample -> learn -> update, the reference's order): 48 envs, 2,500
    slots, B = 16, 40 steps.  A snapshot at step 20 resumed to step 40 equals the uninterrupted run bit for bit: arena (but losses[0..2], logged sums of
    float atomics; losses[3..7] come from fixed-order sums and one thread and stay in the comparison), prio, pmax, marked.  A PER snapshot and a plain engine refuse each other."""
    from hirl4ucav_amd.utils import checkpoint as CK

    e, env, rep = build_loop(SE)
    snap = str(tmp_path / "state.pt")
    for step in range(40):
        if step == 20:
            CK.save_run(snap, e, env, rep, {"step": step})
        e.step_learn(env, act_seed=5, sample_seed=6)
    assert rep.slot_status() == 0
    assert all(torch.isfinite(getattr(e, name)).all() for name in NETS) and torch.isfinite(e.losses).all()
    total, pr = live_invariants(rep)
    assert total > 16 * 40 and np.isfinite(pr).all() and rep.pmax >= 1.0
    assert rep.beta == pytest.approx(0.4 + 40 * 0.001) and e.learning_steps == 40
    assert len(np.unique(pr[:min(total, CAP)])) > 40  # the drawn rows' priorities moved away from the entry value
    e2, env2, rep2 = build_loop(SE)
    assert CK.load_run(snap, e2, env2, rep2) == {"step": 20}
    assert rep2.beta == pytest.approx(0.4 + 20 * 0.001) and rep2.marked == int(rep2.total.item())
    for step in range(20, 40):
        e2.step_learn(env2, act_seed=5, sample_seed=6)
    lo = (e.losses.data_ptr() - e.arena.data_ptr()) // 4
    a, b = e.arena.clone(), e2.arena.clone()
    np.testing.assert_allclose(a[lo:lo + 3].cpu().numpy(), b[lo:lo + 3].cpu().numpy(), rtol=1e-4, atol=1e-6)
    a[lo:lo + 3], b[lo:lo + 3] = 0, 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "arena"
    for name in ("_prio", "bsum", "_header", "ring"):
        assert torch.equal(getattr(rep, name), getattr(rep2, name)), name
    assert rep.beta == rep2.beta and int(rep.total.item()) == int(rep2.total.item())
    # the flag is part of the run's state
    plain = SE.SacEngine(batch=16)
    with pytest.raises(ValueError, match="--per"):
        CK.load_engine_state(plain, CK.engine_state(e))
    with pytest.raises(ValueError, match="--per"):
        CK.load_engine_state(e, CK.engine_state(plain))
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    with pytest.raises(ValueError, match="--per"):
        CK.load_replay_state(DeviceReplay(CAP), CK.replay_state(rep))
    with pytest.raises(ValueError, match="--per"):
        CK.load_replay_state(rep, CK.replay_state(DeviceReplay(CAP)))


def test_engine_refusals(SE):
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.utils.buffer import DeviceReplay, PrioritizedReplay
    from tests.test_isac_gpu import bc_actor_params

    params = sac_params()
    rep = new_replay()
    rep.mark_new()

    def engine():
        e = SE.SacEngine(batch=16)
        e.load_params(params["policy"], params["q1"], params["q2"])
        return e

    e = engine()
    e.set_act_dtype("bf16")
    e.set_update_dtype("bf16")
    with pytest.raises(ValueError, match="prioritized replay is fp32 only"):
        e.set_prioritized(rep)
    e = engine()
    e.set_prioritized(rep)
    with pytest.raises(ValueError, match="prioritized replay is fp32 only"):
        e.set_act_dtype("bf16")
    with pytest.raises(_lib.HxError, match="imitative"):
        e.set_imitative(bc_actor_params())
    e = engine()
    e.set_imitative(bc_actor_params())
    with pytest.raises(_lib.HxError, match="imitative"):
        e.set_prioritized(rep)
    e = engine()
    e.world = 2
    with pytest.raises(_lib.HxError, match="one GPU"):
        e.set_prioritized(rep)
    e = engine()
    e.set_prioritized(rep)
    exp = DeviceReplay(64)
    exp.store_rows(torch.zeros((50, 32)))
    with pytest.raises(_lib.HxError, match="does not mix expert rows"):
        e.sample(rep, exp, n_main=8, seed=1)
    for switch in ("separate_critic_adam", "staged_policy"):
        setattr(e, switch, True)
        e.sample(rep, seed=1)
        with pytest.raises(_lib.HxError, match="no staged entry points"):
            e.learn()
        setattr(e, switch, False)
    with pytest.raises(TypeError):
        e.set_prioritized(DeviceReplay(CAP))
    with pytest.raises(ValueError, match="2\\^24"):
        PrioritizedReplay((1 << 24) + 1)  # (refused before anything is allocated)
    # the library's own refusals
    import ctypes

    from hirl4ucav_amd.utils.buffer import HxPer

    big = HxPer(rep._prio.data_ptr(), rep.bsum.data_ptr(), rep._header.data_ptr(), rep._header[1:].data_ptr(), rep._header[2:].data_ptr(),
                rep.total.data_ptr(), (1 << 24) + 1)
    with pytest.raises(_lib.HxError, match="2\\^24"):
        _lib.call("hx_per_mark_new", ctypes.byref(big), 16, _lib.stream_ptr())
    e.set_update_dtype("f32")
    e.nets.w2_bf16_all = rep._prio.data_ptr()  # (any non-NULL pointer: the check precedes every launch)
    with pytest.raises(_lib.HxError, match="fp32 only"):
        e.sample(rep, seed=1)
        e.learn()
    e.nets.w2_bf16_all = None


def test_facade_per(SE, tmp_path):
    """SacAgent(per=True): append with and without an error, sample -> (batch, indices, weights), update_priority, learn(False)"""
    from hirl4ucav_amd.agents.SAC.agent import PrioritizedDeviceMemory, SacAgent

    box = lambda n: types.SimpleNamespace(shape=(n,), sample=lambda: np.zeros(n, np.float32))  # noqa: E731
    ag = SacAgent(box(13), box(4), str(tmp_path / "log"), batch_size=16, lr=1e-3, hidden_units=[256, 512], memory_size=CAP, per=True, alpha=0.6, beta=0.4,
                  beta_annealing=0.01, log_interval=2, start_steps=0)
    assert isinstance(ag.memory, PrioritizedDeviceMemory) and ag.eng.prioritized is ag.memory
    logged = []
    ag.writer = types.SimpleNamespace(add_scalar=lambda tag, v, step: logged.append((tag, float(v), step)))
    rng = np.random.default_rng(2)
    np.random.seed(5)
    for i in range(300):
        tr = (rng.uniform(-1, 1, 13), rng.uniform(-1, 1, 4), float(rng.uniform(-5, 0)), rng.uniform(-1, 1, 13), False)
        if i % 2:
            ag.memory.append(*tr, error=0.5 + i / 100.0, episode_done=False)
        else:
            ag.memory.append(*tr, episode_done=False)
    assert len(ag.memory) == 300 and ag.memory.marked == 300 == int(ag.memory.total.item())
    pr = ag.memory.prio.cpu().numpy()
    np.testing.assert_allclose(pr[1:300:2], (0.5 + np.arange(1, 300, 2) / 100.0 + 1e-4) ** 0.6, rtol=2e-5)
    assert (pr[300:] == 0).all() and (pr[:300] > 0).all() and pr[0] == 1.0
    assert pr[298] == np.float32(pr[:298].max())  # without an error: the running maximum
    check_sums(ag.memory)
    out = ag.memory.sample(16)
    assert len(out) == 3
    (s, a, r, ns, d), indices, weights = out
    assert s.shape == (16, 13) and a.shape == (16, 4) and r.shape == (16, 1) and ns.shape == (16, 13) and d.shape == (16, 1)
    assert indices.shape == (16,) and int(indices.max()) < 300 and weights.shape == (16, 1) and float(weights.max()) == 1.0
    ag.memory.update_priority(indices.cpu().numpy(), np.full((16, 1), 7.0, np.float32))
    np.testing.assert_allclose(ag.memory.prio[indices.long()].cpu().numpy(), (7.0 + 1e-4) ** 0.6, rtol=2e-5)
    before, beta0, policy0 = ag.memory.prio.clone(), ag.memory.beta, ag.eng.policy.clone()
    for _ in range(4):
        ag.learn(False)
    drawn = ag.eng._idx.long()
    assert not torch.equal(before[drawn], ag.memory.prio[drawn]), "the priorities of the drawn slots change"
    want = P.PerModel(CAP)  # (drawn with replacement: a slot that came up more than once keeps the largest of its new priorities)
    want.update(drawn.cpu().numpy(), ag.eng.per_errors.cpu().numpy())
    np.testing.assert_allclose(ag.memory.prio[drawn].cpu().numpy(), want.prio[drawn.cpu().numpy()], rtol=2e-5)
    assert ag.memory.beta == pytest.approx(beta0 + 4 * 0.01) and not torch.equal(policy0, ag.eng.policy)
    tags = [t for t, _, _ in logged]
    assert tags.count("loss/policy") == 2 and all(np.isfinite(v) for _, v, _ in logged)
    check_sums(ag.memory)


def test_train_all_per_runs(SE, tmp_path, monkeypatch, capsys):
    """--agent SAC --type SAC --per at a small size for a few dozen steps: exits clean, says which loop runs and why, writes both scalars"""
    from hirl4ucav_amd import train_all as T
    from hirl4ucav_amd.utils.scalars import JsonlWriter

    monkeypatch.setattr(T, "make_writer", JsonlWriter)
    run = T.main(T.parse_args(["--agent", "SAC", "--type", "SAC", "--per", "--per_beta_annealing", "0.001", "--env", "serpentine", "--random", "--seed", "3",
                               "--num_envs", "64", "--buffer_size", "4096", "--max_step", "24", "--checkpoint_rate", "1000", "--snapshot_every", "0",
                               "--episodes", "2", "--result_dir", str(tmp_path / "a")]))
    out = capsys.readouterr().out
    assert "vector loop: reference order (--per: the front launch draws before the step's insert" in out and "Episode 2:" in out
    sc = [json.loads(ln) for ln in open(os.path.join(run, "summary", "scalars.jsonl"))]
    beta = [s["value"] for s in sc if s["tag"] == "stats/per_beta"]
    pmax = [s["value"] for s in sc if s["tag"] == "stats/per_max_priority"]
    assert len(beta) == 2 and len(pmax) == 2 and all(np.isfinite(beta + pmax))
    assert beta[0] == pytest.approx(0.4 + 0.001) and beta[1] == pytest.approx(0.4 + 24 * 0.001) and all(p >= 1.0 for p in pmax)


def test_sampling_with_nothing_marked_is_defined(SE):
    """S = 0 (sampled before anything was marked or set) is the caller's error, which the device cannot refuse: every row is slot 0 with weight 1"""
    rep = new_replay()
    idx, w = draw(rep, 48, np.linspace(0, 1, 48), beta=0.7)
    assert (idx == 0).all() and (w == 1.0).all()
    idx, w = draw(rep, 16, seed=3, call=1)
    assert (idx == 0).all() and (w == 1.0).all()


def test_exact_draw_beyond_2_23_slots(SE):
    """Beyond 2^23 slots the sampler's scan holds the block sums in PAIRS (8,192 entries of LDS for up to 16,384 blocks) and resolves the block inside
    the pair afterwards: a path no small ring reaches, so this one test runs at 2^23 + 2,048 slots (8,194 blocks, a 1 GB ring of zeros).  Integer
    priorities with S = 2^6 on the first and second block of several pairs, with empty pairs and empty partners in between: slots equal the model's."""
    from hirl4ucav_amd.utils.buffer import PrioritizedReplay

    cap = (1 << 23) + 2048
    rep = PrioritizedReplay(cap)
    rep.total += cap
    slots = np.array([5, 1023, 1024, 2047, 2 * 1024 * 3000 + 7, 2 * 1024 * 3000 + 1024 + 9, 1024 * 5001 + 100, 1024 * 8191 + 1023, 1024 * 8192, 1024 * 8193 + 1023, cap - 1])
    slots = np.unique(slots)
    pr = np.array([3, 1, 2, 6, 9, 4, 7, 5, 8, 10, 9][:slots.size], np.float64)
    pr[-1] += 64 - pr.sum()
    assert pr.sum() == 64 and (pr > 0).all() and slots.max() == cap - 1
    rep.set_priorities(slots, pr)
    rep.ring[torch.from_numpy(slots).cuda(), 0] = torch.arange(1, slots.size + 1, device="cuda", dtype=torch.float32)
    m = P.PerModel(cap)
    m.set(slots, pr)
    np.testing.assert_array_equal(np.flatnonzero(rep.bsum.cpu().numpy()), np.unique(slots // 1024))
    u = np.concatenate([(np.arange(64) + 0.5) / 64.0, [0.0, 1.0 - 2.0 ** -24, 1.0]]).astype(np.float32)
    for B in (48, 128):
        uu = np.resize(u, B)
        idx, w = draw(rep, B, uu)
        np.testing.assert_array_equal(idx, m.draw(uu.astype(np.float64)))
        assert np.isin(idx, slots).all() and w.max() == 1.0
    assert set(draw(rep, 128, np.resize(u, 128))[0]) == set(slots)  # every slot that holds priority is reachable, none else
