"""The fp32 SAC update and the Gaussian head where the other SAC tests never go: batch sizes other than 128, log_std at both clamps, tanh saturated
to exactly +-1, and min(Q1, Q2) on a tie.  The reference is the DOUBLE-PRECISION evaluation of the SAC oracle (oracle/sac_oracle.py, dtype=float64;
pinned to the reference's recorded run by tests/test_oracle_sac.py): at the lower clamp fp32 torch is not a reference (see
tests/test_oracle_sac.py::test_sac_edge_inputs_are_fair_in_float32), on the other inputs it stays within 0.04 x the gradient rule of fp64.

Inputs: tests/_sac_edges.py.  Tolerances: the project's own (tests/test_sac_gpu.py, tests/test_hirl_gpu.py) — logged outputs rtol 2e-5 / atol 5e-6,
every gradient entry |dg| <= 1e-4 |g| + 2e-5 max|g| with the ReLU-kink check of oracle_checked as the only accepted explanation of a miss, stepped
parameters and targets (d > 2e-6).mean() < 2e-4 and d.max() <= 2.1e-3, actions rtol 1e-5 / atol 2e-6."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sac_oracle as S  # noqa: E402
from tests import _sac_edges as X  # noqa: E402
from tests.test_sac_gpu import grad_bad, sync  # noqa: E402


@pytest.fixture(scope="module")
def SE():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd.agents import sac_engine

    return sac_engine


def head_buffers(e):
    """what the Gaussian heads of the last learn() left in the workspace (hx_sac.hip sac_aux, behind the slots): the actions of policy.sample(s')
    [B, 4], and the aux rows of policy.sample(s) [B, 16] = a[4], sigma eps[4], clamp pass-through mask[4], entropy"""
    B = e.batch
    p = e.ws[e.ws.numel() - 64 - 32 * B:].cpu().numpy()
    return p[:4 * B].reshape(B, 4), p[9 * B:25 * B].reshape(B, 16)


def run_update_case(SE, case, B):
    """CALLS calls of learn() with injected draws, the fp64 oracle synchronised to the engine before each"""
    from tests.test_hirl_gpu import oracle_checked

    params = X.case_params(case)
    ring = torch.from_numpy(X.replay()).cuda().contiguous()
    e = SE.SacEngine(batch=B)
    e.load_params(params["policy"], params["q1"], params["q2"])
    o = S.SacOracle(params["policy"], params["q1"], params["q2"], dtype=torch.float64)
    worst = {}
    for k, (idx, e1, e2) in enumerate(X.calls(case, B)):
        done = X.replay()[idx, 31]
        assert done[0] == 1 and done[1] == 0
        sync(o, e, SE)
        e.assemble(ring, torch.from_numpy(idx).cuda())
        e.learn(torch.from_numpy(e1).cuda(), torch.from_numpy(e2).cuda())
        got = e.losses_host()
        gq, gp = e.grad_critic.cpu().numpy(), e.grad_policy.cpu()
        engine_grads = {}
        for h, name in ((0, "q1"), (1, "q2")):
            engine_grads[name] = SE.unpack_mlp(torch.from_numpy(gq[h * SE.Q_SIZE:(h + 1) * SE.Q_SIZE]), SE.Q_BLOCK, 17, 1)
        engine_grads["policy"] = SE.unpack_mlp(gp, SE.POLICY_BLOCK, 13, 8)

        ratios = {}

        def all_grads(oo):  # every gradient tensor of the three networks against the oracle evaluation `oo` (the last one evaluated is the one accepted)
            bad = []
            for name in ("q1", "q2", "policy"):
                for key in S.MLP_KEYS:
                    x, g = engine_grads[name][key].numpy(), oo.last_grads[name][key].numpy()
                    bad += grad_bad(x, g, f"{case} B={B} call {k} {name} {key}")
                    ratios[(name, key)] = X.grad_ratio(x, g)
            return bad

        ref = oracle_checked(o, lambda oo: oo.learn(X.batch_of(idx), e1, e2), [(None, None, all_grads)], f"sac {case} B={B} call {k} gradients", module=S)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=5e-6, err_msg=f"sac {case} B={B} call {k} vs the fp64 oracle")
        for (name, key), v in ratios.items():
            worst[name] = max(worst.get(name, 0.0), v)
        sd = e.state_dicts()
        for name, ref_net in (("policy", o.policy), ("q1", o.q1), ("q2", o.q2), ("q1_target", o.q1_t), ("q2_target", o.q2_t)):
            d = np.concatenate([np.abs(sd[name][key].cpu().numpy() - ref_net[key].detach().numpy()).ravel() for key in S.MLP_KEYS])
            assert (d > 2e-6).mean() < 2e-4 and d.max() <= 2.1e-3, f"{case} B={B} call {k} {name}: {(d > 2e-6).sum()} off, max {d.max():.2e}"
        act_n, aux = head_buffers(e)
        assert np.isfinite(act_n).all() and np.isfinite(aux).all()
        if case == "upper":
            # the clamp's pass-through mask is 0 for component 0 alone, and both draws hold entries with tanh at exactly +-1
            assert (aux[:, 8] == 0).all() and (aux[:, 9:12] == 1).all()
            assert (np.abs(aux[:, 0]) == 1).any() and (np.abs(act_n[:, 0]) == 1).any(), f"{case} B={B} call {k}: no saturated entry"
            assert (np.abs(aux[:, 0]) < 1).any()
        elif case == "lower":
            assert (aux[:, 9] == 0).all() and (aux[:, [8, 10, 11]] == 1).all()
            # d log_std_1 = 0 in every row: the weight and bias gradients of that output are zeros, not small numbers
            assert not engine_grads["policy"]["4.weight"][5].any() and engine_grads["policy"]["4.bias"][5] == 0
            assert not o.last_grads["policy"]["4.weight"][5].any() and o.last_grads["policy"]["4.bias"][5] == 0
            assert engine_grads["policy"]["4.weight"][4].any() and engine_grads["policy"]["4.bias"][4] != 0
        else:
            assert (aux[:, 8:12] == 1).all()
        if case == "tie":  # identical critics stay identical: same target, same gradient, same step — and the policy sees (1/2 + 1/2) dQ/da
            assert torch.equal(e.critic[:SE.Q_SIZE], e.critic[SE.Q_SIZE:]) and torch.equal(e.target_critic[:SE.Q_SIZE], e.target_critic[SE.Q_SIZE:]), k
            assert torch.equal(e.grad_critic[:SE.Q_SIZE], e.grad_critic[SE.Q_SIZE:]), k
    assert e.learning_steps == X.CALLS == 3
    print(f"\n[sac edges] {case} B={B}: worst |dg| / tol against fp64 — " + ", ".join(f"{n} {worst[n]:.3f}" for n in ("q1", "q2", "policy")))


@pytest.mark.parametrize("case,B", X.UPDATE_CASES)
def test_sac_update_at_ragged_batches_clamp_edges_and_the_tie(SE, case, B):
    """learn() in fp32 against the fp64 oracle: losses, every gradient entry, stepped networks and targets, three calls (the third with the Polyak
    step first).  ragged: B = 16 / 48 / 144 / 272 (one row tile; an odd number of tiles; beyond 128; beyond 256, where the draw leaves the first
    launch, and a multiple of neither 32 nor 64).  upper: log_std_0 clamped at 2 in every row (mask 0) and a = +-1 exactly in part of the rows (the
    1 - a^2 + 1e-6 correction at its end).  lower: log_std_1 clamped at -20 (sigma = e^-20; fp64 is the only reference) — the gradient rows of that
    output are exactly zero.  tie: Q2 = Q1 — each critic takes half of min's gradient, and the two stay bit-equal.  (The tie is what found that the
    one-call learn() once compared "own head, evaluated here" with "other head, evaluated there" in each critic's job: the two evaluations differed in
    the last bit, and half of the rows gave both critics the weight 1 or both 0.  Measured on an MI355X, the engine uses at most 0.023 of the gradient
    rule on these nine cases.)"""
    run_update_case(SE, case, B)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# acting at the edges: both clamps in every row, component 2's mean pushed up, N(0, 1) draws
# ------------------------------------------------------------------------------------------------------------------------------------------------
def acting_inputs(n):
    rng = np.random.default_rng(n)
    return rng.uniform(-1, 1, (n, 13)).astype(np.float32), rng.normal(0, 1, (n, 4)).astype(np.float32)


def acting_reference(p, obs, eps):
    """fp64: exploit actions, explore actions, and the explore pre-activations x = mean + sigma eps"""
    o = S.SacOracle(p["policy"], p["q1"], p["q2"], dtype=torch.float64)
    with torch.no_grad():
        raw = S.mlp(o.policy, torch.as_tensor(obs, dtype=torch.float64))
        mean, log_std = S.policy_forward(o.policy, torch.as_tensor(obs, dtype=torch.float64))
        x = (mean + log_std.exp() * torch.as_tensor(eps, dtype=torch.float64)).numpy()
    raw = raw.numpy()
    assert (raw[:, 4] > S.LOG_STD_MAX).all() and (raw[:, 5] < S.LOG_STD_MIN).all()  # both clamps, every row
    return o.exploit(obs), o.explore(obs, eps), x


def check_edge_actions(got_x, got_e, ref_x, ref_e, x, what):
    for got in (got_x, got_e):
        assert np.isfinite(got).all() and (np.abs(got) <= 1).all(), what
    np.testing.assert_allclose(got_x, ref_x, rtol=1e-5, atol=2e-6, err_msg=f"{what}: exploit")
    np.testing.assert_allclose(got_e, ref_e, rtol=1e-5, atol=2e-6, err_msg=f"{what}: explore")
    far = np.abs(x) > 15
    assert far.any() and (got_e[far] == np.sign(x[far])).all(), f"{what}: tanh beyond |x| = 15 is exactly +-1"


def plain_act(e, obs, mode, eps=None, seed=0, call=0):
    from hirl4ucav_amd import _lib

    out = torch.empty((obs.shape[0], 4), dtype=torch.float32, device="cuda")
    _lib.call("hx_sac_act", e.policy.data_ptr(), None, None, None, obs.data_ptr(), obs.shape[0], out.data_ptr(), mode, _lib.ptr(eps), seed, 0, call, _lib.stream_ptr())
    return out


@pytest.mark.parametrize("n,fmt", [(37, "plain"), (37, "_f32i"), (8213, "_f32i"), (8213, "_x9")])
def test_sac_acting_at_the_clamps_and_saturation(SE, n, fmt):
    """exploit and explore (injected eps) against the fp64 oracle with log_std at both clamps in every row: 37 rows (two 16-row tiles and a tail of 5)
    through hx_sac_act without an image and from the fp32 image, 8,213 rows (the persistent kernel, past the 8,192-row switch) from the fp32 image and from
    the exact split (which falls back to the fp32 image up to 8,192 rows).  One Philox call per format; at 37 rows the two formats are bit-identical."""
    p = X.case_params("acting")
    e = SE.SacEngine(batch=16)
    e.load_params(p["policy"], p["q1"], p["q2"])
    e.x9_rows = 1 if fmt == "_x9" else None
    assert fmt == "plain" or e._act_format(n)[0] == fmt
    obs, eps = acting_inputs(n)
    go, ge = torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda()
    ref_x, ref_e, x = acting_reference(p, obs, eps)
    if fmt == "plain":
        got_x, got_e = plain_act(e, go, 0), plain_act(e, go, 1, eps=ge)
        e.act_calls = 7
        got_p = plain_act(e, go, 2, seed=9, call=8)
    else:
        got_x, got_e = e.act(go, explore=False), e.act(go, eps=ge)
        e.act_calls = 7
        got_p = e.act(go, seed=9)  # Philox(seed 9; row, call 8)
    check_edge_actions(got_x.cpu().numpy(), got_e.cpu().numpy(), ref_x, ref_e, x, f"{fmt} n={n}")
    a = got_p.cpu().numpy()
    assert np.isfinite(a).all() and (np.abs(a) <= 1).all() and (np.abs(a[:, 0]) == 1).any() and a.std() > 0.05
    if fmt == "_f32i" and n == 37:
        assert torch.equal(got_p, plain_act(e, go, 2, seed=9, call=8)) and torch.equal(got_e, plain_act(e, go, 1, eps=ge)) and torch.equal(got_x, plain_act(e, go, 0))


@pytest.mark.parametrize("n", [37, 8213])
def test_sac_bf16_acting_at_the_clamps_and_saturation(SE, n):
    """hx_sac_act from the bf16 image on the same inputs, against the evaluation on rounded operands and against the fp32 policy (the bounds of
    tests/test_sac_bf16_gpu.py); finite and inside [-1, 1], Philox included"""
    from tests.test_sac_bf16_gpu import check_actions, engine, rounded_policy

    p = X.case_params("acting")
    e, f = engine(SE, params=p), engine(SE, act="f32", params=p)
    obs, eps = acting_inputs(n)
    go, ge = torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda()
    mean, log_std = rounded_policy(p["policy"], obs)
    assert (log_std[:, 0] == 2.0).all() and (log_std[:, 1] == -20.0).all()
    got_x, got_e = e.act(go, explore=False).cpu().numpy(), e.act(go, eps=ge).cpu().numpy()
    check_actions(got_x, torch.tanh(mean).numpy(), f.act(go, explore=False).cpu().numpy(), f"edges exploit n={n}")
    check_actions(got_e, torch.tanh(mean + log_std.exp() * torch.from_numpy(eps)).numpy(), f.act(go, eps=ge).cpu().numpy(), f"edges eps n={n}")
    got_p = e.act(go, seed=9).cpu().numpy()
    for a in (got_x, got_e, got_p):
        assert np.isfinite(a).all() and (np.abs(a) <= 1).all()
    assert (np.abs(got_e[:, 0]) == 1).any() and (np.abs(got_p[:, 0]) == 1).any()
