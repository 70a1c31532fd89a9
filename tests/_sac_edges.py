"""Seeded inputs of the SAC edge cases, shared by tests/test_oracle_sac.py (CPU: are the inputs FAIR, i.e. does fp32 torch itself stay within the
gradient rule of the double-precision oracle on them?) and tests/test_sac_edges_gpu.py (the engine against the double-precision oracle).

Cases of the update (the networks of tests/test_oracle_sac.py::sac_params, changed as stated):
  ragged   nothing changed; batch sizes that are one row tile, an odd number of tiles, more than 128, more than 256 and a multiple of neither 32 nor 64
  upper    policy["4.bias"][4] += 3.5: log_std_0 above LOG_STD_MAX in every row (sigma_0 = e^2, clamp pass-through mask 0), and eps component 0 drawn
           so that x_0 = mean_0 + sigma_0 eps_0 is either small (|x| < ~3) or so large (|x| > 15) that tanh is exactly +-1 in fp32.  In between,
           1 - a^2 lies in (0, 1e-3), where one ulp of tanhf moves the gradient by a percent: no tolerance could be honest there.
  lower    policy["4.bias"][5] -= 25: log_std_1 below LOG_STD_MIN in every row (sigma_1 = e^-20)
  tie      q2 is a copy of q1: min(Q1, Q2) ties in every row, forever
Every minibatch holds a done = 1 row at index 0 and a done = 0 row at index 1."""
import copy

import numpy as np
import torch

from oracle import sac_oracle as S
from tests import _hirl_data as D

DATA_SEED, CALLS = 12, 3  # three calls: the third takes the Polyak step of the targets first
UPDATE_CASES = [("ragged", 16), ("ragged", 48), ("ragged", 144), ("ragged", 272), ("upper", 16), ("upper", 144), ("lower", 16), ("lower", 144), ("tie", 48)]
FAIR_IN_FP32 = [c for c in UPDATE_CASES if c[0] != "lower"]
GRAD_RTOL, GRAD_ATOL_OF_MAX = 1e-4, 2e-5  # tests/test_sac_gpu.py::grad_bad

_data = {}


def replay():
    if "replay" not in _data:
        _data["replay"] = D.make_data(DATA_SEED)["replay"]
    return _data["replay"]


def case_params(case):
    from tests.test_oracle_sac import sac_params

    p = sac_params()
    if case == "upper":
        p["policy"]["4.bias"][4] += 3.5
    elif case == "lower":
        p["policy"]["4.bias"][5] -= 25.0
    elif case == "tie":
        p["q2"] = {k: v.copy() for k, v in p["q1"].items()}
    elif case == "acting":  # both clamps in every row, and component 2's mean pushed towards saturation
        p["policy"]["4.bias"][4] += 3.5
        p["policy"]["4.bias"][5] -= 25.0
        p["policy"]["4.bias"][2] += 3.0
    else:
        assert case == "ragged", case
    return p


def _eps(rng, B, case):
    e = rng.normal(0, 1, (B, 4))
    if case == "upper":
        small = rng.random(B) < 0.6
        small[2], small[3] = False, True  # (both kinds in every tensor, whatever the draw)
        e[:, 0] = np.where(small, rng.uniform(-0.3, 0.3, B), rng.choice([-1.0, 1.0], B) * rng.uniform(2.2, 3.0, B))
    return e.astype(np.float32)


def calls(case, B):
    """-> CALLS x (idx int32 [B], eps_next [B, 4], eps_cur [B, 4]), a function of (case, B) alone"""
    rows, rng = replay(), np.random.default_rng(B)
    done, live = np.flatnonzero(rows[:, 31] == 1), np.flatnonzero(rows[:, 31] == 0)
    out = []
    for k in range(CALLS):
        idx = rng.integers(0, rows.shape[0], B).astype(np.int32)
        idx[0], idx[1] = done[k], live[k]
        out.append((idx, _eps(rng, B, case), _eps(rng, B, case)))
    return out


def batch_of(idx):
    r = replay()[idx]
    return r[:, 0:13], r[:, 13:17], r[:, 30], r[:, 17:30], r[:, 31]


def copy_state(dst, src):
    """everything SacOracle.learn reads or steps, from the oracle `src` into `dst` (of any dtype)"""
    with torch.no_grad():
        for a, b in ((dst.policy, src.policy), (dst.q1, src.q1), (dst.q2, src.q2), (dst.q1_t, src.q1_t), (dst.q2_t, src.q2_t), ({"a": dst.log_alpha}, {"a": src.log_alpha})):
            for k in a:
                a[k].copy_(b[k])
        for a, b in ((dst.opt_pi, src.opt_pi), (dst.opt_q1, src.opt_q1), (dst.opt_q2, src.opt_q2), (dst.opt_alpha, src.opt_alpha)):
            for k in a.m:
                a.m[k].copy_(b.m[k])
                a.v[k].copy_(b.v[k])
            a.t = b.t
    dst.alpha = src.alpha.to(dst.log_alpha.dtype)
    dst.learning_steps = src.learning_steps


def grad_ratio(got, ref):
    """max over the entries of |got - ref| / (1e-4 |ref| + 2e-5 max|ref|): the share of the gradient rule that `got` uses (<= 1: inside)"""
    g, x = np.asarray(ref, np.float64).ravel(), np.asarray(got, np.float64).ravel()
    tol = GRAD_RTOL * np.abs(g) + GRAD_ATOL_OF_MAX * max(np.abs(g).max(), 1e-30)
    return float((np.abs(x - g) / tol).max())


def fp32_against_fp64(case, B):
    """The fp32 oracle and the fp64 oracle, each call from the same (fp32) state — what the GPU test does with the engine in the fp32 oracle's place.
    -> the worst grad_ratio over calls, networks and tensors, and the fp64 head pre-activations (mean, raw log_std, x) of the last policy.sample(s)"""
    p = case_params(case)
    lead = S.SacOracle(p["policy"], p["q1"], p["q2"])
    worst, head = 0.0, None
    for idx, e1, e2 in calls(case, B):
        o32, o64 = copy.deepcopy(lead), S.SacOracle(p["policy"], p["q1"], p["q2"], dtype=torch.float64)
        copy_state(o64, lead)
        with torch.no_grad():
            out = S.mlp(o64.policy, torch.as_tensor(batch_of(idx)[0], dtype=torch.float64))
            head = (out[:, :4].numpy(), out[:, 4:].numpy(), (out[:, :4] + out[:, 4:].clamp(S.LOG_STD_MIN, S.LOG_STD_MAX).exp() * torch.as_tensor(e2, dtype=torch.float64)).numpy())
        o32.learn(batch_of(idx), e1, e2)
        o64.learn(batch_of(idx), e1, e2)
        for net in ("q1", "q2", "policy"):
            for k in S.MLP_KEYS:
                worst = max(worst, grad_ratio(o32.last_grads[net][k].numpy(), o64.last_grads[net][k].numpy()))
        lead = o32
    return worst, head
