"""CPU restatement of the two SacAgent keywords the clip pull request builds (TEST INFRASTRUCTURE ONLY), applied to any oracle.sac_oracle.SacOracle
(or a subclass: tests/_isac_check.IsacCheck, tests/_per_check.WeightedSacOracle) — they all hand each gradient dict to `opt.step(net, g)`:

    install_clip(o, max_norm)          update_params(optim, network, loss, grad_clip) (SAC/utils.py:15-21, SAC/agent.py:310-320): the gradient of each of
                                       q1, q2 and the policy is scaled by min(1, max_norm / (norm + 1e-6)) before its Adam step, as
                                       torch.nn.utils.clip_grad_norm_ forms it: the single whole-network clip this project builds.
                                       reference_passes=True: the reference's loop over network.modules(), which applies it to the whole network, to
                                       the inner Sequential (the same parameters again) and to every Linear on its own (reference_clip below).
    install_fixed_alpha(o, ent_coef)   SacAgent(entropy_tuning=False, ent_coef=x) (agent.py:108-110, 322-327): alpha = ent_coef, no log-alpha step,
    fixed_learn(o, ...)                entropy_loss reported as 0.

Pinned against the reference's own run by tests/test_sac_clip_cpu.py (tests/golden/sac_clip_learn.npz, tests/golden/gen_sac_clip_golden.py)."""
import torch

LINEARS = (("0.weight", "0.bias"), ("2.weight", "2.bias"), ("4.weight", "4.bias"))


def total_norm(g, keys=None):
    """clip_grad_norm_'s total norm: the 2-norm of the per-tensor 2-norms, in the gradients' dtype"""
    keys = list(g) if keys is None else keys
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g[k]) for k in keys]))


def clip_once(g, max_norm, keys=None):
    """one clip_grad_norm_(parameters, max_norm) over the tensors `keys` of g, in place -> (norm before, coefficient)"""
    keys = list(g) if keys is None else keys
    norm = total_norm(g, keys)
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    for k in keys:
        g[k].mul_(coef)
    return norm.item(), coef.item()


def reference_clip(g, max_norm):
    """`for p in network.modules(): clip_grad_norm_(p.parameters(), grad_clip)` for QNetwork / GaussianPolicy: the network, its Sequential (the same
    parameters), then Linear, ReLU, Linear, ReLU, Linear (a ReLU has no parameters: nothing happens) -> (norm, coefficient) of the FIRST pass"""
    first = clip_once(g, max_norm)
    clip_once(g, max_norm)
    for pair in LINEARS:
        clip_once(g, max_norm, list(pair))
    return first


class ClippedAdam:
    """an oracle Adam (oracle.hirl_oracle.Adam) behind the clip: step(params, grads) clips a copy of grads, records (norm, coefficient) into the
    shared log under `name`, then steps.  An object, not a closure: copy.deepcopy of the oracle (tests/test_hirl_gpu.oracle_checked) copies it whole."""

    def __init__(self, inner, name, cfg, log):
        self.inner, self.name, self.cfg, self.log = inner, name, cfg, log

    m = property(lambda self: self.inner.m)
    v = property(lambda self: self.inner.v)
    t = property(lambda self: self.inner.t, lambda self, x: setattr(self.inner, "t", x))

    def step(self, params, grads):
        g = {k: v.clone() for k, v in grads.items()}
        c = self.cfg["max_norm"]
        norm, coef = reference_clip(g, c) if self.cfg["reference_passes"] else clip_once(g, c)
        self.log["norms"][self.name], self.log["coefs"][self.name] = norm, coef
        self.inner.step(params, g)


def install_clip(o, max_norm, reference_passes=False):
    """put the three network optimisers of the oracle `o` behind the clip; o.last_norms / o.last_coefs [name] = the whole-network norm before clipping
    and its coefficient at the last step of q1, q2 and policy; o.clip["max_norm"] may be changed between calls.  o.last_grads keeps the gradients
    BEFORE clipping (what the engine's gradient buffers hold)."""
    o.clip = {"max_norm": float(max_norm), "reference_passes": bool(reference_passes)}
    o.last_norms, o.last_coefs = {}, {}
    log = {"norms": o.last_norms, "coefs": o.last_coefs}
    o.opt_q1, o.opt_q2, o.opt_pi = (ClippedAdam(opt, name, o.clip, log) for name, opt in (("q1", o.opt_q1), ("q2", o.opt_q2), ("policy", o.opt_pi)))
    return o


class FrozenAdam:
    """alpha_optim that never steps (it keeps the m / v / t a sync from an engine writes)"""

    def __init__(self, inner):
        self.m, self.v, self.t = inner.m, inner.v, inner.t

    def step(self, params, grads):
        pass


def install_fixed_alpha(o, ent_coef):
    """alpha = ent_coef for good and no log-alpha step; run the calls through fixed_learn(o, ...)"""
    o.ent_coef = float(ent_coef)
    o.opt_alpha = FrozenAdam(o.opt_alpha)
    o.alpha = torch.tensor([o.ent_coef], dtype=o.log_alpha.dtype)
    return o


def fixed_learn(o, *a, **k):
    """o.learn(...) under install_fixed_alpha: alpha = ent_coef before and after (the oracle's own last line sets exp(log_alpha): undone), the log-alpha
    state untouched; reports entropy_loss 0 and alpha = ent_coef as the reference does (agent.py:322-327: neither is computed)"""
    fixed = lambda: torch.tensor([o.ent_coef], dtype=o.log_alpha.dtype)  # noqa: E731
    o.alpha = fixed()
    out = o.learn(*a, **k)
    o.alpha = fixed()
    fix = lambda six: tuple(six[:3]) + (0.0, six[4], float(fixed().item())) + tuple(six[6:])  # noqa: E731
    return (fix(out[0]), out[1]) if isinstance(out[0], tuple) else fix(out)
