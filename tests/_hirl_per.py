"""CPU restatement of HirlEngine.set_prioritized's update (TEST INFRASTRUCTURE ONLY): oracle.hirl_oracle.HirlOracle.learn with importance weights on
the critic loss.  The reference's HIRL.py / TD3.py draw uniformly (a declared extension); the rule is include/hirl4ucav.h "Prioritized
replay for HIRL / TD3":

    critic_loss = mean_r(w_r (Q1 - y)^2) + mean_r(w_r (Q2 - y)^2)     both means over all B rows; w_r = weights[r] for r < n_main, exactly 1 behind
    errors_r    = |Q1(s, a) - y|_r                                     of every row
    the actor half                                                     unweighted: the oracle's own lines

Nothing of the oracle is copied: while its learn() runs, the `mse_loss` its critic lines call (the FIRST TWO calls of a learn(): Q1's and Q2's,
hirl_oracle.py:259) is substituted from outside by the weighted mean, the way tests/_hirl_clip.py puts ClippedAdam behind the oracle's optimisers; every
later call (the BC loss) goes to torch's.  Without weights nothing is substituted: the oracle's own code path.

    weighted_learn(o, batch, bc_batch, noise, w_now, warm, weights=None, n_main=None) -> (the oracle's 6-tuple, errors [B] or None)
    row_weights(B, weights, n_main)                                                   -> float32 [B]: weights[:n_main] ++ ones
    critic_grads64(o, batch, noise, w)                                               -> float64 autograd of the same formula on the oracle's state:
                                                                                        (loss, {key: gradient}, errors, y)"""
import numpy as np
import torch

from oracle import hirl_oracle as H


def row_weights(B, weights, n_main=None):
    n_main = B if n_main is None else int(n_main)
    w = np.ones(B, np.float32)
    w[:n_main] = np.asarray(weights, np.float32).reshape(-1)[:n_main]
    return w


class _WeightedF:
    """torch.nn.functional with mse_loss's first two calls replaced by mean(w (x - y)^2); the first call's |x - y| kept"""

    def __init__(self, real, w):
        self._real, self._w, self.calls, self.errors = real, w, 0, None

    def __getattr__(self, name):
        return getattr(self._real, name)

    def mse_loss(self, x, y, *args, **kw):
        self.calls += 1
        if self.calls > 2:
            return self._real.mse_loss(x, y, *args, **kw)
        if self.calls == 1:
            self.errors = (x.detach() - y).abs().reshape(-1).cpu().numpy().copy()
        return ((x - y).pow(2) * self._w.to(x.dtype).to(x.device)).mean()


def weighted_learn(o, batch, bc_batch, noise, bc_weight_now=0.0, bc_warm_up_weight=0.0, weights=None, n_main=None):
    if weights is None:
        return o.learn(batch, bc_batch, noise, bc_weight_now, bc_warm_up_weight), None
    B = np.asarray(batch[3]).shape[0]
    w = torch.from_numpy(row_weights(B, weights, n_main)).reshape(-1, 1)
    proxy, real = _WeightedF(H.F, w), H.F
    H.F = proxy
    try:
        out = o.learn(batch, bc_batch, noise, bc_weight_now, bc_warm_up_weight)
    finally:
        H.F = real
    assert proxy.calls >= 2
    return out, proxy.errors


def critic_grads64(o, batch, noise, w):
    """the rule's critic half in float64 from the oracle's CURRENT state (call it before the learn() it is compared with)"""
    f64 = torch.float64
    crit = {k: v.detach().to(f64).requires_grad_(True) for k, v in o.critic.items()}
    ta, tc = ({k: v.detach().to(f64) for k, v in net.items()} for net in (o.target_actor, o.target_critic))
    s, a, ns, r, d = (torch.as_tensor(np.asarray(x), dtype=torch.float32).to(f64) for x in batch)
    with H._Maybe(None if o.layer_norm else H.NoLayerNorm()):
        with torch.no_grad():
            eps = torch.as_tensor(np.asarray(noise), dtype=torch.float32).to(f64).clamp(-o.noise_clamp, o.noise_clamp)
            na = (H.actor_forward(ta, ns, o.slope) + eps).clamp(-1, 1)
            tq1, tq2 = H.critic_forward(tc, ns, na, o.slope)
            y = r.reshape(-1, 1) + o.gamma * torch.min(tq1, tq2) * (1 - d).reshape(-1, 1)
        q1, q2 = H.critic_forward(crit, s, a, o.slope)
        wt = torch.as_tensor(np.asarray(w, np.float32)).to(f64).reshape(-1, 1)
        loss = (wt * (q1 - y) ** 2).mean() + (wt * (q2 - y) ** 2).mean()
        keys = list(crit)
        grads = dict(zip(keys, torch.autograd.grad(loss, [crit[k] for k in keys], allow_unused=True)))
    grads = {k: (g if g is not None else torch.zeros_like(crit[k])) for k, g in grads.items()}
    return float(loss.detach()), grads, (q1.detach() - y).abs().reshape(-1).numpy(), y.reshape(-1).numpy()
