"""Checkers for prioritized replay (test infrastructure only).

WeightedSacOracle — oracle.sac_oracle.SacOracle with SacAgent(per=True).learn's importance weights (SAC/agent.py:306-331, 361-374, 405, 408-414):
the per-row weights through the two critic losses, the policy loss and the entropy loss, and errors = |Q1(s, a) - y|.  Pinned against the
reference's own run by tests/test_per_cpu.py (tests/golden/sac_per_learn.npz, tests/golden/gen_sac_per_golden.py).

PerModel — a numpy model of the priority store (include/hirl4ucav.h "Prioritized replay"): float64 prefix sums, searchsorted, weights, the
maximum on duplicates.  The draw rule is this project's definition, so this model IS its statement."""
import numpy as np
import torch

from oracle import sac_oracle as S

EPS = 1e-4
BLOCK = 1024


class WeightedSacOracle(S.SacOracle):
    def learn(self, batch, eps_next, eps_cur, weights=None, dtype=None):
        """as SacOracle.learn, with weights [B] (None: the unweighted call) -> (the six outputs, errors [B])"""
        if weights is None:
            return super().learn(batch, eps_next, eps_cur, dtype=dtype), None
        dtype = self.dtype if dtype is None else dtype
        s, a, r, ns, d = (torch.as_tensor(x, dtype=dtype) for x in batch)
        r, d = r.reshape(-1, 1), d.reshape(-1, 1)
        w = torch.as_tensor(weights, dtype=dtype).reshape(-1, 1)
        e1, e2 = torch.as_tensor(eps_next, dtype=dtype), torch.as_tensor(eps_cur, dtype=dtype)
        self.learning_steps += 1
        if self.learning_steps % self.interval == 0:  # agent.py:278-279 — BEFORE the update
            with torch.no_grad():
                for t, src in ((self.q1_t, self.q1), (self.q2_t, self.q2)):
                    for k in t:
                        t[k].copy_(t[k] * (1.0 - self.tau) + src[k] * self.tau)
        sa = torch.cat([s, a], 1)
        with torch.no_grad():  # calc_target_q
            na, nh, _ = S.sample(self.policy, ns, e1)
            nsa = torch.cat([ns, na], 1)
            next_q = torch.min(S.mlp(self.q1_t, nsa), S.mlp(self.q2_t, nsa)) + self.alpha * nh
            y = r + (1.0 - d) * self.gamma * next_q
        cur_q1, cur_q2 = S.mlp(self.q1, sa), S.mlp(self.q2, sa)
        errors = torch.abs(cur_q1.detach() - y)                   # agent.py:366
        q1_loss = torch.mean((cur_q1 - y).pow(2) * w)             # agent.py:372-373
        q2_loss = torch.mean((cur_q2 - y).pow(2) * w)
        for name, net, opt, loss in (("q1", self.q1, self.opt_q1, q1_loss), ("q2", self.q2, self.opt_q2, q2_loss)):
            keys = list(net)
            g = dict(zip(keys, torch.autograd.grad(loss, [net[k] for k in keys])))
            self.last_grads[name] = {k: v.clone() for k, v in g.items()}
            opt.step(net, g)
        pa, ent, _ = S.sample(self.policy, s, e2)
        psa = torch.cat([s, pa], 1)
        q = torch.min(S.mlp(self.q1, psa), S.mlp(self.q2, psa))
        policy_loss = torch.mean((-q - self.alpha * ent) * w)     # agent.py:405
        keys = list(self.policy)
        g = dict(zip(keys, torch.autograd.grad(policy_loss, [self.policy[k] for k in keys])))
        self.last_grads["policy"] = {k: v.clone() for k, v in g.items()}
        self.opt_pi.step(self.policy, g)
        entropy_loss = -torch.mean(self.log_alpha * (self.target_entropy - ent).detach() * w)  # agent.py:411-413
        ga = torch.autograd.grad(entropy_loss, [self.log_alpha])[0]
        self.opt_alpha.step({"a": self.log_alpha}, {"a": ga})
        self.alpha = self.log_alpha.exp().detach()
        return ((q1_loss.item(), q2_loss.item(), policy_loss.item(), entropy_loss.item(), ent.mean().item(), self.alpha.item()),
                errors.reshape(-1).numpy().copy())


class PerModel:
    """the priority store in numpy: prio float64 [cap] (0 = not live), pmax, marked"""

    def __init__(self, cap, alpha=0.6):
        self.cap, self.alpha = int(cap), float(alpha)
        self.prio = np.zeros(self.cap, np.float64)
        self.pmax, self.marked = 1.0, 0

    def set(self, slots, p):
        slots, p = np.asarray(slots, np.int64), np.asarray(p, np.float64)
        self.prio[np.unique(slots)] = 0.0
        np.maximum.at(self.prio, slots, p)
        self.pmax = max(self.pmax, float(p.max()))

    def update(self, idx, errors):
        self.set(idx, (np.abs(np.asarray(errors, np.float64)) + EPS) ** self.alpha)

    def mark_new(self, total):
        new = total - self.marked
        if new >= self.cap:
            self.prio[:] = self.pmax
        else:
            self.prio[(self.marked + np.arange(new)) % self.cap] = self.pmax
        self.marked = total

    def bsum(self):
        nb = (self.cap + BLOCK - 1) // BLOCK
        pad = np.zeros(nb * BLOCK)
        pad[:self.cap] = self.prio
        return pad.reshape(nb, BLOCK).sum(1)

    def draw(self, u):
        """slots for the uniforms u in [0, 1): the slot whose interval of the running sum holds u S; a target at or past S (or on an empty slot):
        the nearest lower slot that holds priority"""
        cum = np.cumsum(self.prio)
        t = np.asarray(u, np.float64) * cum[-1]
        idx = np.searchsorted(cum, t, side="right")
        nz = np.flatnonzero(self.prio > 0)
        out = []
        for i in idx:
            i = min(int(i), self.cap - 1)
            if self.prio[i] <= 0:
                lower = nz[nz <= i]
                i = int(lower[-1]) if lower.size else int(nz[0])
            out.append(i)
        return np.asarray(out, np.int64)

    def weights(self, idx, beta, n_live):
        v = (n_live * self.prio[np.asarray(idx, np.int64)] / self.prio.sum()) ** (-float(beta))
        return v / v.max()
