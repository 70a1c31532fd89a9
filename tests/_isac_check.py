"""CPU restatement of SacAgent.learn with imitative=True (reference hirl/agents/SAC/agent.py:276-359, 376-403) for the tests of the
imitative SAC branch.  TEST INFRASTRUCTURE ONLY.  Everything up to and including the two critic steps is oracle.sac_oracle.SacOracle's
arithmetic; then, with the UPDATED critics:

    a~, H     = policy.sample(s)                       q    = min(Q1, Q2)(s, a~)
    a_bc      = bc_actor(s)  (frozen)                  bc_q = min(Q1, Q2)(s, a_bc)
    bc_weight = mean(bc_q > q)                         a Python float: no gradient through it
    bc_loss   = mse(a_e, tanh(mean(s_e))) * 10000      on a second batch of B expert rows
    policy_loss = mean(-q - alpha H) (1 - bc_weight) + bc_loss bc_weight

bc_actor is the 13-input LayerNorm actor of oracle.hirl_oracle (leaky slope 0.01, what the reference's Actor.forward applies); the
reference constructs a 14-input one and crashes (departure 1 of the imitative branch).  PINNED by tests/test_isac_cpu.py against
tests/golden/isac_learn.npz, which tests/golden/gen_isac_golden.py records from the reference's own SacAgent.learn."""
import numpy as np
import torch

from oracle import hirl_oracle as H
from oracle import sac_oracle as S

ISAC_SEED0 = 31  # the golden generator steps upward from here until its two input conditions hold and stores the seed it used


def isac_params(seed):
    """policy, q1, q2 as tests/test_oracle_sac.sac_params draws them, then the frozen bc_actor — all a pure function of the seed"""
    rng = np.random.default_rng(seed)
    p = {"policy": S.init_mlp(rng, 13, 8), "q1": S.init_mlp(rng, 17, 1), "q2": S.init_mlp(rng, 17, 1)}
    p["bc_actor"] = H.init_actor(rng)
    return p


class IsacCheck(S.SacOracle):
    def __init__(self, policy, q1, q2, bc_actor, bc_slope=0.01, **kw):
        super().__init__(policy, q1, q2, **kw)
        self.bc_actor, self.bc_slope = H.to_torch(bc_actor), bc_slope
        self.last_gap = None

    def learn(self, batch, eps_next, eps_cur, expert_batch):
        """batch as SacOracle.learn; expert_batch = (s_e [B, 13], a_e [B, 4]).  -> (q1_loss, q2_loss, policy_loss (combined), entropy_loss,
        mean entropy, alpha after the step, bc_loss, bc_weight).  last_gap = (q, bc_q) per row; last_grads as SacOracle's."""
        s, a, r, ns, d = (torch.as_tensor(x, dtype=torch.float32) for x in batch)
        r, d = r.reshape(-1, 1), d.reshape(-1, 1)
        se, ae = (torch.as_tensor(x, dtype=torch.float32) for x in expert_batch)
        e1, e2 = torch.as_tensor(eps_next, dtype=torch.float32), torch.as_tensor(eps_cur, dtype=torch.float32)
        self.learning_steps += 1
        if self.learning_steps % self.interval == 0:  # agent.py:278-279
            with torch.no_grad():
                for t, src in ((self.q1_t, self.q1), (self.q2_t, self.q2)):
                    for k in t:
                        t[k].copy_(t[k] * (1.0 - self.tau) + src[k] * self.tau)
        sa = torch.cat([s, a], 1)
        with torch.no_grad():
            na, nh, _ = S.sample(self.policy, ns, e1)
            nsa = torch.cat([ns, na], 1)
            y = r + (1.0 - d) * self.gamma * (torch.min(S.mlp(self.q1_t, nsa), S.mlp(self.q2_t, nsa)) + self.alpha * nh)
        q1_loss = torch.mean((S.mlp(self.q1, sa) - y).pow(2))
        q2_loss = torch.mean((S.mlp(self.q2, sa) - y).pow(2))
        for name, net, opt, loss in (("q1", self.q1, self.opt_q1, q1_loss), ("q2", self.q2, self.opt_q2, q2_loss)):
            keys = list(net)
            g = dict(zip(keys, torch.autograd.grad(loss, [net[k] for k in keys])))
            self.last_grads[name] = {k: v.clone() for k, v in g.items()}
            opt.step(net, g)
        # calc_policy_loss, imitative (agent.py:376-403), with the UPDATED critics
        pa, ent, _ = S.sample(self.policy, s, e2)
        psa = torch.cat([s, pa], 1)
        q = torch.min(S.mlp(self.q1, psa), S.mlp(self.q2, psa))
        with torch.no_grad():
            bsa = torch.cat([s, H.actor_forward(self.bc_actor, s, self.bc_slope)], 1)
            bc_q = torch.min(S.mlp(self.q1, bsa), S.mlp(self.q2, bsa))
        bc_weight = (bc_q > q).float().mean().item()
        self.last_gap = (q.detach().numpy().ravel().copy(), bc_q.numpy().ravel().copy())
        mean_e, _ = S.policy_forward(self.policy, se)
        bc_loss = torch.nn.functional.mse_loss(ae, torch.tanh(mean_e)) * 10000
        policy_loss = torch.mean(-q - self.alpha * ent) * (1 - bc_weight) + bc_loss * bc_weight
        keys = list(self.policy)
        g = dict(zip(keys, torch.autograd.grad(policy_loss, [self.policy[k] for k in keys])))
        self.last_grads["policy"] = {k: v.clone() for k, v in g.items()}
        self.opt_pi.step(self.policy, g)
        entropy_loss = -torch.mean(self.log_alpha * (self.target_entropy - ent).detach())
        ga = torch.autograd.grad(entropy_loss, [self.log_alpha])[0]
        self.opt_alpha.step({"a": self.log_alpha}, {"a": ga})
        self.alpha = self.log_alpha.exp().detach()
        return (q1_loss.item(), q2_loss.item(), policy_loss.item(), entropy_loss.item(), ent.mean().item(), self.alpha.item(), bc_loss.item(),
                bc_weight)
