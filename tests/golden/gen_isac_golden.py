#!/usr/bin/env python3
"""Generate golden vectors for the IMITATIVE SAC update by running the REFERENCE SacAgent.learn with imitative=True
(hirl/agents/SAC/agent.py:276-359, 376-403).

Development container only.  The stubs are gen_sac_golden.py's (rltorch builder and memories, tensorboard).  After construction
`agent.bc_actor` is replaced by the reference's OWN Actor class with 13 inputs (the reference constructs it with 14 against the
13-wide observation and would crash: departure 1 of the imitative branch), loaded with generated weights, in eval(); and
`agent.expert_memory` is the stub memory, fed B rows of tests/_hirl_data.make_data's `expert_rows` per call.

Two conditions on the inputs are ASSERTED here, so that the reference alone decides whether they hold; the seed steps upward from
tests/_isac_check.ISAC_SEED0 (to 80 at most) until both do, and the seed used is stored:
  * the gate is exercised: 0 < bc_weight < 1 in at least 6 of the 8 calls, and the 8 weights take at least 4 distinct values;
  * no near-ties: over all 8 x 128 rows |bc_q - q| >= 1e-4 max(1, |q|) — 5 x the project's loss tolerance (rtol 2e-5), so an fp32
    evaluation elsewhere cannot flip a row and the integer count must match EXACTLY.
No network is rescaled: the generated weights are used as drawn.

    python tests/golden/gen_isac_golden.py   ->  tests/golden/isac_learn.npz
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "hirl"))

# ---- stubs (as gen_sac_golden.py) ------------------------------------------------------------------------------------
rl = types.ModuleType("rltorch")
rl.network = types.ModuleType("rltorch.network")
rl.memory = types.ModuleType("rltorch.memory")


def create_linear_network(input_dim, output_dim, hidden_units=[], hidden_activation="relu", output_activation=None, initializer="xavier"):
    layers, units = [], input_dim
    for nxt in hidden_units:
        layers += [nn.Linear(units, nxt), nn.ReLU()]
        units = nxt
    layers.append(nn.Linear(units, output_dim))
    return nn.Sequential(*layers)


class _Memory:
    def __init__(self, *a, **k):
        self.next_batch = None

    def sample(self, n):
        return self.next_batch

    def __len__(self):
        return 10 ** 6


rl.network.create_linear_network = create_linear_network
rl.memory.MultiStepMemory = _Memory
rl.memory.PrioritizedMemory = _Memory
sys.modules.update({"rltorch": rl, "rltorch.network": rl.network, "rltorch.memory": rl.memory})
tb = types.ModuleType("torch.utils.tensorboard")


class SummaryWriter:
    def __init__(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass


tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb

from tests import _hirl_data as D  # noqa: E402
from tests import _isac_check as C  # noqa: E402

import agents.SAC.agent as ref_sac  # noqa: E402
import torch.distributions.normal as tdn  # noqa: E402

torch.set_num_threads(1)
K, B = 8, 128


def run(seed):
    """-> (arrays to store, per-call bc_weights, q [K, B], bc_q [K, B]) of the reference's run on the inputs of `seed`"""
    params, data = C.isac_params(seed), D.make_data(D.DATA_SEED)
    rng = np.random.default_rng(seed + 1000)
    box = lambda n: types.SimpleNamespace(shape=(n,))  # noqa: E731
    agent = ref_sac.SacAgent(observation_space=box(13), action_space=box(4), log_dir=tempfile.mkdtemp(), batch_size=B, lr=1e-3,
                             hidden_units=[256, 512], memory_size=2e5, gamma=0.99, tau=0.005, imitative=True, cuda=False)
    sd = lambda p: {k: torch.tensor(v) for k, v in p.items()}  # noqa: E731
    agent.policy.policy.load_state_dict(sd(params["policy"]))
    for net in (agent.critic, agent.critic_target):
        net.Q1.Q.load_state_dict(sd(params["q1"]))
        net.Q2.Q.load_state_dict(sd(params["q2"]))
    agent.bc_actor = ref_sac.Actor(0.0001, 13, 4, 256, 512, True, "x").cpu()
    agent.bc_actor.load_state_dict(sd(params["bc_actor"]))
    agent.bc_actor.eval()
    agent.expert_memory = _Memory()
    draws = []

    def fake_standard_normal(shape, dtype, device):
        e = torch.tensor(rng.normal(0, 1, tuple(shape)).astype(np.float32))
        draws.append(e.numpy().copy())
        return e

    tdn._standard_normal = fake_standard_normal
    idx, idx_e, outs, prb, qs, bqs = [], [], [], [], [], []
    for k in range(K):
        i = rng.choice(D.N_REPLAY, B, replace=False)
        ie = rng.choice(D.N_EXPERT_ROWS, B, replace=False)
        rows, er = data["replay"][i], data["expert_rows"][ie]
        as_batch = lambda x: (torch.tensor(x[:, 0:13]), torch.tensor(x[:, 13:17]), torch.tensor(x[:, 30:31]), torch.tensor(x[:, 17:30]),  # noqa: E731
                              torch.tensor(x[:, 31:32]))  # (s, a, r, s', done)
        agent.memory.next_batch, agent.expert_memory.next_batch = as_batch(rows), as_batch(er)
        rec, seen = {}, []
        orig_c, orig_p, orig_e = agent.calc_critic_loss, agent.calc_policy_loss, agent.calc_entropy_loss

        def cc(b, w, orig=orig_c):
            out = orig(b, w)
            rec["q1"], rec["q2"] = out[0].item(), out[1].item()
            return out

        def cp(b, w, orig=orig_p):
            # the two critic evaluations inside calc_policy_loss, in order: (s, a~) then (s, bc_actor(s))
            hook = agent.critic.register_forward_hook(lambda m, inp, out: seen.append(torch.min(out[0], out[1]).detach().numpy().ravel().copy()))
            out = orig(b, w)
            hook.remove()
            rec["pi"], rec["ent"], rec["bc"], rec["w"] = out[0].item(), out[1].detach().mean().item(), out[2].item(), float(out[3])
            return out

        def ce(e, w, orig=orig_e):
            out = orig(e, w)
            rec["el"] = out.item()
            return out

        agent.calc_critic_loss, agent.calc_policy_loss, agent.calc_entropy_loss = cc, cp, ce
        agent.learn(False)
        agent.calc_critic_loss, agent.calc_policy_loss, agent.calc_entropy_loss = orig_c, orig_p, orig_e
        assert len(seen) == 2, len(seen)
        qs.append(seen[0]); bqs.append(seen[1])  # noqa: E702
        idx.append(i.astype(np.int32)); idx_e.append(ie.astype(np.int32))  # noqa: E702
        outs.append([rec["q1"], rec["q2"], rec["pi"], rec["el"], rec["ent"], agent.alpha.item(), rec["bc"], rec["w"]])
        row = []
        for net in (agent.policy.policy, agent.critic.Q1.Q, agent.critic.Q2.Q, agent.critic_target.Q1.Q, agent.critic_target.Q2.Q):
            flat = np.concatenate([v.detach().numpy().ravel() for v in net.state_dict().values()]).astype(np.float64)
            row.append((np.abs(flat).sum(), flat[D.probe_index(flat.size)]))
        prb.append(row)
    arrays = dict(idx=np.asarray(idx), idx_expert=np.asarray(idx_e), eps=np.asarray(draws, np.float32).reshape(K, 2, B, 4),
                  out=np.asarray(outs, np.float64), probe_abs=np.asarray([[p[0] for p in r] for r in prb]),
                  probe_val=np.asarray([[p[1] for p in r] for r in prb], np.float32), data_checksum=D.checksum(data),
                  param_checksum=D.checksum(params), seed=np.int64(seed))
    return arrays, [o[7] for o in outs], np.asarray(qs), np.asarray(bqs)


def conditions(weights, q, bc_q):
    inner = sum(0.0 < w < 1.0 for w in weights)
    distinct = len({round(w * B) for w in weights})
    gap = np.abs(bc_q - q) / np.maximum(1.0, np.abs(q))
    return inner >= 6 and distinct >= 4, int((gap < 1e-4).sum()), float(gap.min()), gap


def main():
    for seed in range(C.ISAC_SEED0, 81):
        arrays, weights, q, bc_q = run(seed)
        gate_ok, near, gmin, gap = conditions(weights, q, bc_q)
        print(f"seed {seed}: bc_weight*B {[round(w * B) for w in weights]} gate_ok {gate_ok}; rows inside the 1e-4 band {near}, smallest relative gap "
              f"{gmin:.2e}; gap quantiles 1 % {np.quantile(gap, 0.01):.2e} 50 % {np.quantile(gap, 0.5):.2e}")
        if gate_ok and near == 0:
            assert gate_ok and near == 0  # the two input conditions, decided by the reference's run alone
            arrays["min_rel_gap"] = np.float64(gmin)
            np.savez_compressed(os.path.join(HERE, "isac_learn.npz"), **arrays)
            print("stored seed", seed, "outputs of call 0", [round(v, 5) for v in arrays["out"][0]])
            return
    raise SystemExit("no seed in 31 .. 80 satisfies both input conditions: see the gap distribution printed above (the band is not widened)")


if __name__ == "__main__":
    main()
