#!/usr/bin/env python3
"""Generate golden vectors for the SAC update WITH GRADIENT CLIPPING and with a FIXED ENTROPY COEFFICIENT by running the REFERENCE
SacAgent(grad_clip=c).learn and SacAgent(entropy_tuning=False, ent_coef=0.2).learn (hirl/agents/SAC/agent.py:108-110, 310-327, SAC/utils.py:15-21).

Development container only: HIRL_REFERENCE names a checkout of the reference.  `rltorch` (un-vendored, unpinned) and `tensorboard` are absent from
this image: the stubs of tests/golden/gen_sac_per_golden.py stand in (the published builder shape Sequential(Linear, ReLU, Linear, ReLU, Linear), a
memory that returns the minibatch the generator chose), so what these vectors pin is the reference's CLIPPING (update_params' loop over
network.modules(), every pass of it), its update order and the fixed-alpha branch, not rltorch's initialiser or draw.

    HIRL_REFERENCE=<reference checkout> python tests/golden/gen_sac_clip_golden.py   ->  tests/golden/sac_clip_learn.npz
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
REF = os.environ["HIRL_REFERENCE"]
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "hirl"))

GRAD_CLIP = 1.4   # chosen so that q1, q2 AND the policy clip on at least four of the six calls (asserted below)
ENT_COEF = 0.2

# ---- stubs ---------------------------------------------------------------------------------------------------------
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
        self.tags = []

    def add_scalar(self, tag, *a, **k):
        self.tags.append(tag)


tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb

from oracle import sac_oracle as S  # noqa: E402
from tests import _hirl_data as D  # noqa: E402

import agents.SAC.agent as ref_sac  # noqa: E402
import torch.distributions.normal as tdn  # noqa: E402

torch.set_num_threads(1)
K = 6  # the Polyak step of the targets falls on calls 3 and 6


def run(rng, params, data, **kw):
    box = lambda n: types.SimpleNamespace(shape=(n,))  # noqa: E731
    agent = ref_sac.SacAgent(observation_space=box(13), action_space=box(4), log_dir=tempfile.mkdtemp(), batch_size=128, lr=1e-3,
                             hidden_units=[256, 512], memory_size=2e5, gamma=0.99, tau=0.005, cuda=False, **kw)  # train_sac.py:214-215 + the keywords
    sd = lambda p: {k: torch.tensor(v) for k, v in p.items()}  # noqa: E731
    agent.policy.policy.load_state_dict(sd(params["policy"]))
    for net in (agent.critic, agent.critic_target):
        net.Q1.Q.load_state_dict(sd(params["q1"]))
        net.Q2.Q.load_state_dict(sd(params["q2"]))
    draws, norms = [], []

    def fake_standard_normal(shape, dtype, device):
        e = torch.tensor(rng.normal(0, 1, tuple(shape)).astype(np.float32))
        draws.append(e.numpy().copy())
        return e

    tdn._standard_normal = fake_standard_normal
    # every clip_grad_norm_ pass the reference makes, in order: (number of tensors, norm it found)
    orig_clip = torch.nn.utils.clip_grad_norm_

    def recording_clip(parameters, max_norm, *a, **k):
        ps = list(parameters)
        n = orig_clip(ps, max_norm, *a, **k)
        norms.append((len(ps), float(n)))
        return n

    torch.nn.utils.clip_grad_norm_ = recording_clip
    idx, outs, prb, first = [], [], [], []
    for k in range(K):
        i = rng.choice(D.N_REPLAY, 128, replace=False)
        rows = data["replay"][i]
        agent.memory.next_batch = (torch.tensor(rows[:, 0:13]), torch.tensor(rows[:, 13:17]), torch.tensor(rows[:, 30:31]),
                                   torch.tensor(rows[:, 17:30]), torch.tensor(rows[:, 31:32]))  # (s, a, r, s', done)  train_sac.py:242
        rec, norms[:] = {"el": 0.0}, []
        orig_c, orig_p, orig_e = agent.calc_critic_loss, agent.calc_policy_loss, agent.calc_entropy_loss

        def cc(b, w, orig=orig_c):
            out = orig(b, w)
            rec["q1"], rec["q2"] = out[0].item(), out[1].item()
            return out

        def cp(b, w, orig=orig_p):
            out = orig(b, w)
            rec["pi"], rec["ent"] = out[0].item(), out[1].detach().mean().item()
            return out

        def ce(e, w, orig=orig_e):
            out = orig(e, w)
            rec["el"] = out.item()
            return out

        agent.calc_critic_loss, agent.calc_policy_loss, agent.calc_entropy_loss = cc, cp, ce
        agent.learn(False)
        agent.calc_critic_loss, agent.calc_policy_loss, agent.calc_entropy_loss = orig_c, orig_p, orig_e
        idx.append(i.astype(np.int32))
        outs.append([rec["q1"], rec["q2"], rec["pi"], rec["el"], rec["ent"], float(agent.alpha.item())])
        if kw.get("grad_clip") is not None:
            # per network: the wrapper (6 tensors), the Sequential (6), Linear (2), ReLU (0), Linear (2), ReLU (0), Linear (2)
            assert [n for n, _ in norms] == [6, 6, 2, 0, 2, 0, 2] * 3, [n for n, _ in norms]
            first.append([norms[0][1], norms[7][1], norms[14][1]])  # the whole-network norm BEFORE any clip: q1, q2, policy
        else:
            assert not norms
        row = []
        for net in (agent.policy.policy, agent.critic.Q1.Q, agent.critic.Q2.Q, agent.critic_target.Q1.Q, agent.critic_target.Q2.Q):
            flat = np.concatenate([v.detach().numpy().ravel() for v in net.state_dict().values()]).astype(np.float64)
            row.append((np.abs(flat).sum(), flat[D.probe_index(flat.size)]))
        prb.append(row)
    torch.nn.utils.clip_grad_norm_ = orig_clip
    return {"idx": np.asarray(idx), "eps": np.asarray(draws, np.float32).reshape(K, 2, 128, 4), "out": np.asarray(outs, np.float64),
            "probe_abs": np.asarray([[p[0] for p in r] for r in prb]), "probe_val": np.asarray([[p[1] for p in r] for r in prb], np.float32),
            "norms": np.asarray(first, np.float64), "tags": sorted(set(agent.writer.tags))}


def main():
    rng = np.random.default_rng(31)
    params = {"policy": S.init_mlp(rng, 13, 8), "q1": S.init_mlp(rng, 17, 1), "q2": S.init_mlp(rng, 17, 1)}
    data = D.make_data(D.DATA_SEED)
    c = run(rng, params, data, grad_clip=GRAD_CLIP)
    clips = (c["norms"] > GRAD_CLIP).sum(0)
    print("norms before clipping (q1, q2, policy) per call:\n", c["norms"], "\ncalls that clip:", clips)
    assert (clips >= 4).all(), "GRAD_CLIP must make all three networks clip on at least four of the six calls"
    f = run(rng, params, data, entropy_tuning=False, ent_coef=ENT_COEF)
    assert "loss/alpha" in c["tags"] and "loss/alpha" not in f["tags"]  # agent.py:322-327
    assert np.all(f["out"][:, 3] == 0.0) and np.all(f["out"][:, 5] == np.float32(ENT_COEF))
    np.savez_compressed(os.path.join(HERE, "sac_clip_learn.npz"), grad_clip=np.float64(GRAD_CLIP), ent_coef=np.float64(ENT_COEF),
                        data_checksum=D.checksum(data), param_checksum=D.checksum(params),
                        **{k: v for k, v in c.items() if k != "tags"}, **{"fixed_" + k: v for k, v in f.items() if k not in ("tags", "norms")})
    print("clip  q1", [round(o[0], 3) for o in c["out"]], "alpha", [round(o[5], 5) for o in c["out"]])
    print("fixed q1", [round(o[0], 3) for o in f["out"]], "alpha", [round(o[5], 5) for o in f["out"]])


if __name__ == "__main__":
    main()
