"""Drop-in counterpart of agents.SAC.agent.SacAgent (reference hirl/agents/SAC/agent.py:58-448) for what train_sac.py uses:
constructor keywords, .memory.append / len(.memory), .batch_size, .explore / .exploit, .learn(if_expert, expert_num,
expert_data), .expert_memory, .writer, .model_dir / .plot_dir, .save_models — on the HIP kernels (SacEngine).  With
imitative=True (agent.py:315-318, 385-403): load_bc_actor, then learn() draws a second batch from .expert_memory for the
BC-gated policy loss and logs loss/bc and loss/bc_weight.  With per=True (agent.py:112-118, 281-284, 329-331): .memory is a prioritized
device memory — append(..., error), sample(n) -> (batch, indices, weights), update_priority(indices, errors) — and learn() carries the
weights through the three losses (the store and the draw rule are this project's: rltorch.PrioritizedMemory is un-vendored).  With multi_step=n
(2..8, uniform replay, not imitative; agent.py:121-124): .memory applies this project's truncated n-step rule on the host (rltorch.MultiStepMemory is
un-vendored too: include/hirl4ucav.h "n-step returns"), each row's discount folded into its done column, and the engine keeps the one-step gamma.

The networks are the Linear-ReLU stacks of the reference's un-vendored rltorch builder (initialisation: xavier-uniform
weights, zero biases — that builder is not in /root/reference, so its exact initialiser is not claimed).  The known crashes of
the reference (the 14-input bc_actor, train_episode's missing env) are not reproduced: the imitative branch's
bc_actor is the 13-input LayerNorm actor this project's BC agent writes.
"""
import os

import numpy as np
import torch

from ...utils.buffer import NSTEP_MAX, PER_EPS, DeviceReplay, HostNStep, PrioritizedReplay, device
from .. import sac_engine as SE


class _Writer:
    """SummaryWriter stand-in when tensorboard is absent (agent.writer is used by train_sac.py:217)."""

    def add_scalar(self, *a, **k):
        pass


class DeviceMemory(DeviceReplay):
    """rltorch MultiStepMemory's append / sample / len on the device ring (SAC/agent.py:121-124).  multi_step > 1: this project's truncated n-step
    rule (include/hirl4ucav.h "n-step returns") on the host, one transition per append — a row leaves the window once it holds multi_step steps, or
    with fewer at the episode's end (done: terminal; episode_done without done, or a next append that does not continue from the last next_state:
    truncated, bootstrapping from the last state seen), its discount folded into the done column."""

    def __init__(self, capacity, multi_step=1, gamma=0.99):
        super().__init__(int(capacity), device)
        self._len, self._pos = 0, 0
        self.multi_step = int(multi_step)
        self._window = HostNStep(self.multi_step, gamma) if self.multi_step > 1 else None

    def _store(self, row):
        self.ring[self._pos] = torch.from_numpy(row).to(self.device)
        self._pos = (self._pos + 1) % self.capacity
        self._len = min(self._len + 1, self.capacity)
        self.total += 1

    def append(self, state, action, reward, next_state, done, episode_done=None):  # train_sac.py:242
        if self._window is not None:
            for row, _ in self._window.append(state, action, reward, next_state, done, episode_done):
                self._store(row)
            return
        row = np.zeros(32, np.float32)
        row[0:13], row[13:17], row[17:30], row[30], row[31] = state, action, next_state, reward, float(done)
        self._store(row)

    def __len__(self):
        return self._len

    def sample_indices(self, n):
        return np.random.randint(low=0, high=self._len, size=n)  # rltorch memories draw with np.random.randint

    def sample(self, n):
        rows = self.ring[torch.as_tensor(self.sample_indices(n), device=self.device)]
        return rows[:, 0:13], rows[:, 13:17], rows[:, 30:31], rows[:, 17:30], rows[:, 31:32]


class PrioritizedDeviceMemory(PrioritizedReplay):
    """rltorch PrioritizedMemory's append / sample / update_priority / len as SacAgent uses them (SAC/agent.py:115-118, 244-246, 283-284, 331) on the
    device ring with the priority store of utils.buffer.PrioritizedReplay (multi_step = 1)."""

    def __init__(self, capacity, alpha=0.6, beta=0.4, beta_annealing=0.0001):
        super().__init__(int(capacity), device, alpha=alpha, beta=beta, beta_annealing=beta_annealing)
        self._len, self._pos, self._calls = 0, 0, 0
        self._slot = torch.zeros(1, dtype=torch.int32, device=self.device)

    def append(self, state, action, reward, next_state, done, error=None, episode_done=None):  # agent.py:244-246
        row = np.zeros(32, np.float32)
        row[0:13], row[13:17], row[17:30], row[30], row[31] = state, action, next_state, reward, float(done)
        self.ring[self._pos] = torch.from_numpy(row).to(self.device)
        if error is None:  # no TD error given: the row enters at the running maximum
            self.total += 1
            self.mark_new(1)
        else:
            self._slot.fill_(self._pos)
            self.set_priorities(self._slot, torch.full((1,), (abs(float(error)) + PER_EPS) ** self.alpha))
            self.total += 1
            self.marked_t += 1
        self._pos = (self._pos + 1) % self.capacity
        self._len = min(self._len + 1, self.capacity)

    def __len__(self):
        return self._len

    def sample(self, n):
        """-> (batch, indices, weights): batch = (s, a, r, s', d) as MultiStepMemory.sample returns it, indices int32 [n], weights [n, 1]"""
        self._calls += 1
        idx = torch.zeros(n, dtype=torch.int32, device=self.device)
        w = torch.zeros(n, dtype=torch.float32, device=self.device)
        rows = torch.zeros((n, 32), dtype=torch.float32, device=self.device)
        # rltorch memories draw with numpy's generator (a float64 uniform just below 1 rounds to 1.0f: the sampler takes u in [0, 1])
        u = torch.as_tensor(np.random.random_sample(n).astype(np.float32)).to(self.device)
        self.sample_into(n, idx, w, rows, u=u)
        return (rows[:, 0:13], rows[:, 13:17], rows[:, 30:31], rows[:, 17:30], rows[:, 31:32]), idx, w.reshape(-1, 1)

    def update_priority(self, indices, errors):  # agent.py:331
        self.update(torch.as_tensor(np.asarray(indices.cpu() if torch.is_tensor(indices) else indices)),
                    torch.as_tensor(np.asarray(errors.cpu() if torch.is_tensor(errors) else errors, np.float32)))


def _xavier_mlp(n_in, n_out):
    sd = {}
    for key, (o, i) in (("0", (256, n_in)), ("2", (512, 256)), ("4", (n_out, 512))):
        w = torch.empty(o, i)
        torch.nn.init.xavier_uniform_(w)
        sd[key + ".weight"], sd[key + ".bias"] = w, torch.zeros(o)
    return sd


class SacAgent:
    def __init__(self, observation_space, action_space, log_dir, num_steps=3000000, batch_size=256, lr=0.0003, hidden_units=[256, 256],
                 memory_size=1e6, gamma=0.99, tau=0.005, imitative=False, entropy_tuning=True, ent_coef=0.2, multi_step=1, per=False,
                 alpha=0.6, beta=0.4, beta_annealing=0.0001, grad_clip=None, updates_per_step=1, start_steps=10000, log_interval=300,
                 target_update_interval=3, eval_interval=1000, cuda=True):
        if tuple(observation_space.shape) != (13,) or tuple(action_space.shape) != (4,) or list(hidden_units) != [256, 512]:
            raise NotImplementedError("the HIP kernels are built for train_sac.py's shape: 13 / 4 / hidden [256, 512]")
        multi_step = int(multi_step)
        if ((per and imitative) or not 1 <= multi_step <= NSTEP_MAX or (multi_step != 1 and (per or imitative))
                or (imitative and (not entropy_tuning or grad_clip is not None))):
            raise NotImplementedError("built: uniform replay (with or without imitative=True) or prioritized replay (per=True, without imitative); multi_step 1, or "
                                      f"2..{NSTEP_MAX} with uniform replay and without imitative; without imitative also entropy_tuning=False (a fixed ent_coef) and "
                                      "grad_clip; per with imitative=True, multi_step != 1 with per=True or imitative=True, and "
                                      "entropy_tuning=False or grad_clip with imitative=True (SacEngine.set_grad_clip / set_entropy_tuning take them) are not")
        self.observation_space, self.action_space = observation_space, action_space
        self.device = device
        # multi_step > 1: every row carries its own discount in the done column ((1 - d') gamma = gamma^m), so the engine keeps the one-step gamma
        self.eng = SE.SacEngine(batch=batch_size, lr=lr, gamma=gamma, tau=tau, target_entropy=-float(np.prod(action_space.shape)),
                                target_update_interval=target_update_interval, device=device)
        self.eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
        if grad_clip is not None:  # update_params(optim, network, loss, grad_clip), agent.py:310-320
            self.eng.set_grad_clip(grad_clip)
        if not entropy_tuning:  # agent.py:108-110: a constant alpha, no log-alpha optimiser
            self.eng.set_entropy_tuning(False, ent_coef)
        self.grad_clip = grad_clip
        self.per = bool(per)
        if self.per:  # agent.py:112-118
            self.memory = PrioritizedDeviceMemory(memory_size, alpha=alpha, beta=beta, beta_annealing=beta_annealing)
            self.eng.set_prioritized(self.memory)
        else:
            self.memory = DeviceMemory(memory_size, multi_step=multi_step, gamma=gamma)
        self.expert_memory = None
        self.imitative = bool(imitative)  # the BC gate needs load_bc_actor(...) and an expert_memory before the first learn()
        self.log_dir = log_dir
        self.model_dir, self.summary_dir, self.plot_dir = (os.path.join(log_dir, d) for d in ("model", "summary", "plot"))
        for d in (self.model_dir, self.summary_dir, self.plot_dir):
            os.makedirs(d, exist_ok=True)
        try:
            from torch.utils.tensorboard import SummaryWriter

            self.writer = SummaryWriter(log_dir=self.summary_dir)
        except Exception:
            self.writer = _Writer()
        self.steps = self.episodes = 0
        self.batch_size, self.start_steps, self.tau = batch_size, start_steps, tau
        self.gamma_n, self.entropy_tuning, self.log_interval = gamma ** multi_step, entropy_tuning, log_interval
        self.target_update_interval = target_update_interval

    @property
    def learning_steps(self):
        return self.eng.learning_steps

    @property
    def alpha(self):
        return self.eng.alpha_state[3]

    def is_update(self):  # agent.py:170-172
        return len(self.memory) > self.batch_size and self.steps >= self.start_steps

    def explore(self, state):  # agent.py:183-188
        obs = torch.as_tensor(np.asarray(state, np.float32).reshape(1, 13)).to(device)
        eps = torch.randn(1, 4).to(device)  # Normal.rsample draws from torch's generator
        return self.eng.act(obs, eps=eps)[0].cpu().numpy().reshape(-1)

    def exploit(self, state):  # agent.py:191-196
        obs = torch.as_tensor(np.asarray(state, np.float32).reshape(1, 13)).to(device)
        return self.eng.act(obs, explore=False)[0].cpu().numpy().reshape(-1)

    def act(self, state):  # agent.py:175-180
        return self.action_space.sample() if self.start_steps > self.steps else self.explore(state)

    @staticmethod
    def _mlp(sd, x):
        h = torch.relu(x @ sd["0.weight"].T + sd["0.bias"])
        h = torch.relu(h @ sd["2.weight"].T + sd["2.bias"])
        return h @ sd["4.weight"].T + sd["4.bias"]

    @staticmethod
    def _rows(*cols):
        return [torch.as_tensor(c, dtype=torch.float32).to(device).reshape(-1, w) for c, w in zip(cols, (13, 4, 1, 13, 1))]

    def calc_current_q(self, states, actions, rewards, next_states, dones):  # agent.py:198-200
        """-> Q1(s, a), Q2(s, a) as [n, 1] tensors.  A plain forward over the engine's fp32 networks: the reference's train_episode calls it for ONE
        transition per env step (agent.py:234-246) and hands |Q1 - y| to memory.append(..., error); the vector loop's scoring pass is score_new."""
        s, a, _, _, _ = self._rows(states, actions, rewards, next_states, dones)
        sd = self.eng.state_dicts()
        with torch.no_grad():
            sa = torch.cat([s, a], 1)
            return self._mlp(sd["q1"], sa), self._mlp(sd["q2"], sa)

    def calc_target_q(self, states, actions, rewards, next_states, dones, eps=None):  # agent.py:202-210
        """-> y = r + (1 - d) gamma (min Q_target(s', a') + alpha H') as an [n, 1] tensor, a', H' = policy.sample(s') (SAC/model.py:62-82) with one
        torch.randn draw per row and component (eps [n, 4] injects them)"""
        _, _, r, ns, d = self._rows(states, actions, rewards, next_states, dones)
        sd = self.eng.state_dicts()
        with torch.no_grad():
            eps = torch.randn(ns.shape[0], 4).to(device) if eps is None else torch.as_tensor(eps, dtype=torch.float32).to(device).reshape(-1, 4)
            mean, log_std = torch.chunk(self._mlp(sd["policy"], ns), 2, dim=-1)
            log_std = torch.clamp(log_std, -20.0, 2.0)
            std = log_std.exp()
            x = mean + std * eps
            na = torch.tanh(x)
            log_prob = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - 0.5 * float(np.log(2 * np.pi))) - torch.log(1 - na.pow(2) + 1e-6)
            nh = -log_prob.sum(1, keepdim=True)
            nsa = torch.cat([ns, na], 1)
            next_q = torch.min(self._mlp(sd["q1_target"], nsa), self._mlp(sd["q2_target"], nsa)) + self.alpha * nh
            return r + (1.0 - d) * self.gamma_n * next_q

    def load_bc_actor(self, ajan, model_name=None, slope=0.01):  # agent.py:158-160
        """The frozen BC actor of the imitative branch: a state_dict (or a flat block), a path to the file the BC agent of this project
        writes, or the reference's two-argument call load_bc_actor(ajan, model_name) = the file <model_name>/<ajan>Harfang_GYM."""
        if model_name is not None:
            joined = os.path.join(str(model_name), str(ajan) + "Harfang_GYM")
            # (a file written by the reference on Linux is literally named 'dir\\tagName')
            ajan = joined if os.path.exists(joined) else (str(model_name) + "\\{}".format(ajan) + "Harfang_GYM" if os.path.exists(
                str(model_name) + "\\{}".format(ajan) + "Harfang_GYM") else joined)
        if isinstance(ajan, (str, os.PathLike)):
            if not os.path.isfile(ajan):
                raise FileNotFoundError(f"bc_actor checkpoint {ajan} not found (train one with --agent BC)")
            ajan = torch.load(ajan, map_location="cpu")
        self.eng.set_imitative(ajan, slope=slope)

    def _expert_batch(self):
        """expert_memory.sample(batch_size) (agent.py:392) -> the engine's second tile"""
        if not self.eng.imitative:
            raise RuntimeError("SacAgent(imitative=True).learn needs the frozen BC actor: call load_bc_actor(...) first")
        if self.expert_memory is None:
            raise RuntimeError("SacAgent(imitative=True).learn draws a second batch from agent.expert_memory, which is None: "
                               "set it to a memory holding the expert transitions")
        s, a, r, ns, d = self.expert_memory.sample(self.batch_size)
        self.eng.expert_rows.copy_(torch.cat([s, a, ns, r, d], 1).to(device).contiguous().reshape(-1))

    def learn(self, if_expert, expert_num=None, expert_data=None):  # agent.py:276-359
        B = self.batch_size
        if self.imitative:
            self._expert_batch()
        if self.per:  # agent.py:281-284, 306-331: batch, indices, weights from the memory (expert rows are not mixed in), priorities updated at the end
            (s, a, r, ns, d), indices, weights = self.memory.sample(B)
            self.eng.rows.copy_(torch.cat([s, a, ns, r, d], 1).contiguous().reshape(-1))
            self.eng._idx.copy_(indices)
            self.eng.per_weights.copy_(weights.reshape(-1))
            self.eng.learn(torch.randn(B, 4).to(device), torch.randn(B, 4).to(device))  # (ends in memory.update_priority(indices, errors) on the device)
            self._log()
            return
        if if_expert and expert_num:
            # expert rows were drawn by the caller (expert_memory.sample(expert_num), train_sac.py:272-273) and come last
            main = self.memory.ring[torch.as_tensor(self.memory.sample_indices(B - expert_num), device=device)]
            s, a, r, ns, d = expert_data
            rows = torch.cat([main, torch.cat([s, a, ns, r, d], 1).to(device)], 0).contiguous()
        else:
            rows = self.memory.ring[torch.as_tensor(self.memory.sample_indices(B), device=device)].contiguous()
        self.eng.rows.copy_(rows.reshape(-1))
        self.eng.learn(torch.randn(B, 4).to(device), torch.randn(B, 4).to(device))
        self._log()

    def _log(self):  # agent.py:333-359
        if self.eng.learning_steps % self.log_interval == 0:
            q1, q2, pl, el, ent, alpha = self.eng.losses_host()
            for k, v in (("loss/Q1", q1), ("loss/Q2", q2), ("loss/policy", pl), ("stats/alpha", alpha), ("stats/entropy", ent)):
                self.writer.add_scalar(k, v, self.eng.learning_steps)
            if self.imitative:  # agent.py:353-359
                bc_loss, bc_weight = self.eng.imitative_losses_host()
                self.writer.add_scalar("loss/bc", bc_loss, self.eng.learning_steps)
                self.writer.add_scalar("loss/bc_weight", bc_weight, self.eng.learning_steps)

    def save_models(self, ajan):  # agent.py:440-444
        self.eng.save_models(self.model_dir, ajan)
