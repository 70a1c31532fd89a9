"""SacEngine — device-resident state of the SAC agent (reference hirl/agents/SAC/agent.py; set_imitative adds its imitative branch) and the
host-side sequencing of the hx_sac_* stages.  The networks are the plain Linear-ReLU stacks of the reference's (un-vendored)
rltorch builder; they reuse the flat MLP-block layout of include/hirl4ucav.h with the LayerNorm slots pinned to (1, 0)."""
import ctypes
import os

import numpy as np
import torch

from .. import _lib
from . import engine as E

HxSacNets, HxSacImit, HxSacBatch = (_lib.STRUCTS[k] for k in ("HxSacNets", "HxSacImit", "HxSacBatch"))
H1, H2 = E.H1, E.H2
SEQ_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")  # nn.Sequential(Linear, ReLU, Linear, ReLU, Linear)


def _block(in_dim, out_dim):
    """offsets of W1 b1 g1 be1 W2 b2 g2 be2 W3 b3 inside one block (hx_nn.h Mlp)"""
    o, off = {}, 0
    for k, n in (("W1", H1 * in_dim), ("b1", H1), ("g1", H1), ("be1", H1), ("W2", H2 * H1), ("b2", H2), ("g2", H2), ("be2", H2),
                 ("W3", out_dim * H2), ("b3", out_dim)):
        o[k] = (off, n)
        off += n
    return o, (off + 3) & ~3


POLICY_BLOCK, POLICY_SIZE = _block(13, 8)
Q_BLOCK, Q_SIZE = _block(17, 1)
assert Q_SIZE == E.Q_PADDED


def pack_mlp(sd, block, size, in_dim, out_dim, device):
    """Sequential state_dict -> flat block (LayerNorm slots = (1, 0))"""
    flat = torch.zeros(size, dtype=torch.float32, device=device)
    shapes = {"0.weight": (H1, in_dim), "0.bias": (H1,), "2.weight": (H2, H1), "2.bias": (H2,), "4.weight": (out_dim, H2), "4.bias": (out_dim,)}
    for key, slot in zip(SEQ_KEYS, ("W1", "b1", "W2", "b2", "W3", "b3")):
        v = torch.as_tensor(np.asarray(sd[key].detach().cpu() if torch.is_tensor(sd[key]) else sd[key]), dtype=torch.float32)
        assert tuple(v.shape) == shapes[key], (key, v.shape)
        off, n = block[slot]
        flat[off:off + n] = v.reshape(-1).to(device)
    for slot in ("g1", "g2"):
        off, n = block[slot]
        flat[off:off + n] = 1.0
    return flat


def unpack_mlp(flat, block, in_dim, out_dim):
    shapes = {"W1": (H1, in_dim), "b1": (H1,), "W2": (H2, H1), "b2": (H2,), "W3": (out_dim, H2), "b3": (out_dim,)}
    return {key: flat[block[slot][0]:block[slot][0] + block[slot][1]].reshape(shapes[slot])
            for key, slot in zip(SEQ_KEYS, ("W1", "b1", "W2", "b2", "W3", "b3"))}


def _draw(replay, expert, n_main, seed, call, idx, guard=0):
    """the draw of a SAC minibatch as a record (HxSample; no BC table, no smoothing noise): n_main rows of `replay`, the rest of the batch from
    `expert`, Philox(seed; row, call), the indices into `idx`; guard: the newest `guard` slots of the ring are not drawn (a front launch's inserts)"""
    return E.HxSample(replay.total.data_ptr(), replay.capacity, replay.ring.data_ptr(), expert.ring.data_ptr() if expert is not None else None,
                      E.len_of(expert), None, 0, int(n_main), int(seed), call, 0.0, idx.data_ptr(), None, guard)


def _gather(s, batch, rows, noise=None, draw=1, st=None):
    """hx_sample_batch (hx_sample_batch_guarded with s.guard) for the record `s`: `batch` rows into the tile `rows`.  draw=0: the indices in s.idx are given."""
    args = (s.total, s.cap, s.ring, s.expert_ring, s.expert_len, None, 0, batch, s.n_main, draw, s.seed, s.call, 0.0, s.idx, None, _lib.ptr(noise), rows.data_ptr(), None)
    st = _lib.stream_ptr() if st is None else st
    if s.guard:
        _lib.call("hx_sample_batch_guarded", *args, s.guard, st)
    else:
        _lib.call("hx_sample_batch", *args, st)


def _given(ring, idx, batch):
    """the record of a caller-chosen minibatch: rows idx of the table `ring`"""
    return E.HxSample(None, 0, ring.data_ptr(), None, 0, None, 0, batch, 0, 0, 0.0, idx.data_ptr(), None, 0)


class SacEngine:
    def __init__(self, batch=128, lr=1e-3, gamma=0.99, tau=0.005, target_entropy=-4.0, target_update_interval=3, device="cuda", group=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HxError("SacEngine runs on the GPU only (no CPU path in the product)")
        L = _lib.load()
        assert L.hx_sac_policy_param_count() == POLICY_SIZE
        self.batch = int(batch)
        ws = int(L.hx_sac_workspace_floats(self.batch))
        self.arena, c = E.carve([POLICY_SIZE, 2 * Q_SIZE, 2 * Q_SIZE, POLICY_SIZE + 2 * Q_SIZE, POLICY_SIZE, POLICY_SIZE, 2 * Q_SIZE, 2 * Q_SIZE, 64, 64, ws,
                                 self.batch * 32, self.batch * 4, self.batch * 4, self.batch, 64], self.device)
        (self.policy, self.critic, self.target_critic, self.grad, self.m_policy, self.v_policy, self.m_critic, self.v_critic, losses,
         alpha, self.ws, self.rows, self.eps_next, self.eps_cur, ix, noise) = c
        self.grad_critic, self.grad_policy = self.grad[:2 * Q_SIZE], self.grad[2 * Q_SIZE:]
        self.losses, self.alpha_state, self._idx, self._noise = losses[:8], alpha[:4], ix.view(torch.int32), noise[:4]
        self.alpha_state[3] = 1.0  # log_alpha = 0 -> alpha = 1  (agent.py:106-107)
        self.nets = HxSacNets(*(t.data_ptr() for t in (self.policy, self.critic, self.target_critic, self.grad_policy, self.grad_critic,
                                                        self.m_policy, self.v_policy, self.m_critic, self.v_critic, self.losses,
                                                        self.alpha_state, self.ws)), None, None, None, None)
        for i, cls in ((5, HxSacNets), (6, HxSacBatch), (0, _lib.HxStepOpts), (2, E.HxHyper), (4, E.HxSample)):
            _lib.check_struct(i, cls)  # this binding's structs against the loaded library's (hx_abi_sizes)
        # fp32 image of the policy's W2 in the acting kernel's operand order (hx_pack_w2_f32i): kept current by hx_sac_adam(which = 1)
        self.w2_f32i = torch.zeros(512 * 256, dtype=torch.float32, device=self.device)
        self.nets.policy_w2_f32i = self.w2_f32i.data_ptr()
        # From this many rows on the policy's fp32 256 -> 512 product runs through the exact three-way bf16 split of both operands on the bf16 matrix cores
        # (hx_sac_act's w2_x9: every partial product exact, fp32 accumulation; 34 against 45 us at 16,384 rows, tools/ubench/actp_time.py);
        # None: fp32 MFMA at every size.  The hi | mid | lo images are built at the first such call, the policy's optimizer step keeps them current.
        self.x9_rows, self.w2_x9 = 16384, None
        # set_act_dtype / set_update_dtype: fp32 by default; the bf16 images (one block for the bf16 update, or the acting image alone) when asked for
        self.act_dtype, self.update_dtype, self.images, self.w2_bf16 = "f32", "f32", None, None
        self.hyper = E.HxHyper(gamma, tau, lr, lr, 0.0, 0.5, 0.0, 0)
        self.target_entropy, self.interval = float(target_entropy), int(target_update_interval)
        self.learning_steps = 0
        self.group = group
        self.world = torch.distributed.get_world_size(group) if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 1
        self.act_calls, self.sample_calls = 0, 0
        self.imitative, self.imit, self.expert_calls = False, None, 0  # set_imitative
        # learn() on one GPU is ONE library call; these two run its staged forms instead (the bit-identity tests, the sharded rank's sequence on one GPU):
        # staged_policy: the policy half as hx_sac_policy_grads[_imitative] + hx_sac_adam(1); separate_critic_adam: the critic half as
        # hx_sac_critic_grads + hx_sac_adam(0) — and with it the staged policy half
        self.staged_policy, self.separate_critic_adam = False, False
        self._seed = 0  # the seed of the last sample(): learn() without injected draws keys Normal.rsample's Philox eps with it
        self._pending, self._pending_expert = None, None  # draws sample(defer=True) / sample_expert(defer=True) recorded for the next learn()
        self._front_tiles, self._front_drawn = None, None  # step_learn: the two sets of minibatch tiles, and what the set in waiting was drawn for
        self.prioritized, self.per_weights, self.per_errors = None, None, None  # set_prioritized
        self.per_new_rows = "max"  # set_prioritized(new_rows=...): how step_learn gives a step's rows their first priority
        self.grad_clip, self.clip_ws = None, None  # set_grad_clip
        self.multi_step = None  # set_multi_step: the n-step inserter behind act_step
        self.entropy_tuning, self.ent_coef = True, None  # set_entropy_tuning

    def set_grad_clip(self, max_norm):
        """SacAgent(grad_clip=max_norm) (SAC/utils.py:15-21, agent.py:310-320): from now on learn() scales each network's gradient — Q1, Q2 and the policy,
        one norm each — to a global L2 norm of at most max_norm before its Adam step: gradients -> hx_sac_grad_norm -> hx_sac_adam_clipped per half
        (the staged sequence plus one norm launch per half; the one call's optimizer steps ride in the weight-gradient launches and cannot wait for a norm).  The log-alpha step is never clipped.
        None: back to the unclipped update.  One GPU."""
        if max_norm is None:
            self.grad_clip = None
            return
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError(f"grad_clip is a positive maximum norm, got {max_norm}")
        if self.world > 1:
            raise _lib.HxError("gradient clipping runs on one GPU (the norm is taken over this rank's gradient, before any exchange): run it with --gpus 1")
        if self.clip_ws is None:
            L = _lib.load()
            self.clip_ws = torch.zeros(int(L.hx_sac_clip_floats()), dtype=torch.float32, device=self.device)
        self.grad_clip = max_norm

    def set_entropy_tuning(self, on, ent_coef=0.2):
        """SacAgent(entropy_tuning=False, ent_coef=x) (agent.py:108-110, 322-327): alpha = ent_coef for good — alpha_state[3] holds it, the log-alpha state is
        not touched and no log-alpha step runs in any form of learn() (the calls get target_entropy = NaN, HX_SAC_FIXED_ALPHA); losses[3] (entropy_loss) stays 0, losses[5] == ent_coef.  on=True: entropy tuning
        resumes from the log-alpha state as it stands (alpha = exp(log_alpha))."""
        self.entropy_tuning = bool(on)
        if on:
            self.ent_coef = None
            self.alpha_state[3] = torch.exp(self.alpha_state[0])
        else:
            self.ent_coef = float(ent_coef)
            self.alpha_state[3] = self.ent_coef
        self.losses[5] = self.alpha_state[3]

    def _target_entropy(self):
        """what the hx_sac_* calls take as target_entropy: NaN (HX_SAC_FIXED_ALPHA) under a fixed entropy coefficient — no log-alpha step anywhere"""
        return self.target_entropy if self.entropy_tuning else float("nan")

    def grad_norms_host(self):
        """((norm_q1, norm_q2, norm_policy), (coef_q1, coef_q2, coef_policy)) of the last clipped learn(): the norms BEFORE clipping"""
        if self.clip_ws is None:
            raise _lib.HxError("grad_norms_host: no clip was ever set (set_grad_clip)")
        v = self.clip_ws[:6].tolist()
        return tuple(v[:3]), tuple(v[3:])

    def set_prioritized(self, replay, new_rows="max"):
        """SacAgent(per=True) (agent.py:281-284, 306-331): from now on sample() on `replay` (a utils.buffer.PrioritizedReplay) draws proportionally to
        the stored priorities and keeps the importance weights, learn() carries them through the three losses (hx_sac_learn_weighted) and hands
        |Q1(s, a) - y| back as the rows' new priorities (hx_per_update) — all enqueued, no host sync.  fp32, one GPU, not with the imitative branch.
        new_rows: how the loop gives a step's rows their first priority — "max": at the running maximum (replay.mark_new, the default), "td": at a TD
        error of their own as the reference's train_episode computes it (score_new, agent.py:234-246)."""
        from ..utils.buffer import PrioritizedReplay

        if new_rows not in ("max", "td"):
            raise ValueError(f"set_prioritized: new_rows is 'max' or 'td', got {new_rows!r}")
        if not isinstance(replay, PrioritizedReplay):
            raise TypeError("set_prioritized takes a utils.buffer.PrioritizedReplay")
        if self.update_dtype == "bf16" or self.act_dtype == "bf16":
            raise ValueError("prioritized replay is fp32 only: set_update_dtype('f32') and set_act_dtype('f32') before set_prioritized")
        if self.world > 1:
            raise _lib.HxError("prioritized replay runs on one GPU (priorities and block sums are not exchanged between ranks): run it with --gpus 1")
        if self.imitative:
            raise _lib.HxError("prioritized replay does not go with the imitative branch (not built: SacAgent(imitative=True, per=True)): build a SacEngine without set_imitative")
        if new_rows == "td" and self.multi_step is not None:
            raise _lib.HxError("prioritized replay with n-step rows: new_rows='td' is not built (the scoring pass and its chunks are sized by the envs per "
                               "step, a step of n-step rows stores up to n * num_envs): use new_rows='max'")
        if self.multi_step is not None and self.multi_step.replay is not replay:
            raise _lib.HxError("set_prioritized: the n-step inserter given to set_multi_step writes into another replay")
        self.prioritized, self.per_new_rows = replay, new_rows
        self.per_weights = torch.ones(self.batch, dtype=torch.float32, device=self.device)
        self.per_errors = torch.zeros(self.batch, dtype=torch.float32, device=self.device)

    def set_multi_step(self, inserter):
        """SacAgent(multi_step=n) for the vector loop: from now on step_learn runs act_step on an env WITHOUT a replay ring, then inserter.push
        (utils.buffer.NStepInserter: finished n-step rows into inserter.replay), then sample(inserter.replay) and learn() — the reference's order; there
        is no front form, as for prioritized replay.  learn() itself is unchanged in fp32 and bf16: a row's discount sits in its done column and
        hyper.gamma stays the one-step gamma, which must be the inserter's.  With set_prioritized the step's rows enter at pmax (mark_new with the bound
        n * num_envs); new_rows='td' is refused.  None: back to one-step rows.  One GPU."""
        if inserter is None:
            self.multi_step = None
            return
        from ..utils.buffer import NStepInserter

        if not isinstance(inserter, NStepInserter):
            raise TypeError("set_multi_step takes a utils.buffer.NStepInserter")
        if self.world > 1:
            raise _lib.HxError("n-step returns run on one GPU (not built for sharded ranks): run it with --gpus 1")
        if self.imitative:
            raise _lib.HxError("n-step returns do not go with the imitative branch (not built: SacAgent(imitative=True, multi_step=n))")
        if self.prioritized is not None and (self.per_new_rows != "max" or inserter.replay is not self.prioritized):
            raise _lib.HxError("n-step returns with prioritized replay: new_rows='max' only, and the inserter writes into the prioritized replay")
        if abs(inserter.gamma - float(self.hyper.gamma)) > 1e-7:
            raise ValueError(f"set_multi_step: the inserter folds gamma = {inserter.gamma} into its rows, the update bootstraps with gamma = {float(self.hyper.gamma)}")
        self.multi_step = inserter

    def score_new(self, replay, max_new, eps=None, seed=0):
        """the rows stored in `replay` since its last mark_new / score_new enter at |Q1(s, a) - y| of their own, computed with the networks as they
        stand (hx_per_score_new; the reference's train_episode, agent.py:234-246).  Under the conditions of learn() with prioritized replay: one GPU,
        fp32 update and acting, no imitative branch.  Enqueues only."""
        from ..utils.buffer import PrioritizedReplay

        if not isinstance(replay, PrioritizedReplay):
            raise TypeError("score_new takes a utils.buffer.PrioritizedReplay")
        if self.world > 1:
            raise _lib.HxError("score_new runs on one GPU (priorities and block sums are not exchanged between ranks): run it with --gpus 1")
        if self.update_dtype == "bf16" or self.act_dtype == "bf16":
            raise _lib.HxError("score_new is fp32 only (its forward launches have no bf16 form here): set_update_dtype('f32') and set_act_dtype('f32')")
        if self.imitative:
            raise _lib.HxError("score_new does not go with the imitative branch (not built: SacAgent(imitative=True, per=True))")
        replay.score_new(self, max_new, eps=eps, seed=seed)

    def set_imitative(self, bc_actor, slope=0.01):
        """SacAgent(imitative=True) (agent.py:315-318, 385-403): from now on learn() gates a BC term on the expert rows with
        bc_weight = mean(min Q(s, bc_actor(s)) > min Q(s, pi(s))).  bc_actor: the frozen 13-input LayerNorm actor the BC agent writes, as a
        state_dict or a flat block (engine.ACTOR_LAYOUT); slope: its leaky slope (agents/BC.py: 0.01).  fp32, one GPU."""
        if self.update_dtype == "bf16" or self.act_dtype == "bf16":
            raise ValueError("the imitative branch is fp32 only: set_update_dtype('f32') and set_act_dtype('f32') before set_imitative")
        if self.world > 1:
            raise _lib.HxError("the imitative branch runs on one GPU (its gate count is not exchanged between ranks): run it with --gpus 1")
        if self.prioritized is not None:
            raise _lib.HxError("the imitative branch does not go with prioritized replay (not built: SacAgent(imitative=True, per=True)): build a SacEngine without set_prioritized")
        L = _lib.load()
        if L.hx_sac_imit_sizeof() != ctypes.sizeof(HxSacImit):
            raise _lib.HxError(f"ABI mismatch: HxSacImit is {ctypes.sizeof(HxSacImit)} bytes here, {L.hx_sac_imit_sizeof()} in {_lib.SO_PATH}")
        if torch.is_tensor(bc_actor):
            if bc_actor.numel() != E.ACTOR_SIZE:
                raise ValueError(f"a flat bc_actor block has {E.ACTOR_SIZE} floats (engine.ACTOR_LAYOUT), got {bc_actor.numel()}")
            block = bc_actor.detach().to(self.device, torch.float32).reshape(-1).clone()
        else:
            block = E.pack(bc_actor, E.ACTOR_LAYOUT, E.ACTOR_SIZE, self.device)
        B = self.batch
        self.bc_actor = torch.zeros((E.ACTOR_SIZE + 3) & ~3, dtype=torch.float32, device=self.device)
        self.bc_actor[:E.ACTOR_SIZE].copy_(block)
        self.imit_ws = torch.zeros(int(L.hx_sac_imit_workspace_floats(B)), dtype=torch.float32, device=self.device)
        self.expert_rows = torch.zeros(B * 32, dtype=torch.float32, device=self.device)
        self.bc_count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._expert_idx = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.bc_slope = float(slope)
        self.imit = HxSacImit(self.bc_actor.data_ptr(), self.expert_rows.data_ptr(), self.imit_ws.data_ptr(), self.bc_count.data_ptr(), self.bc_slope)
        self.imitative, self._pending_expert = True, None

    def load_params(self, policy, q1, q2, hard_update_target=True):
        self.policy.copy_(pack_mlp(policy, POLICY_BLOCK, POLICY_SIZE, 13, 8, self.device))
        self.critic[:Q_SIZE].copy_(pack_mlp(q1, Q_BLOCK, Q_SIZE, 17, 1, self.device))
        self.critic[Q_SIZE:].copy_(pack_mlp(q2, Q_BLOCK, Q_SIZE, 17, 1, self.device))
        if hard_update_target:  # hard_update(critic_target, critic), agent.py:92
            self.target_critic.copy_(self.critic)
        self.refresh_images()

    def set_act_dtype(self, dtype):
        """"f32": policy inference in fp32 (fp32 MFMA, or the exact bf16 split from x9_rows rows on).  "bf16": the 256 -> 512 product on bf16
        MFMA from a bf16 image of W2 that every policy step keeps current; layer 1 and the Gaussian head stay fp32 (include/hirl4ucav.h
        "SAC bf16 path").  The bf16 update goes with the bf16 acting image: set the update back to "f32" first."""
        if dtype not in ("f32", "bf16"):
            raise ValueError(dtype)
        if dtype == "bf16" and self.imitative:
            raise ValueError("the imitative branch is fp32 only: act in 'f32', or build a SacEngine without set_imitative for bf16 acting")
        if dtype == "bf16" and self.prioritized is not None:
            raise ValueError("prioritized replay is fp32 only: act in 'f32', or build a SacEngine without set_prioritized for bf16 acting")
        if dtype != "bf16" and self.update_dtype == "bf16":
            raise ValueError("the SAC bf16 update goes with the bf16 acting image (set_update_dtype('f32') first)")
        self.act_dtype = dtype
        self._bind_images()
        self.refresh_images()

    def set_update_dtype(self, dtype):
        """"f32": learn() on fp32 MFMA (parity 1e-5 vs the reference).  "bf16": the three products of the 256 <-> 512 layer of the policy,
        both critics and both target critics on bf16 MFMA with fp32 accumulation; master weights, Adam, the Gaussian heads, the log-alpha step
        and the losses stay fp32.  Goes with the bf16 acting image (set_act_dtype("bf16") first)."""
        if dtype not in ("f32", "bf16"):
            raise ValueError(dtype)
        if dtype == "bf16" and self.imitative:
            raise ValueError("the imitative branch is fp32 only: keep the update in 'f32', or build a SacEngine without set_imitative for the bf16 update")
        if dtype == "bf16" and self.prioritized is not None:
            raise ValueError("prioritized replay is fp32 only: keep the update in 'f32', or build a SacEngine without set_prioritized for the bf16 update")
        if dtype == "bf16" and self.act_dtype != "bf16":
            raise ValueError("the SAC bf16 update goes with the bf16 acting image (set_act_dtype('bf16') first)")
        self.update_dtype = dtype
        self._bind_images()
        self.refresh_images()

    def _bind_images(self):
        """which images the kernels see: the bf16 update path holds every image in ONE block (its first image is the acting image; no fp32
        or exact-split image then), a bf16 policy beside the fp32 update its own acting image, the fp32 policy the fp32 image (and, from
        x9_rows rows on, the exact-split images: rebuilt by the next large call)"""
        self.nets.policy_w2_x9, self.w2_x9 = None, None
        if self.update_dtype == "bf16":
            if self.images is None:
                L = _lib.load()
                self.images = torch.zeros(int(L.hx_bf16_images_elems()), dtype=torch.bfloat16, device=self.device)
            self.w2_bf16 = self.images[:H2 * H1]
            self.nets.w2_bf16_all, self.nets.policy_w2_bf16, self.nets.policy_w2_f32i = self.images.data_ptr(), None, None
            return
        self.nets.w2_bf16_all, self.nets.policy_w2_f32i = None, self.w2_f32i.data_ptr()
        if self.act_dtype == "bf16":
            if self.w2_bf16 is None or (self.images is not None and self.w2_bf16.data_ptr() == self.images.data_ptr()):
                self.w2_bf16 = torch.zeros(H2 * H1, dtype=torch.bfloat16, device=self.device)
            self.nets.policy_w2_bf16 = self.w2_bf16.data_ptr()
        else:
            self.nets.policy_w2_bf16 = None

    def refresh_images(self):
        """Rebuild the kernels' images of W2 from the fp32 networks (after load_params / a checkpoint restore or any direct write to a
        network; the optimizer and Polyak steps maintain them otherwise): whatever images are live."""
        st = _lib.stream_ptr()
        if self.update_dtype == "bf16":
            _lib.call("hx_sac_pack_update_images", ctypes.byref(self.nets), st)
            return
        _lib.call("hx_pack_w2_f32i", self.policy.data_ptr(), 13, self.w2_f32i.data_ptr(), st)
        if self.act_dtype == "bf16":
            _lib.call("hx_pack_w2_bf16", self.policy.data_ptr(), 13, self.w2_bf16.data_ptr(), st)
        if self.w2_x9 is not None:
            _lib.call("hx_pack_w2_x9", self.policy.data_ptr(), 13, self.w2_x9.data_ptr(), st)

    def _act_format(self, n):
        """Policy inference for n rows -> (label, the (w2_f32i, w2_x9, w2_bf16) arguments of hx_sac_act / hx_sac_act_step): "_bf16", "_x9" (act_dtype "f32"
        from x9_rows rows on; with the fp32 image for the library's fallback up to 8,192 rows) or "_f32i"."""
        if self.act_dtype == "bf16":
            return "_bf16", (None, None, self.w2_bf16.data_ptr())
        if self.x9_rows is None or n < self.x9_rows:
            return "_f32i", (self.w2_f32i.data_ptr(), None, None)
        if self.w2_x9 is None:  # first large call: build the images; nets.policy_w2_x9 makes every later policy step refresh them
            self.w2_x9 = torch.zeros(3 * H2 * H1, dtype=torch.bfloat16, device=self.device)
            self.nets.policy_w2_x9 = self.w2_x9.data_ptr()
            _lib.call("hx_pack_w2_x9", self.policy.data_ptr(), 13, self.w2_x9.data_ptr(), _lib.stream_ptr())
        return "_x9", (self.w2_f32i.data_ptr(), self.w2_x9.data_ptr(), None)

    refresh_bf16 = refresh_images  # (the name utils/checkpoint.py calls after a restore)

    def replica_checksum(self):
        """int64 sum of the bit patterns of the networks, Adam moments and log-alpha state: equal on all ranks of a sharded run."""
        t = torch.cat([self.policy, self.critic, self.target_critic, self.m_policy, self.v_policy, self.m_critic, self.v_critic, self.alpha_state])
        return int(t.view(torch.int32).to(torch.int64).sum().item())

    def state_dicts(self):
        return {"policy": unpack_mlp(self.policy, POLICY_BLOCK, 13, 8), "q1": unpack_mlp(self.critic[:Q_SIZE], Q_BLOCK, 17, 1),
                "q2": unpack_mlp(self.critic[Q_SIZE:], Q_BLOCK, 17, 1), "q1_target": unpack_mlp(self.target_critic[:Q_SIZE], Q_BLOCK, 17, 1),
                "q2_target": unpack_mlp(self.target_critic[Q_SIZE:], Q_BLOCK, 17, 1)}

    def model_files(self):
        """What SacAgent.save_models writes (SAC/agent.py:440-444): the state_dicts of GaussianPolicy, TwinnedQNetwork and its
        target with the reference's key names (SAC/model.py:21,35-38,58: `policy.N.*`, `Q1.Q.N.*`, `Q2.Q.N.*`)."""
        sd = self.state_dicts()
        cpu = lambda d, pre: {pre + k: v.cpu().clone() for k, v in d.items()}
        return {"policy": cpu(sd["policy"], "policy."),
                "critic": {**cpu(sd["q1"], "Q1.Q."), **cpu(sd["q2"], "Q2.Q.")},
                "critic_target": {**cpu(sd["q1_target"], "Q1.Q."), **cpu(sd["q2_target"], "Q2.Q.")}}

    def save_models(self, model_dir, tag):
        for name, sd in self.model_files().items():
            torch.save(sd, os.path.join(model_dir, f"{name}_{tag}.pth"))

    def load_models(self, model_dir, tag):
        strip = lambda d, pre: {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}
        f = {name: torch.load(os.path.join(model_dir, f"{name}_{tag}.pth"), map_location="cpu") for name in ("policy", "critic", "critic_target")}
        self.load_params(strip(f["policy"], "policy."), strip(f["critic"], "Q1.Q."), strip(f["critic"], "Q2.Q."), hard_update_target=False)
        self.target_critic[:Q_SIZE].copy_(pack_mlp(strip(f["critic_target"], "Q1.Q."), Q_BLOCK, Q_SIZE, 17, 1, self.device))
        self.target_critic[Q_SIZE:].copy_(pack_mlp(strip(f["critic_target"], "Q2.Q."), Q_BLOCK, Q_SIZE, 17, 1, self.device))
        self.refresh_images()  # (the target critics' images follow the loaded targets)

    def act(self, obs, eps=None, explore=True, seed=0, row0=0, out=None):
        """explore (agent.py:183-188): sampled tanh-Gaussian action (eps [N, 4] given, else Philox); exploit (:191-196): tanh(mean)."""
        n = obs.shape[0]
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        mode = 0 if not explore else (1 if eps is not None else 2)
        self.act_calls += 1
        _lib.call("hx_sac_act", self.policy.data_ptr(), *self._act_format(n)[1], obs.data_ptr(), n, out.data_ptr(), mode, _lib.ptr(eps), int(seed), int(row0),
                  self.act_calls, _lib.stream_ptr())
        return out

    def act_step(self, env, eps=None, explore=True, seed=0, out=None):
        """explore / exploit for every env of `env` AND env.step with those actions in one launch (train_sac.py:238-241); same
        results as act(env.obs, ...) followed by env.step(actions).  -> (actions, obs, reward, done, success)."""
        n = env.n
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        mode = 0 if not explore else (1 if eps is not None else 2)
        self.act_calls += 1
        env.steps_issued += 1
        _lib.call("hx_sac_act_step", self.policy.data_ptr(), *self._act_format(n)[1], env.state.data_ptr(), n, env.pitch, env.obs.data_ptr(), out.data_ptr(), mode,
                  _lib.ptr(eps), int(seed), int(env.env_id0), self.act_calls, env.reward.data_ptr(), env.done.data_ptr(), env.success.data_ptr(),
                  ctypes.byref(env._opts), _lib.stream_ptr())
        return out, env.obs, env.reward, env.done, env.success

    def assemble(self, ring, idx):
        _gather(_given(ring, idx, self.batch), self.batch, self.rows, draw=0)

    def sample(self, replay, expert=None, n_main=None, seed=0, defer=False):
        """memory.sample(batch_size) on the device (E-SAC: batch - expert_num rows from the memory followed by expert_num rows of
        the expert memory, SAC/agent.py:286-296, train_sac.py:401-403) + the two standard-normal draw sets of the learn() call.
        defer=True: nothing is launched now — the next learn() draws and gathers inside its first launch (hx_sac_critic_grads_sampled)."""
        self.sample_calls += 1
        n_main = self.batch if (n_main is None or expert is None) else int(n_main)
        self._seed = int(seed)  # learn() without injected draws: Normal.rsample's eps comes from Philox(seed; row, learn call) in-kernel
        if self.prioritized is not None and replay is self.prioritized:  # memory.sample -> batch, indices, weights (agent.py:281-284)
            if n_main < self.batch:
                raise _lib.HxError("prioritized replay does not mix expert rows into the minibatch (the reference's learn() drops them when per is on: "
                                   "agent.py:281-284): sample the prioritized replay alone (n_main = batch)")
            self._pending = None
            replay.sample_into(self.batch, self._idx, self.per_weights, self.rows, seed=seed, call=self.sample_calls)
            return
        draw = _draw(replay, expert, n_main, seed, self.sample_calls, self._idx)
        self._pending = (draw, replay, expert) if defer else None  # (the tensors are referenced by the record: they must outlive the launch)
        if not defer:
            _gather(draw, self.batch, self.rows, self._noise)

    def assemble_expert(self, ring, idx):
        """the imitative branch's second batch by given indices: rows idx of the expert table `ring` -> expert_rows"""
        _gather(_given(ring, idx, self.batch), self.batch, self.expert_rows, draw=0)
        self._pending_expert = None

    def sample_expert(self, expert, seed=0, defer=False):
        """expert_memory.sample(batch_size) of the imitative branch (agent.py:394) on the device: B rows of the expert memory, drawn with
        Philox(seed; row, expert call) as hx_sample_batch draws (the key is offset, so that sample() and sample_expert() given the SAME seed draw
        independent streams).  defer=True: the next learn() draws them inside its call."""
        if not self.imitative:
            raise _lib.HxError("sample_expert is the imitative branch's second batch: call set_imitative first")
        self.expert_calls += 1
        seed = (int(seed) ^ 0x4558504552540000) & 0xFFFFFFFFFFFFFFFF
        draw = _draw(expert, None, self.batch, seed, self.expert_calls, self._expert_idx)
        self._pending_expert = (draw, expert) if defer else None
        if not defer:
            _gather(draw, self.batch, self.expert_rows)

    def imitative_losses_host(self):
        """(bc_loss, bc_weight) of the last imitative learn()"""
        v = self.losses.tolist()
        return v[6], v[7]

    def _allreduce(self, t):
        if self.world > 1:
            torch.distributed.all_reduce(t, group=self.group)

    def learn(self, eps_next=None, eps_cur=None):
        """SacAgent.learn (agent.py:276-327; after set_imitative its imitative branch, one GPU only) on the minibatch last assembled.  Enqueues only.
        One GPU: one library call.  staged_policy / separate_critic_adam / more than one rank: the critic half, then the policy half, as stages —
        the imitative branch too: it honours separate_critic_adam (hx_sac_critic_grads + hx_sac_adam(0), then hx_sac_policy_grads_imitative + hx_sac_adam(1))."""
        st = _lib.stream_ptr()
        if eps_next is not None:  # injected draws (parity tests, the façade's torch.randn)
            self.eps_next.copy_(eps_next.reshape(-1))
            self.eps_cur.copy_(eps_cur.reshape(-1))
            batch = HxSacBatch(self.rows.data_ptr(), self.batch, self.eps_next.data_ptr(), self.eps_cur.data_ptr(), 0, 0)
        else:
            batch = HxSacBatch(self.rows.data_ptr(), self.batch, None, None, self._seed, self.learning_steps + 1)
        nets, hyper, gs, bt = ctypes.byref(self.nets), ctypes.byref(self.hyper), 1.0 / self.world, ctypes.byref(batch)
        te = self._target_entropy()
        self.learning_steps += 1
        pending, self._pending = self._pending, None
        smp = ctypes.byref(pending[0]) if pending is not None else None
        polyak_first = int(self.learning_steps % self.interval == 0)
        if self.imitative and self.world > 1:
            raise _lib.HxError("the imitative branch runs on one GPU (its gate count is not exchanged between ranks): run it with --gpus 1")
        if self.prioritized is not None:  # the weighted update, then memory.update_priority(indices, errors)  (agent.py:306-331)
            if self.world > 1 or self.update_dtype == "bf16" or self.imitative:
                raise _lib.HxError("prioritized replay: one GPU, the fp32 update, no imitative branch")
            if self.separate_critic_adam or self.staged_policy:
                raise _lib.HxError("prioritized replay: the weighted update is one library call (hx_sac_learn_weighted) and has no staged entry points: "
                                   "clear separate_critic_adam and staged_policy")
            if pending is not None:
                raise _lib.HxError("prioritized replay: the minibatch comes from sample() on the prioritized replay, but a deferred uniform draw is pending")
            if self.grad_clip is not None:
                _lib.call("hx_sac_learn_weighted_clipped", nets, bt, hyper, self.per_weights.data_ptr(), self.per_errors.data_ptr(), polyak_first,
                          self.learning_steps, te, self.grad_clip, self.clip_ws.data_ptr(), st)
            else:
                _lib.call("hx_sac_learn_weighted", nets, bt, hyper, self.per_weights.data_ptr(), self.per_errors.data_ptr(), polyak_first, self.learning_steps,
                          te, st)
            _lib.call("hx_per_update", ctypes.byref(self.prioritized.per), self._idx.data_ptr(), self.per_errors.data_ptr(), self.batch, self.prioritized.alpha, st)
            return
        imit = ctypes.byref(self.imit) if self.imitative else None
        pe, self._pending_expert = self._pending_expert, None
        clip = self.grad_clip
        if clip is not None and self.world > 1:
            raise _lib.HxError("gradient clipping runs on one GPU (the norm is taken over this rank's gradient, before any exchange): run it with --gpus 1")
        cw = self.clip_ws.data_ptr() if clip is not None else None
        fused_critic = self.world == 1 and not self.separate_critic_adam and clip is None
        if fused_critic and not self.staged_policy and clip is None:
            # one GPU: the whole learn() in one call (plain: 9 launches, bit-identical to the staged sequence below, 14 launches)
            if imit is not None:
                _lib.call("hx_sac_learn_imitative", nets, bt, hyper, smp, imit, ctypes.byref(pe[0]) if pe is not None else None, polyak_first,
                          self.learning_steps, te, st)
            else:
                _lib.call("hx_sac_learn", nets, bt, hyper, smp, polyak_first, self.learning_steps, te, st)
            return
        if imit is not None and pe is not None:  # the staged form draws the deferred expert rows with a launch of its own
            _gather(pe[0], self.batch, self.expert_rows, st=st)
        # the critic half
        if fused_critic:
            # one GPU: the critics' optimizer steps ride in the weight-gradient launch (bit-identical to the two calls below, one launch less)
            _lib.call("hx_sac_critic_step", nets, bt, hyper, smp, polyak_first, self.learning_steps, st)
        else:
            if smp is not None:
                _lib.call("hx_sac_critic_grads_sampled", nets, bt, hyper, smp, polyak_first, st)
            else:
                _lib.call("hx_sac_critic_grads", nets, bt, hyper, polyak_first, st)
            self._allreduce(self.grad_critic)
            if clip is not None:  # a global norm needs every gradient written before any parameter steps: gradients -> norm -> clipped step
                _lib.call("hx_sac_grad_norm", nets, 0, cw, st)
                _lib.call("hx_sac_adam_clipped", nets, hyper, 0, self.learning_steps, gs, te, clip, cw, st)
            else:
                _lib.call("hx_sac_adam", nets, hyper, 0, self.learning_steps, gs, te, st)
        # the policy half
        if imit is not None:
            _lib.call("hx_sac_policy_grads_imitative", nets, bt, hyper, imit, st)
        else:
            _lib.call("hx_sac_policy_grads", nets, bt, hyper, st)
        if self.world > 1:  # mean entropy and the policy-loss terms are per-shard means: average them with the gradients
            self._allreduce(self.grad_policy)
            self._allreduce(self.losses)
            self.losses.mul_(gs)
        if clip is not None:  # (the imitative branch: on the combined (1 - w) dL + w dL_bc in grad_policy)
            _lib.call("hx_sac_grad_norm", nets, 1, cw, st)
            _lib.call("hx_sac_adam_clipped", nets, hyper, 1, self.learning_steps, gs, te, clip, cw, st)
        else:
            _lib.call("hx_sac_adam", nets, hyper, 1, self.learning_steps, gs, te, st)

    def step_learn(self, env, expert=None, n_main=None, explore=True, act_seed=0, out=None, sample_seed=0):
        """One iteration of the vector loop — act_step(env) then sample(env.replay, ..., defer=True) then learn() — in FRONT form (include/hirl4ucav.h
        hx_sac_front): the env step and the first forward launch of learn() are ONE launch, the minibatch pre-drawn by the previous call.  As in
        HirlEngine.step_learn the minibatch is drawn from the ring as it stood BEFORE this env step, without the env.n slots the step may overwrite.
        Any number of envs with a replay ring (up to 8,192 the per-tile acting workgroups, beyond the persistent acting kernel), one GPU, the one-call
        learn(), batch <= 256, Philox draws.  Acting and update in one format: fp32, or bf16 for both (a bf16 policy beside the fp32 update runs act_step,
        then the sampled learn(); so does the imitative branch).  After set_prioritized there is no front form either: act_step -> mark_new -> sample ->
        learn, the reference's order.  -> (actions, obs, reward, done, success)."""
        ms = self.multi_step
        replay, n, B = (env.replay if ms is None else ms.replay), env.n, self.batch
        if ms is not None and env.replay is not None:
            raise _lib.HxError("SacEngine.step_learn after set_multi_step: the env inserts one-step rows itself: build it with replay=None")
        if self.world > 1 or replay is None or self.separate_critic_adam or self.staged_policy:
            raise _lib.HxError("SacEngine.step_learn: one GPU, the one-call learn(), envs with a replay ring attached")
        if self._pending is not None:
            raise _lib.HxError("step_learn draws its own minibatch: a sample(defer=True) is still pending")
        if ms is not None and self.imitative:
            raise _lib.HxError("n-step returns do not go with the imitative branch (not built)")
        if self.prioritized is not None:
            # no front form: the front loop draws BEFORE the step's insert, so update() could hit slots the step has overwritten.  The reference's order:
            # act_step -> mark_new -> sample -> learn (which ends in update)
            if replay is not self.prioritized:
                raise _lib.HxError("SacEngine.step_learn: the env's replay ring is not the prioritized replay given to set_prioritized")
            if expert is not None and n_main is not None and int(n_main) < B:
                raise _lib.HxError("prioritized replay does not mix expert rows into the minibatch (the reference's learn() drops them when per is on: "
                                   "agent.py:281-284): run step_learn without expert rows")
            return self._step_then_learn(env, explore, act_seed, out, sample_seed, new_rows=self.per_new_rows)
        if ms is not None:  # no front form: the front launch's acting workgroups insert one-step rows; the reference's order (E-SAC's expert rows are mixed in as ever)
            return self._step_then_learn(env, explore, act_seed, out, sample_seed, expert=expert, n_main=n_main, defer=True)
        if self.imitative:  # no front form: the reference's order; `expert` is the imitative branch's expert memory, the minibatch is not expert-mixed
            if expert is None:
                raise _lib.HxError("SacEngine.step_learn: the imitative branch needs the expert memory (expert=...)")
            return self._step_then_learn(env, explore, act_seed, out, sample_seed, defer=True, imit_expert=expert)
        # no front form either: the clipped update is the staged sequence, whose first launch is its own; bf16 acting beside the fp32 update is a mix the
        # front launch does not have
        if self.grad_clip is not None or self.act_dtype != self.update_dtype:
            return self._step_then_learn(env, explore, act_seed, out, sample_seed, expert=expert, n_main=n_main, defer=True)
        if self._front_tiles is None:
            second = torch.zeros(B * 32 + B, dtype=torch.float32, device=self.device)
            self._front_tiles = [(self.rows, self._idx), (second[:B * 32], second[B * 32:].view(torch.int32))]
        cur, nxt = self._front_tiles
        n_main = B if (n_main is None or expert is None) else int(n_main)
        self.sample_calls += 1
        self._seed = int(sample_seed)

        want = (env, env.steps_issued, replay, expert, n_main, int(sample_seed), self.sample_calls, n)
        if self._front_drawn != want:  # no tile in waiting for THIS draw: draw now, as a launch of its own
            _gather(_draw(replay, expert, n_main, sample_seed, self.sample_calls, cur[1], guard=n), B, cur[0], self._noise)
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        self.act_calls += 1
        self.learning_steps += 1
        batch = HxSacBatch(cur[0].data_ptr(), B, None, None, int(sample_seed), self.learning_steps)
        nets, hyper, st = ctypes.byref(self.nets), ctypes.byref(self.hyper), _lib.stream_ptr()
        fmt, b16 = self._act_format(n)[0], self.update_dtype == "bf16"  # (bf16: the acting image is nets.w2_bf16_all's first)
        _lib.call("hx_sac_front", self.policy.data_ptr(), self.w2_x9.data_ptr() if fmt == "_x9" else None, None if b16 else self.w2_f32i.data_ptr(), env.state.data_ptr(), n, env.pitch,
                  env.obs.data_ptr(), out.data_ptr(), 2 if explore else 0, None, int(act_seed), int(env.env_id0), self.act_calls, env.reward.data_ptr(),
                  env.done.data_ptr(), env.success.data_ptr(), ctypes.byref(env._opts), nets, ctypes.byref(batch), st)
        env.steps_issued += 1
        nxt_draw = _draw(replay, expert, n_main, sample_seed, self.sample_calls + 1, nxt[1], guard=n)
        polyak_first = int(self.learning_steps % self.interval == 0)
        _lib.call("hx_sac_learn_back", nets, ctypes.byref(batch), hyper, polyak_first, self.learning_steps, self._target_entropy(), ctypes.byref(nxt_draw),
                  nxt[0].data_ptr(), st)
        self._front_drawn = (env, env.steps_issued, replay, expert, n_main, int(sample_seed), self.sample_calls + 1, n)
        self._front_tiles = [nxt, cur]
        self.rows, self._idx = cur
        return out, env.obs, env.reward, env.done, env.success

    def _step_then_learn(self, env, explore, act_seed, out, sample_seed, expert=None, n_main=None, defer=False, new_rows=None, imit_expert=None):
        """step_learn without a front form, the reference's order: act_step, [set_multi_step: the inserter's push], [the step's rows get their first priority: new_rows "max" | "td"],
        sample(env.replay, expert, n_main), [sample_expert(imit_expert)], learn()"""
        ms = self.multi_step
        replay = env.replay if ms is None else ms.replay
        res = self.act_step(env, explore=explore, seed=act_seed, out=out)
        if ms is not None:  # the acting launch ran without a ring: the step's finished n-step rows enter behind it (at most n * num_envs of them)
            ms.push(env, res[0])
        if new_rows == "td":
            self.score_new(replay, env.n, seed=sample_seed)
        elif new_rows == "max":
            replay.mark_new(env.n if ms is None else ms.max_rows)
        self.sample(replay, expert, n_main=n_main, seed=sample_seed, defer=defer)
        if imit_expert is not None:
            self.sample_expert(imit_expert, seed=sample_seed, defer=defer)
        self.learn()
        return res

    def losses_host(self):
        """(q1_loss, q2_loss, policy_loss, entropy_loss, mean entropy, alpha)"""
        v = self.losses.tolist()
        return v[0], v[1], v[2], v[3], v[4], v[5]
