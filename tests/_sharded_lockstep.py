"""W virtual ranks of the sharded HIRL update in ONE process, on one stream, with no process group — and the numpy model of the merged actor
message's count words.

Each rank is a HirlEngine(batch=B) with identical parameters and staged = True.  Lockstep.learn() issues the stages of HirlEngine._learn_staged for
every rank in turn — the engine's own _begin_call / _stage_* methods, i.e. the entry points and argument values of a sharded rank — and stands in for
the two exchanges with the exact rank-order fp32 sum of tests/_xchg_model.py (or with a transport the caller passes).  What a real sharded run adds
to this is the handshake between concurrent processes: tests/test_sharded_gpu.py.  The reference is one process (hirl/agents/HIRL.py:52)."""
import ctypes

import numpy as np

from tests import _xchg_model as X

GUARD = X.GUARD       # floats behind every rank's actor message that no launch may touch
GUARD_VALUE = -7.0
TAIL = 64             # words behind the two gradients (hx_actor_message_floats() = 2 P + TAIL)
COUNT_DIGITS = 7      # tail words 1..7: the soft count's base-32 digits, least significant first (word 0: the count itself)


# ---- the count words (include/hirl4ucav.h hx_hirl_actor_wgrad_split), numpy ----------------------------------------------------------------------
def count_words(count):
    """one rank's eight count words for a soft count 0 <= count < 2^31: fp32 [1 + COUNT_DIGITS]"""
    c = int(count)
    assert 0 <= c < 1 << 31
    return np.array([np.float32(c)] + [(c >> (5 * k)) & 31 for k in range(COUNT_DIGITS)], np.float32)


def count_from_words(words):
    """the global count hx_adam_mixed rebuilds from the SUMMED count words (word 0 is not read)"""
    return sum(int(np.float32(words[1 + k])) << (5 * k) for k in range(COUNT_DIGITS))


def round_f32(x):
    """an exact Fraction -> the nearest fp32 (ties to even), as np.float32"""
    from fractions import Fraction

    c = np.float32(float(x))
    cands = {float(c), float(np.nextafter(c, np.float32(np.inf))), float(np.nextafter(c, np.float32(-np.inf)))}
    best = min(cands, key=lambda v: (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def soft_weight_f32(count, batch, warm):
    """min(fma(float32(count), float32(1 / batch), float32(warm)), 1) — the BC weight as the kernels form it (effective_w of the one-GPU path compiles to
    one fused multiply-add; adam_w spells the same operation out): ONE rounding of the exact count * inv_batch + warm"""
    from fractions import Fraction

    inv = np.float32(1.0) / np.float32(batch)
    w = round_f32(Fraction(float(np.float32(count))) * Fraction(float(inv)) + Fraction(float(np.float32(warm))))
    return np.float32(1.0) if w > 1 else w


# ---- the virtual ranks ------------------------------------------------------------------------------------------------------------------------------
def tables(data):
    """(replay ring, BC table) of tests/_hirl_data.make_data on the device"""
    import torch

    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    bc = np.zeros((data["expert_s"].shape[0], 32), np.float32)
    bc[:, 0:13], bc[:, 13:17] = data["expert_s"], data["expert_a"]
    return ring, torch.from_numpy(bc).cuda().contiguous()


def make_engine(E, batch, params, use_bc=True, slope=0.0, layer_norm=True, bf16=False):
    e = E.HirlEngine(batch=batch, use_bc=use_bc, slope=slope, layer_norm=layer_norm)
    e.load_params(params["actor"], params["critic"], params["bc_actor"] if use_bc else None)
    if bf16:
        e.set_update_dtype("bf16")
        e.set_act_dtype("bf16")
    return e


def rank_order_sum_device(tensors):
    """the exact rank-order fp32 sum (tests/_xchg_model.rank_order_sum, on the host) of equally long device tensors -> a device tensor"""
    import torch

    host = np.stack([t.detach().cpu().numpy() for t in tensors])
    return torch.from_numpy(X.rank_order_sum(host)).to(tensors[0].device)


def count_read_by_adam_mixed(e, summed):
    """The global soft count as hx_adam_mixed READS it from the summed message `summed`: one call with w_kind 1 (estimate), warm 0 and a batch of 2^20 rows
    leaves losses[5] = float32(count) 2^-20, exact for every count up to 2^20.  STEPS e's actor (use it last, or on a throwaway engine).  Synchronises."""
    from hirl4ucav_amd import _lib

    _lib.call("hx_adam_mixed", ctypes.byref(e.nets), ctypes.byref(e.hyper), 0, max(e.actor_step, 1), 1.0, 1, 0.0, 0.0, 1 << 20, summed.data_ptr(),
              _lib.stream_ptr())
    w = float(e.losses[5].item())
    c = w * float(1 << 20)
    assert c == int(c), ("hx_adam_mixed formed a weight that is no multiple of 2^-20", w)
    return int(c)


class Lockstep:
    """W engines of batch B.  learn(shards, noise, ...) = one sharded learn() call of every rank; the messages and sums of the last call stay readable:
    critic_msgs / critic_sum (device tensors) and, after an actor call, actor_msgs [W, n + GUARD] / actor_sum."""

    def __init__(self, E, W, B, params, data, **kw):
        import torch

        self.E, self.W, self.B = E, W, B
        self.ring, self.bc = tables(data)
        self.engines = [make_engine(E, B, params, **kw) for _ in range(W)]
        for e in self.engines:
            e.staged = True
        from hirl4ucav_amd import _lib

        self.n = int(_lib.load().hx_actor_message_floats())
        assert self.n == 2 * ((E.ACTOR_SIZE + 3) & ~3) + TAIL
        self.actor_msgs = torch.zeros((W, self.n + GUARD), dtype=torch.float32, device="cuda")
        self.actor_msgs[:, self.n:] = GUARD_VALUE
        self.critic_msgs, self.critic_sum, self.actor_sum, self.was_actor_call = None, None, None, False

    def learn(self, shards, noise, bc_weight_now=0.0, bc_warm_up_weight=0.0, before_message=None, reduce_actor=None):
        """shards[r] = (idx, idx_bc or None): rank r's minibatch rows (int32 numpy); noise: the shared (4,) smoothing draw (fp32 numpy).
        before_message(r, e): called after rank r's actor backward, before its message launch (tests write e.soft_count there).
        reduce_actor(msgs [W, n]) -> the summed message every rank steps with (default: the rank-order fp32 sum)."""
        import torch
        from hirl4ucav_amd import _lib

        E, W, B = self.E, self.W, self.B
        noise_d = torch.from_numpy(np.asarray(noise, np.float32)).cuda()
        w_kind, w_given = E._bc_weight_kind(bc_weight_now)
        batches = []
        for e, (idx, ibc) in zip(self.engines, shards):
            if e.use_bc:
                e.assemble(self.ring, torch.from_numpy(idx).cuda(), bc_table=self.bc, idx_bc=torch.from_numpy(ibc).cuda())
            else:
                e.assemble(self.ring, torch.from_numpy(idx).cuda())
            batches.append(E.HxBatch(e.rows.data_ptr(), e.bc_rows.data_ptr() if e.use_bc else None, B, noise_d.data_ptr()))
        phases = [e._begin_call() for e in self.engines]
        assert all(p == phases[0] for p in phases)
        actor_phase, do_polyak = phases[0]
        actor_fwd = (2 if w_kind == 1 else 1) if actor_phase else 0
        for e, b in zip(self.engines, batches):
            _lib.call("hx_hirl_critic_grads", ctypes.byref(e.nets), ctypes.byref(b), ctypes.byref(e.hyper), actor_fwd, _lib.stream_ptr())
        self.critic_msgs = [e.grad_critic.clone() for e in self.engines]
        self.critic_sum = rank_order_sum_device(self.critic_msgs)
        for e in self.engines:
            e._stage_critic_step(self.critic_sum, do_polyak, world=W)
        self.was_actor_call = actor_phase
        if actor_phase:
            for r, (e, b) in enumerate(zip(self.engines, batches)):
                e._stage_actor_backward(b, w_kind)
                if before_message is not None:
                    before_message(r, e)
                e._stage_actor_message(self.actor_msgs[r, :self.n])
            self.actor_sum = (rank_order_sum_device(list(self.actor_msgs[:, :self.n])) if reduce_actor is None
                              else reduce_actor(self.actor_msgs[:, :self.n]))
            for e in self.engines:
                e._stage_actor_step(self.actor_sum, do_polyak, w_kind, w_given, bc_warm_up_weight, world=W)
        for e in self.engines:
            e.actor_trainable = not e.actor_trainable  # HIRL.py:332
        self._keep = (noise_d, batches)  # (referenced by the launches just enqueued)


def state_tensors(e):
    """name -> tensor of everything a learn() call may change: five networks, four moment buffers, wstate, and every live W2 image"""
    out = {k: getattr(e, k) for k in ("actor", "critic", "target_actor", "target_critic", "bc_actor", "m_actor", "v_actor", "m_critic", "v_critic",
                                      "wstate", "w2_f32i")}
    if e.update_dtype == "bf16":
        out["images"] = e.images
    elif e.act_dtype == "bf16":
        out["w2_bf16"] = e.w2_bf16
    if e.nets.actor_w2_x9:
        out["w2_x9"] = e.w2_x9
    return out


def bits_equal(a, b):
    import torch

    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_same_state(a, b, what):
    sa, sb = state_tensors(a), state_tensors(b)
    assert sa.keys() == sb.keys(), (what, sorted(sa), sorted(sb))
    bad = [k for k in sa if not bits_equal(sa[k], sb[k])]
    assert not bad, (what, "differ in bits:", bad)
    assert (a.critic_step, a.actor_step, a.update_count, a.actor_trainable) == (b.critic_step, b.actor_step, b.update_count, b.actor_trainable), what


def copy_state(dst, src):
    """dst <- src: networks, moments, wstate, host counters; dst's W2 images rebuilt from its networks"""
    for k in ("actor", "critic", "target_actor", "target_critic", "bc_actor", "m_actor", "v_actor", "m_critic", "v_critic", "wstate"):
        getattr(dst, k).copy_(getattr(src, k))
    dst.critic_step, dst.actor_step, dst.update_count, dst.actor_trainable = src.critic_step, src.actor_step, src.update_count, src.actor_trainable
    dst.refresh_bf16()
