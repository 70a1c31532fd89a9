"""Bit recordings of SAC's weighted, clipped and scoring paths (hx_sac_learn_weighted[_clipped], hx_sac_grad_norm + hx_sac_adam_clipped,
hx_per_score_new) and of the staged bf16 update (hx_sac_adam with segment images) from a fixed start.

tests/golden/sac_fold_bits.npz was recorded with this module on an MI355X from the library of the commit BEFORE these paths were folded into the
shared code (tests/golden/gen_sac_fold_bits.py); tests/test_per_gpu.py, tests/test_sac_clip_gpu.py, tests/test_per_score_gpu.py and
tests/test_sac_bf16_gpu.py replay it with the current library and compare word for word.  Only entry points that exist on both sides are used.

What is NOT recorded as bits: losses[0..2].  The q and policy losses are float atomicAdd sums over the rows' waves (td_head, q_select, policy_dout,
bwd_l2's prologues), so their last bits follow the arrival order of a run; nothing reads them back.  losses[3..5] (entropy_loss, mean entropy, alpha)
are fixed-order and recorded; of the weighted cases the two q losses are kept as VALUES ("td_losses": sums of 48 non-negative terms, any two orders
of which differ by at most 2 * 47 * 2^-24 of the sum, TD_LOSS_RTOL)."""
import numpy as np
import torch

NETS = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i")
CALLS, BATCH, CAP = 4, 48, 4096  # three 16-row tiles (a ragged last 64-row workgroup); the Polyak step of the targets rides in call 3
TD_LOSS_RTOL = 2 * 47 * 2.0 ** -24
SCORE_LIVE, SCORE_NEW, SCORE_CHUNK = 1004, 40, 16  # slots 1004..1043: across the block boundary at 1,024, three chunks, the last one padded
CASES = ("weighted", "weighted_clipped", "clipped", "score", "staged_bf16")


def _bits(t):
    b = t.detach().contiguous().reshape(-1)
    b = (b.view(torch.int16).to(torch.int32) if b.element_size() == 2 else b.view(torch.int32)).cpu().numpy().astype(np.int64)
    pick = np.linspace(0, b.size - 1, min(b.size, 96)).astype(np.int64)
    return np.concatenate([[b.sum()], [(b * (np.arange(b.size) % 8191 + 1)).sum()], b[pick]]).astype(np.int64)


def _fill(rep):
    rng = np.random.default_rng(17)
    rep.ring.copy_(torch.from_numpy(rng.normal(size=(CAP, 32)).astype(np.float32)))
    rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()


def _engine(SE, params, **kw):
    e = SE.SacEngine(batch=BATCH, **kw)
    e.load_params(params["policy"], params["q1"], params["q2"])
    return e


def _nets(out, label, e):
    for name in NETS:
        out[f"{label}/{name}"] = _bits(getattr(e, name))
    out[f"{label}/losses_fixed"] = _bits(e.losses[3:6])


def _weighted(SE, params, max_norm):
    """-> (engine, per-call [CALLS, 6] clip words or None, per-call q losses)"""
    from hirl4ucav_amd.utils.buffer import PrioritizedReplay

    rep = PrioritizedReplay(CAP)
    _fill(rep)
    rep.total += CAP
    rep.mark_new()
    pr = np.random.default_rng(29).uniform(0.05, 2.0, CAP).astype(np.float32)  # seeded priorities: non-unit importance weights
    rep.set_priorities(np.arange(CAP, dtype=np.int32), pr)
    e = _engine(SE, params)
    e.set_prioritized(rep)
    if max_norm is not None:
        e.set_grad_clip(max_norm)
    clip, errs, weights, td = [], [], [], []
    for _ in range(CALLS):
        e.sample(rep, None, seed=23)
        weights.append(e.per_weights.clone())
        e.learn()
        errs.append(e.per_errors.clone())
        td.append(e.losses[:2].clone())
        if max_norm is not None:
            clip.append(e.clip_ws[:6].clone())
    torch.cuda.synchronize()
    assert float(torch.stack(weights).min()) < 1.0, "the recorded weights must not all be 1"
    return e, rep, (torch.stack(clip) if clip else None), torch.stack(errs), torch.stack(td).cpu().numpy().astype(np.float64)


def _uniform_replay():
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    rep = DeviceReplay(CAP)
    _fill(rep)
    rep.total += CAP
    return rep


def probe_norms(SE, params):
    """the gradient norms [CALLS, 3] (Q1, Q2, policy) of the weighted update under a clip that never binds: what the generator picks max_norm from"""
    _, _, clip, _, _ = _weighted(SE, params, 1.0e30)
    return clip[:, :3].cpu().numpy().astype(np.float64)


def record(SE, params, max_norm, cases=CASES):
    """-> {"<case>/<name>": int64 vectors (position-weighted checksums of the bit patterns plus 96 sampled words), "<case>/td_losses": float64 values}
    after CALLS learn() calls at B = 48 with in-kernel Philox draws; `max_norm`: the recording's, which clips the critics and never the policy in the weighted run (the generator
    looks for it: in the recording 7 of the 8 critic steps are clipped — Q1's norm in the Polyak call lies below every bound that spares the policy)."""
    out = {}
    if "weighted" in cases:  # (a) hx_sac_learn_weighted
        e, rep, _, errs, td = _weighted(SE, params, None)
        _nets(out, "weighted", e)
        out["weighted/per_errors"], out["weighted/prio"], out["weighted/td_losses"] = _bits(errs), _bits(rep._prio), td
    if "weighted_clipped" in cases:  # (b) hx_sac_learn_weighted_clipped
        e, rep, clip, errs, td = _weighted(SE, params, max_norm)
        _nets(out, "weighted_clipped", e)
        out["weighted_clipped/per_errors"], out["weighted_clipped/td_losses"], out["weighted_clipped/clip_ws"] = _bits(errs), td, _bits(clip)
    if "clipped" in cases:  # (c) hx_sac_critic_grads, hx_sac_grad_norm, hx_sac_adam_clipped, hx_sac_policy_grads, ...
        for label, tuning in (("clipped", True), ("clipped_fixed_alpha", False)):
            rep, e = _uniform_replay(), _engine(SE, params)
            e.set_grad_clip(max_norm)
            if not tuning:
                e.set_entropy_tuning(False, 0.2)
            clip = []
            for _ in range(CALLS):
                e.sample(rep, None, seed=23)
                e.learn()
                clip.append(e.clip_ws[:6].clone())
            torch.cuda.synchronize()
            _nets(out, label, e)
            out[f"{label}/clip_ws"] = _bits(torch.stack(clip))
    if "score" in cases:  # (d) hx_per_score_new
        from hirl4ucav_amd.utils.buffer import PrioritizedReplay

        rep = PrioritizedReplay(CAP)
        _fill(rep)
        rep.total += SCORE_LIVE
        rep.mark_new()
        rep.set_priorities(np.arange(SCORE_LIVE, dtype=np.int32), np.random.default_rng(31).uniform(0.05, 2.0, SCORE_LIVE).astype(np.float32))
        rep.total += SCORE_NEW
        rep.score_chunk = SCORE_CHUNK
        e = _engine(SE, params)
        e.score_new(rep, SCORE_NEW, seed=37)
        torch.cuda.synchronize()
        assert rep.marked == SCORE_LIVE + SCORE_NEW
        out["score/prio"], out["score/bsum"] = _bits(rep._prio[:2048]), _bits(rep.bsum[:2])  # the two touched blocks
        out["score/pmax"], out["score/marked"] = _bits(rep.pmax_t), np.asarray([rep.marked], np.int64)
        out["score/errors"] = _bits(rep.errors[:SCORE_NEW])
    if "staged_bf16" in cases:  # (e) hx_sac_critic_grads + hx_sac_adam(0) + hx_sac_policy_grads + hx_sac_adam(1) on the bf16 update path
        rep, e = _uniform_replay(), _engine(SE, params)
        e.set_act_dtype("bf16")
        e.set_update_dtype("bf16")
        e.separate_critic_adam = True
        for _ in range(CALLS):
            e.sample(rep, None, seed=23)
            e.learn()
        torch.cuda.synchronize()
        _nets(out, "staged_bf16", e)
        out["staged_bf16/images"] = _bits(e.images)
    return out


def assert_replays(SE, params, golden, cases):
    """record `cases` with the current library under the recording's max_norm: every vector the recording holds for them word for word; the q losses
    of the weighted cases as values"""
    now = record(SE, params, float(golden["max_norm"][0]), cases=cases)
    labels = {k.split("/")[0] for k in now}
    keys = [k for k in golden.files if "/" in k and k.split("/")[0] in labels]
    assert len(labels) >= len(cases) and sorted(keys) == sorted(now), (cases, sorted(keys), sorted(now))
    for k in keys:
        if k.endswith("/td_losses"):
            np.testing.assert_allclose(now[k], golden[k], rtol=TD_LOSS_RTOL, atol=0, err_msg=k)
        else:
            np.testing.assert_array_equal(now[k], golden[k], err_msg=k)
