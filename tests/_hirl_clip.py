"""CPU restatement of HirlEngine.set_grad_clip (TEST INFRASTRUCTURE ONLY): torch.nn.utils.clip_grad_norm_ once per optimizer of an
oracle.hirl_oracle.HirlOracle — opt_critic over BOTH Q heads and their LayerNorm parameters (one norm), opt_actor over the whole actor.  The reference's
HIRL.py / TD3.py have no clip (a declared extension); the rule is tests/_sac_clip.clip_once, the very function SAC's clip is pinned with.

    install_clip(o, max_norm)   o.opt_critic / o.opt_actor behind tests/_sac_clip.ClippedAdam; o.last_norms / o.last_coefs ["critic" | "actor"] = the norm
                                before clipping and the coefficient of the last step; o.clip["max_norm"] may be changed between calls; o.last_grads keeps
                                the gradients BEFORE clipping (what the engine's gradient buffers hold)
    norm64(flat, live)          float64 2-norm of the live words of a flat gradient (numpy)
    live_words(E, which)        indices of the words that count: every word below size() of each block, LayerNorm included, never the padding"""
import numpy as np

from tests._sac_clip import ClippedAdam, clip_once, total_norm  # noqa: F401


def install_clip(o, max_norm):
    o.clip = {"max_norm": float(max_norm), "reference_passes": False}
    o.last_norms, o.last_coefs = {}, {}
    log = {"norms": o.last_norms, "coefs": o.last_coefs}
    o.opt_critic, o.opt_actor = ClippedAdam(o.opt_critic, "critic", o.clip, log), ClippedAdam(o.opt_actor, "actor", o.clip, log)
    return o


def live_words(E, which):
    """which 0: the critic's flat gradient (two blocks of Q_PADDED words, the last Q_PADDED - size of each are padding); 1: the actor's"""
    if which == 1:
        return np.arange(E.ACTOR_SIZE)
    size = max(off + int(np.prod(shp)) for _, off, shp in E.CRITIC_LAYOUT if off < E.Q_PADDED)
    return np.concatenate([np.arange(size), E.Q_PADDED + np.arange(size)])


def padding_words(E):
    live = set(live_words(E, 0).tolist())
    return np.array([i for i in range(E.CRITIC_SIZE) if i not in live], np.int64)


def layernorm_words(layout):
    return np.concatenate([off + np.arange(int(np.prod(shp))) for k, off, shp in layout if k.startswith("layernorm")])


def norm64(flat, live):
    x = np.asarray(flat, np.float64)[live]
    return float(np.sqrt((x * x).sum()))


def coef_f32(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) evaluated in fp32 from an fp32 norm, as the stepping kernel forms it (one add, one division: each correctly
    rounded or within an ulp)"""
    return float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))
