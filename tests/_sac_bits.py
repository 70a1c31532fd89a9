"""Bit recordings of the UNCHANGED SAC update paths (hx_sac_learn, and the staged sequence that ends in hx_sac_adam) from a fixed start.

tests/golden/sac_unchanged_bits.npz was recorded with this module on an MI355X from the library of the commit BEFORE prioritized replay was
added (tests/golden/gen_sac_unchanged_bits.py); tests/test_per_gpu.py replays it with the current library and compares bit for bit.
Only entry points that exist on both sides are used."""
import numpy as np
import torch

NAMES = ("policy", "critic", "target_critic", "m_policy", "v_policy", "m_critic", "v_critic", "alpha_state", "w2_f32i")
CALLS = 4  # the Polyak step of the targets rides in call 3


def _bits(t):
    b = t.detach().contiguous().view(torch.int32).cpu().numpy()
    pick = np.linspace(0, b.size - 1, min(b.size, 96)).astype(np.int64)
    return np.concatenate([[np.int64(b.astype(np.int64).sum())], [np.int64((b.astype(np.int64) * (np.arange(b.size) % 8191 + 1)).sum())], b[pick].astype(np.int64)])


def record(SE, params):
    """-> {"one_call/<name>", "staged/<name>": int64 vectors}: position-weighted checksums of the bit patterns plus 96 sampled words of every network,
    moment, the alpha state and the acting image after CALLS learn() calls at B = 128 with in-kernel Philox draws."""
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    out = {}
    for label, staged in (("one_call", False), ("staged", True)):
        rng = np.random.default_rng(17)
        rep = DeviceReplay(4096)
        rep.ring.copy_(torch.from_numpy(rng.normal(size=(4096, 32)).astype(np.float32)))
        rep.ring[:, 31] = (rep.ring[:, 31] > 1.0).float()
        rep.total += 4096
        e = SE.SacEngine(batch=128)
        e.separate_critic_adam = staged  # hx_sac_critic_grads + hx_sac_adam(0) + hx_sac_policy_grads + hx_sac_adam(1)
        e.load_params(params["policy"], params["q1"], params["q2"])
        for _ in range(CALLS):
            e.sample(rep, None, seed=23)
            e.learn()
        torch.cuda.synchronize()
        for name in NAMES:
            out[f"{label}/{name}"] = _bits(getattr(e, name))
    return out
