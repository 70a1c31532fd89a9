"""Child process of tests/test_wgrad_two_slot_gpu.py: the library reads HX_WGRAD_TWO_SLOT once per process, so every case is run in a process of its
own setting and leaves what the actor's weight-gradient launch produced in <out dir>/<case>.npz.   python tests/_wgrad_two_slot_child.py <out dir>"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _hirl_data as D  # noqa: E402

# case -> (batch, staged, slope)
HIRL_CASES = {"b16": (16, False, 0.0), "b48": (48, False, 0.0), "b128": (128, False, 0.0), "b144": (144, False, 0.0),
              "staged128": (128, True, 0.0), "slope128": (128, False, 0.01)}


def bits(t):
    """a tensor's bits as integers (bf16 has no numpy type; NaNs must compare equal to themselves)"""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def hirl_case(engine, name):
    from tests.test_hirl_gpu import device_tables

    B, staged, slope = HIRL_CASES[name]
    params, data = D.make_params(21), D.make_data(22, outliers=True)
    ring, exp, bc = device_tables(data)
    rng = np.random.default_rng(5)
    e = engine.HirlEngine(batch=B, slope=slope)
    e.staged = staged
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    e.set_act_dtype("f32x9")  # the exact-split acting images are bound: the tile workgroups' hi | mid | lo stores run
    out = {}
    for k in range(6):  # calls 0, 2, 4 are actor calls; call 4 also moves the targets
        idx = rng.integers(0, D.N_REPLAY, B).astype(np.int32)
        ibc = rng.integers(0, D.N_EXPERT, B).astype(np.int32)
        noise = rng.normal(0, 0.2, 4).astype(np.float32)
        w = {0: 100, 2: None, 4: 0.3}.get(k)  # the actor calls: estimated now, the stored one, a given one
        e.assemble(ring, torch.from_numpy(idx).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc).cuda())
        e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=w, bc_warm_up_weight=0.05)
        out[f"losses{k}"] = np.asarray(e.losses_host(), np.float32)
        out[f"wstate{k}"] = bits(e.wstate)
        out[f"grad_actor{k}"] = bits(e.grad_actor)
    assert e.update_count == 3
    for name_ in ("actor", "m_actor", "v_actor", "target_actor", "w2_f32i", "w2_x9"):
        out[name_] = bits(getattr(e, name_))
    return out


def sac_case(sac_engine):
    from tests.test_isac_gpu import bc_actor_params, make_rings
    from tests.test_oracle_sac import sac_params

    rep, exp = make_rings()
    e = sac_engine.SacEngine(batch=128)
    params = sac_params()
    e.load_params(params["policy"], params["q1"], params["q2"])
    e.set_imitative(bc_actor_params(), slope=0.01)
    out = {}
    for k in range(4):
        e.sample(rep, None, seed=11)
        e.sample_expert(exp, seed=11)
        e.learn()
        out[f"losses{k}"] = e.losses.detach().cpu().numpy().copy()
        out[f"grad_policy{k}"] = bits(e.grad_policy)
    for name_ in ("policy", "m_policy", "v_policy", "alpha_state", "w2_f32i"):
        out[name_] = bits(getattr(e, name_))
    return out


def main():
    from hirl4ucav_amd.agents import engine, sac_engine

    outdir = sys.argv[1]
    for name in HIRL_CASES:
        np.savez(os.path.join(outdir, name + ".npz"), **hirl_case(engine, name))
    np.savez(os.path.join(outdir, "sac128.npz"), **sac_case(sac_engine))
    torch.cuda.synchronize()
    print("two-slot child ok")


if __name__ == "__main__":
    main()
