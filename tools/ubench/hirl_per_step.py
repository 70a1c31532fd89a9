"""Cost of prioritized replay for HIRL on the MI355X -> profiles/hirl_per_step.json: the reference-order vector step (act_step -> [mark_new] -> sample ->
learn [-> update]) with and without HirlEngine.set_prioritized on the same build, 4,096 straight_line envs, HIRL soft fp32, B = 128, n_main = 128 (the
state behind the warm-up: every row of the minibatch is a replay row).  Device events, warm-up, median of repeated regions, the two variants
alternating in one process (the plain variant is timed before and after the other).  Library calls and kernel launches per step are counted from the
calls the engine makes (each entry point's launches at B = 128: LAUNCHES).

    python tools/ubench/hirl_per_step.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hirl4ucav_amd import _lib
from hirl4ucav_amd.agents import engine as E
from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
from hirl4ucav_amd.train_all import init_actor_state_dict, init_critic_state_dict
from hirl4ucav_amd.utils.buffer import DeviceReplay, PrioritizedReplay

# kernel launches behind one library call at B = 128 (hx_hirl.hip's header: 4 on a critic-only call, 8 on an actor call, draw and optimizer steps
# included; the staged entry points: launches A, B, the TD head, C, D / G, H, I)
LAUNCHES = {"hx_actor_act_step": 1, "hx_per_mark_new": 1, "hx_sample_batch": 1, "hx_per_sample": 1, "hx_per_update": 1, "hx_adam": 1,
            "hx_hirl_critic_grads_weighted": 5, "hx_hirl_actor_backward": 3, "hx_hirl_actor_wgrad": 1, "hx_hirl_learn_sampled": (4, 8)}


def timed(fn, reps, regions=9, warm=3):
    for _ in range(warm):
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out)), "regions": regions, "steps_per_region": reps}


def make(per, n_envs, cap, B, expert, bc):
    torch.manual_seed(0)
    rep = PrioritizedReplay(cap) if per else DeviceReplay(cap)
    env = BatchedHarfangEnv(n_envs, scenario="straight_line", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=rep)
    env.reset()
    eng = E.HirlEngine(batch=B, use_bc=True)
    eng.load_params(init_actor_state_dict(), init_critic_state_dict(), init_actor_state_dict())
    if per:
        eng.set_prioritized(rep)
    out = torch.zeros((n_envs, 4), device="cuda")
    for _ in range(4):  # rows in the ring before the first draw
        eng.act_step(env, sigma=0.1, seed=2, out=out)
    if per:
        rep.mark_new()
    first = [True]

    def step():  # train_all.step_reference, call for call
        eng.act_step(env, sigma=0.1, seed=2, out=out)
        if per:
            rep.mark_new(n_envs)
        eng.sample(rep, expert, bc, n_main=B, seed=3, defer=True)
        eng.learn(bc_weight_now=100 if first[0] else None, bc_warm_up_weight=0.0)
        first[0] = False

    return step, eng


def counted(step, eng):
    """library calls and kernel launches of two consecutive steps (a critic-only call and an actor call)"""
    names, real = [], _lib.call
    out = {}
    for _ in range(2):
        del names[:]
        actor_call = eng.actor_trainable
        _lib.call = lambda name, *args: names.append(name) or real(name, *args)
        try:
            step()
        finally:
            _lib.call = real
        n = sum((LAUNCHES[k][int(actor_call)] if isinstance(LAUNCHES[k], tuple) else LAUNCHES[k]) for k in names)
        out["actor_call" if actor_call else "critic_only_call"] = {"library_calls": list(names), "kernel_launches": n}
    return out


def main():
    n_envs, cap, B = 4096, 1 << 20, 128
    rng = np.random.default_rng(0)
    expert = DeviceReplay(1024)
    expert.store_rows(torch.from_numpy(rng.normal(size=(1000, 32)).astype(np.float32)))
    bc = torch.from_numpy(rng.uniform(-1, 1, (1000, 32)).astype(np.float32)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "method": "device events around `steps_per_region` back-to-back reference-order vector steps on one stream "
           "(launch gaps included), 3 warm-up regions, median of 9 regions; the variants alternate in one process; 4,096 straight_line envs, HIRL soft fp32, "
           "B = 128, n_main = 128, ring of 2^20 slots, max_step 1500, auto_reset, random_reset"}
    plain, plain_eng = make(False, n_envs, cap, B, expert, bc)
    per, per_eng = make(True, n_envs, cap, B, expert, bc)
    res["without_hirl_per"] = timed(plain, 200)
    res["with_hirl_per"] = timed(per, 200)
    res["without_hirl_per_again"] = timed(plain, 200)
    res["with_hirl_per_again"] = timed(per, 200)
    res["calls_without_hirl_per"] = counted(plain, plain_eng)
    res["calls_with_hirl_per"] = counted(per, per_eng)
    assert not [n for c in res["calls_without_hirl_per"].values() for n in c["library_calls"] if "per" in n or "weighted" in n]  # flag off: the parent's calls
    assert torch.isfinite(per_eng.critic).all() and torch.isfinite(plain_eng.critic).all()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "hirl_per_step.json")
    json.dump(res, open(path, "w"), indent=1)
    for k, v in res.items():
        print(k, v if not isinstance(v, dict) else {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()})


if __name__ == "__main__":
    main()
