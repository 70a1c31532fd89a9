"""Cost of the n-step insert launch on the MI355X -> profiles/nstep_push.json: SacEngine.act_step on an env WITHOUT a ring plus NStepInserter.push,
against act_step with the in-launch one-step insert, at 4,096 and 16,384 serpentine envs for n = 1, 3, 8.  Device events, warm-up, median of
repeated regions, the variants alternating in one process (the with-ring variant is timed before and after the others).

    python tools/ubench/nstep_push.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hirl4ucav_amd.agents import sac_engine as SE
from hirl4ucav_amd.agents.SAC.agent import _xavier_mlp
from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
from hirl4ucav_amd.utils.buffer import DeviceReplay, NStepInserter


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
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out)), "regions": regions, "calls_per_region": reps}


def main():
    res = {"device": torch.cuda.get_device_name(0), "method": "device events around `calls_per_region` back-to-back calls on one stream (launch gaps included), "
           "3 warm-up regions, median of 9 regions; variants alternate in one process; max_step 1500, auto_reset, random_reset; ring of 2^20 slots"}
    cap = 1 << 20
    torch.manual_seed(0)
    eng = SE.SacEngine(batch=128)
    eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
    for n_envs in (4096, 16384):
        out = torch.zeros((n_envs, 4), device="cuda")

        def make(n):
            rep = DeviceReplay(cap)
            env = BatchedHarfangEnv(n_envs, scenario="serpentine", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=rep if n == 0 else None)
            env.reset()
            if n == 0:
                return lambda: eng.act_step(env, seed=2, out=out)
            ins = NStepInserter(rep, n_envs, n, 0.99)
            ins.reset(env)

            def step():
                eng.act_step(env, seed=2, out=out)
                ins.push(env, out)

            def push_only():
                ins.push(env, out)
            return step, push_only

        with_ring = make(0)
        no_ring_env = BatchedHarfangEnv(n_envs, scenario="serpentine", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=None)
        no_ring_env.reset()
        key = f"{n_envs}_serpentine"
        res[f"act_step_with_insert_{key}"] = timed(with_ring, 200)
        res[f"act_step_without_ring_{key}"] = timed(lambda: eng.act_step(no_ring_env, seed=2, out=out), 200)
        for n in (1, 3, 8):
            step, push_only = make(n)
            res[f"act_step_without_ring_plus_push_n{n}_{key}"] = timed(step, 200)
            res[f"push_alone_n{n}_{key}"] = timed(push_only, 200)  # (the env's outputs stand still: steady-state traffic, one finished row per env and call)
        res[f"act_step_with_insert_{key}_again"] = timed(with_ring, 200)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "nstep_push.json")
    json.dump(res, open(path, "w"), indent=1)
    for k, v in res.items():
        print(k, v if not isinstance(v, dict) else {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()})


if __name__ == "__main__":
    main()
