"""Cost of n-step returns for HIRL on the MI355X -> profiles/hirl_nstep.json: one vector step (env step + draw + learn()) at 4,096 straight_line envs,
fp32, B = 128, in both loop forms — HirlEngine.step_learn (the front launch) and act_step + sample(defer=True) + learn() (the reference order) — with
set_multi_step(N = 3) on an env WITHOUT a ring against the same form with the in-launch one-step insert; and hx_nstep_label on a 20,000-row expert
table (run once per run).  Device events, warm-up, median of repeated regions, the variants alternating in one process (the one-step variants are
timed before and after the others).

    python tools/ubench/hirl_nstep.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hirl4ucav_amd.agents import engine as E
from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
from hirl4ucav_amd.train_all import init_actor_state_dict, init_critic_state_dict
from hirl4ucav_amd.utils.buffer import DeviceReplay, NStepInserter, nstep_relabel

N_ENVS, BATCH, N_STEP, CAP = 4096, 128, 3, 1 << 20


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


def make(n_step, bc):
    """-> (front step, reference-order step, engine) of one engine, env and ring; n_step 1: the env inserts one-step rows itself"""
    torch.manual_seed(0)
    eng = E.HirlEngine(batch=BATCH)
    eng.load_params(init_actor_state_dict(), init_critic_state_dict(), init_actor_state_dict())
    rep = DeviceReplay(CAP)
    env = BatchedHarfangEnv(N_ENVS, scenario="straight_line", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=rep if n_step == 1 else None)
    env.reset()
    out = torch.zeros((N_ENVS, 4), device="cuda")
    ins = None
    if n_step > 1:
        ins = NStepInserter(rep, N_ENVS, n_step, 0.99)
        ins.reset(env)
        eng.set_multi_step(ins)
    for _ in range(8):  # rows in the ring before the first draw
        eng.act_step(env, sigma=0.1, seed=2, out=out)
        if ins is not None:
            ins.push(env, out)

    def front():
        eng.step_learn(env, None, bc, n_main=BATCH, act_sigma=0.1, act_seed=2, out=out, sample_seed=3, bc_weight_now=0.3)

    def reference():
        eng.act_step(env, sigma=0.1, seed=2, out=out)
        if ins is not None:
            ins.push(env, out)
        eng.sample(rep, None, bc, n_main=BATCH, seed=3, defer=True)
        eng.learn(bc_weight_now=0.3)

    return front, reference, eng


def main():
    res = {"device": torch.cuda.get_device_name(0),
           "method": "device events around `calls_per_region` back-to-back vector steps on one stream (launch gaps included), 3 warm-up regions, median of 9 "
                     f"regions; variants alternate in one process; {N_ENVS} straight_line envs, fp32 (acting in the engine's default format), B = {BATCH}, "
                     f"HIRL with a fixed BC weight, max_step 1500, auto_reset, random_reset; ring of 2^20 slots; N = {N_STEP}"}
    rng = np.random.default_rng(0)
    bc = torch.from_numpy(rng.uniform(-1, 1, (20000, 32)).astype(np.float32)).cuda()
    front1, ref1, eng1 = make(1, bc)
    front3, ref3, eng3 = make(N_STEP, bc)
    res["front_one_step"] = timed(front1, 200)
    res[f"front_n{N_STEP}"] = timed(front3, 200)
    res["reference_one_step"] = timed(ref1, 200)
    res[f"reference_n{N_STEP}"] = timed(ref3, 200)
    res["front_one_step_again"] = timed(front1, 200)
    res["reference_one_step_again"] = timed(ref1, 200)
    for e in (eng1, eng3):
        e.front_check()
    for form in ("front", "reference"):
        base = 0.5 * (res[f"{form}_one_step"]["median_us"] + res[f"{form}_one_step_again"]["median_us"])
        res[f"{form}_n{N_STEP}_minus_one_step_us"] = res[f"{form}_n{N_STEP}"]["median_us"] - base
    # the expert table's relabelling: once per run
    rows = torch.from_numpy(rng.uniform(-1, 1, (20000, 32)).astype(np.float32)).cuda()
    last = torch.from_numpy((rng.random(20000) < 0.01).astype(np.uint8)).cuda()
    res[f"nstep_label_20000_rows_n{N_STEP}"] = timed(lambda: nstep_relabel(rows, last, N_STEP, 0.99), 50)
    res["nstep_label_20000_rows_n8"] = timed(lambda: nstep_relabel(rows, last, 8, 0.99), 50)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "hirl_nstep.json")
    json.dump(res, open(path, "w"), indent=1)
    for k, v in res.items():
        print(k, v if not isinstance(v, dict) else {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()})


if __name__ == "__main__":
    main()
