"""SacEngine.step_learn (the SAC front launch + the rest of learn()) at BASELINE.json configs[2]'s shape — 16,384 serpentine envs, B = 128 — in fp32
and in bf16 (set_act_dtype / set_update_dtype "bf16": MODE 2 acting, the bf16 first launch and the bf16 update), in turn in ONE process.  Device
events around STEPS back-to-back steps after a warm-up; REPS repetitions per dtype, interleaved; the median per dtype, one JSON line.
  python tools/ubench/sac_dtype_step.py            (STEPS=2000 REPS=3 WARMUP=200 ENVS=16384 DTYPES=f32,bf16 in the environment to change them)
profiles/sac_dtype_step.json is the default run.  profiles/sac_bf16_kernel_stats.csv is the bf16 side alone under the tracer, in a run of its own:
  DTYPES=bf16 STEPS=700 REPS=1 WARMUP=0 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sac_bf16 -- python tools/ubench/sac_dtype_step.py
(700 front launches; the few act_step / pack launches of the set-up are in it too)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from hirl4ucav_amd.agents.sac_engine import SacEngine  # noqa: E402
from hirl4ucav_amd.agents.SAC.agent import _xavier_mlp  # noqa: E402
from hirl4ucav_amd.environments.batched import BatchedHarfangEnv  # noqa: E402
from hirl4ucav_amd.utils.buffer import DeviceReplay  # noqa: E402

STEPS, REPS, WARMUP = int(os.environ.get("STEPS", 2000)), int(os.environ.get("REPS", 3)), int(os.environ.get("WARMUP", 200))
N, B = int(os.environ.get("ENVS", 16384)), 128
DTYPES = [d for d in os.environ.get("DTYPES", "f32,bf16").split(",") if d]


def setup(dtype):
    torch.manual_seed(0)
    eng = SacEngine(batch=B, lr=1e-3, device="cuda")
    eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
    if dtype == "bf16":
        eng.set_act_dtype("bf16")
        eng.set_update_dtype("bf16")
    replay = DeviceReplay(1 << 20)
    env = BatchedHarfangEnv(N, scenario="serpentine", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=replay)
    env.reset()
    out = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    while int(replay.total.item()) < 4 * N:  # a ring to draw from (the guard leaves out the n slots a step may overwrite)
        eng.act_step(env, seed=1, out=out)
    return eng, env, out


def run(eng, env, out, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        eng.step_learn(env, act_seed=1, out=out, sample_seed=2)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    sides = {d: setup(d) for d in DTYPES}
    for d, s in sides.items():
        if WARMUP > 0:
            run(*s, WARMUP)
    us = {d: [] for d in sides}
    for _ in range(REPS):
        for d, s in sides.items():
            us[d].append(run(*s, STEPS))
    for d, (eng, _, _) in sides.items():
        assert np.isfinite(eng.losses_host()).all(), d
    res = {"what": f"SacEngine.step_learn, {N} serpentine envs, B = {B}", "steps_per_rep": STEPS, "reps": REPS, "warmup": WARMUP,
           "us_per_step": {d: sorted(v) for d, v in us.items()}, "median_us": {d: float(np.median(v)) for d, v in us.items()}}
    if "f32" in us and "bf16" in us:
        res["bf16_over_f32"] = res["median_us"]["bf16"] / res["median_us"]["f32"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
