"""SacEngine.step_learn in FRONT form (hx_sac_front: the per-tile acting role + the first forward launch of learn() in one launch) against the
reference's order (act_step + sample(defer=True) + learn(): what the driver ran at these sizes before) at 1,024 / 4,096 / 8,192 serpentine envs,
B = 128, fp32 and bf16.  Device events around STEPS back-to-back steps after a warm-up, the ring pre-filled to 4 n; per size and dtype the two legs
run in ONE process on engines of their own, interleaved over REPS repetitions.
The tiling knob of the front leg (HX_SAC_FRONT_F32_NRT2_ROWS / HX_SAC_FRONT_BF16_NRT2_ROWS) is read once per process, so the default run starts one
child per setting, one after the other — 16-row acting workgroups at every size, 32-row ones at every size — and prints ONE JSON line with both:
  python tools/ubench/sac_front_small.py           (STEPS=1500 REPS=3 WARMUP=200 ENVS=1024,4096,8192 DTYPES=f32,bf16 in the environment to change them)
profiles/sac_front_small.json is the default run.  TILING=16 or TILING=32 (or TILING=default: the library's own rule) runs one setting in this process;
for per-kernel averages run one under the tracer, in a run of its own, and keep its kernel_stats.csv as profiles/sac_front_small_kernel_stats.csv:
  TILING=default LEGS=front STEPS=500 REPS=1 WARMUP=0 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sac_front_small -- python tools/ubench/sac_front_small.py"""
import json
import os
import subprocess
import sys

import numpy as np

STEPS, REPS, WARMUP = int(os.environ.get("STEPS", 1500)), int(os.environ.get("REPS", 3)), int(os.environ.get("WARMUP", 200))
ENVS = [int(x) for x in os.environ.get("ENVS", "1024,4096,8192").split(",") if x]
DTYPES = [d for d in os.environ.get("DTYPES", "f32,bf16").split(",") if d]
LEGS = [x for x in os.environ.get("LEGS", "front,reference").split(",") if x]
B = 128
KNOBS = ("HX_SAC_FRONT_F32_NRT2_ROWS", "HX_SAC_FRONT_BF16_NRT2_ROWS")
ROWS_OF = {"16": "1000000000", "32": "1"}  # the knob's value: 32-row workgroups from that many envs on


def measure():
    import torch

    sys.path.insert(0, ".")
    from hirl4ucav_amd.agents.sac_engine import SacEngine
    from hirl4ucav_amd.agents.SAC.agent import _xavier_mlp
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    def setup(n, dtype):
        torch.manual_seed(0)
        eng = SacEngine(batch=B, lr=1e-3, device="cuda")
        eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
        if dtype == "bf16":
            eng.set_act_dtype("bf16")
            eng.set_update_dtype("bf16")
        replay = DeviceReplay(1 << 20)
        env = BatchedHarfangEnv(n, scenario="serpentine", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=replay)
        env.reset()
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        while int(replay.total.item()) < 4 * n:
            eng.act_step(env, seed=1, out=out)
        return eng, env, out

    def front(eng, env, out):
        eng.step_learn(env, act_seed=1, out=out, sample_seed=2)

    def reference(eng, env, out):
        eng.act_step(env, seed=1, out=out)
        eng.sample(env.replay, None, seed=2, defer=True)
        eng.learn()

    def run(leg, side, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            leg(*side)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / steps

    legs = {"front": front, "reference": reference}
    res = {}
    for n in ENVS:
        for d in DTYPES:
            sides = {k: setup(n, d) for k in LEGS}
            if WARMUP > 0:
                for k, s in sides.items():
                    run(legs[k], s, WARMUP)
            us = {k: [] for k in sides}
            for _ in range(REPS):
                for k, s in sides.items():
                    us[k].append(run(legs[k], s, STEPS))
            for k, (eng, _, _) in sides.items():
                assert np.isfinite(eng.losses_host()).all(), (n, d, k)
            res[f"{n}/{d}"] = {k: {"us_per_step": sorted(v), "median_us": float(np.median(v)), "spread_us": max(v) - min(v)} for k, v in us.items()}
            del sides
    return res


def main():
    tiling = os.environ.get("TILING")
    if tiling:
        if tiling in ROWS_OF:
            for k in KNOBS:
                os.environ[k] = ROWS_OF[tiling]  # before the library's first launch_front_sac reads them
        print(json.dumps({"tiling": tiling, "results": measure()}), flush=True)
        return
    out = {"what": f"SacEngine.step_learn (front) against act_step + sample(defer) + learn() (reference order), serpentine envs, B = {B}",
           "steps_per_rep": STEPS, "reps": REPS, "warmup": WARMUP, "acting_rows_per_workgroup": {}}
    for t in ("16", "32"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, TILING=t), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"the {t}-row run ended with status {r.returncode}")
        out["acting_rows_per_workgroup"][t] = json.loads(r.stdout.strip().splitlines()[-1])["results"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
