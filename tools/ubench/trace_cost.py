"""Cost of the episode record on the MI355X -> profiles/trace_cost.json: train_all.validate() with and without an EpisodeRecorder, at 50 episodes
(the drivers' validation; --plot tracks the last one) and at 4,096 envs, all tracked, plus hx_trace_push alone.  Device events around whole
validate() calls on a prepared, freshly reset env (its host synchronisations every 64 steps included), warm-up, median of repeated regions, the
variants alternating in one process.

    python tools/ubench/trace_cost.py [out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ubench/trace_cost.py --push-only N   (the kernel's own duration: 3,500 pushes of N envs, all tracked)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hirl4ucav_amd import train_all as T
from hirl4ucav_amd.agents import sac_engine as SE
from hirl4ucav_amd.agents.SAC.agent import _xavier_mlp
from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
from hirl4ucav_amd.utils.trace import EpisodeRecorder

STEPS = 1500  # the drivers' validationStep in straight_line / serpentine


def stats(out, **kw):
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out)), "regions": len(out), **kw}


def push_only(n):
    """hx_trace_push alone, for a kernel trace: nothing is timed here"""
    dev = torch.device("cuda")
    env = BatchedHarfangEnv(n, scenario="serpentine", device=dev, seed=1, auto_reset=False, random_reset=True, collect_stats=False)
    env.reset()
    env.step(torch.zeros((n, 4), device=dev))
    rec = EpisodeRecorder(env, None, max_steps=STEPS)
    for _ in range(3500):
        rec.t = 0
        rec.push()
    torch.cuda.synchronize()
    print("pushed", n, "envs; still running", rec.alive())


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--push-only":
        return push_only(int(sys.argv[2]))
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"device events around one train_all.validate() of {STEPS} steps (SAC policy, exploit; serpentine, random reset, seed 1) on a prepared env, "
                     "reset before every region; 2 warm-up rounds, median of 7 rounds, the variants alternating inside every round; "
                     "push_alone: events around 500 back-to-back hx_trace_push launches on one stream (launch gaps included), every tracked env still running"}
    torch.manual_seed(0)
    eng = SE.SacEngine(batch=128)
    eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
    dev = torch.device("cuda")
    for n, tracked in ((50, "last"), (50, "all"), (4096, "all")):
        env = BatchedHarfangEnv(n, scenario="serpentine", device=dev, seed=1, auto_reset=False, random_reset=True, collect_stats=False)
        rec = EpisodeRecorder(env, [n - 1] if tracked == "last" else None, max_steps=STEPS)
        times = {"without": [], "with": []}
        results = {}
        for rnd in range(9):
            for variant in (("without", "with") if rnd % 2 == 0 else ("with", "without")):
                env.reset()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                results[variant] = T.validate(eng, "serpentine", n, STEPS, True, 1, dev, sac=True, env=env, recorder=rec if variant == "with" else None)
                b.record()
                torch.cuda.synchronize()
                if rnd >= 2:
                    times[variant].append(a.elapsed_time(b) * 1000.0)
        assert results["with"] == results["without"], results
        key = f"{n}_envs_{tracked}_tracked"
        sm = rec.summary()
        res[f"validate_without_recorder_{key}"] = stats(times["without"], steps=STEPS)
        res[f"validate_with_recorder_{key}"] = stats(times["with"], steps=STEPS, records=int(sm["nrec"].sum()), still_running=rec.alive())
        res[f"recorder_per_step_{key}_us"] = (res[f"validate_with_recorder_{key}"]["median_us"] - res[f"validate_without_recorder_{key}"]["median_us"]) / STEPS
        env.reset()
        env.step(torch.zeros((n, 4), device=dev))
        rec.reset()

        def push():
            rec.t = 0
            rec.push()

        out = []
        for rnd in range(10):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(500):
                push()
            b.record()
            torch.cuda.synchronize()
            if rnd >= 3:
                out.append(a.elapsed_time(b) * 1000.0 / 500)
        res[f"push_alone_{key}"] = stats(out, calls_per_region=500, still_running=rec.alive())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "trace_cost.json")
    json.dump(res, open(path, "w"), indent=1)
    for k, v in res.items():
        print(k, v if not isinstance(v, dict) else {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()})


if __name__ == "__main__":
    main()
