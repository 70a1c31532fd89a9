"""Cost of gradient-norm clipping (and of the fixed entropy coefficient) on the MI355X -> profiles/sac_clip.json: the 16,384-env serpentine SAC vector
step, fp32 and bf16, with and without a clip — device events, warm-up, median of repeated regions, every tree in fresh child processes that alternate.

    python tools/ubench/clip_time.py [out.json]                      this tree alone
    python tools/ubench/clip_time.py --against PARENT_TREE [out.json]   PARENT_TREE: a built checkout of the parent commit; children alternate
                                                                        parent, this, parent, this — the unclipped step of this tree must sit inside
                                                                        the parent's run-to-run spread (min .. max over its regions, both runs)
    python tools/ubench/clip_time.py --child TREE                    one measurement process (prints one JSON line)

A tree without SacEngine.set_grad_clip (the parent) measures the unclipped variants only.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def child(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch

    from hirl4ucav_amd.agents import sac_engine as SE
    from hirl4ucav_amd.agents.SAC.agent import _xavier_mlp
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    def timed(fn, reps=100, regions=7, warm=2):
        for _ in range(warm * reps):
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

    n, cap = 16384, 1 << 20

    def loop(dtype, clip=None, fixed=None, front=True):
        torch.manual_seed(0)
        rep = DeviceReplay(cap)
        env = BatchedHarfangEnv(n, scenario="serpentine", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=rep)
        env.reset()
        eng = SE.SacEngine(batch=128)
        eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
        if dtype == "bf16":
            eng.set_act_dtype("bf16")
            eng.set_update_dtype("bf16")
        if clip is not None:
            eng.set_grad_clip(clip)
        if fixed is not None:
            eng.set_entropy_tuning(False, fixed)
        out = torch.zeros((n, 4), device="cuda")
        eng.act_step(env, seed=2, out=out)  # rows in the ring before the first draw
        if front:
            return lambda: eng.step_learn(env, act_seed=2, sample_seed=3, out=out)

        def step():
            eng.act_step(env, seed=2, out=out)
            eng.sample(rep, None, seed=3, defer=True)
            eng.learn()
        return step

    has_clip = hasattr(SE.SacEngine, "set_grad_clip")
    res = {"tree": tree, "device": torch.cuda.get_device_name(0), "has_clip": has_clip}
    for dtype in ("f32", "bf16"):
        res[f"step_{dtype}_front"] = timed(loop(dtype))
        res[f"step_{dtype}_reference_order"] = timed(loop(dtype, front=False))
        if has_clip:
            res[f"step_{dtype}_grad_clip_1"] = timed(loop(dtype, clip=1.0))  # (step_learn takes the reference's order under a clip)
            res[f"step_{dtype}_fixed_alpha_front"] = timed(loop(dtype, fixed=0.2))
        res[f"step_{dtype}_front_again"] = timed(loop(dtype))
    print("CLIP_TIME " + json.dumps(res), flush=True)


def run_child(tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True, text=True, timeout=420)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("CLIP_TIME ")]
    if out.returncode != 0 or not lines:
        raise SystemExit(f"measurement child for {tree} failed (exit {out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return json.loads(lines[-1][len("CLIP_TIME "):])


def main(argv):
    if argv[:1] == ["--child"]:
        return child(argv[1])
    parent = None
    if argv[:1] == ["--against"]:
        parent, argv = os.path.abspath(argv[1]), argv[2:]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "sac_clip.json")
    res = {"method": "device events around 100 back-to-back vector steps on one stream (launch gaps included), 2 warm-up regions, median of 7 regions; "
                     "16,384 serpentine envs, batch 128, one update per step; every run a fresh child process, the trees alternating",
           "runs": []}
    order = [("parent", parent), ("this", ROOT)] * 2 if parent else [("this", ROOT)]
    for label, tree in order:
        r = run_child(tree)
        r["tree"] = label
        res["runs"].append(r)
        print(label, {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict)}, flush=True)
    if parent:
        cond = {}
        for key in ("step_f32_front", "step_bf16_front", "step_f32_reference_order", "step_bf16_reference_order"):
            keys = [key] + ([key + "_again"] if key.endswith("front") else [])
            pr = [r[k] for r in res["runs"] if r["tree"] == "parent" for k in keys]
            th = [r[k]["median_us"] for r in res["runs"] if r["tree"] == "this" for k in keys]
            lo, hi = min(p["min_us"] for p in pr), max(p["max_us"] for p in pr)
            cond[key] = {"parent_spread_us": [lo, hi], "parent_medians_us": [p["median_us"] for p in pr], "this_medians_us": th,
                         "within_parent_spread": all(lo <= t <= hi for t in th)}
        res["unclipped_within_parent_spread"] = cond
    json.dump(res, open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv[1:])
