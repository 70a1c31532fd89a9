"""SacEngine.learn() at B = 128 by device events: plain SAC and imitative SAC (set_imitative: the BC-gated policy loss), each built from the PARENT
commit and from this tree — alternating, each side a process of its own (two builds of the library cannot
share one), on one box in one call.  Each process: the minibatch (and the expert tile) assembled once, WARMUP calls, then REPS repetitions
of CALLS back-to-back learn() calls between two events; it reports its median and its own spread.  The driver alternates the sides ROUNDS
times and reports, per side, the median over the rounds and the run-to-run spread (min .. max of the rounds' medians).
  python tools/ubench/isac_time.py --parent-tree DIR      (DIR: a checkout of the parent commit with its library built)
  gate 1: imitative learn() <= 2.0 x the parent's plain learn();  gate 2: this tree's plain (and imitative) learn() within the parent's spread.
profiles/isac_learn_ab.txt is the default run.  Launch counts come from a tracer run of its own, one side at a time:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <side> -- python tools/ubench/isac_time.py --worker <plain|isac> --trace"""
import argparse
import json
import os
import subprocess
import sys

CALLS, REPS, WARMUP, ROUNDS, B = (int(os.environ.get(k, d)) for k, d in (("CALLS", 2000), ("REPS", 10), ("WARMUP", 500), ("ROUNDS", 5), ("BATCH", 128)))


def worker(side, tree, trace):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch

    from hirl4ucav_amd.agents.sac_engine import SacEngine
    from hirl4ucav_amd.agents.SAC.agent import _xavier_mlp
    from hirl4ucav_amd.agents.HIRL import init_actor_state_dict
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    torch.manual_seed(0)
    eng = SacEngine(batch=B, lr=1e-3, device="cuda")
    eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
    rng = np.random.default_rng(0)
    rep = DeviceReplay(4096)
    rows = rng.normal(size=(4096, 32)).astype(np.float32)
    rows[:, 31] = rows[:, 31] > 1.0
    rep.store_rows(torch.from_numpy(rows))
    eng.sample(rep, None, seed=1)
    if side == "isac":
        eng.set_imitative(init_actor_state_dict(), slope=0.01)
        exp = DeviceReplay(1024)
        er = rng.normal(size=(1000, 32)).astype(np.float32)
        er[:, 13:17] = rng.uniform(-1, 1, (1000, 4))
        exp.store_rows(torch.from_numpy(er))
        eng.sample_expert(exp, seed=1)

    def run(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            eng.learn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / calls

    if trace:  # under the tracer: CALLS learn() calls and nothing timed (the set-up's few launches are in the trace too)
        run(CALLS)
        print(json.dumps({"side": side, "learn_calls": CALLS}), flush=True)
        return
    run(WARMUP)
    us = sorted(run(CALLS) for _ in range(REPS))
    assert np.isfinite(eng.losses_host()).all()
    print(json.dumps({"side": side, "median_us": float(np.median(us)), "min_us": us[0], "max_us": us[-1]}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--worker", choices=["plain", "isac"], default=None)
    p.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    p.add_argument("--trace", action="store_true")
    p.add_argument("--parent-tree", dest="parent_tree", default=None)
    a = p.parse_args()
    if a.worker:
        return worker(a.worker, a.tree, a.trace)
    import numpy as np

    sides = ([("parent_plain", "plain", a.parent_tree), ("parent_isac", "isac", a.parent_tree)] if a.parent_tree else []) + \
            [("plain", "plain", a.tree), ("isac", "isac", a.tree)]
    got = {name: [] for name, _, _ in sides}
    for _ in range(ROUNDS):
        for name, side, tree in sides:  # a fresh child process per side and round: nothing of one build lives in the other's process
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", side, "--tree", tree], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"{name}: the worker exited with {out.returncode}; stopping")
            got[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    res = {"what": f"SacEngine.learn(), B = {B}, {CALLS} calls per repetition, {REPS} repetitions per process, {ROUNDS} alternating rounds", "sides": {}}
    for name, v in got.items():
        med = [x["median_us"] for x in v]
        res["sides"][name] = {"median_us": float(np.median(med)), "round_medians_us": [round(x, 3) for x in med], "spread_us": [min(med), max(med)],
                              "within_process_us": [min(x["min_us"] for x in v), max(x["max_us"] for x in v)]}
    s = res["sides"]
    if "parent_plain" in s:
        res["gate1_isac_over_parent_plain"] = s["isac"]["median_us"] / s["parent_plain"]["median_us"]
        res["gate1_ok"] = res["gate1_isac_over_parent_plain"] <= 2.0
    for side in ("plain", "isac"):  # gate 2, per side the parent has: no slower than the parent's own slowest round (lo .. hi: its run-to-run spread)
        if "parent_" + side in s:
            res[f"gate2_{side}_minus_parent_us"] = s[side]["median_us"] - s["parent_" + side]["median_us"]
            res[f"gate2_{side}_ok"] = s[side]["median_us"] <= s["parent_" + side]["spread_us"][1]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
