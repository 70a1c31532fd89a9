"""Cost of the prioritized-replay path on the MI355X -> profiles/per_sac.json: device events, warm-up, median of repeated regions, the variants
alternating in one process.  The comparison point of every PER figure is the same run without PER from the same build.

    python tools/ubench/per_time.py [out.json]
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
from hirl4ucav_amd.utils.buffer import DeviceReplay, PrioritizedReplay


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
           "3 warm-up regions, median of 9 regions; variants alternate in one process"}
    cap, B, n = 1 << 20, 256, 16384
    torch.manual_seed(0)
    per = PrioritizedReplay(cap)
    per.ring.normal_()
    per.ring[:, 31] = 0
    per.total += cap
    per._prio[:cap] = torch.rand(cap, device="cuda") + 0.1
    per.resum()
    uni = DeviceReplay(cap)
    uni.ring.copy_(per.ring)
    uni.total += cap
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    w = torch.zeros(B, device="cuda")
    rows = torch.zeros(B * 32, device="cuda")
    err = torch.rand(B, device="cuda")
    e = SE.SacEngine(batch=B)
    calls = [0]

    def per_sample():
        calls[0] += 1
        per.sample_into(B, idx, w, rows, seed=1, call=calls[0], beta=0.4)

    def uni_sample():
        calls[0] += 1
        SE._gather(SE._draw(uni, None, B, 1, calls[0], idx), B, rows)

    def mark():
        per.total += n  # (a device add of its own: subtracted below)
        per.mark_new(n)

    def total_add():
        per.total += n

    per_sample()
    res["hx_sample_batch_uniform_B256"] = timed(uni_sample, 200)
    res["hx_per_sample_B256_cap2^20"] = timed(per_sample, 200)
    res["hx_sample_batch_uniform_B256_again"] = timed(uni_sample, 200)
    res["hx_per_update_B256_cap2^20"] = timed(lambda: per.update(idx, err), 200)
    res["total_add_only"] = timed(total_add, 200)
    res["hx_per_mark_new_n16384_plus_total_add"] = timed(mark, 200)
    res["hx_per_mark_new_n16384"] = {"median_us": res["hx_per_mark_new_n16384_plus_total_add"]["median_us"] - res["total_add_only"]["median_us"],
                                     "note": "difference of the two medians above"}
    # the update: weighted against the one call, B = 256, on the same tile
    ew, ep = SE.SacEngine(batch=B), SE.SacEngine(batch=B)
    small = PrioritizedReplay(1 << 14)
    small.ring.normal_(); small.ring[:, 31] = 0; small.total += 1 << 14; small.mark_new()
    for eng in (ew, ep):
        eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
    ew.set_prioritized(small)
    ew.sample(small, seed=3)
    ep.rows.copy_(ew.rows)
    plain = timed(lambda: ep.learn(), 100)
    weighted = timed(lambda: ew.learn(), 100)
    plain2 = timed(lambda: ep.learn(), 100)
    res["hx_sac_learn_B256"] = plain
    res["hx_sac_learn_weighted_plus_hx_per_update_B256_cap2^14"] = weighted
    res["hx_sac_learn_B256_again"] = plain2
    # the vector step of configs[2]'s shape, reference order, with and without PER (both from this build)
    def loop(with_per):
        rep = PrioritizedReplay(cap) if with_per else DeviceReplay(cap)
        env = BatchedHarfangEnv(n, scenario="serpentine", seed=1, max_step=1500, auto_reset=True, random_reset=True, replay=rep)
        env.reset()
        eng = SE.SacEngine(batch=128)
        eng.load_params(_xavier_mlp(13, 8), _xavier_mlp(17, 1), _xavier_mlp(17, 1))
        out = torch.zeros((n, 4), device="cuda")
        if with_per:
            eng.set_prioritized(rep)

            def step():
                eng.step_learn(env, act_seed=2, sample_seed=3, out=out)
        else:
            def step():
                eng.act_step(env, seed=2, out=out)
                eng.sample(rep, None, seed=3, defer=True)
                eng.learn()
        return step

    s_plain, s_per = loop(False), loop(True)
    res["vector_step_16384_serpentine_sac_f32_reference_order"] = timed(s_plain, 100, regions=7)
    res["vector_step_16384_serpentine_sac_f32_reference_order_per"] = timed(s_per, 100, regions=7)
    res["vector_step_16384_serpentine_sac_f32_reference_order_again"] = timed(s_plain, 100, regions=7)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "profiles", "per_sac.json")
    json.dump(res, open(out, "w"), indent=1)
    for k, v in res.items():
        print(k, v if not isinstance(v, dict) else {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()})


if __name__ == "__main__":
    main()
