"""Time the cost of coloured exploration noise (profiles/noise_cost.txt) — tools/ubench/selfimit_step.py's method:

    python tools/ubench/noise_step.py ROOT LABEL front|reference [train_all flags, e.g. --explore_noise pink]
    python tools/ubench/noise_step.py ROOT LABEL fill

front | reference: HIRL soft, fp32, 4,096 straight_line envs, B = 128.  ROOT is a built checkout: this one, or the parent commit's for the A/B (its own
Python and library).  One process = one configuration: alternate the processes (parent, this tree without the flags, with them) on one box and compare
the medians.  The step is train_all's own step_front_hirl / step_reference (expert_num is put back to the batch size every 1,000 steps, in every
configuration alike), 500 warm-up steps, then STEP_W (5) windows of STEP_K (4,000) steps, each between two device synchronisations on the host clock.
fill: hx_noise_fill alone by device events, 4,096 envs, pink at 6 octaves, chunk 16 — 200 warm-up fills, then 5 windows of 2,000 fills back to back
between two events (us per fill; / 16 = per vector step), and the same at chunk 1 and 64.  Prints one RESULT line."""
import json
import os
import sys
import tempfile
import time

root, label, loop, extra = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3], sys.argv[4:]
sys.path.insert(0, root)
import torch  # noqa: E402

from hirl4ucav_amd import train_all as T  # noqa: E402

assert os.path.abspath(T.__file__).startswith(root), T.__file__

if loop == "fill":
    from hirl4ucav_amd.utils.noise import ColoredNoise

    out = {"label": label, "loop": loop}
    for chunk in (16, 1, 64):
        gen = ColoredNoise(4096, "pink", octaves=6, sigma=0.1, sigma_max=0.4, seed=1, chunk=chunk, device="cuda")
        for _ in range(200):
            gen.fill(0, chunk, gen.out)
        us = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(2000):
                gen.fill(i * chunk, chunk, gen.out)
            b.record()
            torch.cuda.synchronize()
            us.append(round(a.elapsed_time(b) * 1e3 / 2000, 3))
        out[f"us_per_fill_chunk{chunk}"] = us
        out[f"median_chunk{chunk}"] = sorted(us)[2]
    print("RESULT " + json.dumps(out), flush=True)
    raise SystemExit(0)

cfg = T.parse_args(["--agent", "HIRL", "--type", "soft", "--env", "straight_line", "--num_envs", "4096", "--loop", loop, "--synthetic_expert", "--seed", "1",
                    "--random", "--snapshot_every", "0", "--status_check_every", "0", "--result_dir", tempfile.mkdtemp()] + extra)
run = T.start_run(cfg)
for phase in (T.check_agent_flags, T.build_env, T.build_engine, T.load_expert_tables, T.set_dtype, T.open_run_dir, getattr(T, "build_explore", None),
              T.restore_or_explore, T.choose_loop):
    if phase is not None:  # (the parent commit has no build_explore)
        phase(run)
if run.writer is not None:  # no logging inside the timed windows
    run.writer.close()
run.writer = None
assert run.front == (loop == "front")
step = (lambda i, w: T.step_front_hirl(run, i, w, 0.0)) if run.front else (lambda i, w: T.step_reference(run, i, w, 0.0))


def window(k):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(k):
        if i % 1000 == 0:
            run.expert_num = run.batch  # every 1,000 steps, in every configuration alike
        step(1 + i % 1000, None)  # (never an episode's last step: every step learns)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / k * 1e6


step(1, 100)  # the soft weight is estimated once, as at an episode's first learn()
window(500)
us = [round(window(int(os.environ.get("STEP_K", "4000"))), 2) for _ in range(int(os.environ.get("STEP_W", "5")))]
if run.front and run.eng.front_status():
    raise SystemExit(f"front launch tripped (status word {run.eng.front_status()}): the windows are void")
print("RESULT " + json.dumps({"label": label, "loop": loop, "flags": extra, "us_per_step": us, "median": sorted(us)[len(us) // 2]}), flush=True)
