"""Time the vector step of train_all for the cost of self-imitation (profiles/selfimit_cost.txt) — tools/ubench/branch_step.py's method with the loop form as an
argument:

    python tools/ubench/selfimit_step.py ROOT LABEL front|reference [train_all flags, e.g. --expert_self 16384 --expert_self_steps 256]

HIRL soft, fp32, 4,096 straight_line envs, B = 128.  ROOT is a built checkout: this one, or the parent commit's for the A/B (its own Python and library).  One
process = one configuration: alternate the processes (parent, this tree without the flag, with it) on one box and compare the medians.  The step is
train_all's own step_front_hirl / step_reference with after_env_step behind the acting launch (expert_num is put back to the batch size every 1,000 steps:
the self rows are pushed only while the expert ring has a reader — so the timed step is the driver's step during the warm-up, or under --expert_floor), 500 warm-up steps, then STEP_W (5) windows of STEP_K (4,000) steps, each between two device
synchronisations on the host clock.  Prints one RESULT line."""
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
cfg = T.parse_args(["--agent", "HIRL", "--type", "soft", "--env", "straight_line", "--num_envs", "4096", "--loop", loop, "--synthetic_expert", "--seed", "1",
                    "--random", "--snapshot_every", "0", "--status_check_every", "0", "--result_dir", tempfile.mkdtemp()] + extra)
run = T.start_run(cfg)
for phase in (T.check_agent_flags, T.build_env, T.build_engine, T.load_expert_tables, T.set_dtype, T.open_run_dir, T.restore_or_explore, T.choose_loop):
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
            run.expert_num = run.batch  # every 1,000 steps, in every configuration alike: the warm-up's expert rows never run out, so the ring keeps a reader
        step(1 + i % 1000, None)  # (never an episode's last step: every step learns)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / k * 1e6


step(1, 100)  # the soft weight is estimated once, as at an episode's first learn()
window(500)
us = [round(window(int(os.environ.get("STEP_K", "4000"))), 2) for _ in range(int(os.environ.get("STEP_W", "5")))]
if run.front and run.eng.front_status():
    raise SystemExit(f"front launch tripped (status word {run.eng.front_status()}): the windows are void")
out = {"label": label, "loop": loop, "us_per_step": us, "median": sorted(us)[len(us) // 2]}
if getattr(run, "selfx", None) is not None:
    out["self_counters"] = run.selfx.counters()
print("RESULT " + json.dumps(out), flush=True)
