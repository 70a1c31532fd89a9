"""bench.py's launcher logic without a GPU: it must refuse to print a smaller run under a bigger --gpus."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_fails_loudly_without_n_gpus():
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--steps", "5", "--warmup", "1"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300, env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")})
    assert p.returncode != 0 and "8 GPUs requested" in p.stderr and p.stdout.strip() == ""


def test_world_size_must_match_gpus():
    env = {**os.environ, "WORLD_SIZE": "2", "RANK": "0"}
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "5", "--warmup", "1"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr


def test_cpu_baseline_legs_run_without_a_gpu():
    sys.path.insert(0, ROOT)
    import bench

    b0 = bench.baseline_reference_plumbing(1.0)
    assert b0["value"] > 0 and "messages per step" in b0["sample"]
    port = bench.baseline_port(bench.parse(["--envs", "512"]), 1.0)
    assert port["kind"] == "port" and port["value"] > 0
    b1 = bench.baseline_batched_cpu(0.5)
    assert b1["value"] > port["value"]
    sac = bench.baseline_port_sac(bench.parse(["--agent", "sac", "--envs", "512", "--scenario", "serpentine"]), 1.0)
    assert sac["kind"] == "port" and sac["value"] > 0 and "SAC" in sac["sample"]


def test_plain_run_times_exactly_the_steps_and_full_keeps_the_rest():
    """A plain run: no settle phase, no dry region, ONE timed region of --steps steps; --full: 1.5 s, 1 and 3 (0 s of settling when dumping
    outputs: a time-bounded phase would make the dumped step depend on the clock); explicit values always win."""
    sys.path.insert(0, ROOT)
    import bench

    a = bench.parse(["--steps", "7", "--warmup", "3"])
    assert (a.full, a.settle_s, a.dry_regions, a.reps, a.steps, a.warmup, a.dump_outputs) == (False, 0.0, 0, 1, 7, 3, None)
    f = bench.parse(["--full"])
    assert (f.full, f.settle_s, f.dry_regions, f.reps) == (True, 1.5, 1, 3)
    assert bench.parse(["--full", "--dump-outputs", "out"]).settle_s == 0.0 and bench.parse(["--dump-outputs", "out"]).dump_outputs == "out"
    e = bench.parse(["--full", "--settle-s", "0.3", "--dry-regions", "0", "--reps", "5"])
    assert (e.settle_s, e.dry_regions, e.reps) == (0.3, 0, 5)
    assert bench.parse(["--reps", "2", "--settle-s", "0.5"]).reps == 2
    # ring slots in row-tile order (repeatable outputs) where outputs are dumped; one atomic per workgroup otherwise, unless asked
    assert not a.ordered_slots and bench.parse(["--dump-outputs", "out"]).ordered_slots and bench.parse(["--ordered-slots"]).ordered_slots
    assert not bench.parse(["--dump-outputs", "out", "--no-ordered-slots"]).ordered_slots


def test_dump_outputs_writes_npy_files_within_64_mb(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import pytest

    import bench

    arrays = {"obs": np.arange(26, dtype=np.float32).reshape(2, 13), "losses": np.ones(6, np.float32)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["losses.npy", "obs.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "obs.npy"), arrays["obs"])
    with pytest.raises(AssertionError, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros((64 << 20) // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists()


def test_snapshot_of_a_large_population_is_a_fixed_seeded_sample(monkeypatch):
    """Beyond bench.DUMP_MAX_ROWS envs the per-env arrays are the same sorted, seeded sample of rows in every run (their ids in env_rows); the
    whole dump stays within 64 MB.  A stand-in for the loop, on CPU tensors."""
    sys.path.insert(0, ROOT)
    import types

    import numpy as np
    import torch

    import bench

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    n = bench.DUMP_MAX_ROWS + 1000
    env = types.SimpleNamespace(n=n, obs=torch.arange(n * 13, dtype=torch.float32).reshape(n, 13), reward=torch.arange(n, dtype=torch.float32),
                                done=torch.ones(n, dtype=torch.uint8), success=torch.zeros(n, dtype=torch.int8))
    eng = types.SimpleNamespace(losses_host=lambda: (1.0, 2.0, 3.0, 4.0, 5.0, 6.0), actor=torch.ones(10), critic=torch.ones(20))
    loop = types.SimpleNamespace(env=env, eng=eng, sac=False, actions=torch.zeros(n, 4))
    a, b = bench.snapshot_outputs(loop), bench.snapshot_outputs(loop)
    rows = a["env_rows"]
    assert rows.dtype == np.float64 and rows.shape == (bench.DUMP_MAX_ROWS,) and (np.diff(rows) > 0).all() and rows[-1] < n
    np.testing.assert_array_equal(rows, b["env_rows"])
    np.testing.assert_array_equal(a["reward"], rows.astype(np.float32))
    np.testing.assert_array_equal(a["obs"][:, 0], rows * 13)
    assert a["obs"].shape == (bench.DUMP_MAX_ROWS, 13) and a["done"].dtype == np.float32 and (a["done"] == 1).all()
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20


def test_ring_slot_header_is_opt_in():
    """DeviceReplay(ordered_slots=True) — bench.py's ring — carries the header of include/hirl4ucav.h HX_LAYOUT_ORDERED_SLOTS behind `total`
    (3 + cap / 16 words: total, launch sequence, status, one word per row tile); every other ring keeps a one-word counter."""
    sys.path.insert(0, ROOT)
    import torch

    from hirl4ucav_amd.utils.buffer import DeviceReplay

    plain = DeviceReplay(64, "cpu")
    assert plain.slot_header is None and plain.total.numel() == 1 and plain.slot_status() == 0
    r = DeviceReplay(64, "cpu", ordered_slots=True)
    assert r.slot_header.numel() == 3 + 64 // 16 and r.total.data_ptr() == r.slot_header.data_ptr()
    r.store_rows(torch.ones(5, 32))
    assert int(r.slot_header[0]) == 5 and len(r) == 5 and r.slot_status() == 0
    r.slot_header[2] = 1  # what a launch whose wait gave up leaves
    assert r.slot_status() == 1


def test_workload_label_names_a_baseline_config_only_when_the_arguments_match():
    sys.path.insert(0, ROOT)
    import bench

    assert "configs[1]" in bench.workload_label(bench.parse([]))
    assert "configs[" not in bench.workload_label(bench.parse(["--envs", "2048"]))
    assert "configs[" not in bench.workload_label(bench.parse(["--actions", "uniform"]))
    assert "configs[3]" in bench.workload_label(bench.parse(["--envs", "8192", "--scenario", "circular", "--type", "linear"]))
    assert "configs[4]" in bench.workload_label(bench.parse(["--envs", "16384", "--scenario", "mixed", "--dtype", "bf16"]))
    assert "configs[4]" not in bench.workload_label(bench.parse(["--envs", "16384", "--scenario", "mixed", "--dtype", "bf16_policy"]))
    assert "configs[2]" in bench.workload_label(bench.parse(["--agent", "sac", "--envs", "16384", "--scenario", "serpentine"]))


def test_loop_choice_never_takes_in_launch_waits_on_a_shared_gpu():
    """ranks that share a device run the reference's order unless --front asks for the other; every refusal names its reason."""
    sys.path.insert(0, ROOT)
    import bench

    front, why = bench.loop_choice(bench.parse([]), 1, False)
    assert front and "default" in why
    front, why = bench.loop_choice(bench.parse(["--gpus", "8"]), 8, True)
    assert not front and "8 ranks share a GPU" in why
    front, why = bench.loop_choice(bench.parse(["--gpus", "8"]), 8, False)  # a GPU each: the front loop, sharded
    assert front
    front, why = bench.loop_choice(bench.parse(["--gpus", "2", "--front"]), 2, True)  # asked for explicitly (soak tests)
    assert front and "--front given" in why and "ranks share a GPU" in why
    assert bench.loop_choice(bench.parse(["--no-front"]), 1, False) == (False, "--no-front given")
    for argv, word in ((["--batch", "512"], "batch > 256"), (["--actions", "uniform"], "uniform actions"), (["--dtype", "bf16_policy"], "bf16_policy"),
                       (["--agent", "sac"], "beyond 8,192 envs"), (["--overlap"], "--overlap"), (["--sample-launch"], "--sample-launch"),
                       (["--envs", "16384", "--front-acting", "mfma"], "at most 8,192 envs")):
        front, why = bench.loop_choice(bench.parse(argv), 1, False)
        assert not front and word in why, (argv, why)
    assert bench.loop_choice(bench.parse(["--agent", "sac", "--envs", "16384"]), 1, False)[0]
    assert not bench.loop_choice(bench.parse(["--agent", "sac", "--envs", "16384", "--gpus", "2"]), 2, False)[0]
    import pytest

    with pytest.raises(SystemExit, match="batch > 256"):
        bench.loop_choice(bench.parse(["--front", "--batch", "512"]), 1, False)


def test_roofline_fractions_stay_inside_the_roof_they_name():
    """the exact-split launches are priced by the bf16 FLOPs they execute; round 5's 131,072-env fp32 line (117.9 us at 65,536 envs,
    242 us at 131,072) read `frac` 0.93 / 1.04 against the fp32 matrix peak."""
    sys.path.insert(0, ROOT)
    from tools import bench_roofline as RL

    for envs, us in ((4096, 21.6), (65536, 117.86), (131072, 228.0)):
        flop = RL.ACTOR_FLOP * envs
        r = RL.matrix_roof(flop, envs, us, "x9")
        assert r["peak"] == 2500.0 and 0 < r["frac"] < 1 and r["flop_per_launch"] == flop + 5 * RL.PRODUCT_FLOP * envs
        eq = r["fp32_equivalent"]
        assert eq["peak"] == 157.3 and abs(eq["ratio_to_peak"] - flop / us / 1e6 / 157.3) < 1e-3 and "frac" not in eq
    assert RL.matrix_roof(RL.ACTOR_FLOP * 131072, 131072, 228.0, "x9")["fp32_equivalent"]["ratio_to_peak"] > 0.99  # what used to be printed as frac
    assert RL.matrix_roof(RL.ACTOR_FLOP * 4096, 4096, 19.2, "f32")["peak"] == 157.3 and RL.matrix_roof(1e9, 4096, 19.2, "bf16")["peak"] == 2500.0
