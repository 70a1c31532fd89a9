"""Zero-edit drop-in of the module paths: the reference's drivers import SCRIPT-RELATIVE modules
(`agents.HIRL`, `utils.buffer`, `environments.HarfangEnv_GYM`, ... — hirl/train_all.py:1-9, train_sac.py:4-9) while its agents import
PACKAGE-ABSOLUTE ones (`hirl.utils.buffer`, hirl/agents/HIRL.py:7).  The `hirl/` alias package of this repository must satisfy both
forms at once, exactly as they are written in the reference, from a process whose sys.path[0] is the `hirl/` directory — the
situation of `python hirl/train_all.py`."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (module path as the driver writes it, names the driver uses from it) — the API surface of SURVEY.md 8b
SCRIPT_RELATIVE = [
    ("agents.TD3", ["Agent"]), ("agents.HIRL", ["Agent"]), ("agents.BC", ["Agent"]), ("agents.SAC.agent", ["SacAgent"]),
    ("utils.plot", ["plot_3d_trajectories", "plot_distance"]), ("utils.data_processor", ["read_data"]),
    ("utils.buffer", ["UniformMemory", "torch", "np", "device"]),  # star-import: the driver takes torch / np / device from here
    ("utils.seed", ["set_seed"]),
    ("environments.HarfangEnv_GYM", ["HarfangEnv", "HarfangSerpentineEnv", "HarfangCircularEnv", "HarfangSerpentineInfiniteEnv"]),
    ("environments.dogfight_client", ["connect", "disable_log", "set_renderless_mode", "set_client_update_mode"]),
]
PACKAGE_ABSOLUTE = [("hirl.utils.buffer", ["UniformMemory", "Transition", "device"]), ("hirl.agents.HIRL", ["Agent"]),
                    ("hirl.environments.HarfangEnv_GYM", ["HarfangEnv"])]


def driver_style_program():
    lines = ["import sys, os", f"sys.path[0] = {os.path.join(ROOT, 'hirl')!r}  # what `python hirl/train_all.py` gives", f"sys.path.insert(1, {ROOT!r})"]
    for mod, names in SCRIPT_RELATIVE + PACKAGE_ABSOLUTE:
        lines.append(f"import importlib; m = importlib.import_module({mod!r})")
        for n in names:
            lines.append(f"assert hasattr(m, {n!r}), ({mod!r}, {n!r})")
    # the star-import forms of train_all.py:6-8 must leave these names in the driver's namespace
    lines += ["from utils.buffer import *", "from utils.seed import *", "from environments.HarfangEnv_GYM import *",
              "import environments.dogfight_client as df",
              "assert torch.__name__ == 'torch' and np.__name__ == 'numpy' and callable(set_seed) and callable(df.connect)",
              "assert HarfangEnv.__module__.startswith('hirl4ucav_amd.') and UniformMemory.__module__.startswith('hirl4ucav_amd.')",
              "import yaml; cfg = yaml.safe_load(open(os.path.join(sys.path[0], 'local_config.yaml')))",
              "assert cfg['experiment']['result_dir'] and cfg['network']['ip'] and 'straight_line' in cfg['experiment']['bc_actor_name']",
              "print('DROPIN_OK')"]
    return "\n".join(lines)


def test_reference_import_forms_resolve_with_zero_edits():
    p = subprocess.run([sys.executable, "-c", driver_style_program()], cwd=os.path.join(ROOT, "hirl"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300, env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"})
    assert p.returncode == 0 and "DROPIN_OK" in p.stdout, p.stderr[-3000:]

