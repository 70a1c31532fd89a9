"""CPU side of the SAC bf16 path: the binding's HxSacNets carries the two image fields of include/hirl4ucav.h, the header declares the new entry
points, and train_all's --dtype / resume decision (resolve_dtype) returns the right result for every case."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hirl4ucav.h")


def test_binding_carries_the_sac_image_fields():
    pytest.importorskip("torch")
    from hirl4ucav_amd.agents import sac_engine as SE

    names = [f for f, _ in SE.HxSacNets._fields_]
    assert names[-2:] == ["w2_bf16_all", "policy_w2_bf16"]
    assert names.index("policy_w2_x9") == len(names) - 3  # appended behind the existing fields: the ABI's order


def test_header_declares_the_sac_bf16_entry_points():
    hdr = open(HEADER).read()
    for name in ("hx_sac_act", "hx_sac_act_step", "hx_sac_pack_update_images"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    for name in ("hx_sac_act", "hx_sac_act_step"):  # the bf16 acting image is an argument of the one entry point
        assert re.search(r"\bint %s\(const float\* policy, const float\* w2_f32i, const uint16_t\* w2_x9, const uint16_t\* w2_bf16," % name, hdr), name
    body = re.search(r"typedef struct HxSacNets \{(.*?)\} HxSacNets;", hdr, re.S).group(1)
    assert re.search(r"uint16_t\* w2_bf16_all;", body) and re.search(r"uint16_t\* policy_w2_bf16;", body)
    assert int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1)) >= 115


@pytest.mark.parametrize("sac,requested,snap,want", [
    # fresh runs
    (True, "f32", None, ("f32", False, False)),
    (True, "bf16", None, ("bf16", False, False)),
    (True, "bf16_policy", None, ("bf16_policy", False, False)),
    (True, "f32x9", None, ("f32", True, False)),  # SAC has no exact-split format
    (False, "bf16", None, ("bf16", False, False)),
    (False, "f32x9", None, ("f32x9", False, False)),
    # marked SAC snapshots: the dtype must match
    (True, "bf16", {"dtype": "bf16", "dtype_honoured": True}, ("bf16", False, False)),
    (True, "f32", {"dtype": "bf16", "dtype_honoured": True}, ("f32", False, True)),
    (True, "bf16", {"dtype": "f32", "dtype_honoured": True}, ("bf16", False, True)),
    (True, "bf16_policy", {"dtype": "bf16", "dtype_honoured": True}, ("bf16_policy", False, True)),
    (True, "f32x9", {"dtype": "f32", "dtype_honoured": True}, ("f32", True, False)),
    # unmarked SAC snapshots (written before SAC had bf16: a --dtype bf16 run stored "f32"): fp32 with the warning
    (True, "bf16", {"dtype": "f32"}, ("f32", True, False)),
    (True, "bf16_policy", {"dtype": "f32"}, ("f32", True, False)),
    (True, "f32", {"dtype": "f32"}, ("f32", False, False)),
    (True, "bf16", {}, ("f32", True, False)),
    # HIRL / TD3: unchanged rule, marked or not
    (False, "bf16", {"dtype": "f32"}, ("bf16", False, True)),
    (False, "bf16", {"dtype": "bf16"}, ("bf16", False, False)),
    (False, "f32", {"dtype": "bf16", "dtype_honoured": True}, ("f32", False, True)),
])
def test_resolve_dtype(sac, requested, snap, want):
    pytest.importorskip("torch")
    from hirl4ucav_amd.train_all import resolve_dtype

    dtype, warning, refusal, mark = resolve_dtype(sac, requested, snap)
    assert (dtype, warning is not None, refusal is not None) == want
    if refusal:
        assert f"--dtype {snap['dtype']}" in refusal
    # the mark is withheld exactly where the legacy fallback applied
    legacy = sac and requested in ("bf16", "bf16_policy") and snap is not None and not snap.get("dtype_honoured")
    assert mark == (not legacy)


@pytest.mark.parametrize("requested", ["bf16", "bf16_policy"])
def test_legacy_sac_run_keeps_resuming_with_its_own_command_line(requested):
    """A chain of resumes of a SAC run from before SAC had bf16, each with the run's own --dtype: every link runs fp32 with the warning and is
    never refused, because the snapshots it writes stay unmarked.  A fresh run with the same flag is marked from its first snapshot on."""
    pytest.importorskip("torch")
    from hirl4ucav_amd.train_all import resolve_dtype

    snap = {"dtype": "f32", "seed": 2}  # what the old driver stored for --dtype bf16
    for _ in range(3):
        dtype, warning, refusal, mark = resolve_dtype(True, requested, snap)
        assert dtype == "f32" and warning and refusal is None and not mark
        snap = {"dtype": dtype, "seed": 2, **({"dtype_honoured": True} if mark else {})}  # what train_all writes next
    dtype, warning, refusal, mark = resolve_dtype(True, requested, None)
    assert (dtype, warning, refusal, mark) == (requested, None, None, True)
    snap = {"dtype": dtype, "dtype_honoured": True}
    for _ in range(2):
        dtype, warning, refusal, mark = resolve_dtype(True, requested, snap)
        assert (dtype, warning, refusal, mark) == (requested, None, None, True)
