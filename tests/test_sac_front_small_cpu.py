"""The SAC front launch up to 8,192 envs, the parts that need no GPU: the ABI version moved with the widened contract of hx_sac_front, the header says
what the entry point now takes, and train_all's --loop help no longer keeps SAC's front form to large populations."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "hirl4ucav.h")).read()


def test_abi_version_moved_in_header_and_binding():
    from hirl4ucav_amd import _lib

    declared = int(re.search(r"#define HX_ABI_VERSION (\d+)", header()).group(1))
    assert declared == _lib.ABI_VERSION and declared >= 117


def test_header_describes_the_front_launch_at_every_size():
    hdr = header()
    start = hdr.index("/* The SAC front launch")
    block = hdr[start:hdr.index("*/", start)]
    flat = " ".join(block.replace("*", " ").split())
    assert "n > 8,192" not in flat and "any n >= 1" in flat
    # which kernel acts at which size, the image rules, the unchanged draw rule, the bit-identity statement against the acting entry point
    for words in ("up to 8,192 envs the per-tile workgroups", "streaming persistent kernel", "w2_x9 is accepted and ignored", "HxSample.guard = n",
                  "hx_sac_act_step from the fp32 or the bf16 image", "Bit-identical to hx_sac_act_step with the same images for the same n"):
        assert words in flat, words
    # the signatures stand
    assert re.search(r"int hx_sac_front\(const float\* policy, const uint16_t\* w2_x9, const float\* w2_f32i, float\* state, int64_t n,", hdr)
    assert re.search(r"int hx_sac_learn_back\(const HxSacNets\* nets, const HxSacBatch\* batch, const HxHyper\* hyper, int32_t polyak_first,", hdr)


def test_loop_help_does_not_keep_sac_to_large_populations():
    from hirl4ucav_amd import train_all as T

    loop = [a for a in T.parser()._actions if "--loop" in a.option_strings][0]
    text = " ".join(loop.help.split())
    assert "beyond 8,192 envs" not in text and "SAC / E-SAC at every number of envs" in text
    assert loop.default == "front" and list(loop.choices) == ["front", "reference"]


def test_engine_no_longer_names_a_minimum_population():
    import inspect

    from hirl4ucav_amd.agents import sac_engine

    src = inspect.getsource(sac_engine.SacEngine.step_learn)
    assert "n <= 8192" not in src and "more than 8,192 envs" not in src
