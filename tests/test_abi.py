"""The C-ABI library loads without a GPU and exports every symbol include/hirl4ucav.h (product) and include/hirl4ucav_debug.h
(measurement helpers) declare — and nothing else named hx_* (no compute)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers=("hirl4ucav.h", "hirl4ucav_debug.h")):
    out = set()
    for h in headers:
        text = open(os.path.join(REPO, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        out |= set(re.findall(r"\b(hx_[a-z0-9_]+)\s*\(", text))
    return sorted(out)


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for must in ("hx_env_step", "hx_env_reset", "hx_label_transitions", "hx_last_error"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    so = os.path.join(REPO, "hirl4ucav_amd", "libhx_mi355.so")
    if not os.path.exists(so):
        import __graft_entry__ as g

        g.build()
    L = ctypes.CDLL(so)
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    assert not missing, missing
    L.hx_version.restype = ctypes.c_int
    assert L.hx_version() >= 100
    # ... and exports nothing the headers do not declare; the debug helpers live in their own header
    import subprocess

    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    exported = sorted({ln.split()[-1] for ln in nm.splitlines() if ln.split() and ln.split()[-1].startswith("hx_") and " T " in ln})
    assert exported == declared_symbols(), sorted(set(exported) ^ set(declared_symbols()))
    assert not [s for s in declared_symbols(("hirl4ucav.h",)) if s.startswith("hx_debug")]


def test_argument_errors_are_reported_not_swallowed():
    from hirl4ucav_amd import _lib

    with pytest.raises(_lib.HxError, match="hx_env_step"):
        _lib.call("hx_env_step", None, 0, 0, None, None, None, None, None, None, None)


def test_product_does_not_import_the_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    bad = []
    for root, _, files in os.walk(os.path.join(REPO, "hirl4ucav_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                if "oracle" in open(os.path.join(root, f), errors="ignore").read().replace("the scalar oracle", ""):
                    bad.append(os.path.join(root, f))
    assert not bad, bad


def test_abi_version_and_struct_sizes_match_the_binding():
    """HX_ABI_VERSION of the header == hx_version() of the library == the binding's, and every struct that crosses the boundary has the size
    the library was compiled with (hx_abi_sizes) — the check _lib.load() / the engines run at construction (a binding that had
    drifted from the header handed the kernels a 9-word statistics buffer under a library that adds into 512 words)."""
    import re

    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents import engine as E
    from hirl4ucav_amd.agents import sac_engine as SE

    hdr = open(os.path.join(REPO, "include", "hirl4ucav.h")).read()
    declared = int(re.search(r"#define HX_ABI_VERSION (\d+)", hdr).group(1))
    L = _lib.load()
    assert declared == _lib.ABI_VERSION == L.hx_version()
    sizes = (ctypes.c_int32 * 8)()
    L.hx_abi_sizes.argtypes = [ctypes.POINTER(ctypes.c_int32)]
    assert L.hx_abi_sizes(sizes) == 0
    for i, cls in enumerate((_lib.HxStepOpts, E.HxNets, E.HxHyper, E.HxBatch, E.HxSample, SE.HxSacNets, SE.HxSacBatch)):
        assert sizes[i] == ctypes.sizeof(cls), (cls.__name__, sizes[i], ctypes.sizeof(cls))
        _lib.check_struct(i, cls)
    assert sizes[7] == _lib.STAT_WAYS * _lib.STAT_PITCH

    class Short(ctypes.Structure):
        _fields_ = [("a", ctypes.c_void_p)]

    with pytest.raises(_lib.HxError, match="ABI mismatch"):
        _lib.check_struct(1, Short)


# ---- the binding is read from the headers (hirl4ucav_amd/_abi.py) ----------------------------------------------------------------------
_vp, _i32, _i64, _u32, _u64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float


def _struct_ptr(name):
    from hirl4ucav_amd import _lib

    return ctypes.POINTER(_lib.STRUCTS[name])


def test_every_declared_symbol_has_a_derived_signature_and_no_other():
    from hirl4ucav_amd import _abi

    assert sorted(_abi.abi().functions) == declared_symbols()


def test_a_bare_load_binds_every_declared_function(monkeypatch):
    """_lib.load() alone — a fresh CDLL object that no engine module has touched — sets argtypes and restype of every declared function, so a
    return type no longer depends on which module ran first (hx_actor_message_floats returns int64_t and used to be called with the default int)"""
    from hirl4ucav_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    L = _lib.load()
    for name in declared_symbols():
        assert getattr(L, name).argtypes is not None, name
    assert L.hx_actor_message_floats.restype is ctypes.c_int64
    with pytest.raises(TypeError):  # too few arguments stop in Python instead of reaching C
        L.hx_trace_workspace_words(1)


def test_pinned_signatures():
    """written out by hand once: between them every type word of the headers, every return type and the multi-line form"""
    from hirl4ucav_amd import _abi

    P = _struct_ptr
    pinned = {
        "hx_hirl_front": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _f32, _u64, _u32, _u32, _vp, _vp, _vp, P("HxStepOpts"), P("HxNets"), P("HxBatch"),
                                         P("HxHyper"), _i32, _i32, P("HxFront"), _vp]),
        "hx_allreduce_twostage": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _u32, _i32, _i32, _vp]),
        "hx_event_create": (_vp, []),
        "hx_last_error": (ctypes.c_char_p, []),
        "hx_trace_workspace_words": (_i64, [_i64, _i32]),
        "hx_env_step": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, P("HxStepOpts"), _vp]),
    }
    assert len(pinned["hx_hirl_front"][1]) == 22
    for name, (restype, argtypes) in pinned.items():
        got = _abi.abi().functions[name]
        assert got[0] is restype and got[1] == argtypes, (name, got)


def test_derived_structs_have_the_librarys_sizes():
    from hirl4ucav_amd import _lib

    L = _lib.load()
    sizes = (ctypes.c_int32 * 8)()
    assert L.hx_abi_sizes(sizes) == 0
    for i, name in enumerate(("HxStepOpts", "HxNets", "HxHyper", "HxBatch", "HxSample", "HxSacNets", "HxSacBatch")):
        assert ctypes.sizeof(_lib.STRUCTS[name]) == sizes[i], name
    for fn, name in (("hx_per_sizeof", "HxPer"), ("hx_ups_sizeof", "HxUps"), ("hx_nstep_sizeof", "HxNStep"), ("hx_trace_sizeof", "HxTrace"),
                     ("hx_epstat_sizeof", "HxEpStat"), ("hx_sac_imit_sizeof", "HxSacImit")):
        assert ctypes.sizeof(_lib.STRUCTS[name]) == getattr(L, fn)(), name
    assert len(_lib.STRUCTS) == 14


def test_one_class_per_struct():
    """a POINTER(HxName) argument takes only the class it was built from: every module hands out the same object"""
    from hirl4ucav_amd import _abi, _lib
    from hirl4ucav_amd.agents import engine, sac_engine
    from hirl4ucav_amd.utils import buffer

    assert engine.HxSample is sac_engine.E.HxSample is _lib.STRUCTS["HxSample"]
    assert _lib.HxStepOpts is _abi.abi().functions["hx_env_step"][1][8]._type_
    for mod, names in ((_lib, "HxStepOpts HxTrace HxEpStat"), (engine, "HxBatch HxSample HxFront HxNets HxHyper"), (sac_engine, "HxSacNets HxSacImit HxSacBatch"),
                       (buffer, "HxPer HxUps HxNStep")):
        for name in names.split():
            assert getattr(mod, name) is _lib.STRUCTS[name], name


@pytest.mark.parametrize("text, names", [
    ("int hx_a(size_t n);", "hx_a.*size_t"),                                                       # a parameter of an unknown type
    ("typedef struct HxA { float noise[4]; } HxA;\nint hx_a(void);", "HxA.*noise"),                # an array field
    ("int hx_a(int32_t n)\nint hx_b(void);", "hx_a"),                                              # cut off before its `;`: the count self-check
    ("typedef struct HxA { int32_t a : 3; } HxA;", "HxA.*a : 3"),                                  # a bit-field
    ("typedef struct HxA { float x; } HxA;\ntypedef struct HxB { HxA inner; } HxB;", "HxB.*HxA"),  # a nested struct
    ("typedef struct HxA { struct { float x; } in; } HxA;", "HxA"),
    ("double hx_a(void);", "hx_a.*double"),                                                        # an unknown return type
    ("int hx_a(const HxNope* p);", "hx_a.*HxNope"),                                                # a pointer to a struct nobody declared
])
def test_the_reader_refuses_what_it_does_not_understand(text, names):
    from hirl4ucav_amd import _abi

    with pytest.raises(_abi.HxError, match=names):
        _abi.parse(text)


def test_the_reader_reads_what_the_headers_use():
    from hirl4ucav_amd import _abi

    a = _abi.parse("#define HX_A 7\n#define HX_B (-2)\n#define HX_C (1u << 3)\n#define HX_D (1 << 16) /* c */\n#define HX_M(x) ((x) + 1)\n#define HX_N (__builtin_nanf(\"\"))\n"
                   "typedef struct HxS { float a, b; const uint64_t* p; // c\n int64_t n; } HxS;\n"
                   "int64_t hx_f(const HxS* s, uint32_t* const* q,\n          float x /* host */, void* stream);\nconst char* hx_g(void);")
    assert a.defines == {"HX_A": 7, "HX_B": -2, "HX_C": 8, "HX_D": 65536}
    assert a.structs["HxS"]._fields_ == [("a", _f32), ("b", _f32), ("p", _vp), ("n", _i64)]
    assert a.functions == {"hx_f": (_i64, [ctypes.POINTER(a.structs["HxS"]), _vp, _f32, _vp]), "hx_g": (ctypes.c_char_p, [])}


def test_register_checks_a_signature_against_the_header():
    from hirl4ucav_amd import _lib

    L = _lib.load()
    before = L.hx_sim_readback.argtypes
    _lib.register("hx_sim_readback", [_vp, _i64, _i64, _vp, _vp])
    _lib.register("hx_event_elapsed_us", [_vp, _vp, ctypes.POINTER(_f32)])  # any pointer that is not one of the header's structs reads as void*
    _lib.register("hx_trace_reset", [ctypes.POINTER(_lib.HxTrace), _vp])
    with pytest.raises(_lib.HxError, match="hx_sim_readback"):
        _lib.register("hx_sim_readback", [_vp, _i64, _i32, _vp, _vp])
    with pytest.raises(_lib.HxError, match="hx_trace_reset"):
        _lib.register("hx_trace_reset", [ctypes.POINTER(_lib.HxEpStat), _vp])
    with pytest.raises(_lib.HxError, match="hx_not_there"):
        _lib.register("hx_not_there", [_vp])
    assert L.hx_sim_readback.argtypes == before
