"""ctypes binding of libhx_mi355.so (the C ABI declared in include/hirl4ucav.h).

There is NO fallback: if the HIP extension is missing or a call fails, this raises.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C hirl4ucav_amd/csrc``.
"""
import ctypes
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# HX_LIBRARY selects another build of the same library (A/B timing of two builds on one box, the phase-stamp build); never a fallback
SO_PATH = os.environ.get("HX_LIBRARY") or os.path.join(_HERE, "libhx_mi355.so")

_ABI = _abi.abi()  # structs, signatures and constants as include/hirl4ucav.h declares them: nothing below restates the header
HxError = _abi.HxError
DEFINES = _ABI.defines  # "HX_NAME" -> int


def _defines(names):
    return (DEFINES["HX_" + k] for k in names.split())


ENV_WORDS, OBS_DIM, ACT_DIM, ROW_WORDS = _defines("ENV_WORDS OBS_DIM ACT_DIM ROW_WORDS")
STAT_NAMES = ("episodes", "kills", "fire_success_episodes", "time_limit", "fires", "good_fires", "locked_steps", "env_steps", "nonfinite_actions")
STAT_WAYS, STAT_PITCH = _defines("STAT_WAYS STAT_PITCH")  # the counters are kept 32 times (way = workgroup % 32, one 128-byte line each); a statistic = the sum

F_LOCKED_PREV, F_LOCKED, F_SLOT_PREV, F_SLOT, F_FIRED, F_FIRE_SUCCESS, F_EPISODE_SUCCESS, F_DONE = _defines(
    "F_LOCKED_PREV F_LOCKED F_SLOT_PREV F_SLOT F_FIRED F_FIRE_SUCCESS F_EPISODE_SUCCESS F_DONE")
F_SCEN_SHIFT, F_SERP_POS, F_SERP_LONG, F_M_ACTIVE, F_M_GUIDED, F_SIM_SLOT = _defines("F_SCEN_SHIFT F_SERP_POS F_SERP_LONG F_M_ACTIVE F_M_GUIDED F_SIM_SLOT")
LAYOUT_ORDERED_SLOTS, = _defines("LAYOUT_ORDERED_SLOTS")  # the ring behind HxStepOpts.total carries the slot header (DeviceReplay(ordered_slots=True))
TRACE_FIELDS, TRACE_SUMMARIES = _defines("TRACE_FIELDS TRACE_SUMMARIES")
EPSTAT_BINS, EPSTAT_SUMS, EPSTAT_SLOT_WORDS = _defines("EPSTAT_BINS EPSTAT_SUMS EPSTAT_SLOT_WORDS")
ABI_VERSION, = _defines("ABI_VERSION")

STRUCTS = _ABI.structs  # name -> the ONE ctypes class of a `typedef struct Hx…` (a POINTER(HxName) argument takes only that class)
HxStepOpts = STRUCTS["HxStepOpts"]
HxTrace = STRUCTS["HxTrace"]  # the episode record's buffers (utils/trace.py carves them out of one workspace)
HxEpStat = STRUCTS["HxEpStat"]  # the episode statistics' buffers (utils/epstat.py carves them out of one workspace)


def layout(pair, envs_per_block):
    """HX_LAYOUT(pair, envs_per_block) of include/hirl4ucav.h: force the env-step launch shape (0 = library's choice)."""
    return ((1 if pair else 0) << 8) | (int(envs_per_block) // 4)


_lib = None


def check_struct(index, cls):
    """Compare ctypes.sizeof(cls) with the library's sizeof of the same struct (hx_abi_sizes): a binding that has drifted from the header
    would hand the kernels short buffers (a 9-word statistics buffer under a library that adds into 512 words)."""
    sizes = (ctypes.c_int32 * 8)()
    L = load()
    if L.hx_abi_sizes(sizes) != 0 or sizes[index] != ctypes.sizeof(cls):
        raise HxError(f"ABI mismatch: {cls.__name__} is {ctypes.sizeof(cls)} bytes here, {sizes[index]} in {SO_PATH}")
    if sizes[7] != STAT_WAYS * STAT_PITCH:
        raise HxError(f"ABI mismatch: a statistics buffer is {STAT_WAYS * STAT_PITCH} words here, {sizes[7]} in {SO_PATH}")


def load():
    """Load the shared library (once).  Raises HxError with build instructions when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise HxError(f"{SO_PATH} not found: the HIP extension is not built (run __graft_entry__.build() or "
                      f"`make -C hirl4ucav_amd/csrc`). There is no CPU fallback.")
    # torch first: libhx_mi355.so must bind to the SAME HIP runtime (libamdhip64) torch has loaded, because
    # device pointers and streams are shared with torch.  Loaded the other way round the process would hold two
    # runtimes and ours would see no device.
    import torch  # noqa: F401

    L = ctypes.CDLL(SO_PATH)
    _abi.bind(L)  # argtypes and restype of every function the headers declare
    if L.hx_version() != ABI_VERSION:
        raise HxError(f"{SO_PATH} implements ABI version {L.hx_version()}, the headers this binding is read from declare {ABI_VERSION} (include/hirl4ucav.h "
                      f"HX_ABI_VERSION): rebuild the library (make -C hirl4ucav_amd/csrc)")
    if L.hx_epstat_sizeof() != ctypes.sizeof(HxEpStat):
        raise HxError(f"ABI mismatch: HxEpStat is {ctypes.sizeof(HxEpStat)} bytes here, {L.hx_epstat_sizeof()} in {SO_PATH}")
    _lib = L
    return L


def register(name, argtypes):
    """Callers outside the package that still state a signature: it is compared with the header's (any pointer but one to a struct of the
    header counts as void*) and refused when it differs; nothing is overwritten."""
    if name not in _ABI.functions:
        raise HxError(f"{name} is not declared in the headers of {_abi.INCLUDE_DIR}")
    declared = _ABI.functions[name][1]
    given = [ctypes.c_void_p if issubclass(t, ctypes._Pointer) and t._type_ not in STRUCTS.values() else t for t in argtypes]
    if given != declared:
        raise HxError(f"{name}: the signature given, {[t.__name__ for t in argtypes]}, is not the header's, {[t.__name__ for t in declared]}")


def call(name, *args):
    L = load()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise HxError(f"{name} failed ({rc}): {L.hx_last_error().decode()}")


def ptr(t):
    """device pointer of a torch tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch

    return torch.cuda.current_stream().cuda_stream
