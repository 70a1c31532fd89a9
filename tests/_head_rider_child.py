"""Child process of tests/test_head_rider_gpu.py: the library reads HX_HEAD_RIDER once per process, so every case is run in a process of its own
setting and leaves what six consecutive learn() calls produced in <out dir>/<case>.npz.   python tests/_head_rider_child.py <out dir> [case ...]

Large arrays (networks, moments, gradients, W2 images) are stored as the SHA-256 of their bytes — equal digests are equal bits; the small ones (losses,
the BC weight, the slots' action rows and LayerNorm statistics) as their words."""
import ctypes
import hashlib
import itertools
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _hirl_data as D  # noqa: E402

BATCHES = (16, 48, 128, 256)
MODES = ("soft", "fixed", "td3", "noln")
DTYPES = ("f32", "bf16")
ORDERS = ("ref", "front")
SEQS = ("one", "staged")
CASES = ["-".join((dt, order, seq, mode, f"b{B}")) for dt, order, seq, mode, B in itertools.product(DTYPES, ORDERS, SEQS, MODES, BATCHES)]

# workspace slot layout (hx_update.h Slot / carve_slot, S_* order)
XP, H1, H2, OW, KC = 20, 256, 512, 8, 8
SLOT_FIELDS = (("x", XP), ("z1", H1), ("st1", 2), ("h1", H1), ("z2", H2), ("st2", 2), ("outv", OW), ("dz2", H2), ("dh1", H1), ("dout", OW), ("lnp", 2 * KC))
SLOTS = ["TA", "C1", "C2", "TC1", "TC2", "API", "ABC", "BCS", "CPI", "CSOFT"]
PER_ROW = sum(n for _, n in SLOT_FIELDS)
SENTINEL = -12345.0
NETS = ("actor", "critic", "target_actor", "target_critic", "bc_actor", "m_actor", "v_actor", "m_critic", "v_critic")


def field(e, slot, name):
    """a view of one field of one workspace slot, [B][width]"""
    B = e.batch
    o = SLOTS.index(slot) * PER_ROW * B
    for k, n in SLOT_FIELDS:
        if k == name:
            return e.ws[o:o + B * n].view(B, n)
        o += B * n
    raise KeyError(name)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().copy()


def digest(t):
    return np.frombuffer(hashlib.sha256(bits(t).tobytes()).digest(), np.uint8).copy()


def make_engine(engine, dtype, seq, mode, B):
    params = D.make_params(21)
    kw = {"soft": {}, "fixed": {}, "td3": {"use_bc": False, "slope": 0.01}, "noln": {"layer_norm": False}}[mode]
    e = engine.HirlEngine(batch=B, **kw)
    e.staged = seq == "staged"  # the sharded rank's stages on one rank: hx_hirl_critic_grads[_back], hx_adam, hx_hirl_actor_backward(fwd_done = 2), ...
    e.load_params(params["actor"], params["critic"], params["bc_actor"] if e.use_bc else None)
    if dtype == "bf16":
        e.set_update_dtype("bf16")
        e.set_act_dtype("bf16")
    return e


def weight(mode, k):
    """bc_weight_now of call k.  soft: estimated in the first call (two head jobs), the stored weight after that; fixed: given; TD3: none"""
    if mode == "td3":
        return 0.0
    if mode == "fixed":
        return 0.3
    return 100 if k == 0 else None


def record(e, out, k, mode):
    out[f"losses{k}"] = np.asarray(e.losses_host(), np.float32)
    out[f"wstate{k}"] = bits(e.wstate)
    out[f"grad_actor{k}"] = digest(e.grad_actor)
    out[f"grad_critic{k}"] = digest(e.grad_critic)
    if k % 2 == 0:  # an actor call: the action rows and LayerNorm statistics launch G feeds on
        out[f"outv_api{k}"] = bits(field(e, "API", "outv")[:, :4])
        out[f"st2_api{k}"] = bits(field(e, "API", "st2"))
        if mode in ("soft", "noln") and k == 0:
            out[f"outv_bcs{k}"] = bits(field(e, "BCS", "outv")[:, :4])
            out[f"st2_bcs{k}"] = bits(field(e, "BCS", "st2"))


def finish(e, out):
    for name in NETS:
        out[name] = digest(getattr(e, name))
    out["w2_f32i"] = digest(e.w2_f32i)
    if e.w2_x9 is not None:
        out["w2_x9"] = digest(e.w2_x9)
    if e.images is not None:
        out["images"] = digest(e.images)
    assert e.update_count == 3


def ref_case(engine, tables, dtype, seq, mode, B):
    ring, _, bc = tables
    e = make_engine(engine, dtype, seq, mode, B)
    rng = np.random.default_rng(5)
    out = {}
    for k in range(6):  # calls 0, 2, 4 are actor calls; call 4 also moves the targets
        idx = torch.from_numpy(rng.integers(0, D.N_REPLAY, B).astype(np.int32)).cuda()
        ibc = torch.from_numpy(rng.integers(0, D.N_EXPERT, B).astype(np.int32)).cuda()
        noise = torch.from_numpy(rng.normal(0, 0.2, 4).astype(np.float32)).cuda()
        if e.use_bc:
            e.assemble(ring, idx, bc_table=bc, idx_bc=ibc)
        else:
            e.assemble(ring, idx)
        e.learn(noise=noise, bc_weight_now=weight(mode, k), bc_warm_up_weight=0.05)
        record(e, out, k, mode)
    finish(e, out)
    return out


def front_case(engine, tables, dtype, seq, mode, B):
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv
    from hirl4ucav_amd.utils.buffer import DeviceReplay

    ring, _, bc = tables
    e = make_engine(engine, dtype, seq, mode, B)
    rep = DeviceReplay(4096, ordered_slots=True)  # ring slots in row-tile order: the same inputs fill the ring alike in both processes
    rep.store_rows(ring)
    env = BatchedHarfangEnv(64, scenario="straight_line", seed=5, auto_reset=True, replay=rep)
    env.reset()
    out = {}
    for k in range(6):
        acts = e.step_learn(env, None, bc if e.use_bc else None, act_sigma=0.1, act_seed=3, sample_seed=11, bc_weight_now=weight(mode, k), bc_warm_up_weight=0.05)[0]
        e.front_check()
        out[f"actions{k}"] = bits(acts)
        out[f"idx{k}"] = bits(e._idx)
        record(e, out, k, mode)
    finish(e, out)
    return out


def guard_case(engine, tables):
    """hx_hirl_critic_grads(actor_fwd = 1) alone at B = 48 (three of the sixteen spare workgroup slots are row tiles): a sentinel in everything around what
    the rider may write — columns 4..7 of actor(s)'s action rows, the words behind them (rows beyond the batch would land there), the whole slot of
    bc_actor(s) (no second head job on this call)."""
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents.engine import HxBatch

    ring, _, bc = tables
    B = 48
    e = make_engine(engine, "f32", "one", "fixed", B)
    rng = np.random.default_rng(7)
    idx = torch.from_numpy(rng.integers(0, D.N_REPLAY, B).astype(np.int32)).cuda()
    ibc = torch.from_numpy(rng.integers(0, D.N_EXPERT, B).astype(np.int32)).cuda()
    e.assemble(ring, idx, bc_table=bc, idx_bc=ibc)
    e._noise.copy_(torch.from_numpy(rng.normal(0, 0.2, 4).astype(np.float32)))
    for name in ("st2", "outv"):
        field(e, "API", name).fill_(SENTINEL)
    field(e, "API", "dz2").view(-1)[:2048].fill_(SENTINEL)
    for name, _ in SLOT_FIELDS:
        field(e, "BCS", name).fill_(SENTINEL)
    batch = HxBatch(e.rows.data_ptr(), e.bc_rows.data_ptr(), B, e._noise.data_ptr())
    _lib.call("hx_hirl_critic_grads", ctypes.byref(e.nets), ctypes.byref(batch), ctypes.byref(e.hyper), 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = {"outv": field(e, "API", "outv").cpu().numpy().copy(), "st2": field(e, "API", "st2").cpu().numpy().copy(),
           "behind": field(e, "API", "dz2").view(-1)[:2048].cpu().numpy().copy()}
    o = SLOTS.index("BCS") * PER_ROW * B
    out["bcs"] = e.ws[o:o + PER_ROW * B].cpu().numpy().copy()
    return out


def main():
    from hirl4ucav_amd.agents import engine
    from tests.test_hirl_gpu import device_tables

    outdir, names = sys.argv[1], sys.argv[2:] or CASES + ["guard"]
    tables = device_tables(D.make_data(22, outliers=True))
    for name in names:
        t0 = time.perf_counter()
        if name == "guard":
            out = guard_case(engine, tables)
        else:
            dtype, order, seq, mode, b = name.split("-")
            out = (ref_case if order == "ref" else front_case)(engine, tables, dtype, seq, mode, int(b[1:]))
        np.savez(os.path.join(outdir, name + ".npz"), **out)
        print(f"{name}: {time.perf_counter() - t0:.2f} s", flush=True)
    torch.cuda.synchronize()
    print("head-rider child ok")


if __name__ == "__main__":
    main()
