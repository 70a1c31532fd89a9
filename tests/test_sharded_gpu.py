"""The exchange step of the PRODUCT engine with 2, 3 and 8 ranks on a GPU box (gloo for the RCCL-shaped path, hipIpc mappings for the peer-read
kernels; all ranks share the one GPU): one message per phase, replicas bit-identical, and the result equal to ONE engine updating the
global batch (128 x world rows = the shards' minibatches) — SURVEY.md 8e "grad of global batch = mean of shard grads".  World 8 is the form
BASELINE.json configs[3] / configs[4] run in (kMaxWorld flag / red arrays, seven peer mappings per rank, the 8-way slices of hx_allreduce_twostage);
world 3 is the odd one (slices that do not divide the message).  The reference is one process (hirl/agents/HIRL.py:52)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _hirl_data as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def single_engine_reference(world=2):
    """6 learn() calls of ONE engine with batch 128 x world: rows = rank 0's 128 ++ rank 1's 128 ++ ... of tests/_sharded_check.py"""
    from hirl4ucav_amd.agents import engine as E

    params, data = D.make_params(31), D.make_data(32)
    ring = torch.from_numpy(data["replay"]).cuda().contiguous()
    bc = np.zeros((D.N_EXPERT, 32), np.float32)
    bc[:, 0:13], bc[:, 13:17] = data["expert_s"], data["expert_a"]
    bc = torch.from_numpy(bc).cuda()
    e = E.HirlEngine(batch=128 * world)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    rng = np.random.default_rng(7)
    for k in range(6):
        idx, ibc = rng.integers(0, D.N_REPLAY, (world, 128)).astype(np.int32), rng.integers(0, D.N_EXPERT, (world, 128)).astype(np.int32)
        noise = rng.normal(0, 0.2, 4).astype(np.float32)
        e.assemble(ring, torch.from_numpy(idx.reshape(-1)).cuda(), bc_table=bc, idx_bc=torch.from_numpy(ibc.reshape(-1)).cuda())
        e.learn(noise=torch.from_numpy(noise).cuda(), bc_weight_now=100 if k % 4 == 0 else None, bc_warm_up_weight=0.05)
    torch.cuda.synchronize()
    return {k: getattr(e, k).cpu().numpy() for k in ("actor", "critic", "target_actor", "target_critic")}, np.asarray(e.losses_host())


CASES = [(2, x) for x in ("rccl", "oneshot", "twostage", "twostage-bf16")] + [(3, "oneshot"), (3, "twostage")] + \
        [(8, x) for x in ("rccl", "oneshot", "twostage", "twostage-bf16")]


_RAN = {}  # world -> (directory, stdout, stderr, returncode): ONE launch per world size runs every exchange of that size


def sharded_run(world, tmp_path_factory):
    if world not in _RAN:
        out = str(tmp_path_factory.mktemp(f"sharded{world}") / "sharded")
        names = ",".join(x for w, x in CASES if w == world)
        port = str(29800 + os.getpid() % 150 + world)
        p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                            "--master-port", port, os.path.join(ROOT, "tests", "_sharded_check.py"), names], cwd=ROOT,
                           env={**os.environ, "SHARDED_OUT": out, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=900)
        _RAN[world] = (out, p.stdout, p.stderr, p.returncode)
    return _RAN[world]


@pytest.mark.parametrize("world,exchange", CASES)
def test_sharded_update_equals_the_global_batch_update(world, exchange, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out, stdout, stderr, rc = sharded_run(world, tmp_path_factory)
    done = [ln.split()[1] for ln in stdout.splitlines() if ln.split()[:1] == ["SHARDED_OK"] and len(ln.split()) == 2]  # whole lines, the token after SHARDED_OK
    assert exchange in done, (rc, done, stdout[-1500:], stderr[-3000:])
    if (world, exchange) == [c for c in CASES if c[0] == world][-1]:  # the last case of this launch answers for its return code (e.close(), the group's end)
        assert rc == 0, (rc, stdout[-1500:], stderr[-3000:])
    out = out + "." + exchange + ".npz"
    got = np.load(out)
    assert int(got["world"]) == world
    ref, ref_losses = single_engine_reference(world)
    # same global batch, different summation tree (`world` shard sums added vs one reduction over all rows) and, in the sharded run, the two actor
    # losses combined AFTER the exchange: fp32 rounding only.  Adam turns a rounding-level gradient difference on a near-zero entry
    # into up to 2 lr of parameter difference, so: 99.9 % of the entries within 2e-5, none beyond 6 x 2 lr.
    # twostage-bf16: the SUMMED gradient is rounded to bf16 before Adam (2^-9 relative per entry) — replicas stay bit-identical (asserted in
    # the ranks), the parameters follow the fp32 run to Adam's resolution of such a perturbation: 99 % within 2e-4
    frac, tol = (0.99, 2e-4) if exchange == "twostage-bf16" else (0.999, 2e-5)
    for k in ("actor", "critic", "target_actor", "target_critic"):
        d = np.abs(got[k] - ref[k])
        assert (d <= tol).mean() >= frac and d.max() <= 1.2e-2, (k, (d <= tol).mean(), d.max())
    # (rank 0's logged loss values are its own shard's means; only the weight is a global quantity)
    assert abs(got["losses"][5] - ref_losses[5]) < 1e-6  # the BC weight comes from the GLOBAL soft count: equal to the single engine's


def test_oneshot_exchange_fails_stop():
    """A peer that never arrives: the waiting rank's status word becomes 1 within the timeout and STAYS set, dst is untouched, its own flag
    carries the poison value, every later exchange returns at once, the optimizer steps guarded by the word change nothing — and a rank
    that polls the poisoned flag fails too (status 2) instead of waiting or summing (hx_xchg.hip "fail-stop")."""
    import ctypes
    import time

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents import engine as E

    _lib.load()
    vp = ctypes.c_void_p
    n = 1024

    def words(ptr, k):
        return torch.as_tensor(E._DeviceWords(ptr, k), device="cuda").view(torch.int32)

    flag_mem, stat_mem = vp(), vp()
    _lib.call("hx_ipc_alloc", 256, 1, ctypes.byref(flag_mem))  # word 0: rank 0's flag, word 16: rank 1's flag
    _lib.call("hx_ipc_alloc", 256, 1, ctypes.byref(stat_mem))  # word 0: rank 0's status, word 16: rank 1's
    msg = torch.ones(2 * n, dtype=torch.float32, device="cuda")
    dst = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    bufs = (vp * 2)(msg.data_ptr(), msg.data_ptr() + 4 * n)
    flags = (vp * 2)(flag_mem.value, flag_mem.value + 64)
    # rank 0 waits for rank 1, which never announces
    t0 = time.perf_counter()
    _lib.call("hx_allreduce_oneshot", dst.data_ptr(), bufs, flags, stat_mem.value, 2, 0, n, 1, 200, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert 0.15 < time.perf_counter() - t0 < 5.0  # bounded by the device clock, not by a spin count
    assert int(words(stat_mem.value, 1)[0]) == 1 and torch.all(dst == -7.0)
    assert int(words(flag_mem.value, 1)[0]) == -1  # 0xFFFFFFFF: poison
    # sticky: the next exchange returns at once and leaves dst alone, whatever the peer does meanwhile
    words(flag_mem.value + 64, 1)[0] = 2
    t0 = time.perf_counter()
    _lib.call("hx_allreduce_oneshot", dst.data_ptr(), bufs, flags, stat_mem.value, 2, 0, n, 2, 200, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 0.1 and int(words(stat_mem.value, 1)[0]) == 1 and torch.all(dst == -7.0)
    # global: rank 1 polls rank 0's poisoned flag and fails with status 2
    dst1 = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    _lib.call("hx_allreduce_oneshot", dst1.data_ptr(), bufs, flags, stat_mem.value + 64, 2, 1, n, 2, 200, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(words(stat_mem.value + 64, 1)[0]) == 2 and torch.all(dst1 == -7.0)
    # the optimizer step guarded by the status word changes nothing
    params = D.make_params(3)
    e = E.HirlEngine(batch=128)
    e.load_params(params["actor"], params["critic"], params["bc_actor"])
    e.grad_critic.fill_(1.0)
    before = e.critic.clone()
    e.nets.xchg_status = stat_mem.value
    _lib.call("hx_adam", ctypes.byref(e.nets), ctypes.byref(e.hyper), 0, 1, 1.0, 0, 0.0, 0.0, 128, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(e.critic, before) and float(e.m_critic.abs().sum()) == 0.0
    words(stat_mem.value, 1)[0] = 0  # (and with the word cleared the same call steps)
    _lib.call("hx_adam", ctypes.byref(e.nets), ctypes.byref(e.hyper), 0, 1, 1.0, 0, 0.0, 0.0, 128, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.equal(e.critic, before)
    e.nets.xchg_status = None
    for m in (flag_mem, stat_mem):
        _lib.call("hx_ipc_free", m)
