"""The four acting entry points (hx_actor_act, hx_actor_act_step, hx_sac_act, hx_sac_act_step) and the W2 images they are offered, through the C ABI:
ONE format per launch — the bf16 image, else the exact split, else the fp32 image, else W2 itself (include/hirl4ucav.h "W2 IMAGES") — so offering
more images than the chosen one changes no bit, and what the entry points refuse about their images comes back as HX_ERR_ARG.

Sizes: 37 rows (two 16-row tiles and a tail of 5) and 8,213 (past the 8,192-row switch into the persistent kernel, ragged tail).  Every comparison
is torch.equal.  The act_step cases use envs without a replay ring (ring slots are handed out by an atomic)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _hirl_data as D  # noqa: E402

SIZES = (37, 8213)


@pytest.fixture(scope="module")
def nets():
    """head -> (flat network, (w2_f32i, w2_x9, w2_bf16) image tensors packed from it)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hirl4ucav_amd import _lib
    from hirl4ucav_amd.agents import engine as E
    from hirl4ucav_amd.agents import sac_engine as SE
    from tests.test_oracle_sac import sac_params

    h = E.HirlEngine(batch=128)
    p = D.make_params(D.PARAM_SEED)
    h.load_params(p["actor"], p["critic"], p["bc_actor"])
    s = SE.SacEngine(batch=16)
    p = sac_params()
    s.load_params(p["policy"], p["q1"], p["q2"])
    out = {}
    for head, net in (("actor", h.actor), ("sac", s.policy)):
        f32i = torch.zeros(512 * 256, dtype=torch.float32, device="cuda")
        x9 = torch.zeros(3 * 512 * 256, dtype=torch.bfloat16, device="cuda")
        bf16 = torch.zeros(512 * 256, dtype=torch.bfloat16, device="cuda")
        _lib.call("hx_pack_w2_f32i", net.data_ptr(), 13, f32i.data_ptr(), _lib.stream_ptr())
        _lib.call("hx_pack_w2_x9", net.data_ptr(), 13, x9.data_ptr(), _lib.stream_ptr())
        _lib.call("hx_pack_w2_bf16", net.data_ptr(), 13, bf16.data_ptr(), _lib.stream_ptr())
        out[head] = (net, (f32i, x9, bf16))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def envs():
    """n -> (env without a replay ring, its state and observations after reset): every act_step case starts from the same envs"""
    from hirl4ucav_amd.environments.batched import BatchedHarfangEnv

    out = {}
    for n in SIZES:
        env = BatchedHarfangEnv(n, scenario="serpentine", seed=3, auto_reset=False, collect_stats=False)
        env.reset()
        out[n] = (env, env._state_store.clone(), env.obs.clone())
    return out


def pointers(images, offered):
    """the three image arguments: slot k of `offered` true -> the image's pointer (+ offered[k] bytes when it is an int beyond 1), else NULL"""
    return [None if not o else t.data_ptr() + (o if o > 1 else 0) for t, o in zip(images, offered)]


def act_args(head, n):
    """the arguments between `actions` and `stream`: Philox exploration noise with a fixed seed and call"""
    return (3, None, 0.1, 11, 0, 5, 0.0) if head == "actor" else (2, None, 11, 0, 5)


def run(head, nets, offered, n, envs=None):
    """one launch of hx_<head>_act (envs None) or hx_<head>_act_step with the offered images -> every tensor it wrote"""
    from hirl4ucav_amd import _lib

    net, images = nets[head]
    name = "hx_actor_act" if head == "actor" else "hx_sac_act"
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    if envs is None:
        obs = torch.from_numpy(np.random.default_rng(n).uniform(-1, 1, (n, 13)).astype(np.float32)).cuda()
        _lib.call(name, net.data_ptr(), *pointers(images, offered), obs.data_ptr(), n, out.data_ptr(), *act_args(head, n), _lib.stream_ptr())
        return (out,)
    env, state0, obs0 = envs[n]
    env._state_store.copy_(state0)
    env.obs.copy_(obs0)
    a = act_args(head, n)
    _lib.call(name + "_step", net.data_ptr(), *pointers(images, offered), env.state.data_ptr(), n, env.pitch, env.obs.data_ptr(), out.data_ptr(), *a,
              env.reward.data_ptr(), env.done.data_ptr(), env.success.data_ptr(), ctypes.byref(env._opts), _lib.stream_ptr())
    return out, env.obs.clone(), env.reward.clone(), env.done.clone(), env.success.clone(), env._state_store.clone()


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("step", [False, True], ids=["act", "act_step"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("head", ["actor", "sac"])
def test_offering_more_images_than_the_chosen_one_changes_no_bit(nets, envs, head, n, step):
    """(w2_f32i, w2_x9, w2_bf16): all three == bf16 alone; f32i + x9 == x9 alone (deterministic head; the Gaussian head refuses x9 alone) and, for the
    Gaussian head at 37 rows, == f32i alone (the split acts beyond 8,192 rows only); no image == f32i alone (the fp32 image is W2 re-ordered)."""
    r = lambda *offered: run(head, nets, offered, n, envs if step else None)
    bf16, f32i = r(0, 0, 1), r(1, 0, 0)
    assert same(r(1, 1, 1), bf16)
    assert same(r(0, 0, 0), f32i)
    both = r(1, 1, 0)
    if head == "actor":
        x9 = r(0, 1, 0)
        assert same(both, x9)
        assert n == 37 or not same(x9, f32i)  # (another summation order: over 8,213 rows some bit differs, so the comparison above compares something)
    elif n == 37:
        assert same(both, f32i)
    else:
        assert not same(both, f32i)
    assert not same(bf16, f32i)
    assert all(torch.isfinite(t.float()).all() for t in bf16 + f32i + both)


@pytest.mark.parametrize("step", [False, True], ids=["act", "act_step"])
@pytest.mark.parametrize("head", ["actor", "sac"])
def test_what_the_entry_points_refuse_about_their_images(nets, envs, head, step):
    """a pointer off by 4 bytes in each slot (alone and beside the images that would be chosen before it), and for the Gaussian head w2_x9 without
    w2_f32i: HX_ERR_ARG, naming the entry point, and nothing is launched (the envs of a refused act_step stay as they were)"""
    from hirl4ucav_amd import _lib

    name = ("hx_actor_act" if head == "actor" else "hx_sac_act") + ("_step" if step else "")
    n = 37
    cases = [(4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 1, 1), (1, 4, 1), (1, 1, 4)]
    if head == "sac":
        cases.append((0, 1, 0))
    for offered in cases:
        with pytest.raises(_lib.HxError) as err:
            run(head, nets, offered, n, envs if step else None)
        assert f"{name} failed ({_lib.DEFINES['HX_ERR_ARG']}): {name}: " in str(err.value), (offered, str(err.value))
    if head == "actor" and not step:  # + 32 is hx_hirl_front's way of asking for the exact split: refused where the split is the chosen format
        net, images = nets[head]
        obs = torch.zeros((n, 13), dtype=torch.float32, device="cuda")
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        with pytest.raises(_lib.HxError) as err:
            _lib.call(name, net.data_ptr(), *pointers(images, (1, 1, 0)), obs.data_ptr(), n, out.data_ptr(), 3 | 32, None, 0.1, 11, 0, 5, 0.0, _lib.stream_ptr())
        assert f"{name} failed ({_lib.DEFINES['HX_ERR_ARG']}): {name}: " in str(err.value)
    if step:
        env, state0, obs0 = envs[n]
        assert torch.equal(env._state_store, state0) and torch.equal(env.obs, obs0)
