// hx_act.hip — batched policy inference (gfx950): the whole policy for 16 / 32 observation rows in ONE workgroup, optionally with the
// env step of the same rows in the kernel's tail, and the re-ordered images of W2 it reads.
//   Agent.chooseAction / chooseActionSmallNoise / chooseActionNoNoise   hirl/agents/HIRL.py:192-212   (U5)  -> hx_actor_act
//   chooseAction + HarfangEnv.step                                      hirl/train_all.py:343-345           -> hx_actor_act_step
//   SacAgent.explore / exploit                                          hirl/agents/SAC/agent.py:183-196    -> hx_sac_act, hx_sac_act_step
#include <hip/hip_ext.h>

#include "hx_act_body.h"

using namespace hxnn;
using namespace hxu;
using namespace hxact;

namespace {

// the per-tile acting workgroup lives in hx_act_body.h (hx_front.hip runs it beside learn()'s first launches)
template <int NRT, bool GAUSS, bool ENV, bool BF16, bool RELU, bool F32I = false, bool X3 = false>
__global__ __launch_bounds__(kWide) void act_fused_kernel(ActFusedArgs A) {
    __shared__ ActLds<NRT, ENV, BF16, F32I, X3> SL;
    act_fused_body<NRT, GAUSS, ENV, BF16, RELU, F32I, X3>(A, (int)blockIdx.x, SL);
}

// 16 rows per workgroup fill the chip up to 4,096 rows; from 8,192 rows on 32 rows per workgroup reuse every W2 chunk twice.
// The env tail on wave 0 pays while the launch is ONE round of workgroups (256 CUs x 16 or 32 rows: kFuseEnvMax, hx_act.h); beyond that the
// persistent kernel of hx_actp.hip takes the launch (its env tail runs on all 16 waves, once per workgroup).

// (ENV launches carry HxStepOpts: launch_stamped, hx_act.h)
template <bool GAUSS, bool BF16, bool RELU, bool F32I = false, bool X3 = false>
static void launch_act_t(const ActFusedArgs& H, hipStream_t st) {
    const bool env = H.state != nullptr;
    // 32 rows per workgroup: fp32 MFMA from 8,192 rows on (below that, 16-row workgroups fill the chip and the fp32 MFMA work per workgroup
    // is the longer pole); bf16 and the exact-split format [r5]: as soon as 16-row workgroups would need a second round (4,097 rows: there the launch is
    // bound by every workgroup pulling its images through L2, not by MFMA)
    static const int nrt2_bf16 = getenv("HX_ACT_BF16_NRT2_ROWS") ? atoi(getenv("HX_ACT_BF16_NRT2_ROWS")) : 4097;  // tuning knob; [r5] 4,097 (was 8,192): 5,120 rows 22.6 -> 14.3 us (profiles/r05_act_x9_tiling_time.txt)
    static const int nrt2_f32 = getenv("HX_ACT_F32_NRT2_ROWS") ? atoi(getenv("HX_ACT_F32_NRT2_ROWS")) : 8192;     // tuning knob (tools/ubench/merge_probe.sh)
    // tuning knob; default [r5]: 32-row workgroups as soon as 16-row ones would need a second round (4,097 .. 8,192 rows: 5,120 rows 30.5 -> 19.2 us, 8,192 rows
    // 31.7 -> 21.5 us act + env + insert, tools/ubench/act_x9_tiling_time.py, profiles/r05_act_x9_tiling_time.txt; fp32 MFMA from the fp32 image 35.0 / 27.9);
    // up to 4,096 rows 256 16-row workgroups fill the chip; beyond 8,192 the persistent kernel runs
    static const int nrt2_x9 = getenv("HX_ACT_X9_NRT2_ROWS") ? atoi(getenv("HX_ACT_X9_NRT2_ROWS")) : 4097;
    {
        if (H.rows >= (X3 ? nrt2_x9 : BF16 ? nrt2_bf16 : nrt2_f32)) {
            const dim3 grid((unsigned)((H.rows + 2 * RT - 1) / (2 * RT)));
            if (env) launch_stamped(act_fused_kernel<2, GAUSS, true, BF16, RELU, F32I, X3>, grid, st, H.o, H);
            else launch_stamped(act_fused_kernel<2, GAUSS, false, BF16, RELU, F32I, X3>, grid, st, H.o, H);
            return;
        }
    }
    {
        const dim3 grid((unsigned)((H.rows + RT - 1) / RT));
        if (env) launch_stamped(act_fused_kernel<1, GAUSS, true, BF16, RELU, F32I, X3>, grid, st, H.o, H);
        else launch_stamped(act_fused_kernel<1, GAUSS, false, BF16, RELU, F32I, X3>, grid, st, H.o, H);
    }
}
// HX_ACT_PERSIST=0 keeps act_fused_kernel at every size (A/B timing, bit-identity tests of the two kernels)
static bool persist_enabled() {
    const char* e = getenv("HX_ACT_PERSIST");
    return !(e && e[0] == '0');
}
template <bool GAUSS>
static void launch_act(const ActFusedArgs& H, hipStream_t st) {
    // beyond one round of workgroups: persistent workgroups that fetch W2 once (hx_actp.hip)
    if (H.rows > kFuseEnvMax && persist_enabled() && launch_act_persist(H, GAUSS, st)) return;
    // the activation is a compile-time ReLU when the slope is 0 (HIRL, SAC; the Gaussian policy is a Linear-ReLU stack by definition)
    if (!GAUSS && H.w2b && H.x9) {  // fp32 through the exact bf16 split (deterministic head only)
        if (H.slope == 0.0f) launch_act_t<false, false, true, false, true>(H, st);
        else launch_act_t<false, false, false, false, true>(H, st);
        return;
    }
    if (GAUSS || H.slope == 0.0f) {
        if (H.w2b) launch_act_t<GAUSS, true, true>(H, st);  // bf16 (the Gaussian head: its head in fp32)
        else if (H.w2f) launch_act_t<GAUSS, false, true, true>(H, st);
        else launch_act_t<GAUSS, false, true>(H, st);
    } else {
        if (H.w2b) launch_act_t<false, true, false>(H, st);
        else if (H.w2f) launch_act_t<false, false, false, true>(H, st);
        else launch_act_t<false, false, false>(H, st);
    }
}

// H with its env part.  Up to one round of workgroups the env step rides in wave 0 of each; beyond, the persistent kernel takes the launch (env tail on all
// waves) — and where no persistent instantiation does (no replay ring, HX_ACT_PERSIST=0) two launches: the same rows without the env part, then hx_env_step
template <bool GAUSS>
static int launch_act_step(const ActFusedArgs& H, const HxStepOpts* opts, const char* who, const char* who_act, hipStream_t st) {
    if (H.rows <= kFuseEnvMax) {
        launch_act<GAUSS>(H, st);
    } else if (!(persist_enabled() && launch_act_persist(H, GAUSS, st))) {
        ActFusedArgs A = H;
        A.state = nullptr; A.stride = 0; A.reward = nullptr; A.done = nullptr; A.success = nullptr; A.o = HxStepOpts{}; A.inv_cap = 0.0;
        launch_act<GAUSS>(A, st);
        HX_CHECK_LAUNCH(who_act);
        return hx_env_step(H.state, H.rows, H.stride, H.actions, H.obs, H.reward, H.done, H.success, opts, st);
    }
    HX_CHECK_LAUNCH(who);
    return 0;
}

// bf16 image of a [n] fp32 array (round to nearest even): the policy's W2 for the BF16 acting kernels
__global__ __launch_bounds__(kThreads) void pack_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int n) {
    const int i = (blockIdx.x * kThreads + threadIdx.x) * 2;  // row-major element (column i / 256, k = i % 256); pairs stay adjacent in the image
    if (i + 1 < n) {
        const float2 v = *reinterpret_cast<const float2*>(src + i);
        typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
        const v2bf r = {(__bf16)v.x, (__bf16)v.y};
        *reinterpret_cast<unsigned*>(dst + w2_image_index((uint32_t)i / H1, (uint32_t)i % H1)) = __builtin_bit_cast(unsigned, r);
    }
}

// the TRANSPOSED bf16 image (w2t_image_index): what bwd_l2's dh1 = dz2 W2 reads as its B operand
__global__ __launch_bounds__(kThreads) void pack_bf16_t_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;  // row-major element (row n_ = i / 256, k = i % 256): coalesced reads
    if (i < n) {
        const __bf16 v = (__bf16)src[i];
        dst[w2t_image_index((uint32_t)i % H1, (uint32_t)i / H1)] = __builtin_bit_cast(uint16_t, v);
    }
}

// the hi | mid | lo images of W2 (split3_bf16), each in the bf16 image order
__global__ __launch_bounds__(kThreads) void pack_x9_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int n) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        uint16_t hi, mid, lo;
        split3_bf16(src[i], hi, mid, lo);
        const uint32_t ix = w2_image_index((uint32_t)i / H1, (uint32_t)i % H1);
        dst[ix] = hi; dst[kImgElems + ix] = mid; dst[2 * kImgElems + ix] = lo;
    }
}

__global__ __launch_bounds__(kThreads) void pack_f32i_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = (blockIdx.x * kThreads + threadIdx.x) * 4;  // four consecutive k of one column: adjacent in the image too
    if (i < n) *reinterpret_cast<float4*>(dst + w2f_image_index((uint32_t)i / H1, (uint32_t)i % H1)) = *reinterpret_cast<const float4*>(src + i);
}

}  // namespace

namespace hxu {
void launch_pack_bf16(const float* w2, uint16_t* image, bool transposed, hipStream_t st) {
    const int n = H2 * H1;
    if (transposed) hipLaunchKernelGGL(pack_bf16_t_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, w2, image, n);
    else hipLaunchKernelGGL(pack_bf16_kernel, dim3((n / 2 + kThreads - 1) / kThreads), dim3(kThreads), 0, st, w2, image, n);
}
}  // namespace hxu

extern "C" {

/* The four acting entry points take the three images of W2 as nullable pointers (include/hirl4ucav.h "W2 IMAGES"): act_args (hx_act.h) picks the one format. */

/* chooseAction / chooseActionSmallNoise / chooseActionNoNoise for `rows` observations (HIRL.py:192-212):
 * actions = clamp(actor(obs) + noise, -1, 1).  noise_mode 0: none, 1: noise[4] shared by all rows, 2: noise[rows][4],
 * 3: N(0, sigma^2) per row and component from Philox(seed; row0 + row, call); + 16: layerNorm = False. */
int hx_actor_act(const float* actor, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, const float* obs, int64_t rows, float* actions,
                 int32_t noise_mode, const float* noise, float sigma, uint64_t seed, uint32_t row0, uint32_t call, float slope, void* stream) {
    HX_REQUIRE(actor && obs && actions && rows > 0, "hx_actor_act: bad arguments");
    if (int rc = check_noise_mode(noise_mode, noise, "hx_actor_act")) return rc;
    const ActImages im{w2_f32i, w2_x9, w2_bf16};
    if (int rc = check_act_images(im, noise_mode, "hx_actor_act")) return rc;
    launch_act<false>(act_args_det(actor, const_cast<float*>(obs), rows, actions, noise_mode, noise, sigma, seed, row0, call, slope, im), (hipStream_t)stream);
    HX_CHECK_LAUNCH("hx_actor_act");
    return 0;
}
/* chooseAction + HarfangEnv.step for n envs in ONE launch (train_all.py:343-345): actions = clamp(actor(obs_io) + noise, -1, 1) as
 * hx_actor_act, then hx_env_step with those actions in the tail of the same kernel — obs_io in: current observation, out: next. */
int hx_actor_act_step(const float* actor, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, float* state, int64_t n, int64_t stride,
                      float* obs_io, float* actions, int32_t noise_mode, const float* noise, float sigma, uint64_t seed, uint32_t row0, uint32_t call,
                      float slope, float* reward, uint8_t* done, int8_t* success, const HxStepOpts* opts, void* stream) {
    HX_REQUIRE(actor, "hx_actor_act_step: null actor");
    if (int rc = check_noise_mode(noise_mode, noise, "hx_actor_act_step")) return rc;
    const ActImages im{w2_f32i, w2_x9, w2_bf16};
    if (int rc = check_act_images(im, noise_mode, "hx_actor_act_step")) return rc;
    const ActEnv E{state, stride, reward, done, success, opts ? *opts : HxStepOpts{}};
    if (int rc = check_step_args(obs_io, n, actions, E, "hx_actor_act_step")) return rc;
    return launch_act_step<false>(act_args_det(actor, obs_io, n, actions, noise_mode, noise, sigma, seed, row0, call, slope, im, &E), opts, "hx_actor_act_step",
                                  "hx_actor_act", (hipStream_t)stream);
}

/* bf16 image (round to nearest even) of an MLP block's W2 [512][256]; in_dim = 13 (actor / policy) or 17 (Q head) locates it. */
int hx_pack_w2_bf16(const float* net, int32_t in_dim, uint16_t* w2_bf16, void* stream) {
    HX_REQUIRE(net && w2_bf16 && (in_dim == 13 || in_dim == 17), "hx_pack_w2_bf16: bad arguments");
    const Mlp m{in_dim, 1, 0};
    const int n = H2 * H1;
    hipLaunchKernelGGL(pack_bf16_kernel, dim3((n / 2 + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, net + m.W2(), w2_bf16, n);
    HX_CHECK_LAUNCH("hx_pack_w2_bf16");
    return 0;
}
/* The hi | mid | lo images of the exact three-way bf16 split of W2 (see the header; hx_act.h HX_X9_TERMS). */
int hx_pack_w2_x9(const float* net, int32_t in_dim, uint16_t* w2_x9, void* stream) {
    HX_REQUIRE(net && (in_dim == 13 || in_dim == 17), "hx_pack_w2_x9: bad arguments");
    if (int rc = check_images16("hx_pack_w2_x9", "bad arguments", {w2_x9})) return rc;
    const Mlp m{in_dim, 1, 0};
    const int n = H2 * H1;
    hipLaunchKernelGGL(pack_x9_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, net + m.W2(), w2_x9, n);
    HX_CHECK_LAUNCH("hx_pack_w2_x9");
    return 0;
}
/* The re-ordered fp32 image of W2: acting from it is bit-identical to acting from W2 itself. */
int hx_pack_w2_f32i(const float* net, int32_t in_dim, float* w2_f32i, void* stream) {
    HX_REQUIRE(net && (in_dim == 13 || in_dim == 17), "hx_pack_w2_f32i: bad arguments");
    if (int rc = check_images16("hx_pack_w2_f32i", "bad arguments", {w2_f32i})) return rc;
    const Mlp m{in_dim, 1, 0};
    const int n = H2 * H1;
    hipLaunchKernelGGL(pack_f32i_kernel, dim3((n / 4 + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, net + m.W2(), w2_f32i, n);
    HX_CHECK_LAUNCH("hx_pack_w2_f32i");
    return 0;
}

// The Gaussian head's images.  im.w2x: the exact split exists for the Gaussian head in the persistent kernel only — up to 8,192 rows (or with HX_ACT_PERSIST=0)
// im.w2f serves, so a caller that offers the split (and no bf16 image, which would be chosen before either) must offer the fp32 image with it.
static int sac_images(ActImages& im, int64_t rows, const char* who) {
    if (int rc = check_act_images(im, 0, who)) return rc;
    HX_REQUIRE(im.w2b || !im.w2x || im.w2f, "%s: w2_x9 needs w2_f32i beside it (the exact split acts beyond 8,192 rows only; up to there the fp32 image does)", who);
    if (!(rows > kFuseEnvMax && persist_enabled())) im.w2x = nullptr;
    return 0;
}
/* SacAgent.explore / exploit (SAC/agent.py:183-196) for `rows` observations.  mode 0: exploit = tanh(mean); 1: sample with the
 * standard-normal draws eps[rows][4]; 2: sample with Philox(seed; row0 + row, call).  With w2_bf16: the 256 -> 512 product from the bf16 image, layer 1
 * and the head in fp32 (include/hirl4ucav.h "SAC bf16 path"); up to 8,192 rows the per-tile kernel, beyond that the streaming persistent kernel
 * (MODE 2): the same bits for a row either way. */
int hx_sac_act(const float* policy, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, const float* obs, int64_t rows, float* actions,
               int32_t mode, const float* eps, uint64_t seed, uint32_t row0, uint32_t call, void* stream) {
    HX_REQUIRE(policy && obs && actions && rows > 0 && mode >= 0 && mode <= 2 && (mode != 1 || eps), "hx_sac_act: bad arguments");
    ActImages im{w2_f32i, w2_x9, w2_bf16};
    if (int rc = sac_images(im, rows, "hx_sac_act")) return rc;
    launch_act<true>(act_args_gauss(policy, const_cast<float*>(obs), rows, actions, mode, eps, seed, row0, call, im), (hipStream_t)stream);
    HX_CHECK_LAUNCH("hx_sac_act");
    return 0;
}
/* SacAgent.explore / exploit + HarfangEnv.step in one launch (train_sac.py:238-241): hx_sac_act, then hx_env_step in the kernel's tail. */
int hx_sac_act_step(const float* policy, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, float* state, int64_t n, int64_t stride,
                    float* obs_io, float* actions, int32_t mode, const float* eps, uint64_t seed, uint32_t row0, uint32_t call, float* reward, uint8_t* done,
                    int8_t* success, const HxStepOpts* opts, void* stream) {
    HX_REQUIRE(policy && mode >= 0 && mode <= 2 && (mode != 1 || eps), "hx_sac_act_step: bad arguments");
    const ActEnv E{state, stride, reward, done, success, opts ? *opts : HxStepOpts{}};
    if (int rc = check_step_args(obs_io, n, actions, E, "hx_sac_act_step")) return rc;
    ActImages im{w2_f32i, w2_x9, w2_bf16};
    if (int rc = sac_images(im, n, "hx_sac_act_step")) return rc;
    return launch_act_step<true>(act_args_gauss(policy, obs_io, n, actions, mode, eps, seed, row0, call, im, &E), opts, "hx_sac_act_step", "hx_sac_act",
                                 (hipStream_t)stream);
}

}  // extern "C"

HX_DEFINE_DEBUG_COLLECTORS(act, 56, 80)
