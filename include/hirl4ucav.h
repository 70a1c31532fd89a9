/*
 * hirl4ucav.h — C ABI of the MI355X-native hot path of HIRL4UCAV (libhx_mi355.so).
 *
 * The reference (zrc0622/HIRL4UCAV) is pure Python and has no FFI; its "operator interface" for this path is
 * the duck-typed env / agent API.  The Python mirror of that API lives in hirl4ucav_amd/ and
 * calls ONLY the functions below (ctypes).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Every pointer is DEVICE memory owned by the caller unless it says
 *     "host".  The library never allocates caller-visible memory and never synchronises: all work is enqueued
 *     on `stream` (a hipStream_t passed as void*; NULL = the default stream).
 *   - return value: 0 = ok, negative = error (HX_ERR_*); hx_last_error() returns a thread-local message.
 *   - thread-compatible: no global mutable state besides the thread-local error string.
 *
 * Env state layout (struct-of-arrays, fp32 words): word w of env i is state[w * stride + i], stride >= n.
 * HX_ENV_WORDS = 37 words = 148 B per env (SURVEY.md 8d canonical state):
 *     0..2  ally position (x, y = altitude, z)      13..15 opponent position
 *     3..5  ally velocity                           16..18 opponent velocity
 *     6..9  ally attitude quaternion (w, x, y, z)   19..22 opponent quaternion
 *    10..12 ally control levels (pitch, roll, yaw)  23..25 opponent control levels
 *    26..28 missile position   29..31 missile velocity
 *    32 opponent health   33 lock timer [s]   34 missile age [s]
 *    35 flags (u32 bit-cast)   36 counters (u32: lo16 episode step, hi16 opponent-script step)
 */
#ifndef HIRL4UCAV_H
#define HIRL4UCAV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HX_ENV_WORDS 37
#define HX_OBS_DIM 13
#define HX_ACT_DIM 4
#define HX_ROW_WORDS 32 /* replay row: s[13] a[4] s'[13] r done */

/* flags word (state word 35) */
#define HX_F_LOCKED_PREV (1u << 0)     /* Ally_target_locked   HarfangEnv_GYM.py:227 */
#define HX_F_LOCKED (1u << 1)          /* n_Ally_target_locked HarfangEnv_GYM.py:228 */
#define HX_F_SLOT_PREV (1u << 2)       /* missile1_state       HarfangEnv_GYM.py:250 */
#define HX_F_SLOT (1u << 3)            /* n_missile1_state     HarfangEnv_GYM.py:251 */
#define HX_F_FIRED (1u << 4)           /* now_missile_state    HarfangEnv_GYM.py:150-156 */
#define HX_F_FIRE_SUCCESS (1u << 5)    /* fire_success         HarfangEnv_GYM.py:129 */
#define HX_F_EPISODE_SUCCESS (1u << 6) /* episode_success      HarfangEnv_GYM.py:167 */
#define HX_F_DONE (1u << 7)            /* done                 HarfangEnv_GYM.py:163-166 */
#define HX_F_SCEN_SHIFT 8              /* bits 8..9: 0 straight_line, 1 serpentine, 2 circular */
#define HX_F_SERP_POS (1u << 10)
#define HX_F_SERP_LONG (1u << 11)
#define HX_F_M_ACTIVE (1u << 12)
#define HX_F_M_GUIDED (1u << 13)
#define HX_F_SIM_SLOT (1u << 14)

#define HX_ERR_ARG (-1)
#define HX_ERR_HIP (-2)

/* stats[] slots accumulated by hx_env_step (uint64 each) */
enum { HX_STAT_EPISODES = 0, HX_STAT_KILLS, HX_STAT_FIRE_SUCCESS_EPISODES, HX_STAT_TIME_LIMIT, HX_STAT_FIRES,
       HX_STAT_GOOD_FIRES, HX_STAT_LOCKED_STEPS, HX_STAT_ENV_STEPS,
       HX_STAT_NONFINITE_ACTIONS, /* env steps whose action held a NaN / Inf component: the component is taken as 0 (and stored as 0 in the
                                     replay row), so a diverged policy cannot poison the simulator state — the stand-in for the reference's
                                     missing failure detection */
       HX_STAT_COUNT };
/* The counters are kept HX_STAT_WAYS times: workgroup b adds to way b % HX_STAT_WAYS, each way in its own 128-byte line
 * (stats[way * HX_STAT_PITCH + k]); a statistic is the SUM over the ways.  One set of counters put every workgroup's atomics of a launch
 * on one cache line — one memory channel, ~12 ns each: 0.75 us of a 65,536-env launch. */
#define HX_STAT_WAYS 32
#define HX_STAT_PITCH 16

const char* hx_last_error(void);
/* HX_ABI_VERSION of the library that is loaded.  The structs below are part of the ABI: a caller built against another header version must
 * not call in (round 3 widened HxStepOpts.stats from 9 to HX_STAT_WAYS * HX_STAT_PITCH words and appended fields to HxNets / HxHyper without
 * bumping this: a 9-word stats buffer then took atomics up to word 504).  110: round 4 (hx_abi_sizes, hx_rccl_*, hx_allreduce_twostage).
 * 113: round 5.  114: round 6 (hx_rccl_allreduce_bf16).  115: the SAC bf16 path (HxSacNets.w2_bf16_all / policy_w2_bf16, hx_sac_*_bf16).
 * 116: SAC's imitative branch (HxSacImit, hx_sac_imit_*, hx_sac_policy_grads_imitative, hx_sac_learn_imitative).
 * 117: hx_sac_front takes any number of envs (the per-tile acting role up to 8,192; it refused them before).
 * 118: prioritized replay for SAC (HxPer, hx_per_*, hx_sac_learn_weighted).
 * 119: gradient-norm clipping and the fixed entropy coefficient for SAC (HX_SAC_FIXED_ALPHA, hx_sac_grad_norm, hx_sac_adam_clipped,
 * hx_sac_learn_weighted_clipped).
 * 120: priorities at insert for SAC's prioritized replay (hx_per_score_workspace_floats, hx_per_score_new).
 * 121: n-step returns for SAC (HxNStep, hx_nstep_*).
 * 122: the record of validation episodes (HxTrace, hx_trace_*).
 * 123: per-episode statistics by scenario (HxEpStat, hx_epstat_*).
 * 124: the merged actor message carries the soft count as base-32 digit words too, and hx_adam_mixed reads those (exact on the bf16 transports).
 * 125: success upsampling of the replay draw and the BC minibatch's fire row (HxUps, hx_ups_*).
 * 126: the pursuit pilot as a kernel and the online region of the BC table (hx_pilot_act, hx_pilot_refresh).
 * 127: four acting entry points instead of sixteen: hx_actor_act, hx_actor_act_step, hx_sac_act and hx_sac_act_step take the W2 images as three nullable
 * pointers (w2_f32i, w2_x9, w2_bf16) after the network; their _f32i / _x9 / _bf16 variants, the `ws` argument and hx_act_workspace_floats are gone.
 * 128: expert branches: one pilot step per pick fills the online region of the labelled expert ring (hx_pilot_branch).
 * 129: expert branches of up to H steps: resident branches in a device workspace, one step per call (hx_pilot_branch_steps,
 * hx_branch_workspace_bytes).
 * 130: gradient-norm clipping for HIRL and TD3 (hx_hirl_clip_floats, hx_hirl_clip_shape, hx_hirl_grad_norm, hx_adam_clipped).
 * 131: prioritized replay for HIRL and TD3: the weighted TD head (hx_hirl_critic_grads_weighted).
 * 132: n-step returns for HIRL and TD3: n-step relabelling of a labelled expert table (hx_nstep_label).
 * 133: self-imitation: the learner's own kill episodes join the online region of the labelled expert ring (hx_self_*).
 * 134: correlated exploration noise: a bank of AR(1) processes per env and action component (hx_noise_*). */
#define HX_ABI_VERSION 134
int hx_version(void);
/* sizes[0..7] (host) <- sizeof HxStepOpts, HxNets, HxHyper, HxBatch, HxSample, HxSacNets, HxSacBatch, and the words of a statistics buffer
 * (HX_STAT_WAYS * HX_STAT_PITCH): a binding checks these against its own declarations at load time (hirl4ucav_amd/_lib.py does). */
int hx_abi_sizes(int32_t* sizes8);
/* Kernel-duration events for HxStepOpts.ev_start / ev_stop (bench.py's live roofline measurement). */
void* hx_event_create(void);
int hx_event_destroy(void* ev);
int hx_event_elapsed_us(void* start, void* stop, float* us /* host */);

/* Optional per-call behaviour of hx_env_step.  All pointers device memory (or NULL = feature off). */
typedef struct HxStepOpts {
    int32_t max_step;      /* > 0: episode time limit (train_all.py:159-183 maxStep); the step that reaches it is
                              executed, NOT stored, and ends the episode without done (train_all.py:346-347) */
    int32_t auto_reset;    /* 1: an env whose episode ended (done or time limit) is reset in place and obs_io gets
                              the reset observation (vectorised counterpart of train_all.py:320-323) */
    int32_t randomize;     /* resets use random_reset (HarfangEnv_GYM.py:51-81) instead of reset (:34-49) */
    uint32_t env_id0;      /* global id of env 0 of this shard (Philox counter word 0 = env_id0 + i) */
    uint64_t seed;         /* Philox key */
    uint32_t* episode_ctr; /* [n] per-env episode counter (Philox counter word 1); required if auto_reset */
    float* ring;           /* [cap][HX_ROW_WORDS] replay ring or NULL: fused UniformMemory.store (buffer.py:20-36) */
    int8_t* ring_success;  /* [cap] step_success of each stored row, or NULL */
    int64_t cap;
    uint64_t* total;       /* transitions ever stored; slot = total % cap (buffer.py:36 position).  A 64-bit counter in every consumer (the
                              inserts, the draws, PER's `marked`, the host): the documented domain is total < 2^52 — the inserts take total % cap
                              from an fp64 quotient estimate with one correction step —, tested up to there (tests/test_ring_counter_*.py) */
    uint64_t* stats;       /* [HX_STAT_WAYS][HX_STAT_PITCH] or NULL: see HX_STAT_WAYS */
    void* ev_start;        /* measurement only (host handles from hx_event_create, or NULL): the launch stamps the kernel's own */
    void* ev_stop;         /* begin / end into them — the duration rocprofv3 reports, without the dispatch gap around it */
    int32_t layout;        /* 0: the library picks the launch shape from n.  HX_LAYOUT(pair, envs_per_block) forces one (tuning,
                              tests): pair = 1 steps each env on two adjacent lanes (ally + shared | opponent), 0 on one lane;
                              envs_per_block in {32, 64, 128, 256, 512} (pair) / {64, 128, 256} (solo).  Same results bit for bit. */
} HxStepOpts;
#define HX_LAYOUT(pair, envs_per_block) ((((pair) ? 1 : 0) << 8) | ((envs_per_block) / 4))
/* Opt-in, OR-ed into HxStepOpts.layout: `total` is the first of 3 + cap / 16 words (total, launch sequence, status, one word per row tile) and the
 * PER-TILE acting launches that step the envs (hx_actor_act_step / hx_sac_act_step up to one round of acting workgroups, the front launch's acting
 * workgroups) hand out ring slots in row-tile order instead of in the order their workgroups reach the counter: the same inputs fill the ring in
 * the same order.  Each tile waits in-launch for the lower tiles' counts; a wait that gives up sets bit 0 of the status word (sticky) and its slots
 * may collide.  The persistent acting kernels and hx_env_step keep one atomic per workgroup.  Without the flag (raw callers with a one-word
 * `total`) every launch does. */
#define HX_LAYOUT_ORDERED_SLOTS (1 << 16)

/* HarfangEnv.reset / random_reset (+ Serpentine/Circular variants): HarfangEnv_GYM.py:34-81,171-188,374-406,440-474.
 * mask: NULL = all envs, else only envs with mask[i] != 0.  scenario: per-env ids (NULL = scenario_all for all).
 * Writes the reset observation to obs[i*13..] (obs may be NULL). */
int hx_env_reset(float* state, int64_t n, int64_t stride, const uint8_t* mask, const int32_t* scenario,
                 int32_t scenario_all, int32_t randomize, uint64_t seed, uint32_t env_id0, uint32_t* episode_ctr,
                 float* obs, void* stream);

/* HarfangEnv.step for n envs: _apply_action -> one simulator tick -> _get_observation -> _get_reward ->
 * _get_termination (HarfangEnv_GYM.py:83-90,101-169,193-268; scripted opponents :342-353,412-421).
 * actions [n][4]; obs_io [n][13] in: previous observation (read only when opts->ring), out: next observation;
 * reward [n]; done [n] (0/1); success [n] (-1/0/+1). */
int hx_env_step(float* state, int64_t n, int64_t stride, const float* actions, float* obs_io, float* reward,
                uint8_t* done, int8_t* success, const HxStepOpts* opts /* host, may be NULL */, void* stream);

/* df.rearm_machine before a step (HarfangSerpentineInfiniteEnv.step_test, HarfangEnv_GYM.py:484-486) */
int hx_env_rearm(float* state, int64_t n, int64_t stride, const uint8_t* mask, void* stream);

/* Simulator-level access for the wire-protocol server (hirl4ucav_amd/environments/wire.py), i.e. what the external simulator does
 * for the reference between the client's SET_PLANE_PITCH/ROLL/YAW / FIRE_MISSILE calls and its read-backs (dogfight_client.py:
 * UPDATE_SCENE; GET_PLANE_STATE, GET_HEALTH, GET_MISSILESDEVICE_SLOTS_STATE) — no wrapper latches, no scripted opponent.
 * hx_sim_tick: one tick with the commanded (pitch, roll, yaw) levels of both aircraft [n][3] and the fire flags [n].
 * hx_sim_readback: out[n][16] = ally position 3, ally Euler (pitch, heading, roll) 3, opponent position 3, opponent Euler 3,
 * target angle in degrees, opponent health, target_locked (0/1), missile slot 0 loaded (0/1). */
int hx_sim_tick(float* state, int64_t n, int64_t stride, const float* ally_cmd, const float* opp_cmd, const uint8_t* fire,
                void* stream);
int hx_sim_readback(const float* state, int64_t n, int64_t stride, float* out, void* stream);

/* The N = 1 facade's read-back (hirl4ucav_amd/environments/HarfangEnv_GYM.py: the attributes the reference's wrapper caches after every step,
 * HarfangEnv_GYM.py:193-268) in one 64-float row: out[0..36] the state words of env i, [37..49] obs_io row i, [50] reward, [51] done,
 * [52] success, [53..63] zero — ONE device-to-host copy per step instead of five. */
int hx_env_pack_row(const float* state, int64_t n, int64_t stride, int64_t i, const float* obs, const float* reward, const uint8_t* done,
                    const int8_t* success, float* out /* [64] */, void* stream);

/* get_reward / get_termination for expert labelling (HarfangEnv_GYM.py:299-336, train_all.py:289-306):
 * s, ns [n][13], a [n][4] -> reward [n], success [n], done [n]. */
int hx_label_transitions(const float* s, const float* a, const float* ns, int64_t n, float* reward, int8_t* success,
                         uint8_t* done, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Actor / critic side.  Parameters, gradients and Adam moments are FLAT fp32 buffers in the reference's
 * state_dict order (hirl/agents/HIRL.py:19-146): an MLP block is
 *   full{1|3}.weight [256][in], .bias [256], layernorm{1|3}.weight [256], .bias [256], full{2|4}.weight [512][256],
 *   .bias [512], layernorm{2|4}.weight [512], .bias [512], final{|1|2}.weight [out][512], .bias [out]
 * Actor = one block (in 13, out 4) = 138,756 floats; Critic = two blocks (in 17, out 1), each padded from 138,241
 * to 138,244 floats so that the second head stays 16-byte aligned (hx_critic_param_count() = 276,488).
 * ------------------------------------------------------------------------------------------------------------ */
int hx_actor_param_count(void);
int hx_critic_param_count(void);
int64_t hx_hirl_workspace_floats(int32_t batch);
/* W2 IMAGES.  The four acting entry points (hx_actor_act, hx_actor_act_step, hx_sac_act, hx_sac_act_step) take three nullable pointers right after the
 * network: the copies of its 256 -> 512 matrix W2 that the caller offers, each written by its packer below and kept current by the optimizer steps
 * through HxNets / HxSacNets.  NULL means "not offered" (until version 126 an entry point per format refused a NULL image).  ONE acting format per
 * launch: the bf16 image (w2_bf16) if given, else the exact split (w2_x9: hi | mid | lo) if given, else the fp32 image (w2_f32i) if given, else
 * row-major W2 read from the network itself — all three NULL.  For the Gaussian head the split is used only beyond 8,192 rows with the persistent
 * kernel enabled; up to there the fp32 image serves, so hx_sac_act / hx_sac_act_step refuse w2_x9 without w2_f32i unless w2_bf16 is given.
 * Refused with HX_ERR_ARG: a non-NULL image that is not 16-byte aligned; noise_mode + 32 (hx_hirl_front's bit) where the exact split is the chosen format.
 *
 * w2_f32i, hx_pack_w2_f32i: a RE-ORDERED fp32 copy of W2 (512 x 256 floats).  The same arithmetic, bit for bit, as acting from W2 itself — but every
 * wave reads its 32 columns of W2 as contiguous kilobytes straight into registers (MFMA operand order) instead of streaming the row-major matrix
 * through LDS with a barrier per 16 k-values.  The image order is an internal format (w2f_image_index in hx_update.h).
 *
 * w2_bf16, hx_pack_w2_bf16: bf16 policy inference (BASELINE.json configs[4] "bf16 actor/critic + fp32 dynamics"): the 256 -> 512 layer — 96 % of the
 * policy's FLOPs — runs on v_mfma_f32_16x16x32_bf16 with h1 rounded to bf16 once and W2 read from w2_bf16[512][256] = bf16(W2), round to nearest
 * even; accumulation, layer 1, both LayerNorms and the head stay fp32, and so do the dynamics, the update and the optimizer.  Tolerance vs the fp32
 * policy: |da| <= 2e-2 on tanh outputs (tests/test_hirl_gpu.py); vs an fp32 evaluation on the SAME rounded operands: 1e-4.
 *
 * w2_x9, hx_pack_w2_x9: fp32 policy inference with the 256 -> 512 product on the bf16 matrix cores, EXACTLY: every fp32 operand is the sum of three
 * bf16 numbers (x = hi + mid + lo: 3 x 8 significand bits = fp32's 24, the split loses nothing), every one of the 9 partial products of a pair is
 * exact in fp32, and v_mfma_f32_16x16x32_bf16 accumulates them in fp32 — the small ones in an accumulator of their own that joins hi x hi at the end.
 * The same products as fp32 arithmetic, summed in another order: results within the fp32 kernels' own rounding noise (tests/test_x9_gpu.py measures
 * both against an fp64 evaluation), NOT bit-identical to the fp32 formats.  9 bf16 MFMAs per 32 k cost 144 matrix-core cycles against 256 for fp32
 * MFMA (the bf16 units are 16 x faster).  w2_x9 = [3][512][256] bf16: hi | mid | lo images of W2 in the bf16 acting kernels' format.
 * The packers read the MLP block at `net` (in_dim 13 or 17). */
int hx_pack_w2_f32i(const float* net, int32_t in_dim, float* w2_f32i, void* stream);
int hx_pack_w2_bf16(const float* net, int32_t in_dim, uint16_t* w2_bf16, void* stream);
int hx_pack_w2_x9(const float* net, int32_t in_dim, uint16_t* w2_x9, void* stream);

/* Agent.chooseAction / chooseActionSmallNoise / chooseActionNoNoise for `rows` observations at once
 * (hirl/agents/HIRL.py:192-212): actions = clamp(actor(obs) + noise, -1, 1).
 * noise_mode 0: none (NoNoise); 1: noise[4] shared by all rows (the reference's one draw per call); 2: noise[rows][4];
 * 3: N(0, sigma^2) per row and component from Philox4x32-10(key = seed; counter = (row0 + row, call)).
 * slope: 0 = ReLU nets (HIRL.py), 0.01 = LeakyReLU nets (TD3.py / BC.py).
 * noise_mode + 16: the actor was built with layerNorm = False (HIRL.py:135-138): no LayerNorm in its forward. */
int hx_actor_act(const float* actor, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, const float* obs, int64_t rows,
                 float* actions, int32_t noise_mode, const float* noise, float sigma, uint64_t seed, uint32_t row0, uint32_t call, float slope,
                 void* stream);
/* chooseAction + HarfangEnv.step for n envs in ONE launch (train_all.py:343-345): the actions of hx_actor_act (also written to
 * `actions`), then hx_env_step with them in the tail of the same kernel.  obs_io in: current observations, out: next. */
int hx_actor_act_step(const float* actor, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, float* state, int64_t n,
                      int64_t stride, float* obs_io, float* actions, int32_t noise_mode, const float* noise, float sigma, uint64_t seed,
                      uint32_t row0, uint32_t call, float slope, float* reward, uint8_t* done, int8_t* success,
                      const HxStepOpts* opts /* host, may be NULL */, void* stream);

/* Minibatch of Agent.learn (HIRL.py:223-251), already assembled by hx_sample_batch into compact row tiles:
 * rows[batch][HX_ROW_WORDS] = s[13] a[4] s'[13] r done (buffer rows first, then expert rows, HIRL.py:229-233);
 * bc_rows[batch][HX_ROW_WORDS]: cols 0..12 state, 13..16 action of the BC minibatch (HIRL.py:248-251; NULL for TD3). */
typedef struct HxBatch {
    const float* rows;
    const float* bc_rows;
    int32_t batch;      /* multiple of 16 */
    const float* noise; /* [4] target-smoothing noise, unclamped: ONE draw for the whole batch (HIRL.py:265) */
} HxBatch;

typedef struct HxNets {
    float* actor; float* critic; float* target_actor; float* target_critic; const float* bc_actor;
    float* grad_actor; float* grad_critic;
    float* m_actor; float* v_actor; float* m_critic; float* v_critic;
    float* losses;       /* [8]: critic_loss, actor_loss, bc_loss, rl_loss, bc_fire_loss, bc_weight (HIRL.py:334) */
    int32_t* soft_count; /* [1] count(soft_Q > rl_Q) (HIRL.py:303) — all-reduce it when the batch is sharded */
    float* wstate;       /* [1] the BC weight in force */
    float* ws;           /* hx_hirl_workspace_floats(batch) */
    uint16_t* actor_w2_bf16; /* NULL, or [512][256] bf16 image of the actor's full2.weight: every Adam step of the actor refreshes it
                                (hx_adam which = 1 / 2), the acting entry points' w2_bf16 */
    float* actor_w2_f32i;    /* NULL, or the fp32 image of the same matrix (hx_pack_w2_f32i), refreshed likewise; the acting entry points' w2_f32i */
    uint16_t* w2_bf16_all;   /* NULL: the update computes in fp32 (parity 1e-5 vs the reference).  Else hx_bf16_images_elems() bf16 elements =
                                the bf16 images of every W2 the update reads: the bf16 UPDATE path (below).  Its first 512 x 256 elements are
                                the actor's image in the bf16 acting kernels' format: actor_w2_bf16 must then be NULL or point at them */
    const uint32_t* xchg_status; /* NULL, or the status word of hx_allreduce_oneshot: while it is non-zero (an exchange failed: the summed
                                gradient is garbage) hx_adam / hx_adam_mixed change nothing — no parameter, moment, target or image */
    uint16_t* actor_w2_x9;   /* NULL, or the [3][512][256] hi | mid | lo bf16 images of the actor's full2.weight (hx_pack_w2_x9): refreshed by
                                every Adam step of the actor like the other two; the acting entry points' w2_x9 */
} HxNets;

/* bf16 update path (BASELINE.json configs[4] "bf16 actor/critic + fp32 dynamics"; SURVEY.md 7 "bf16 config").  With HxNets.w2_bf16_all set,
 * every hx_hirl_* / hx_bc_train_actor call runs the three products of the 256 <-> 512 layer of all five networks (Actor / Critic forward
 * HIRL.py:55-97,126-140 inside learn() HIRL.py:259-325, and their backward passes) on v_mfma_f32_16x16x32_bf16:
 *     z2 = bf16(h1) bf16(W2)^T + b2        dh1 = bf16(dz2) bf16(W2)        dW2 = bf16(dz2)^T bf16(h1)       (fp32 accumulation)
 * Master weights, Adam moments, LayerNorm statistics, layer 1 (K = 13 / 17), the heads, TD targets and loss sums stay fp32.  The images
 * (forward order for z2, transposed for dh1; actor, critic x 2, the three targets, bc_actor) are kept current by every optimizer / Polyak
 * step (hx_hirl_learn*, hx_adam*, hx_polyak, hx_bc_train_actor); after any OTHER write to a network (loading parameters) call
 * hx_pack_update_images.  Tolerance against an fp32 evaluation on the same rounded operands: tests/test_bf16_update_gpu.py. */
int64_t hx_bf16_images_elems(void);
int hx_pack_update_images(const HxNets* nets, void* stream);

typedef struct HxHyper {
    float gamma, tau, lr_actor, lr_critic, slope, noise_clamp, loss_lambda;
    int32_t use_bc; /* 1: HIRL (TD3+BC, HIRL.py), 0: TD3 (TD3.py:201-260) */
    int32_t no_layernorm; /* 1: the agent was built with layerNorm = False: the networks' forward skips both LayerNorms (HIRL.py:70-80,92-97,
                             135-138).  The LayerNorm slots of the flat buffers must hold (1, 0) — the reference constructs the modules either
                             way (HIRL.py:28,33,114,119) and never trains them in this mode — and stay that way (their gradients are zero) */
} HxHyper;

/* Agent.learn, split at the points where a sharded run exchanges data; single-GPU callers run the
 * stages back to back on one stream:
 *   hx_hirl_critic_grads    TD target + critic loss + grad_critic          HIRL.py:259-286   -> [all-reduce grad_critic]
 *   hx_adam(which = 0)      critic.optimizer.step()                         HIRL.py:288
 *   -- every second call (actorTrainable, HIRL.py:291,332) --
 *   hx_hirl_actor_backward  pi, rl_Q with the updated critic, soft count,  HIRL.py:293-319   -> [all-reduce soft_count]
 *                           BC loss, backward down to the actor's dz2/dh1
 *   hx_hirl_actor_wgrad     grad_actor = w dL_bc + (1 - w) dL_rl            HIRL.py:321-324   -> [all-reduce grad_actor]
 *   hx_adam(which = 1)      actor.optimizer.step(); actor_loss, bc_weight   HIRL.py:325,334
 *   hx_polyak               every 3rd actor step (HIRL.py:327-330) */
/* actor_fwd: 0 = critic phase only; 1 = also run the delayed actor step's critic-independent forward passes actor(s),
 * actor(s_bc) in the same first launch; 2 = plus bc_actor(s) for the soft estimate (then pass fwd_done = 1 or 2 below).
 * With actor_fwd != 0 the call's last launch (the critics' parameter gradients) also evaluates the HEAD of actor(s) [and of bc_actor(s)] once
 * per row — LayerNorm 2, final layer, tanh — on workgroups of its own, and leaves the action rows in the workspace (HX_HEAD_RIDER=0: not).
 * hx_hirl_actor_backward's fwd_done: 0 = it runs the actor call's forward passes itself; 1 = they are done, its Q1(s, pi(s)) launch evaluates
 * the heads it feeds on in each of its workgroups; 2 = forwards and heads are done (this call's actor_fwd != 0, or hx_hirl_critic_grads_back's
 * c_in_front + 2 / + 4), the launch reads the action rows — same bits either way. */
int hx_hirl_critic_grads(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, int32_t actor_fwd, void* stream);
int hx_hirl_actor_backward(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, int32_t estimate_soft,
                           int32_t fwd_done, void* stream);
/* w_kind 0: w = w_given (linear / fixed, train_all.py:328-333); 1: w = soft_count / count_batch + warm (HIRL.py:304-306);
 * 2: the stored weight.  w is clipped to <= 1 (HIRL.py:308). */
int hx_hirl_actor_wgrad(const HxNets* nets, const HxHyper* hyper, int32_t batch, int32_t count_batch, int32_t w_kind,
                        float w_given, float warm, void* stream);
/* which 0 critic / 1 actor / 2 actor alone (BC pre-training), + 16: also soft_update (HIRL.py:11-13) this network's target with the new
 * parameters in the same launch; step = 1-based Adam step; grad is scaled by grad_scale first (1/world after a SUM). */
int hx_adam(const HxNets* nets, const HxHyper* hyper, int32_t which, int32_t step, float grad_scale, int32_t w_kind,
            float w_given, float warm, int32_t batch, void* stream);
int hx_polyak(const HxNets* nets, const HxHyper* hyper, void* stream); /* both targets in a launch of their own */
/* Sharded runs with ONE exchange for the actor phase (SURVEY.md 8e "all-reduce dL_bc, dL_rl and the count in one message and combine
 * locally"): hx_hirl_actor_wgrad_split writes msg = [dL_rl | dL_bc | tail] (hx_actor_message_floats() floats, each gradient
 * hx_actor_param_count() floats padded to a multiple of 4; the padding is not written), unweighted; after the all-reduce of msg, hx_adam_mixed forms
 * w = count / batch + warm from the GLOBAL count (w_kind 1; given / stored weight otherwise), g = w dL_bc + (1 - w) dL_rl (HIRL.py:321),
 * and steps the actor (grad_scale = 1 / world; polyak != 0: soft_update of targetActor in the same launch).
 * The 64-word tail: word 0 = the local soft count as a float (for the reader of a dump; nothing computes with it), words 1..7 = the count's base-32
 * digits as floats, least significant first, words 8..63 are not written (keep them 0).  hx_adam_mixed rebuilds the global count from the SUMMED digit
 * words: a digit is at most 31, so every partial sum over up to 8 ranks is at most 248, and integers up to 256 are exact in bf16 — the count arrives
 * exactly through every transport and summation order, the bf16 ones included (word 0 does not: bf16 keeps 8 bits, 8 ranks x 128 rows need 11).
 * The launch writes grad_actor nowhere.  TD3 (hyper->use_bc == 0): dL_rl and the eight count words (all 0) are written, the dL_bc half is left as it
 * was, and hx_adam_mixed reads neither the dL_bc half nor the tail. */
int64_t hx_actor_message_floats(void);
int hx_hirl_actor_wgrad_split(const HxNets* nets, const HxHyper* hyper, int32_t batch, float* msg, void* stream);
int hx_adam_mixed(const HxNets* nets, const HxHyper* hyper, int32_t polyak, int32_t step, float grad_scale, int32_t w_kind, float w_given,
                  float warm, int32_t batch /* global */, const float* msg, void* stream);
/* Gradient-norm clipping for HIRL and TD3: torch.nn.utils.clip_grad_norm_(optimizer's parameters, max_norm) in front of each optimizer step, two
 * launches per step.  The reference's agents have no clip (a declared extension); an optimizer covers ALL of its parameters — both Q heads and the
 * LayerNorm weights for the critic (ONE norm), the whole actor —, never the padding behind a block's parameters.
 *   hx_hirl_grad_norm  one launch: workgroup c of a block writes the sum of squares of its fixed 4,096-word chunk — a fixed order, no atomics, no
 *                      workgroup waits for another — into clip_ws (hx_hirl_clip_floats() floats, 16-byte aligned).  which 0: nets->grad_critic (what
 *                      hx_adam(0) steps on: after an exchange, the summed gradient); which 1: nets->grad_actor, or with msg the merged message
 *                      [dL_rl | dL_bc | tail] squared AFTER mixing w dL_bc + (1 - w) dL_rl with hx_adam_mixed's own w (TD3: the dL_rl half alone)
 *   hx_adam_clipped    hx_adam's (msg NULL) / hx_adam_mixed's (msg) step on (g * grad_scale) * coef: every workgroup re-adds the partial sums in the same
 *                      fixed order, norm = sqrt(sum) * grad_scale (the norm of the AVERAGED gradient on a sharded rank), coef = min(1, max_norm /
 *                      (norm + 1e-6)); coef == 1 leaves hx_adam's bits.  which 0 | 1, + 16 as hx_adam; which 2 and a msg with which 0 are refused.
 *                      Honours nets->xchg_status like hx_adam.  clip_ws[0..1] <- the norms (critic, actor), clip_ws[2..3] <- the coefficients.
 * w_kind / w_given / warm / batch: as hx_adam / hx_adam_mixed (read in the message form only by hx_hirl_grad_norm). */
int64_t hx_hirl_clip_floats(void);
/* shape[0..7] (host) <- float4 per thread, words per chunk, partials one wave re-adds at most, chunks of a Q head, chunks of the actor, the depth in
 * additions (squares included) of the critic's and of the actor's sum, the word of clip_ws where the partials begin (Q head 0 | Q head 1 | actor,
 * shape[2] words each) */
int hx_hirl_clip_shape(int32_t* shape8);
int hx_hirl_grad_norm(const HxNets* nets, const HxHyper* hyper, int32_t which, int32_t w_kind, float w_given, float warm, int32_t batch,
                      const float* msg, float* clip_ws, void* stream);
int hx_adam_clipped(const HxNets* nets, const HxHyper* hyper, int32_t which, int32_t step, float grad_scale, int32_t w_kind, float w_given,
                    float warm, int32_t batch, const float* msg, float max_norm, float* clip_ws, void* stream);
/* Prioritized replay for HIRL / TD3.  A declared extension: the reference ships a SumTree beside UniformMemory (hirl/utils/buffer.py) and HIRL.py:236,283
 * guard on isinstance(self.buffer, UniformMemory), but its prioritized branch is dead — there is no live counterpart to reproduce.  The rule:
 *     store, draw, weights   "Prioritized replay" below, unchanged: p = (|delta| + 1e-4)^alpha, proportional draws with replacement,
 *                            w = (n p / S)^-beta / max, new rows at pmax (hx_per_mark_new)
 *     which rows             the minibatch is n_main replay rows, then batch - n_main expert rows (HIRL.py:226-227).  Only rows [0, n_main) are drawn by
 *                            priority, carry a weight and give their error back; expert rows weigh exactly 1 and touch no priority; the BC minibatch
 *                            is untouched.  Unlike SAC's --per the expert rows are KEPT (warm-up, --expert_floor, --expert_branch keep working)
 *     loss                   y = r + gamma min(Q1', Q2') (1 - d) (HIRL.py:270-274; the discount folded into the done column keeps working);
 *                            critic_loss = mean_r(w_r (Q1 - y)^2) + mean_r(w_r (Q2 - y)^2), both means over all `batch` rows -> losses[0];
 *                            head gradients 2 w_r (Q_h - y) / batch; errors_out[r] = |Q1(s, a) - y|_r, as hx_per_update expects
 *     the actor half         UNWEIGHTED and unchanged — the rule's one design decision: its loss already mixes a second (BC) batch and a counted gate, and
 *                            PER-TD3 in its usual form weights the critic alone
 *     order per vector step  act_step -> hx_per_mark_new(n) -> draw -> learn -> hx_per_update(idx[:n_main], errors[:n_main]): the reference's step order
 *                            only (the front launch draws before the step's insert, so the priorities of the drawn rows could be written into
 *                            overwritten slots)
 * hx_hirl_critic_grads_weighted: stage 1 (hx_hirl_critic_grads) with the weights.  Launches A and B as there (actor_fwd's riding forwards included); the TD
 * head as a per-row kernel of its own (one wave per row: y, errors_out, losses[0], both critics' head gradients and LayerNorm stats; fp32 on the bf16
 * update path too); both critics' backward from the given head gradient; the weight-gradient launch without Adam (actor_fwd's head riders kept).  The
 * caller follows with hx_adam(0) or hx_hirl_grad_norm + hx_adam_clipped.  n_weighted in 0..batch: rows [0, n_weighted) weigh weights[r], the rows
 * behind them 1 — weights is not read there and may be NULL when n_weighted == 0.  errors_out[batch] is required and written for EVERY row.  batch: a
 * positive multiple of 16. */
int hx_hirl_critic_grads_weighted(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, const float* weights, int32_t n_weighted,
                                  float* errors_out, int32_t actor_fwd, void* stream);
/* BC.Agent.train_actor (hirl/agents/BC.py:160-185): one behaviour-cloning step on batch->bc_rows: loss = mse(actor(s_bc),
 * a_bc), backward, actor.optimizer.step(); losses[2] receives the loss.  hyper->slope = 0.01 gives BC.py's LeakyReLU actor.
 * (hx_adam's which = 2 is the actor step without HIRL's actor_loss / bc_weight bookkeeping.) */
int hx_bc_train_actor(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, int32_t step, void* stream);
/* The stages above back to back in one host call, for a single GPU (no gradient exchange).  actor_phase: this is an
 * actorTrainable call (HIRL.py:291,332); do_polyak: update_count reaches a multiple of 3 in it (HIRL.py:327-330);
 * critic_step / actor_step: 1-based Adam step numbers of this call; w_kind / w_given / warm as in hx_hirl_actor_wgrad. */
int hx_hirl_learn(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, int32_t critic_step, int32_t actor_phase,
                  int32_t actor_step, int32_t do_polyak, int32_t w_kind, float w_given, float warm, void* stream);

/* Minibatch assembly for one learn() call: replaces UniformMemory.sample (hirl/utils/buffer.py:38-48, random.sample without
 * replacement), the buffer/expert mixing and np.random.choice(replace=False) of HIRL.py:223-251, and the noise draw
 * HIRL.py:265.  do_sample = 1: draws idx[batch] (rows < n_main index `ring`, whose live length min(*total, cap) is read on
 * the device; the rest index `expert_ring`), idx_bc[batch] into bc_table, noise[4] = sigma N(0,1); Philox4x32-10(seed; row,
 * call).  do_sample = 0: idx / idx_bc are inputs (caller-chosen minibatch).  Either way the selected rows are copied into the
 * compact tiles rows[batch][32] and bc_rows[batch][32] (bc_table / idx_bc / bc_rows may be NULL) that HxBatch points at.
 * batch <= 1024. */
int hx_sample_batch(const uint64_t* total, int64_t cap, const float* ring, const float* expert_ring, int64_t expert_len,
                    const float* bc_table, int64_t bc_len, int32_t batch, int32_t n_main, int32_t do_sample, uint64_t seed,
                    uint32_t call, float sigma, int32_t* idx, int32_t* idx_bc, float* noise, float* rows, float* bc_rows,
                    void* stream);
/* The same with the `guard` ring slots behind the head *total left out of the draw (see HxSample.guard / hx_hirl_front). */
int hx_sample_batch_guarded(const uint64_t* total, int64_t cap, const float* ring, const float* expert_ring, int64_t expert_len,
                            const float* bc_table, int64_t bc_len, int32_t batch, int32_t n_main, int32_t do_sample, uint64_t seed,
                            uint32_t call, float sigma, int32_t* idx, int32_t* idx_bc, float* noise, float* rows, float* bc_rows,
                            uint32_t guard, void* stream);

/* The draw of hx_sample_batch(do_sample = 1) as a description instead of a launch: hx_hirl_learn_sampled / hx_hirl_critic_grads_sampled
 * draw the indices and gather the rows inside the FIRST launch of the update (every workgroup repeats the cheap draw, each gathers
 * its own 16 rows straight from the rings) — the same indices, noise, row tiles and results, bit for bit, as hx_sample_batch followed
 * by hx_hirl_learn / hx_hirl_critic_grads, with one launch and one kernel boundary less (UniformMemory.sample buffer.py:38-48 + the
 * minibatch assembly HIRL.py:223-251 + the noise draw HIRL.py:265).  The tiles HxBatch points at (rows, bc_rows, noise) are OUTPUTS
 * then (the later launches read them); idx / idx_bc receive the drawn indices.  batch <= 256 takes the fused path, larger batches run
 * the separate sampling launch inside the same call. */
typedef struct HxSample {
    const uint64_t* total; int64_t cap; const float* ring;   /* main replay ring (hx_env_step's HxStepOpts.total / cap / ring) */
    const float* expert_ring; int64_t expert_len;            /* NULL / 0: no expert rows (n_main == batch) */
    const float* bc_table; int64_t bc_len;                   /* NULL / 0: no BC minibatch (TD3) */
    int32_t n_main;                                          /* rows [0, n_main) from the main ring, the rest from the expert ring */
    uint64_t seed; uint32_t call; float sigma;               /* Philox4x32-10(seed; row, call); noise[4] = sigma N(0, 1) */
    int32_t* idx; int32_t* idx_bc;                           /* [batch] out (idx_bc NULL without a BC table) */
    uint32_t guard;                                          /* 0: UniformMemory.sample over the whole buffer.  > 0 (fused draws only): the `guard`
                                                              * slots behind the ring head *total are not drawn — see hx_hirl_front */
} HxSample;
/* hx_hirl_critic_grads / hx_hirl_learn with the minibatch drawn and gathered in their first launch (arguments as theirs + the draw). */
int hx_hirl_critic_grads_sampled(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, const HxSample* sample, int32_t actor_fwd,
                                 void* stream);
int hx_hirl_learn_sampled(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, const HxSample* sample, int32_t critic_step,
                          int32_t actor_phase, int32_t actor_step, int32_t do_polyak, int32_t w_kind, float w_given, float warm, void* stream);

/* The FRONT launch (opt-in; fp32 networks — noise_mode + 32: the policy's W2 from HxNets.actor_w2_x9, the exact three-way bf16 split, as
 * hx_actor_act_step with w2_x9, else from HxNets.actor_w2_f32i — or the bf16 update path, HxNets.w2_bf16_all, with the bf16 acting image
 * HxNets.actor_w2_bf16; n <= 8,192 — with a replay ring any number in the exact-split format and in bf16): hx_actor_act_step with that one image for n envs (chooseAction + HarfangEnv.step + replay insert,
 * train_all.py:343-345) AND the first two launches of the learn() call that follows it (targetActor(s'), Q1/Q2(s, a) [+ the actor call's forwards];
 * then targetCritic Q1/Q2 — HIRL.py:259-272) as workgroups of ONE launch: the acting workgroups take 32 rows each and so leave half of the CUs to
 * the update's workgroups, which would otherwise wait for the env step to finish although they depend on nothing it computes EXCEPT the ring it
 * inserts into.  Hence the one change of meaning: the minibatch (`batch`'s tiles, filled before this launch) is drawn from the ring as it stood
 * BEFORE this env step, leaving out the n slots the step may overwrite (HxSample.guard = n) — i.e. uniformly from every transition that is in the
 * buffer both before and after the step (the reference draws after its one-transition append, buffer.py:45; at n envs per step the population
 * differs by the newest and, once the ring is full, the oldest n transitions).  Who fills the tiles: the previous hx_hirl_learn_back (its `next`:
 * one more workgroup of the critics' gradient launch draws and gathers, on a CU that launch leaves idle), or hx_sample_batch_guarded as a launch of its own.
 * Bit-identical to hx_actor_act_step with the same image followed by hx_hirl_learn_sampled with HxSample.total read before the step and HxSample.guard = n
 * (and launch B in 64-column workgroups: hx_debug_set_fwd_nt).  The target critics wait IN the launch for the target actor's rows (per-row-tile
 * counters `flags`, agent-scope relaxed accesses, bounded wait ~1 s: bit 0 of *status is set if a launch-B workgroup gives up, bit 1 if a launch-C
 * workgroup does (HxFront.with_c)).
 * WHY THE WAITS END.  Every workgroup of the launch is a whole CU; the acting workgroups and launch A's never wait and leave within ~20 us; the waiting
 * ones are launch B's two target-critic jobs (16 per 16-row tile: 128 at B = 128) and, with launch C riding, its TD jobs (256 more).  While the waiting
 * workgroups are FEWER than the CUs (256) — the default shape: B = 128, launch C on its own — a pending producer always finds a CU under ANY dispatch
 * order that places pending workgroups on free CUs, and a wait ends within the acting workgroups' ~20 us (HirlEngine.front_waiting_workgroups).
 * ONE PROCESS PER GPU: processes that share a GPU share its CUs, and their waiters add up — the argument above is void there.  Three processes
 * free-running the default shapes on one GPU never tripped (100,000 steps each in every acting role; with launch C riding the third process made the
 * waits time out and the status word caught it: profiles/r05_soak_front_shared_gpu.txt); EIGHT did, on a fresh box, and took round 5's test run with
 * them (GPUTEST_r05: 1,024 waiters on 256 CUs).  So the callers decide by design, not by soak [r6]: bench.py and train_all take this entry point only
 * when every rank has a device of its own (world <= visible devices) and run the reference's order otherwise; asked for explicitly on a shared device
 * (bench.py --front, HX_FRONT_SHARED_GPU=1) the status word + fallback below are what stands between a trip and a wrong number.
 * At B = 256 or with launch C riding the waiting workgroups can fill the chip, and there THE ASSUMPTION BEHIND THE WAITS is needed: the workgroups of one
 * launch START in index order (producers have the lower indices), so a waiting workgroup's producers are running or done.  That is what gfx950 /
 * ROCm 7.2 does (free-running soaks of every acting role, launch C riding included: profiles/archive/r04c_front_soak_*.json, profiles/r05_soak_front_roles.jsonl);
 * HIP promises no dispatch order.  Under another order a wait still ends as soon as the producers get a CU (the acting workgroups never wait and leave
 * after ~20 us); only if EVERY resident workgroup were a waiting consumer could a wait run into its bound — then the status word says so, the minibatch
 * of that launch may have been read half-written, and the caller must not go on: read *status at least every few hundred launches (hirl4ucav_amd/
 * train_all.py --status_check_every, default 256: on a trip it reloads its last snapshot and continues in the reference's order in the same process, or
 * exits with code 3; bench.py reads it after the timed region and the second pass — one decision for all ranks — and on a trip repeats the whole run in
 * the reference's order in the same process and labels the line `reference order (front tripped)`) and fall back to hx_actor_act_step +
 * hx_hirl_learn_sampled (no in-launch waits; `train_all --loop reference`, `bench.py --no-front`).
 * (Roles taken in START order from a ticket would need no such assumption; measured, that costs 2.8 us of a 51.4 us step: docs/LEVERS.md, Round 5.)
 * hx_hirl_learn_back = the rest of the call (critic backward + gradients + Adam [+ the delayed actor step]) on the same `batch`; next / next_tiles
 * (or NULL): the draw of the NEXT front launch (guard = its n; *next->total is read inside this call's second launch, i.e. after this step's
 * inserts and before the next step's) into tiles of their own. */
typedef struct HxFront {
    uint32_t* flags;       /* [64] device words, zero before the first use (and whenever epoch starts over at 1) */
    uint32_t* status;      /* device word, sticky */
    uint32_t epoch;        /* 1, 2, 3, ... : one per front launch on these flags */
    uint32_t with_c;       /* 0, or 1, 2, 3, ... = this is the k-th front launch on these flags WITH launch C: the critics' backward launch (y, loss, dq, dh1: HIRL.py:270-286) rides in this launch too, waiting in-launch for the forward
                            * workgroups it reads; then pass c_in_front = 1 to hx_hirl_learn_back / hx_hirl_critic_grads_back.  Same bits; it pays only where the
                            * acting workgroups leave the other CUs time to spare (around 8,192 envs in the exact-split format: HirlEngine.front_c_for) */
} HxFront;
int hx_hirl_front(float* state, int64_t n, int64_t stride, float* obs_io, float* actions, int32_t noise_mode,
                  const float* noise, float sigma, uint64_t seed, uint32_t row0, uint32_t call, float* reward, uint8_t* done, int8_t* success,
                  const HxStepOpts* opts, const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, int32_t actor_phase, int32_t w_kind,
                  const HxFront* front, void* stream);
int hx_hirl_learn_back(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, int32_t critic_step, int32_t actor_phase, int32_t actor_step,
                       int32_t do_polyak, int32_t w_kind, float w_given, float warm, const HxSample* next, const HxBatch* next_tiles, int32_t c_in_front,
                       void* stream);
/* A sharded rank's form: what hx_hirl_critic_grads leaves behind (grad_critic, ready for the exchange; no optimizer step) after a front launch, + the predraw.
 * c_in_front: 0 / 1 as above, + 2 on an actor call (the head of actor(s) rides in the gradient launch, as with hx_hirl_critic_grads' actor_fwd = 1),
 * + 4 instead on a soft-estimate call of a BC agent (bc_actor(s)'s head too, actor_fwd = 2); then hx_hirl_actor_backward takes fwd_done = 2. */
int hx_hirl_critic_grads_back(const HxNets* nets, const HxBatch* batch, const HxHyper* hyper, const HxSample* next, const HxBatch* next_tiles, int32_t c_in_front,
                              void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * SAC (hirl/agents/SAC, the non-imitative branch train_sac.py uses).  Networks are the plain Linear-ReLU stacks of the
 * un-vendored rltorch builder (SAC/model.py:21,58): policy 13 -> 256 -> 512 -> 8 (mean ++ log_std), Q heads 17 -> 256 -> 512
 * -> 1.  They use the SAME flat block layout as above; the LayerNorm slots hold (1, 0) and are never updated.
 * hx_sac_policy_param_count() floats for the policy, hx_critic_param_count() for the twinned Q.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct HxSacNets {
    float* policy; float* critic; float* target_critic;
    float* grad_policy; float* grad_critic;
    float* m_policy; float* v_policy; float* m_critic; float* v_critic;
    float* losses;      /* [8]: q1_loss, q2_loss, policy_loss, entropy_loss, mean entropy, alpha, -, -  (imitative calls: [6] bc_loss, [7] bc_weight) */
    float* alpha_state; /* [4]: log_alpha, its Adam m and v, alpha = exp(log_alpha)  (SAC/agent.py:106-108) */
    float* ws;          /* hx_sac_workspace_floats(batch) */
    float* policy_w2_f32i; /* NULL, or the fp32 image of the policy's W2 (hx_pack_w2_f32i(policy, 13, ...)): hx_sac_adam(which = 1) keeps it
                              current; hx_sac_act's w2_f32i */
    uint16_t* policy_w2_x9; /* NULL, or the hi | mid | lo bf16 images of the policy's W2 (hx_pack_w2_x9(policy, 13, ...), 3 x 512 x 256): the
                               policy's optimizer step keeps them current; hx_sac_act's w2_x9 */
    uint16_t* w2_bf16_all;  /* NULL: the update computes in fp32.  Else hx_bf16_images_elems() bf16 elements: the SAC bf16 path (below).  Its first
                               512 x 256 elements are the policy's image in the bf16 acting format (hx_sac_act's w2_bf16) */
    uint16_t* policy_w2_bf16; /* NULL, or the bf16 image of the policy's W2 (hx_pack_w2_bf16(policy, 13, ...)) for bf16 acting beside an fp32
                               update: the policy's optimizer step keeps it current.  With w2_bf16_all set it must be NULL or its first image */
} HxSacNets;

/* SAC bf16 path (BASELINE.json configs[4] "bf16 actor/critic + fp32 dynamics" for SacAgent).  With HxSacNets.w2_bf16_all set, every hx_sac_*
 * update call runs the three products of the 256 <-> 512 layer of the policy, both critics and both target critics on v_mfma_f32_16x16x32_bf16:
 *     z2 = bf16(h1) bf16(W2)^T + b2        dh1 = bf16(dz2) bf16(W2)        dW2 = bf16(dz2)^T bf16(h1)       (fp32 accumulation)
 * Images: IM_ACTOR / IM_ACTOR_T = the policy's forward / transposed W2, IM_C1, IM_C2 (+ _T) the critics', IM_TC1, IM_TC2 the target critics'.
 * Master weights, Adam moments, layer 1 (K = 13 / 17), the Gaussian heads (mean, clamped log_std, exp, tanh, entropy), q_select, the policy's head
 * gradient, the log-alpha step, TD targets and loss sums stay fp32.  Every optimizer step refreshes the forward and transposed images of the network
 * it steps (the policy's forward image is the acting image); every Polyak step refreshes IM_TC1 / IM_TC2.  After any OTHER write to a network call
 * hx_sac_pack_update_images.  Acting (hx_sac_act / hx_sac_act_step with w2_bf16): the 256 -> 512 product as above from the policy's image, layer 1 and the head in fp32 — NOT
 * the deterministic policy's bf16 head (hx_actor_act with w2_bf16): exp(log_std) amplifies head error, and the update's head is fp32 too.
 * Tolerances (tests/test_sac_bf16_gpu.py): actions against an fp32 evaluation on the same rounded operands: 99 % within 1e-4, all within 2e-3;
 * against the fp32 policy: |da| <= 2e-2, mean |da| <= 2e-3.  learn() against the rounded-operand oracle: losses rtol 1e-4; parameters after Adam
 * as tests/test_bf16_update_gpu.py. */
int hx_sac_pack_update_images(const HxSacNets* nets, void* stream);

typedef struct HxSacBatch {
    const float* rows;     /* [batch][HX_ROW_WORDS] compact minibatch (hx_sample_batch) */
    int32_t batch;         /* multiple of 16 */
    const float* eps_next; /* [batch][4] standard-normal draws of policy.sample(next_states) (SAC/agent.py:204) */
    const float* eps_cur;  /* [batch][4] draws of policy.sample(states) in calc_policy_loss (SAC/agent.py:380) */
    uint64_t seed;         /* eps_next / eps_cur NULL: the draws come from Philox4x32-10(seed; row, call) inside the kernels */
    uint32_t call;         /* (distinct streams for the two samples), no draw buffers and no launches to fill them */
} HxSacBatch;

int hx_sac_policy_param_count(void);
int64_t hx_sac_workspace_floats(int32_t batch);
/* SacAgent.explore / exploit (SAC/agent.py:183-196): mode 0 exploit = tanh(mean); 1 sample with eps[rows][4]; 2 sample with
 * Philox4x32-10(seed; row0 + row, call).  The images: "W2 IMAGES" above (w2_x9 = hx_pack_w2_x9(policy, 13, ...) is the large-population format of the
 * fp32 policy — beyond 8,192 rows the persistent kernel streams the three images; up to 8,192 rows w2_f32i, which must be given with it, serves).
 * With w2_bf16 ("SAC bf16 path" above): the per-tile kernel up to 8,192 rows, the streaming persistent kernel beyond (the same bits for a row). */
int hx_sac_act(const float* policy, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, const float* obs, int64_t rows,
               float* actions, int32_t mode, const float* eps, uint64_t seed, uint32_t row0, uint32_t call, void* stream);
/* SacAgent.explore / exploit + HarfangEnv.step in one launch (train_sac.py:238-241). */
int hx_sac_act_step(const float* policy, const float* w2_f32i, const uint16_t* w2_x9, const uint16_t* w2_bf16, float* state, int64_t n,
                    int64_t stride, float* obs_io, float* actions, int32_t mode, const float* eps, uint64_t seed, uint32_t row0, uint32_t call,
                    float* reward, uint8_t* done, int8_t* success, const HxStepOpts* opts /* host, may be NULL */, void* stream);
/* SacAgent.learn (SAC/agent.py:276-327) in the stages a sharded run separates:
 *   hx_sac_critic_grads   [soft_update of the target critics first on every 3rd call :278-279]; target y = r + (1-d) gamma
 *                         (min Q_target(s', a') + alpha H') :202-210; q1_loss, q2_loss :361-374 -> losses[0..1]; grad_critic
 *   hx_sac_adam(0)        q1_optim.step(), q2_optim.step() :310-313                                  [after all-reduce]
 *   hx_sac_policy_grads   policy_loss = mean(-min Q(s, a~) - alpha H) with the updated critics :376-406 -> losses[2], grad_policy
 *   hx_sac_adam(1)        policy_optim.step() :318-319, then entropy_loss and alpha_optim.step() :322-325,408-414 */
int hx_sac_critic_grads(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, int32_t polyak_first, void* stream);
/* hx_sac_critic_grads with the minibatch drawn and gathered in its first launch (HxSample without a BC table; batch->rows is the output
 * tile; batch <= 256 draws in-launch, larger batches run the sampling launch inside the call): same indices, tile and results. */
int hx_sac_critic_grads_sampled(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const HxSample* sample,
                                int32_t polyak_first, void* stream);
/* one GPU: critic gradients AND q1_optim / q2_optim steps (SAC/agent.py:278-313) in one call — the optimizer step rides in the weight-gradient
 * launch; sample may be NULL (minibatch already assembled); step is 1-based.  Bit-identical to hx_sac_critic_grads[_sampled] + hx_sac_adam(0). */
int hx_sac_critic_step(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const HxSample* sample, int32_t polyak_first,
                       int32_t step, void* stream);
int hx_sac_policy_grads(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, void* stream);
/* One GPU: the whole SacAgent.learn (SAC/agent.py:276-327) in one call and 9 launches — the soft_update and policy.sample(s) in the launch of
 * policy.sample(s'), every optimizer step (log-alpha included) in its weight-gradient launch, the min(Q1, Q2) selection and the policy's head
 * gradient in the prologues of the backward launches that consume them.  Bit-identical to hx_sac_critic_step +
 * hx_sac_policy_grads + hx_sac_adam(which = 1); sample may be NULL (minibatch already assembled); step is 1-based. */
int hx_sac_learn(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const HxSample* sample, int32_t polyak_first, int32_t step,
                 float target_entropy, void* stream);
/* The SAC front launch (any n >= 1 envs with a replay ring): hx_sac_act_step with the same images — explore / exploit +
 * HarfangEnv.step + replay insert (train_sac.py:238-241) — AND the first forward launch of the SacAgent.learn call that follows it (policy(s'), policy(s),
 * Q1/Q2(s, a), E-SAC's extra jobs: SAC/agent.py:198-210, 276-290) as workgroups of ONE launch, on the minibatch `batch->rows` holds already.  No workgroup of it
 * waits for another.
 * Which kernel acts: up to 8,192 envs the per-tile workgroups of hx_sac_act_step from the fp32 or the bf16 image (one round of 16- or 32-row workgroups: the tiling is a choice per
 * size and format, HX_SAC_FRONT_F32_NRT2_ROWS / HX_SAC_FRONT_BF16_NRT2_ROWS, and a row's action does not depend on it), the forward workgroups on the CUs they
 * leave free; beyond, the streaming persistent kernel on every CU, the forward workgroups starting as the acting ones leave.
 * Images: the acting format is taken from nets.  With nets->w2_bf16_all set: the bf16 acting image (its first one) and the bf16 first launch; w2_x9 and w2_f32i
 * must be NULL then.  Else fp32: beyond 8,192 envs from w2_x9 (the exact split) when given, else from w2_f32i; up to 8,192 envs from w2_f32i, which must
 * then be given — a non-NULL w2_x9 is accepted and ignored there, as in hx_sac_act_step.  bf16 acting beside the fp32 update has no front form.
 * The draw rule is the same at every size.  As for hx_hirl_front the
 * minibatch is drawn from the ring as it stood BEFORE this env step without the n slots the step may overwrite (HxSample.guard = n): by the previous
 * hx_sac_learn_back (its `next`: one more workgroup of the policy's gradient launch draws and gathers into next_rows) or by hx_sample_batch_guarded.
 * Bit-identical to hx_sac_act_step with the same images for the same n followed by hx_sac_learn with
 * HxSample.total read before the step and HxSample.guard = n.
 * hx_sac_learn_back = the rest of hx_sac_learn (8 launches). */
int hx_sac_front(const float* policy, const uint16_t* w2_x9, const float* w2_f32i, float* state, int64_t n, int64_t stride, float* obs_io, float* actions,
                 int32_t mode, const float* eps, uint64_t seed, uint32_t row0, uint32_t call, float* reward, uint8_t* done, int8_t* success,
                 const HxStepOpts* opts, const HxSacNets* nets, const HxSacBatch* batch, void* stream);
int hx_sac_learn_back(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, int32_t polyak_first, int32_t step, float target_entropy,
                      const HxSample* next, float* next_rows, void* stream);
int hx_sac_adam(const HxSacNets* nets, const HxHyper* hyper, int32_t which, int32_t step, float grad_scale, float target_entropy,
                void* stream);
/* SacAgent(entropy_tuning=False, ent_coef=x) (SAC/agent.py:108-110, 322-327): a constant alpha and no log-alpha optimiser — the reference then has no
 * target entropy at all, and neither has this ABI: every hx_sac_* call that takes target_entropy runs WITHOUT its log-alpha step when it is NaN
 * (hx_sac_learn, hx_sac_learn_back, hx_sac_learn_imitative, hx_sac_learn_weighted[_clipped], hx_sac_adam, hx_sac_adam_clipped; the fused weight-gradient
 * launch, adam_kernel and the weighted call's own log-alpha launch alike).  The caller stores ent_coef in alpha_state[3] and in losses[5] once:
 * alpha_state[0..3] and losses[5] are never written, losses[3] (entropy_loss) stays 0.  No launch structure changes. */
#define HX_SAC_FIXED_ALPHA (__builtin_nanf(""))

/* Gradient-norm clipping (update_params(optim, network, loss, grad_clip): SAC/utils.py:15-21, SAC/agent.py:310-320): each network's gradient is scaled
 * to a global L2 norm of at most max_norm before its Adam step, as torch.nn.utils.clip_grad_norm_ does: coef = min(1, max_norm / (norm + 1e-6)).
 * Three segments, each with its own norm: Q1 and Q2 (the two halves of grad_critic: q1_optim, q2_optim) and the policy (grad_policy).  A norm is over
 * the reference's parameter words only — W1, b1, W2, b2, W3, b3 of the block; the LayerNorm slots and the padding contribute nothing, whatever they hold.
 * ONE whole-network clip per optimizer (the reference's loop over network.modules() clips the same parameters again per sub-module: after the first
 * clip those passes scale by a factor within about 1e-6 / max_norm of 1 — DESIGN.md 5).  The log-alpha step is never clipped.
 *   hx_sac_grad_norm     one launch: workgroup c of a segment writes the sum of squares of its fixed 4,096-word chunk — a fixed order, no atomics, no
 *                        workgroup waits for another — into clip_ws (hx_sac_clip_floats() floats, 16-byte aligned)
 *   hx_sac_adam_clipped  hx_sac_adam's step on g * grad_scale * coef[segment]: every workgroup re-adds its segments' partial sums in the same fixed order
 *                        and forms the coefficient itself; coef == 1 multiplies exactly, so a max_norm that never binds gives hx_sac_adam's bits.
 *                        Keeps every live image of W2 current and (which = 1, entropy tuning on) steps log-alpha, as hx_sac_adam does.
 * clip_ws[0..2] = the norms before clipping (of g * grad_scale) of Q1, Q2 and the policy, clip_ws[3..5] = their coefficients, as of the last clipped step
 * of each; the words behind hold the partial sums.  The same gradients give the same bits on every run.
 * Sequence: hx_sac_critic_grads[_sampled], hx_sac_grad_norm(0), hx_sac_adam_clipped(0), hx_sac_policy_grads[_imitative], hx_sac_grad_norm(1),
 * hx_sac_adam_clipped(1) — the imitative branch is clipped on the combined (1 - w) dL + w dL_bc it leaves in grad_policy. */
int64_t hx_sac_clip_floats(void);
/* shape6[0..5] (host) <- the summation shape of one segment's sum of squares: float4 per thread, words per chunk, the most partials one wave re-adds,
 * the chunks of a Q segment, of the policy segment, and the depth of the whole sum in roundings (the squares included): the sum is within
 * depth * 2^-24 (relative) of the exact one — every term is non-negative */
int hx_sac_clip_shape(int32_t* shape6);
int hx_sac_grad_norm(const HxSacNets* nets, int32_t which, float* clip_ws, void* stream);
int hx_sac_adam_clipped(const HxSacNets* nets, const HxHyper* hyper, int32_t which, int32_t step, float grad_scale, float target_entropy,
                        float max_norm, float* clip_ws, void* stream);

/* SAC, imitative branch (SAC/agent.py:315-318, 353-359, 385-403; SacAgent(imitative=True)).  After the two critic steps, with the UPDATED critics:
 *     a~, H     = policy.sample(s)                          q    = min(Q1, Q2)(s, a~)
 *     a_bc      = bc_actor(s)   (frozen, no gradient)       bc_q = min(Q1, Q2)(s, a_bc)
 *     bc_weight = mean(bc_q > q)                            strict >, over the batch rows; a plain number: no gradient through it
 *     bc_loss   = mse(a_e, tanh(mean(s_e))) * 10000         on a SECOND batch of B rows from the expert memory; mean = first half of the policy head
 *     policy_loss = mean(-q - alpha H) (1 - bc_weight) + bc_loss bc_weight
 * then policy_optim.step() and the log-alpha step exactly as in the plain call.  losses[2] = the COMBINED policy loss, losses[6] = bc_loss,
 * losses[7] = bc_weight.  The gate is an INTEGER count (imit->count), so the weight does not depend on arrival order; bc_loss is a fixed-order sum.
 * Launch sequence of the policy half (+ = added to the plain call's): [policy.sample(s)] + bc_actor(s) + its tanh head; Q1 / Q2 (s, a~);
 * + Q1 / Q2 (s, a_bc) and policy(s_e); + the gate's count and the BC head gradient (zero for the four log_std outputs); + policy(s_e) backward;
 * the critics' and policy(s)'s backward as in the plain call; + the loss combination; ONE weight-gradient launch over both policy slots,
 * policy(s) scaled (1 - w) and policy(s_e) scaled w (with Adam and the log-alpha step inside it in the one call).
 * Departures from the reference: (1) it builds bc_actor with 14 inputs against the 13-wide observation and so crashes as written; here bc_actor
 * is the 13-input LayerNorm actor (hx_actor_param_count() floats, the flat actor layout) that the BC agent of this project writes, leaky slope
 * bc_slope (0.01 there); (2) which expert rows are drawn is not claimed: Philox on the device, as hx_sample_batch.  fp32 only: with
 * nets->w2_bf16_all set both entry points return an error.  One GPU. */
typedef struct HxSacImit {
    const float* bc_actor; /* the frozen BC actor's flat block */
    float* expert_rows;    /* [batch][HX_ROW_WORDS]: the second minibatch, B rows of the expert memory (s_e in columns 0..12, a_e in 13..16) */
    float* ws;             /* hx_sac_imit_workspace_floats(batch), beside HxSacNets.ws */
    int32_t* count;        /* one word: rows whose bc_q > q in the last call */
    float bc_slope;        /* leaky slope of bc_actor */
} HxSacImit;
int hx_sac_imit_sizeof(void); /* sizeof(HxSacImit) of the loaded library (hx_abi_sizes has no free word) */
int64_t hx_sac_imit_workspace_floats(int32_t batch);
/* Staged form of the imitative policy half: gradients only (grad_policy holds (1 - w) dL_rl + w dL_bc); follow with hx_sac_adam(which = 1). */
int hx_sac_policy_grads_imitative(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const HxSacImit* imit, void* stream);
/* One GPU: the whole imitative learn() in one call; its critic half is hx_sac_learn's.  expert_sample NULL: imit->expert_rows holds the expert
 * rows already; else it describes the expert memory as the main ring of an HxSample (total / cap / ring, n_main = batch, idx) and the rows are
 * drawn as hx_sample_batch draws them.  Bit-identical to hx_sac_critic_step + hx_sac_policy_grads_imitative + hx_sac_adam(which = 1). */
int hx_sac_learn_imitative(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const HxSample* sample, const HxSacImit* imit,
                           const HxSample* expert_sample, int32_t polyak_first, int32_t step, float target_entropy, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Prioritized replay (SacAgent(per=True): SAC/agent.py:112-118, 281-284, 306-331).  The reference takes `batch, indices, weights` from
 * rltorch.PrioritizedMemory, carries the per-row weights through its three losses and hands |Q1(s, a) - y| back as the new priorities.  The
 * memory class is un-vendored, so the store and the draw are THIS project's definition (the loss arithmetic is the reference's: below):
 *     stored priority  p_i = (|delta_i| + 1e-4)^alpha; 0 = the slot is not live
 *     draw             row r: target u_r S with S = sum of all priorities -> the slot whose interval of the running sum holds it: independent,
 *                      proportional to p, WITH replacement; never a slot of priority 0, never one beyond the live length
 *     weight           w_r = (n p_r / S)^-beta / max_r(.), n = min(*total, cap): the largest weight of a batch is exactly 1
 *     new rows         enter at the running maximum priority pmax (hx_per_mark_new: the default), or at a TD error of their own as the reference's
 *                      train_episode computes it for every append (hx_per_score_new: "priorities at insert" below)
 * State beside a replay ring of `cap` <= 2^24 slots, all device memory owned by the caller:
 *     prio   [hx_per_prio_floats(cap)] = cap rounded up to a multiple of 1,024, 16-byte aligned; the padding stays 0
 *     bsum   [ceil(cap / 1024)] one sum per block of 1,024 consecutive slots, always formed in one fixed order (never by float atomics):
 *            the same bits for the same prio
 *     pmax   one float: the running maximum of stored priorities (start it at 1); marked: the `total` up to which slots have been given a
 *            priority (start 0); ticket: one zeroed word the launches use among themselves
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct HxPer {
    float* prio; float* bsum; float* pmax;
    uint64_t* marked; uint32_t* ticket;
    const uint64_t* total; /* the ring's counter (HxStepOpts.total) */
    int64_t cap;
} HxPer;
int hx_per_sizeof(void); /* sizeof(HxPer) of the loaded library (hx_abi_sizes has no free word) */
int64_t hx_per_prio_floats(int64_t cap);
/* Every slot in [marked, *total) mod cap <- pmax, the touched blocks re-summed, marked <- *total; more than cap new rows: the whole ring.  One
 * launch; max_new = the caller's upper bound on the rows stored since the last call (the envs stepped) sizes its grid — if more arrived, the
 * first max_new are marked and `marked` advances by as much.  Works with the unordered slot allocation: the slots a step claims are the
 * contiguous range of `total`. */
int hx_per_mark_new(const HxPer* per, int64_t max_new, void* stream);
/* prio[slots[i]] <- p[i] (already raised to alpha; several values for one slot: the largest), blocks re-summed, pmax raised.  A pair with a
 * slot outside [0, cap) or a negative / non-finite value is skipped.  (memory.append(..., error), resume, tests) */
int hx_per_set(const HxPer* per, const int32_t* slots, const float* p, int32_t n, void* stream);
/* memory.update_priority(indices, errors) (SAC/agent.py:329-331): prio[idx[r]] <- (|errors[r]| + 1e-4)^alpha (powf); a slot drawn several times
 * keeps the MAXIMUM (unsigned atomicMax on the bits of a non-negative float: order-independent); blocks re-summed, pmax raised.  A non-finite
 * error leaves its slot as it was. */
int hx_per_update(const HxPer* per, const int32_t* idx, const float* errors, int32_t n, float alpha, void* stream);
/* every block sum again from prio (after prio was written directly: a restored snapshot) */
int hx_per_resum(const HxPer* per, void* stream);
/* memory.sample(batch_size) -> batch, indices, weights (SAC/agent.py:281-284).  One workgroup, as hx_sample_batch.  u[batch] in [0, 1] injected (u = 1, which a
 * float64 uniform below 1 can round to, is a target AT S and resolves like one that rounded to it), or NULL: Philox4x32-10(seed; row, call, a stream
 * word of its own).  The block by an inclusive scan of bsum in LDS, the slot by one wave's scan of the
 * block's 1,024 priorities; a target that rounds to S or lands on empty slots resolves to the nearest LOWER slot that holds priority.  Writes
 * idx[batch], weights[batch] (powf) and the rows into the compact tile rows[batch][HX_ROW_WORDS].  batch <= 1024.  The promise "never a slot of
 * priority 0, never one beyond the live length" needs SOME slot to hold priority: sampling while S = 0 (nothing marked or set yet) is the caller's
 * error, which the device cannot refuse — every row is then slot 0 with weight 1.  Beyond 2^23 slots the scan holds the block sums in pairs (8,192
 * entries of LDS); tests/test_per_gpu.py runs that form at 2^23 + 2,048 slots. */
int hx_per_sample(const HxPer* per, const float* ring, int32_t batch, const float* u, uint64_t seed, uint32_t call, float beta, int32_t* idx,
                  float* weights, float* rows, void* stream);
/* SacAgent.learn with per-row importance weights (SAC/agent.py:306-331, 361-374, 405, 408-414), one GPU, fp32 (with nets->w2_bf16_all set: an
 * error), on the minibatch in batch->rows:
 *     q_h_loss     = mean((Q_h(s, a) - y)^2 w)            -> losses[0..1]        errors_out[r] = |Q1(s, a) - y|_r
 *     policy_loss  = mean((-min Q(s, a~) - alpha H) w)    -> losses[2]           losses[4] = mean H, UNWEIGHTED (agent.py:351)
 *     entropy_loss = -mean(log_alpha (target_entropy - H) w) -> losses[3]; the log-alpha step takes its gradient mean(w H) - target_entropy mean(w)
 * Built from hx_sac_learn's STAGED helpers with per-row kernels of its own in between (+) — 13 launches against the one call's 9: forward (policy(s'),
 * policy(s), Q1/Q2(s, a)); Gaussian heads [+ Polyak]; target critics forward; + the weighted TD head (y, errors, both critics' head gradients);
 * critics backward (head gradient given); critics weight gradient + Adam; Q1/Q2(s, a~) forward; + weighted min(Q1, Q2) selection; critics backward;
 * + weighted policy head gradient; policy backward; policy weight gradient + Adam (without the log-alpha step); + the log-alpha step.  With weights == 1 the call is NOT
 * bit-identical to hx_sac_learn: its TD head is a per-row kernel (head_row from global memory) where the one call's is a backward prologue (head_regs
 * from an LDS image) — one formula, two instruction sequences that do not round alike.  Measured after 3 calls at B = 128: up to 1.5e-8 in parameters
 * (about 5,000 policy and 7,000 critic entries differ), one ulp in the alpha state; tests/test_per_gpu.py holds every network, Adam moment, the alpha
 * state and the acting image to bars of their own (parameters: tests/test_sac_gpu.py's bar).  The policy half and the log-alpha step are the staged
 * arithmetic on the same numbers (at w == 1, mean(w) is exactly 1 and mean(w H) has the mean entropy's bits).  step is 1-based. */
int hx_sac_learn_weighted(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const float* weights, float* errors_out,
                          int32_t polyak_first, int32_t step, float target_entropy, void* stream);
/* Priorities at insert (SAC/agent.py:198-210, 234-246: train_episode scores every transition it appends).  Every row (s, a, r, s', d) in
 * [marked, *total) mod cap — max_new as in hx_per_mark_new: the caller's bound; the first max_new are covered and `marked` advances by as much — is
 * scored with the networks AS THEY ARE when the launches run (d = the masked done the ring holds):
 *     a', H' = policy.sample(s')        one standard-normal draw per row and component
 *     y      = r + (1 - d) gamma (min(Q1_target, Q2_target)(s', a') + alpha H')        alpha = alpha_state[3], gamma = hyper->gamma
 *     error  = |Q1(s, a) - y|           prio[slot] = (error + 1e-4)^per_alpha (powf, as hx_per_update stores it)
 * A row whose error is not finite enters at pmax AS IT WAS WHEN THE CALL STARTED (where hx_per_mark_new would place it): a live slot always holds a
 * priority.  The touched blocks are re-summed in hx_per_*'s fixed order (no float atomics: the same errors give the same bsum bits), pmax is raised to
 * the largest priority stored, marked advances.  More than cap new rows: the last cap of them — all the ring still holds — are scored, which gives
 * every slot a priority, and marked <- *total; row i of the call is then the row in slot (*total + i) mod cap.
 * Only enqueues: *total and *marked are read on the device.  The range is worked through in chunks of exactly chunk_rows rows (a positive multiple of
 * 16), ceil(min(max_new, cap) / chunk_rows) of them, six launches each: the chunk's slots and its rows gathered into a tile; the forward launch of
 * policy(s') and Q1(s, a); the Gaussian head; the forward launch of target Q1 / Q2 (s', a'); the per-row TD error; the store.  Every chunk's forward
 * launches have the same shape — the last chunk is padded with a live row whose results are dropped, never shortened — because the forward kernel
 * picks its column tiling, and with it the order of its sums, from the launch shape: a row's score depends on the row, the networks, its draw and
 * chunk_rows, never on how many rows were stored with it or where in the range it falls.
 * eps [max_new][4]: the draws, row i of the call at eps[4 i ..]; NULL: Philox4x32-10(key = seed; counter = (0xC0000000 + i, call), the Gaussian
 * head's stream word) — learn() draws at rows 0x40000000 + r and 0x80000000 + r, the acting calls at env ids counted from 0: no collision for the
 * same (seed, call).  errors_out [max_new] or NULL: error of row i, written for i < the rows covered only.  ws: hx_per_score_workspace_floats(chunk_rows)
 * floats, 16-byte aligned, the caller's between calls.  fp32 only (nets->w2_bf16_all set: an error); one GPU.  Not built: bf16, scoring inside the front
 * launch, sharded ranks, the imitative / E-SAC branches, scoring with the acting kernels' formats. */
int64_t hx_per_score_workspace_floats(int32_t chunk_rows); /* 0 unless chunk_rows is a positive multiple of 16 */
int hx_per_score_new(const HxPer* per, const float* ring, const HxSacNets* nets, const HxHyper* hyper, int64_t max_new, int32_t chunk_rows,
                     float per_alpha, const float* eps /* NULL or [max_new][4] */, uint64_t seed, uint32_t call, float* ws,
                     float* errors_out /* NULL or [max_new] */, void* stream);
/* The same under gradient-norm clipping ("Gradient-norm clipping" above): its two weight-gradient launches run without Adam, each followed by
 * hx_sac_grad_norm and the clipped step (4 launches more); the log-alpha step stays the launch of its own, unclipped. */
int hx_sac_learn_weighted_clipped(const HxSacNets* nets, const HxSacBatch* batch, const HxHyper* hyper, const float* weights, float* errors_out,
                                  int32_t polyak_first, int32_t step, float target_entropy, float max_norm, float* clip_ws, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * n-step returns (SacAgent(multi_step=n): SAC/agent.py:121-124).  The reference's rltorch.MultiStepMemory is un-vendored, so the rule is THIS
 * project's definition — truncated n-step returns, no transition dropped (rltorch drops an episode's last n - 1 windows and discounts every row by
 * one scalar gamma^n; neither is done here and its bits are not claimed).  The acting launch runs WITHOUT a ring (HxStepOpts.ring = NULL);
 * hx_nstep_push behind it keeps up to n pending heads per env and writes finished rows into the ordinary ring in the ordinary 32-word format with
 * the per-row discount folded into the done column: a row of m steps has r = sum_k gamma^k r_k and (1 - d') gamma = gamma^m, so every consumer of
 * the ring (hx_sac_learn*, the samplers, hx_per_score_new) runs unchanged with the ONE-step gamma in HxHyper.
 * Per env and call, fp32 without contraction, in this order (tests/_nstep_model.py is the same in numpy, bit for bit):
 *     trunc = episode_ctr != last_ctr && !done          (the time-limit step: executed, not stored — HxStepOpts.max_step)
 *     trunc: every pending head, oldest first, leaves as (s_j, a_j, s' = obs_prev, r = acc_j, d' = 1 - boot_j); the window is cleared; no push
 *     else:  push (s = obs_prev, a = action, acc = 0, age = 0, step_success); then for every head, the new one included,
 *                w = age == 0 ? 1 : boot * gamma;  acc = acc + w * reward;  boot = w;  age += 1
 *            done: every head, oldest first, leaves with s' = obs_new and d' = 1 (that s' is the next episode's first observation under
 *                  auto_reset; it is multiplied by 1 - d' = 0), the window is cleared
 *            else, the oldest head at age n: it leaves with s' = obs_new and d' = 1 - boot
 *     obs_prev = obs_new; last_ctr = episode_ctr
 * At n = 1: w = 1, acc = 0 + r, d' = 0 or 1 — the rows hx_env_step's insert writes, apart from the s' of terminal rows (and a done ON the time-limit
 * step, which the insert drops and this rule stores as terminal).  Actions are stored as given.
 * State, all device memory owned by the caller, hx_nstep_workspace_floats(n_envs, n) 4-byte words in all:
 *     win       [HX_NSTEP_FIELDS][n][n_envs]  field-major, then head position, then env: s[13] a[4] acc boot step_success(as a float); a head's
 *               age is not stored — heads enter one per stored step, so head j of `count` (oldest = 0) has age count - j
 *     hc        [n_envs]  position of the oldest head (bits 0-7) | pending heads << 8 (0 .. n - 1 between calls): a circular index, nothing moves
 *     obs_prev  [13][n_envs]      last_ctr  [n_envs]
 * ------------------------------------------------------------------------------------------------------------ */
#define HX_NSTEP_MAX 8
#define HX_NSTEP_FIELDS 20
typedef struct HxNStep {
    float* win; uint32_t* hc; float* obs_prev; uint32_t* last_ctr;
    int64_t n_envs;
    int32_t n;   /* 1 .. HX_NSTEP_MAX */
    float gamma; /* the one-step discount, HxHyper.gamma */
} HxNStep;
int hx_nstep_sizeof(void); /* sizeof(HxNStep) of the loaded library (hx_abi_sizes has no free word) */
int64_t hx_nstep_workspace_floats(int64_t n_envs, int32_t n); /* 0 for n outside 1 .. HX_NSTEP_MAX or n_envs <= 0 */
/* after env.reset(): every window empty (win zeroed), obs_prev <- obs [n_envs][13], last_ctr <- episode_ctr */
int hx_nstep_reset(const HxNStep* ns, const float* obs, const uint32_t* episode_ctr, void* stream);
/* One step of every env, exactly as an acting launch or hx_env_step left it: obs_new [n_envs][13] (16-byte aligned), actions [n_envs][4], reward,
 * done, success, episode_ctr [n_envs].  One launch, one env per lane, 64 envs per workgroup.  Ring slots as hx_env_step's insert claims them: the
 * workgroup's rows are counted (a prefix over its lanes), ONE atomicAdd on *total per workgroup, rows laid out by env, then oldest head first, and
 * written as whole 128-byte lines; with one workgroup (n_envs <= 64) the slot order is therefore the same for the same inputs, beyond that it
 * depends on the order in which workgroups reach the counter.  No workgroup waits for another, no float atomics.  One call can emit n * n_envs
 * rows: cap >= n * n_envs (and < 2^31).  ring_success may be NULL.  Enqueues only. */
int hx_nstep_push(const HxNStep* ns, const float* obs_new, const float* actions, const float* reward, const uint8_t* done, const int8_t* success,
                  const uint32_t* episode_ctr, float* ring, int8_t* ring_success, int64_t cap, uint64_t* total, void* stream);
/* n-step returns for a labelled expert table (HIRL / TD3 on n-step rows, a declared extension: HirlEngine.set_multi_step, train_all --hirl_multi_step).
 * rows_in [E][32]: what hx_label_transitions leaves once the reference's pairs have been picked (train_all.label_expert) — one-step rows in recording
 * order, done exactly 0 or 1, and within a segment row j + 1 starts where row j ended.  last[j] != 0 marks the final row of a segment: a terminal row,
 * the last row of a file, or the row in front of any gap.  Per row j, fp32 without contraction, in this order — the fold a head performs in
 * hx_nstep_push (tests/_nstep_label_model.py is the same in numpy, bit for bit):
 *     m = min(n, rows from j to the end of j's segment, inclusive)
 *     acc = 0; boot = 1;  for k = 0 .. m - 1:  w = k == 0 ? 1 : boot * gamma;  acc = acc + w * r[j + k];  boot = w
 *     rows_out[j] = (s_j, a_j, s' = s'[j + m - 1], r = acc, d' = done[j + m - 1] ? 1 : 1 - boot)
 * Row j stays row j, so success bytes, fire-row indices and an expert ring's layout stay valid; a terminal row keeps its recorded s' (it is multiplied
 * by 1 - d' = 0).  At n = 1 the output equals the input in value (0 + r turns a -0 reward into +0).  One launch, one row per lane, 64 rows per
 * workgroup, rows written as whole 128-byte lines; a row's gathers reach up to n - 1 rows past its workgroup's last row, never past E and never past a
 * `last` row.  No atomics, no workgroup waits for another.  rows_in and rows_out 16-byte aligned; rows_out must not overlap rows_in.  n in
 * 1 .. HX_NSTEP_MAX, 0 < E < 2^31, gamma in [0, 1].  Enqueues only. */
int hx_nstep_label(const float* rows_in, const uint8_t* last, int64_t E, int32_t n, float gamma, float* rows_out, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Episode record (validate() with --plot: train_all.py:22-102, train_sac.py:24-91).  The reference collects the last validation episode's track on
 * the host, one get_pos() per step_test; here the state stays on the device and validation steps all its episodes in one launch, so a launch of its
 * own behind every env step appends to a device log and latches what the reference reads when it SEES done.  k tracked envs (env_ids, or envs
 * 0..k-1), steps t = 0, 1, ... < cap_steps.  Rule per tracked env j at hx_trace_push(t) (tests/_trace_model.py is the same in numpy, bit for bit):
 *     end_step[j] >= 0: nothing is written — the kernels keep simulating an env after its done, and everything after the first done stays out of
 *                       the record and out of the score
 *     else:  log[.][t][j] <- the eight words below;  total = total + reward (fp32, step order);  launches += success != 0;  hits += success == 1;
 *            nrec = t + 1;  done != 0: end_step = t, end_flags = the flags word, the env leaves `alive`
 * The step that raises done IS recorded (the reference appends before it looks at done, train_all.py:38-57).  An id outside [0, n) records nothing.
 * State, all device memory owned by the caller, hx_trace_workspace_words(k, cap_steps) 4-byte words in all:
 *     log       [HX_TRACE_FIELDS][cap_steps][k]  field-major, then step, then tracked env: 0..2 ally position (state words 0..2), 3..5 opponent
 *               position (state words 13..15), 6 reward, 7 bits 0..15 of the flags word (state word 35) | (uint8)success << 16; the words are copied
 *               as bits; hx_trace_reset does not clear it (nrec says how much of it holds)
 *     total (fp32), nrec, end_step (-1: running), end_flags (u32), launches, hits   [k] each, in this order behind the log
 *     alive     [1]  tracked envs whose episode is still running: the host's early exit reads this one word
 * ------------------------------------------------------------------------------------------------------------ */
#define HX_TRACE_FIELDS 8
#define HX_TRACE_SUMMARIES 6
typedef struct HxTrace {
    uint32_t* log;
    float* total; int32_t* nrec; int32_t* end_step; uint32_t* end_flags; int32_t* launches; int32_t* hits;
    int32_t* alive;
    int64_t k;
    int32_t cap_steps;
} HxTrace;
int hx_trace_sizeof(void); /* sizeof(HxTrace) of the loaded library */
int64_t hx_trace_workspace_words(int64_t k, int32_t cap_steps); /* 0 for k <= 0 (or >= 2^31) or cap_steps <= 0 */
/* every summary zero, end_step = -1, alive = k */
int hx_trace_reset(const HxTrace* tr, void* stream);
/* Step t of every tracked env, from the env's buffers exactly as hx_env_step or an acting launch left them: state (word w of env i at
 * state[w * stride + i]), reward, done, success [n]; env_ids: k device ints, or NULL = envs 0..k-1 (then k <= n).  One launch, one tracked env per
 * lane, 64 per workgroup; at most one integer atomic per wave (alive -= the wave's ending lanes), no float atomics, no workgroup waits for another.
 * t < 0 or t >= cap_steps: HX_ERR_ARG, nothing is launched.  Enqueues only. */
int hx_trace_push(const HxTrace* tr, const float* state, int64_t n, int64_t stride, const float* reward, const uint8_t* done, const int8_t* success,
                  const int32_t* env_ids, int32_t t, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Episode statistics (the reference's totalReward and step of a training episode, train_all.py:341-354, 383-385), binned by scenario: what a mixed
 * population (per-env scenario ids, hx_env_reset) needs to tell which manoeuvre the policy fails.  AUTO-RESET ENVS ONLY: the rule reads an episode's
 * end off done and off episode_ctr moving, which is what an acting launch with HxStepOpts.auto_reset = 1 leaves.  hx_epstat_push runs behind every
 * acting launch (a front launch or hx_env_step).  Per env and call, fp32 without contraction, in this order (tests/_epstat_model.py is the same in
 * numpy, bit for bit):
 *     bin   = (flags word, state word 35, >> 8) & 3        (the scenario id survives every auto-reset)
 *     fire_good[bin] += success == +1;  fire_bad[bin] += success == -1        (every executed step, the time-limit step too)
 *     trunc = episode_ctr != last_ctr && !done             (the time-limit step: executed, not stored — HxStepOpts.max_step)
 *     trunc: the episode leaves with (acc, len) as they are — the reference breaks before `totalReward += reward` on that step
 *            (train_all.py:346-354), so its reward is not in the return
 *     else:  acc = acc + reward;  len += 1;  done: the episode leaves           (a done ON the time-limit step is a done: n_done)
 *     an episode that leaves adds to its bin count, n_done or n_time_limit, sum_len, sum_ret, sum_ret_sq, min_ret, max_ret; then acc = 0, len = 0
 *     last_ctr = episode_ctr
 * Kills cannot be attributed here: HX_F_EPISODE_SUCCESS is cleared by the auto-reset inside the same acting launch, before this launch reads the
 * flags word.  Per-scenario kill rates come from validation.
 * Accumulation: workgroup g (envs 64 g .. 64 g + 63, the same on every call) owns slot g of `part` and adds the call's contribution to it: for each
 * word of the slot, c = 0, then the lanes of that bin in lane order 0..63 (c = c + value), then word = word + c.  Sums are float64 (return and
 * return squared are the fp32 return widened first; the counts are exact integers held as float64), min / max are fp32 and start at +inf / -inf.
 * No atomics, no workgroup waits for another, the same inputs give the same bits.  The host reads `part` and adds the slots in index order.
 * State, all device memory owned by the caller, hx_epstat_workspace_words(n_envs) 4-byte words in all, in this order:
 *     part      [ceil(n_envs / 64)][HX_EPSTAT_SLOT_WORDS] 8-byte words (8-byte aligned).  Words 0..31 of a slot: [bin][HX_EPSTAT_SUMS] float64 —
 *               count, n_done, n_time_limit, sum_len, sum_ret, sum_ret_sq, fire_good, fire_bad; words 32..35: [bin] min_ret (low half) and
 *               max_ret (high half) as fp32
 *     acc (fp32), len (u32), last_ctr (u32)   [n_envs] each
 * ------------------------------------------------------------------------------------------------------------ */
#define HX_EPSTAT_BINS 4
#define HX_EPSTAT_SUMS 8
#define HX_EPSTAT_SLOT_WORDS 36
typedef struct HxEpStat {
    double* part;
    float* acc; uint32_t* len; uint32_t* last_ctr;
    int64_t n_envs;
} HxEpStat;
int hx_epstat_sizeof(void); /* sizeof(HxEpStat) of the loaded library */
int64_t hx_epstat_workspace_words(int64_t n_envs); /* 0 for n_envs <= 0 (or >= 2^31) */
/* after env.reset(): every slot cleared, acc = 0, len = 0, last_ctr <- episode_ctr [n_envs] */
int hx_epstat_reset(const HxEpStat* es, const uint32_t* episode_ctr, void* stream);
/* the partial sums only (sums 0, min +inf, max -inf): the host has read them; running episodes keep their acc, len and last_ctr */
int hx_epstat_clear(const HxEpStat* es, void* stream);
/* One step of every env, from the env's buffers exactly as an acting launch or hx_env_step left them: state (word w of env i at
 * state[w * stride + i]; only word 35 is read), reward, done, success, episode_ctr [n], n = n_envs.  One launch, one env per lane, 64 per
 * workgroup; plain vector stores, each one contiguous run per wave.  Enqueues only. */
int hx_epstat_push(const HxEpStat* es, const float* state, int64_t n, int64_t stride, const float* reward, const uint8_t* done, const int8_t* success,
                   const uint32_t* episode_ctr, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Success upsampling (the reference's buffer_upsample and expert_upsample switches: HIRL.py:184-185, 189, 217-219, 253-257; buffer.py:18-29,
 * 39-43; BC.py:152-158, 171-176).  UniformMemory(upsample=True) stores priority 1.0 for a transition whose step_success == 1 and 0.1 for every
 * other and draws np.random.choice(len, B, p = priorities / sum): proportional, with replacement, no importance weights.  Here the weights are
 * INTEGERS — `boost` (default 10) for a success row, 1 for any other, the same distribution — so every sum is an exact count: no float
 * arithmetic, the same labels and random words give the same indices on any run.
 *     live length   n = min(*total, cap)
 *     weight        slot i < n: boost if ring_success[i] == 1, else 1;  slot i >= n: 0, whatever stale label it holds
 *     W             = n + (boost - 1) sum(cnt)                                   (fits 32 bits: cap <= 2^24, boost <= 255)
 *     draw          row r takes a 64-bit word x_r -> target t = (x_r W) >> 64, an integer in [0, W) -> the slot whose interval of the
 *                   running integer weight holds t: independent draws, WITH replacement (tests/_upsample_model.py is the same in Python integers)
 * State beside a replay ring of `cap` <= 2^24 slots, all device memory owned by the caller:
 *     cnt    [hx_ups_words(cap)] = ceil(cap / 1024) uint32: the live slots of each block of 1,024 consecutive slots whose label is exactly 1
 *     marked one uint64: the `total` up to which the counts are current (start 0)
 * ring_success is HxStepOpts.ring_success, cap bytes, 16-byte aligned; nothing behind cap is read.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct HxUps {
    uint32_t* cnt;
    uint64_t* marked;
    const uint64_t* total;      /* the ring's counter (HxStepOpts.total) */
    const int8_t* ring_success; /* the labels beside the ring (HxStepOpts.ring_success) */
    int64_t cap;
    int32_t boost;              /* 2 .. 255: the weight of a success row against 1; 10 = the reference's 1.0 : 0.1 */
} HxUps;
int hx_ups_sizeof(void); /* sizeof(HxUps) of the loaded library (hx_abi_sizes has no free word) */
int64_t hx_ups_words(int64_t cap); /* ceil(cap / 1024); 0 for cap <= 0 or cap > 2^24 */
/* Every block touched by the slots of [marked, *total) mod cap is RECOUNTED from the labels, masked by the live length (so slots overwritten
 * after the ring wrapped are handled by construction), then marked advances.  max_new = the caller's upper bound on the rows stored since the
 * last call; if more arrived, the first max_new are covered and `marked` advances by as much; cap or more rows to cover: the whole ring, and
 * marked <- *total.  One launch of ONE workgroup: each of its 16 waves takes one touched block at a time (16 bytes of labels per lane, ballot /
 * popcount), and the workgroup's barrier stands between every wave's read of `marked` and the one store to it — with one workgroup per block
 * that store would need a ticket atomic or a launch of its own.  No atomics, nothing waits.  Enqueues only. */
int hx_ups_mark_new(const HxUps* ups, int64_t max_new, void* stream);
/* every block again from the labels, marked <- *total (a restored snapshot, labels written directly, tests); one wave per block */
int hx_ups_recount(const HxUps* ups, void* stream);
/* The draw, ONE workgroup (as hx_per_sample and hx_sample_batch), behind a plain hx_sample_batch over the same tiles:
 *   rows r < n_main: x_r = x[r] when x is given, else the Philox4x32-10 words 0 (high half) and 1 (low half) of (key = seed; counter = (r, call,
 *     a stream word of its own, 0)).  The block by binary search in an inclusive scan of the block weights live_in_block + (boost - 1) cnt held
 *     in LDS (beyond 2^23 slots in pairs, as hx_per_sample holds its sums), the slot by one wave's scan of the block's 1,024 labels.
 *     idx[r] <- the slot, rows[r] <- ring[slot] (whole 128-byte rows).  Rows [n_main, batch) of idx and rows are NOT touched.
 *   fire_idx [n_fire] given (n_fire > 0): j = (w0 n_fire) >> 64, k = (w1 batch) >> 64 with w0 = x[n_main], w1 = x[n_main + 1] when x is given
 *     (x then holds n_main + 2 words), else words (0, 1) and (2, 3) of Philox(seed; (0xFFFFFFF1, call, the stream word, 0));
 *     idx_bc[k] <- fire_idx[j], bc_rows[k] <- bc_table[fire_idx[j]] (the reference replaces ONE row of the BC minibatch by a fire row).  Every
 *     entry of fire_idx must index bc_table: the caller's promise.  ups may be NULL with n_main = 0: the BC replacement alone.
 * batch <= 1024, 0 <= n_main <= batch.  Drawing while W == 0 (an empty ring) is the caller's error, which the device cannot refuse: every row
 * is then slot 0.  If the counts are stale (rows stored since the last hx_ups_mark_new) a target can pass the end of its block's labels: it
 * resolves to the block's last live slot, never to a slot beyond the live length. */
int hx_ups_draw(const HxUps* ups, const float* ring, int32_t batch, int32_t n_main, const uint64_t* x, uint64_t seed, uint32_t call, int32_t* idx,
                float* rows, const int32_t* fire_idx, int32_t n_fire, const float* bc_table, int32_t* idx_bc, float* bc_rows, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The pilot as a kernel (an EXTENSION: the reference's expert is Harfang's IA inside an external simulator and can only be replayed from
 * recordings).  data/expert_pilot.py pursuit_actions, the scripted pursuit law the expert CSVs of this build are flown by, on the state words in
 * HBM — so the expert can label the states the learner reaches (dataset aggregation).  Per env, fp32 without contraction, correctly rounded divide
 * and square root, in this order (tests/_pilot_model.py is the same in numpy, bit for bit):
 *     w, x, y, z = state words 6..9;  d_i = state[13 + i] - state[i], i = 0..2
 *     rows of R^T:  ax = (1 - 2 (yy + zz), 2 (xy + wz), 2 (xz - wy))
 *                   ay = (2 (xy - wz), 1 - 2 (xx + zz), 2 (yz + wx))
 *                   az = (2 (xz + wy), 2 (yz - wx), 1 - 2 (xx + yy))
 *     b_r = (r0 d0 + r1 d1) + r2 d2 for r = ax, ay, az;  nrm = sqrt((b0 b0 + b1 b1) + b2 b2);  nrm < 1e-6: nrm = 1e-6 (a comparison: NaN stays NaN)
 *     levels = (-4 (b1 / nrm), -2 (b0 / nrm), 4 (b0 / nrm)), + noise[i][0..2] when given, each clamped to [-1, 1] by comparisons
 *     fire = +1 iff obs[7] > 0 && obs[8] > 0 (locked, and the missile still on the rail), else -1
 * ------------------------------------------------------------------------------------------------------------ */
/* actions[i] <- (levels, fire) of env i, i < n: state as hx_env_step leaves it (word w of env i at state[w * stride + i]), obs [n][13], noise NULL or
 * [n][3] (already scaled), actions [n][4], 16-byte aligned.  One env per lane, 64 per workgroup; every state word one contiguous run per wave, one
 * 16-byte store per lane.  Enqueues only. */
int hx_pilot_act(const float* state, int64_t n, int64_t stride, const float* obs, const float* noise, float* actions, void* stream);
/* The online region of a BC table [offline_rows + online_rows][HX_ROW_WORDS]: behind an acting launch, k = per_call envs are relabelled by the pilot and
 * stored over the oldest online rows.  For j in [0, k):
 *     env   e_j  = (call + j floor(n / k)) mod n            (k distinct envs spread over the population; the window moves by one env per call)
 *     slot       = offline_rows + ((call k + j) mod M)      (M = online_rows; exact for every 64-bit call: FIFO over the online region)
 *     row        = obs[e_j] (words 0..12), the pilot's NOISE-FREE action (13..16), zeros (17..31), written as one whole 128-byte line
 *     a row with a non-finite word among its 17 is NOT written: the slot keeps what it had
 * Rows [0, offline_rows) are never touched.  1 <= k <= min(n, M), table 128-byte aligned, else HX_ERR_ARG and nothing is launched.  Between launches
 * every slot holds a complete row.  No atomics, no workgroup waits for another.  Enqueues only. */
int hx_pilot_refresh(const float* state, int64_t n, int64_t stride, const float* obs, float* table, int64_t offline_rows, int64_t online_rows,
                     int32_t per_call, uint64_t call, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Expert branches (an EXTENSION beside the online region of the BC table above: that one holds (s, a) rows, this one full transitions).  The
 * labelled expert ring [offline_rows + online_rows][HX_ROW_WORDS] with its step_success bytes [offline_rows + online_rows] is what HIRL's expert
 * rows, E-SAC's expert rows and ISAC's expert batch are drawn from.  Behind an acting launch, k = per_call envs are each flown ONE step under the
 * pilot's action, in registers, and that branch is stored over the oldest online rows.  For pick j in [0, k), M = online_rows:
 *     env   e_j  = (call + j floor(n / k)) mod n            (hx_pilot_refresh's picks)
 *     slot       = offline_rows + ((call k + j) mod M)      (hx_pilot_refresh's slots; both exact for every 64-bit call, formed from residues)
 *     s          = obs[e_j]: the stored observation, what the learner saw
 *     a_E        = the pilot's NOISE-FREE action on the state words of env e_j ("The pilot as a kernel"), clamped by comparisons,
 *                  fire = +1 iff s[7] > 0 && s[8] > 0, else -1
 *     one step   = the env state of e_j is loaded and stepped under a_E exactly as hx_env_step steps it: scripted opponent, the latches taken
 *                  BEFORE the action, missile launch and tick, lock update, the wrapper's observation / reward / termination, the Euler entries.
 *                  Left out: auto-reset and the time-limit rule (the branch ends nobody's episode), the env's own ring insert, the statistics.
 *                  NOTHING is stored back to `state` or `obs`.
 *     row        = [s 0..12 | a_E 13..16 | s' 17..29 | r 30 | done 31] (the replay row's column order), s' assembled as hx_env_step assembles its
 *                  next observation, r the step's reward, done 1.0 or 0.0 (the env's own _get_reward / _get_termination, NOT hx_label_transitions'
 *                  get_reward: the altitude penalties and the fire-success latch are in it); written as one whole 128-byte line
 *     success[slot] = the step's step_success, -1 / 0 / +1
 *     if any of the 32 words is not finite, neither the row nor the byte is written: the slot keeps what it had
 * Rows [0, offline_rows) and success[0 .. offline_rows) are never touched.  1 <= k <= min(n, M), ring 128-byte aligned, fewer than 2^31 rows in
 * all, 0 < n < 2^31, stride >= n, else HX_ERR_ARG and nothing is launched.  Between launches every slot holds a complete row.  One pick per lane, 64
 * per workgroup; no atomics, no workgroup waits for another.  tests/_branch_model.py is the same rule on the CPU, bit for bit.  Enqueues only.
 * ------------------------------------------------------------------------------------------------------------ */
int hx_pilot_branch(const float* state, int64_t n, int64_t stride, const float* obs, float* ring, int8_t* success, int64_t offline_rows,
                    int64_t online_rows, int32_t per_call, uint64_t call, void* stream);
/* Branches of up to H = max_steps steps, as a conveyor: the k = per_call branches stay RESIDENT in a device workspace, every call advances each of
 * them ONE step and writes that step's row by the rule above, and a branch that has ended is reseeded from the population on the next call.  The
 * cost of a call is hx_pilot_branch's plus one coalesced load and store of 50 words per lane, whatever H is; the rows of one pilot flight reach the
 * ring one per call.
 * Workspace (part of the ABI): struct-of-arrays over branches, kpad = k rounded up to 64 columns, hx_branch_workspace_bytes(k) = 228 kpad bytes:
 *     float    bstate[37][kpad]     the branch's env state, word w of branch j at bstate[w kpad + j] ("Env state layout")
 *     float    bobs[13][kpad]       the observation the branch's pilot fires on: the s' of its last step
 *     uint32_t age[kpad]            steps flown by the resident flight; 0: not resident, the next call seeds it
 *     uint64_t counters[3][kpad]    per lane: rows written, rows written with done = 1, kills
 * The caller zeroes it once (age = 0 everywhere) and passes work_stride = kpad.  For lane j < k at call c:
 *     source     age[j] == 0: seeded from env e_j = (c + j floor(n / k)) mod n, its state and stored observation gathered as above;
 *                otherwise the state and observation of workspace column j
 *     step       a_E = the pilot's noise-free action on the source's state words, fire = +1 iff s[7] > 0 && s[8] > 0; one env step as above;
 *                row = [s | a_E | s' | r | done]
 *     write      all 32 words finite: the row and its step_success byte go to slot offline_rows + ((c k + j) mod M), as above; otherwise nothing
 *     advance    row written, done == 0 and age[j] + 1 < max_steps: the stepped state and s' go to column j, age[j] += 1;
 *                otherwise age[j] = 0, the column is left as it is, and the next call reseeds
 *     episode    no time limit, no auto-reset; done is the env's own termination; the opponent's script runs on from the counters the branch carries
 *     counters   rows written += 1; with done: rows with done += 1; with done, health < 0.1f and the fire-success latch set (the comparison the
 *                reward's +600 is paid on): kills += 1.  Each lane adds to its own words.
 * max_steps == 1 is hx_pilot_branch: the same bits in ring and bytes, bstate / bobs / age neither read nor written, only the counters move.
 * `state` and `obs` are read-only.  Columns >= k are never touched.  1 <= max_steps <= 65,535 (the episode counter's range), work 16-byte aligned,
 * work_stride == kpad, the other arguments as hx_pilot_branch, else HX_ERR_ARG and nothing is launched.  No atomics, no workgroup waits for
 * another.  tests/_branch_steps_model.py is the same rule on the CPU, bit for bit.  Enqueues only. */
int64_t hx_branch_workspace_bytes(int32_t per_call);  /* 0 for per_call < 1 */
int hx_pilot_branch_steps(const float* state, int64_t n, int64_t stride, const float* obs, float* ring, int8_t* success, int64_t offline_rows,
                          int64_t online_rows, int32_t per_call, int32_t max_steps, uint64_t call, void* work, int64_t work_stride, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Self-imitation (an EXTENSION beside the expert branches above, after Oh et al. 2018: the rows above are all the scripted pilot's actions, these are
 * the LEARNER's own, taken from the episodes it won).  An episode tape keeps the last L executed steps of every env.  One hx_self_push follows every
 * acting launch (a front launch or hx_env_step) and reads the buffers as that launch left them: obs_new [n][13], actions [n][4], reward, done, success,
 * episode_ctr [n]; envs are auto-reset, as for hx_epstat_push.  Per env and call, in this order (tests/_selfimit_model.py is the same in numpy, rows
 * as bit patterns):
 *     trunc = episode_ctr != last_ctr && !done      (the time-limit step: executed, not stored; hx_nstep_push's rule)
 *     trunc: len = 0, nothing recorded
 *     else:  record (s = obs_prev, a = action as given, r = reward, step_success) as the episode's newest step;  len = min(len + 1, L)
 *            done: kill = reward > 0;  a kill episode EMITS its m = len recorded steps, oldest first;  len = 0 either way
 *     obs_prev = obs_new;  last_ctr = episode_ctr
 * The kill test is reward > 0 on the done step: every term of the env's reward is <= 0 except the +600 paid on health < 0.1f with the fire-success
 * latch set (hx_env_dev.h), the comparison hx_pilot_branch_steps counts its kills on; HX_F_EPISODE_SUCCESS itself is gone by the time a trailing launch
 * runs (see hx_epstat_push).  The negative terms are bounded by 1e-4 dist + 30, so the identification holds for dist < 5.7e6 m.
 * Emitted row j of an episode is [s_j | a_j | s'_j | r_j | done_j] in the replay row's column order: s'_j = s_{j+1} for every row but the last, whose
 * s' is obs_new as found (under auto-reset the next episode's first observation, multiplied by 1 - done = 0: hx_nstep_push's convention); done is 1.0 on
 * the last row and 0.0 before it; the row's step_success byte comes from the tape.
 * Destination: the online region of the labelled expert ring, [offline_rows + M][32] + success bytes, M = online_rows.  A 64-bit device cursor
 * drives the slots: the k-th row accepted by a call goes to slot offline_rows + ((cursor + k) mod M) — the sum taken exactly, so the slots of one call
 * are distinct for EVERY cursor value —, then cursor = (cursor + accepted) mod 2^64.  Order within a call: kill envs in ascending env index, each
 * episode oldest row first.  Overflow: with P_e the rows of all kill episodes of this call up to and including env e, env e's episode is accepted iff
 * P_e <= M, else dropped whole: acceptance is a function of the prefix alone and the accepted episodes form a leading run.  A row with a non-finite
 * word among its 32 is written nowhere: its slot keeps what it had, the cursor still advances (hx_pilot_branch's rule).  Rows [0, offline_rows) are
 * never touched; between launches every slot holds a complete row.  bc_table: NULL, or [bc_offline_rows + M][32]: the same accepted rows go to
 * bc_offline_rows + ((cursor + k) mod M) as (s, a, zeros), hx_pilot_refresh's row format.
 * Workspace `work` (part of the ABI; one pointer, carved by the library as hx_pilot_branch_steps carves its own: no struct crosses the boundary),
 * caller-owned device memory of hx_self_workspace_words(n, L) 4-byte words, 16-byte aligned — the caller states that count as work_words and a call
 * whose work_words is not hx_self_workspace_words(n_envs, L) is refused, so a wrong (n_envs, L) pair cannot write outside the buffer —, G = ceil(n / 64) groups,
 * Gp = G rounded up to even, in this order:
 *     float    tape[L][HX_SELF_FIELDS][n]   indexed by the CALL: the step of call c lies at position c mod L, fields s[13] a[4] r step_success (as a
 *                                           float); an env's episode is the last len positions ending at the current one
 *     float    obs_prev[13][n]
 *     uint32_t len[n]  last_ctr[n]  klen[n] klen: rows the env emits in the current call, 0 if none
 *     uint32_t wcount[Gp]  wkills[Gp]       per 64-env group: the sum of klen, and the number of kill episodes
 *     (one pad word if the count so far is odd)
 *     uint64_t cursor[2]                    double-buffered by call parity: call c reads cursor[c & 1] and writes cursor[(c + 1) & 1]
 *     uint64_t counters[HX_SELF_COUNTERS][G]  per group, each word added to by its group alone; a statistic is the SUM over the groups:
 *                                           kills seen, episodes written (accepted), rows written (non-finite rows left out), episodes dropped
 * Two launches per call.  record: one env per lane, 64 per workgroup, updates the tape and stores klen / wcount / wkills.  flush: one workgroup per
 * group; wcount[g] == 0 leaves after one load; the others add wcount[0 .. g), take the lane prefix of klen, apply the acceptance rule and copy, 8
 * lanes per row, whole 128-byte lines.  The same inputs give the same bits in ring, bytes, table, cursor and counters at every n, however workgroups
 * are scheduled: no atomics of any kind, no workgroup waits for another, no workgroup reads a word that another writes in the same launch.
 * `call` must advance by one per push (it selects the tape position and the cursor's parity); 1 <= L <= HX_SELF_MAX_STEPS, L <= M, 0 < n < 2^31,
 * fewer than 2^31 rows in ring and table, ring and table 128-byte aligned, obs_new and actions 16-byte aligned, else HX_ERR_ARG and nothing is
 * launched.  hx_self_reset (after env.reset(), and after a snapshot came back: the tape is not part of one) zeroes tape, len, klen, wcount and
 * wkills and sets obs_prev <- obs, last_ctr <- episode_ctr; it leaves cursor and counters alone.  Both enqueue only.
 * ------------------------------------------------------------------------------------------------------------ */
#define HX_SELF_FIELDS 19
#define HX_SELF_MAX_STEPS 65535
#define HX_SELF_COUNTERS 4
#define HX_SELF_KILLS 0
#define HX_SELF_EPISODES 1
#define HX_SELF_ROWS 2
#define HX_SELF_DROPPED 3
int64_t hx_self_workspace_words(int64_t n_envs, int32_t L); /* 0 for L outside 1 .. HX_SELF_MAX_STEPS or n_envs outside (0, 2^31) */
int hx_self_reset(void* work, int64_t work_words, int64_t n_envs, int32_t L, const float* obs, const uint32_t* episode_ctr, void* stream);
int hx_self_push(void* work, int64_t work_words, int64_t n_envs, int32_t L, const float* obs_new, const float* actions, const float* reward, const uint8_t* done, const int8_t* success,
                 const uint32_t* episode_ctr, float* ring, int8_t* ring_success, int64_t offline_rows, int64_t online_rows, float* bc_table,
                 int64_t bc_offline_rows, uint64_t call, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exploration noise (hx_noise.hip): temporally correlated action noise for the per-row noise input of the acting kernels (noise_mode 2 of
 * hx_actor_act / hx_actor_act_step / hx_hirl_front, the Gaussian head's eps of hx_sac_act / hx_sac_act_step).  An extension: the reference draws white
 * Gaussian noise (chooseAction, HIRL.py:192-212).  Per env i and action component c a bank of `poles` (1 .. HX_NOISE_MAX_POLES) stationary AR(1)
 * processes, every coefficient from the host; per vector step t, all in fp32:
 *     z[k] <- a[k] * z[k] + b[k] * eps[k]        one product, one product, one sum, each rounded: no fused multiply-add
 *     x    <- ((w[0] * z[0]) + w[1] * z[1]) + ...  k ascending, every product rounded, then added
 *     out[t][i][c] = s_i * x                       s_i = sigma_env[i] if sigma_env is given, else sigma
 * With b[k] = sqrt(1 - a[k]^2) and sum w[k]^2 = 1 every z[k] and x has unit variance, so sigma means what the acting kernels' own sigma means.  poles = 1
 * with a = exp(-1 / tau) is Ornstein-Uhlenbeck noise, poles = K with a[k] = exp(-2^-k), w[k] = 1 / sqrt(K) approximates a 1 / f spectrum between
 * 1 / (2 pi 2^(K - 1)) and 1 / (2 pi) cycles per step, a = 0 is white noise: the library knows a, b, w alone, the colours are the caller's recipes
 * (hirl4ucav_amd/utils/noise.py; the rule in numpy: tests/_noise_model.py).
 *   z        [poles][4][n_envs] device floats (hx_noise_workspace_floats of them): the state, struct-of-arrays over envs
 *   coef     [3][HX_NOISE_MAX_POLES] HOST floats: a | b | w, the first `poles` of each row are read
 *   out      [steps][n_envs][4]: out[t] is the [n, 4] tensor of vector step step0 + t
 *   eps_in   [steps][poles][n_envs][4] standard-normal draws, or NULL: Philox4x32-10, key = seed, counter (row0 + i, lo32(step0 + t), hi32(step0 + t),
 *            0x4E4F4900 | k); the four words go through u01 and Box-Muller as the acting kernels' draws do (cos / sin per pair), so one Philox call gives
 *            one pole's four components.  The acting kernels' counters have 0 in the fourth word: no draw is shared.
 *   eps_out  the same shape or NULL: receives the draws that were USED, whichever source they came from
 *   row0     the env id of env 0 (HxStepOpts.env_id0): a shard's envs draw what they would draw in one population
 * hx_noise_init: z <- N(0, 1) from the counter (row0 + i, 0, 0, 0x4E4F4980 | k) — the stationary law, so the first step is coloured already.  Episodes
 * do NOT reset z: a stationary process continued across an auto-reset is, for the new episode, a stationary draw.  hx_noise_fill advances z by `steps`
 * (1 .. HX_NOISE_MAX_STEPS) steps in ONE launch: one env per lane, the 4 poles words of an env in registers, no atomics, no workgroup waits for another,
 * the same inputs give the same bits; fills of s1 + s2 steps equal one fill of s1 + s2.  poles or steps out of range, n_envs <= 0 or >= 2^31, a NULL z,
 * out or coef, an out / eps_in / eps_out that is not 16-byte aligned, an a[k] outside [0, 1), a non-finite a, b, w or sigma: HX_ERR_ARG and nothing is
 * launched.  Both enqueue only.  (The arguments are scalars and plain pointers, no struct: the binding's header reader takes no array fields.)
 * ------------------------------------------------------------------------------------------------------------ */
#define HX_NOISE_MAX_POLES 8
#define HX_NOISE_MAX_STEPS 64
int64_t hx_noise_workspace_floats(int64_t n_envs, int32_t poles); /* 4 poles n_envs; 0 for poles outside 1 .. HX_NOISE_MAX_POLES or n_envs outside (0, 2^31) */
int hx_noise_init(float* z, int64_t n_envs, int32_t poles, uint64_t seed, uint32_t row0, void* stream);
int hx_noise_fill(float* z, const float* sigma_env, int64_t n_envs, int32_t poles, float sigma, const float* coef /* host */, uint64_t seed, uint32_t row0,
                  uint64_t step0, int32_t steps, float* out, const float* eps_in, float* eps_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exchange step of a sharded update without a collective library (selectable beside RCCL): one-shot all-reduce over hipIpc peer
 * mappings (hx_xchg.hip).  The reference has no counterpart (single process); SURVEY.md 5 / 8e motivate it: 0.5-1.1 MB messages on a
 * fully connected xGMI fabric.  hx_ipc_*: device memory peers can map; handle64 = 64 bytes (hipIpcMemHandle_t) exchanged by any channel.
 * ------------------------------------------------------------------------------------------------------------ */
int hx_ipc_alloc(int64_t bytes, int32_t finegrained /* 1: flag / status words */, void** dev_ptr);
int hx_ipc_free(void* dev_ptr);
int hx_ipc_export(void* dev_ptr, void* handle64 /* host, out */);
int hx_ipc_import(const void* handle64 /* host */, void** dev_ptr);
int hx_ipc_close(void* dev_ptr);
/* dst[i] = bufs[0][i] + bufs[1][i] + ... (rank order: bit-identical on every rank), n floats (multiple of 4).  bufs / flags: host arrays of
 * `world` (<= 8) device pointers, own memory at index `rank`; every rank calls with the same epoch word = 1, 2, 3, ..., 0xFFFFFFFE, then 1
 * again (never 0, never 0xFFFFFFFF: refused); messages are double-buffered by the CALLER (the parity of its own call count), see hx_xchg.hip. *status != 0 afterwards: a peer did not arrive within timeout_ms (1) or
 * reported failure (2) — sticky and global (fail-stop): see hx_xchg.hip.  EXPERIMENTAL until it has run on two physical GPUs. */
int hx_allreduce_oneshot(float* dst, const float* const* bufs, uint32_t* const* flags, uint32_t* status, int32_t world, int32_t rank,
                         int64_t n, uint32_t epoch, int32_t timeout_ms, void* stream);

/* The same sum in TWO stages — reduce-scatter, then all-gather: rank r sums its slice [n r / world, n (r + 1) / world) of every rank's
 * message into reds[r] (its peer-mapped buffer of n floats), then copies the peers' reduced slices: 2 (world - 1) / world x n floats per rank
 * over xGMI instead of world x n.  Two launches; flags2: a second flag word per rank; bf16 != 0: the reduced slices travel as
 * bf16 (the fp32 sum rounded to nearest even, on every rank alike).  Otherwise as hx_allreduce_oneshot, the same fail-stop rules.  EXPERIMENTAL. */
int hx_allreduce_twostage(float* dst, const float* const* bufs, void* const* reds, uint32_t* const* flags, uint32_t* const* flags2, uint32_t* status,
                          int32_t world, int32_t rank, int64_t n, uint32_t epoch, int32_t timeout_ms, int32_t bf16, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The exchange on RCCL without torch.distributed in the loop (hx_rccl.hip): ncclAllReduce enqueued on the caller's stream.  librccl.so is
 * opened at run time — the copy the process already holds when there is one.  hx_rccl_unique_id on ONE rank, its 128 bytes to every rank by
 * any channel, hx_rccl_init on every rank (collective; one GPU per rank), then hx_rccl_allreduce per message: buf <- sum over ranks, in place
 * (dtype 0 fp32, 1 bf16), the same bits on every rank.  SURVEY.md 8e: the flat critic gradient and the merged actor message.
 * ------------------------------------------------------------------------------------------------------------ */
int hx_rccl_available(void); /* 0: the library and its entry points bind in this process (local, no collective) — ask on every rank before hx_rccl_init */
int hx_rccl_unique_id(uint8_t* id128 /* host, out */);
int hx_rccl_init(const uint8_t* id128 /* host */, int32_t world, int32_t rank, void** comm /* host, out */);
int hx_rccl_allreduce(void* comm, void* buf, int64_t n, int32_t dtype, void* stream);
/* The same exchange with the message on the wire as bf16 (half the bytes; RCCL sums in bf16): buf[i] (fp32) -> scratch[i] (bf16, round to nearest even) ->
 * ncclAllReduce(bf16) -> buf[i] (fp32), three enqueues on `stream`.  Every rank receives the same bits (replicas stay identical); opt-in
 * (`--exchange rccl-bf16`), n a multiple of 4, scratch: n bf16 device words.  EVERY word of the message is rounded and summed as bf16, whatever it
 * means: an integer travels exactly only while every partial sum stays within 256.  The merged actor message is built for that (its soft count as
 * base-32 digit words, see hx_hirl_actor_wgrad_split); a caller's own integer words need the same care or hx_rccl_allreduce. */
int hx_rccl_allreduce_bf16(void* comm, float* buf, uint16_t* scratch, int64_t n, void* stream);
int hx_rccl_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* HIRL4UCAV_H */
