// tools/asan_act_host.cpp — the host paths of the four acting entry points (hx_actor_act, hx_actor_act_step, hx_sac_act, hx_sac_act_step) under
// AddressSanitizer, as a stand-alone program on a box WITHOUT a GPU: every combination of offered W2 images at every size class (per-tile 16- and
// 32-row workgroups, the persistent kernel), alone and with the env step, with and without a replay ring — the image choice, the launch-shape choices
// and the packing of the kernel-argument struct (dry runs in the asan-host build) — and every refusal.  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_act_host.cpp -o /tmp/asan_act_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_act_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0, ran = 0, refusals = 0;
#define OK(x) do { int rc_ = (x); ++ran; if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
// refused with HX_ERR_ARG, and the message names the entry point
#define REFUSED(who, x) do { int rc_ = (x); ++refusals; if (rc_ != HX_ERR_ARG || strncmp(hx_last_error(), who ": ", strlen(who) + 2)) { \
    printf("NOT REFUSED AS %s (rc %d, %s): %s\n", who, rc_, hx_last_error(), #x); ++fails; } } while (0)
int main() {
    const int64_t NMAX = 131072, sizes[] = {1, 37, 4096, 4097, 8192, 8193, NMAX};
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 127) ++fails;
    float* actor = (float*)dev((size_t)hx_actor_param_count() * 4); float* policy = (float*)dev((size_t)hx_sac_policy_param_count() * 4);
    float* F = (float*)dev(512 * 256 * 4); uint16_t* X = (uint16_t*)dev(3 * 512 * 256 * 2); uint16_t* B = (uint16_t*)dev(512 * 256 * 2);
    float* state = (float*)dev(37 * NMAX * 4); float* obs = (float*)dev(NMAX * 13 * 4); float* act = (float*)dev(NMAX * 16);
    float* noise = (float*)dev(NMAX * 16); float* rew = (float*)dev(NMAX * 4);
    uint8_t* done = (uint8_t*)dev(NMAX); int8_t* succ = (int8_t*)dev(NMAX); uint32_t* epi = (uint32_t*)dev(NMAX * 4);
    const int64_t cap = 2 * NMAX;
    float* ring = (float*)dev(cap * 128); int8_t* ring_s = (int8_t*)dev(cap); uint64_t* total = (uint64_t*)dev(8);
    uint64_t* stats = (uint64_t*)dev(HX_STAT_WAYS * HX_STAT_PITCH * 8);
    const HxStepOpts plain{1500, 1, 1, 0, 7, epi, nullptr, nullptr, 0, nullptr, stats, nullptr, nullptr, 0};
    const HxStepOpts ringed{1500, 1, 1, 0, 7, epi, ring, ring_s, cap, total, stats, nullptr, nullptr, 0};
    OK(hx_pack_w2_f32i(actor, 13, F, nullptr)); OK(hx_pack_w2_x9(actor, 13, X, nullptr)); OK(hx_pack_w2_bf16(actor, 13, B, nullptr));
    // (w2_f32i, w2_x9, w2_bf16): none, each single image, all three, the split beside the fp32 image; sac: whether the Gaussian head takes it (not x9 alone)
    const struct { const float* f; const uint16_t* x; const uint16_t* b; bool sac; } fmts[] = {
        {nullptr, nullptr, nullptr, true}, {F, nullptr, nullptr, true}, {nullptr, X, nullptr, false}, {nullptr, nullptr, B, true}, {F, X, B, true}, {F, X, nullptr, true},
        {nullptr, X, B, true}, {F, nullptr, B, true}};
    for (const auto& m : fmts)
        for (int64_t n : sizes) {
            for (int mode : {0, 1, 2, 3, 3 + 16})
                for (float slope : {0.0f, 0.01f})
                    OK(hx_actor_act(actor, m.f, m.x, m.b, obs, n, act, mode, noise, 0.1f, 7, 0, 1, slope, nullptr));
            OK(hx_actor_act(actor, m.f, m.x, m.b, obs, n, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
            for (const HxStepOpts* o : {(const HxStepOpts*)nullptr, &plain, &ringed}) {
                OK(hx_actor_act_step(actor, m.f, m.x, m.b, state, n, n, obs, act, 3, nullptr, 0.1f, 7, 0, 1, 0.0f, rew, done, succ, o, nullptr));
                OK(hx_actor_act_step(actor, m.f, m.x, m.b, state, n, NMAX, obs, act, 2 + 16, noise, 0.0f, 7, 5, 1, 0.01f, rew, done, succ, o, nullptr));
            }
            if (!m.sac) {
                REFUSED("hx_sac_act", hx_sac_act(policy, m.f, m.x, m.b, obs, n, act, 2, nullptr, 7, 0, 1, nullptr));
                REFUSED("hx_sac_act_step", hx_sac_act_step(policy, m.f, m.x, m.b, state, n, n, obs, act, 2, nullptr, 7, 0, 1, rew, done, succ, &ringed, nullptr));
                continue;
            }
            for (int mode : {0, 1, 2}) {
                OK(hx_sac_act(policy, m.f, m.x, m.b, obs, n, act, mode, noise, 7, 0, 1, nullptr));
                for (const HxStepOpts* o : {(const HxStepOpts*)nullptr, &plain, &ringed})
                    OK(hx_sac_act_step(policy, m.f, m.x, m.b, state, n, n, obs, act, mode, noise, 7, 0, 1, rew, done, succ, o, nullptr));
            }
        }
    // ---- refusals ----
    const int64_t n = 37;
    // a non-NULL image that is not 16-byte aligned, in each slot, alone and beside images that would be chosen before it
    const float* F4 = F + 1; const uint16_t* X4 = X + 2; const uint16_t* B4 = B + 2; const uint16_t* B8 = B + 4;
    const struct { const float* f; const uint16_t* x; const uint16_t* b; } bad[] = {{F4, nullptr, nullptr}, {nullptr, X4, nullptr}, {nullptr, nullptr, B4}, {F4, X, B},
                                                                                      {F, X4, B}, {F, X, B4}, {nullptr, nullptr, B8}, {F4, X4, B4}};
    for (const auto& m : bad) {
        REFUSED("hx_actor_act", hx_actor_act(actor, m.f, m.x, m.b, obs, n, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
        REFUSED("hx_actor_act_step", hx_actor_act_step(actor, m.f, m.x, m.b, state, n, n, obs, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, rew, done, succ, &plain, nullptr));
        REFUSED("hx_sac_act", hx_sac_act(policy, m.f, m.x, m.b, obs, n, act, 0, nullptr, 7, 0, 1, nullptr));
        REFUSED("hx_sac_act_step", hx_sac_act_step(policy, m.f, m.x, m.b, state, n, n, obs, act, 0, nullptr, 7, 0, 1, rew, done, succ, &plain, nullptr));
    }
    // the Gaussian head: w2_x9 without w2_f32i when no bf16 image is offered (at the sizes where the split would act, too)
    REFUSED("hx_sac_act", hx_sac_act(policy, nullptr, X, nullptr, obs, NMAX, act, 0, nullptr, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act_step", hx_sac_act_step(policy, nullptr, X, nullptr, state, NMAX, NMAX, obs, act, 0, nullptr, 7, 0, 1, rew, done, succ, &ringed, nullptr));
    // bit 32 of noise_mode (hx_hirl_front's) when the exact split is the chosen format — and only then
    REFUSED("hx_actor_act", hx_actor_act(actor, nullptr, X, nullptr, obs, n, act, 3 + 32, nullptr, 0.1f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, F, X, nullptr, obs, n, act, 3 + 32, nullptr, 0.1f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act_step", hx_actor_act_step(actor, nullptr, X, nullptr, state, n, n, obs, act, 32, nullptr, 0.0f, 7, 0, 1, 0.0f, rew, done, succ, &plain, nullptr));
    OK(hx_actor_act(actor, F, X, B, obs, n, act, 3 + 32, nullptr, 0.1f, 7, 0, 1, 0.0f, nullptr));
    OK(hx_actor_act(actor, F, nullptr, nullptr, obs, n, act, 3 + 32, nullptr, 0.1f, 7, 0, 1, 0.0f, nullptr));
    // check_noise_mode
    REFUSED("hx_actor_act", hx_actor_act(actor, F, nullptr, nullptr, obs, n, act, 4, noise, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, F, nullptr, nullptr, obs, n, act, 1, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, F, nullptr, nullptr, obs, n, act, 2 + 16, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act_step", hx_actor_act_step(actor, F, nullptr, nullptr, state, n, n, obs, act, 5, noise, 0.0f, 7, 0, 1, 0.0f, rew, done, succ, &plain, nullptr));
    REFUSED("hx_actor_act_step", hx_actor_act_step(actor, F, nullptr, nullptr, state, n, n, obs, act, 2, nullptr, 0.0f, 7, 0, 1, 0.0f, rew, done, succ, &plain, nullptr));
    // the bad-argument checks
    REFUSED("hx_actor_act", hx_actor_act(nullptr, F, nullptr, nullptr, obs, n, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, F, nullptr, nullptr, nullptr, n, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, F, nullptr, nullptr, obs, n, nullptr, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, F, nullptr, nullptr, obs, 0, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act", hx_actor_act(actor, nullptr, nullptr, nullptr, obs, -3, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, nullptr));
    REFUSED("hx_actor_act_step", hx_actor_act_step(nullptr, F, nullptr, nullptr, state, n, n, obs, act, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, rew, done, succ, &plain, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(nullptr, F, nullptr, nullptr, obs, n, act, 0, nullptr, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(policy, F, nullptr, nullptr, nullptr, n, act, 0, nullptr, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(policy, F, nullptr, nullptr, obs, n, nullptr, 0, nullptr, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(policy, F, nullptr, nullptr, obs, 0, act, 0, nullptr, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(policy, F, nullptr, nullptr, obs, n, act, 3, noise, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(policy, F, nullptr, nullptr, obs, n, act, -1, noise, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act", hx_sac_act(policy, F, nullptr, nullptr, obs, n, act, 1, nullptr, 7, 0, 1, nullptr));
    REFUSED("hx_sac_act_step", hx_sac_act_step(nullptr, F, nullptr, nullptr, state, n, n, obs, act, 0, nullptr, 7, 0, 1, rew, done, succ, &plain, nullptr));
    REFUSED("hx_sac_act_step", hx_sac_act_step(policy, F, nullptr, nullptr, state, n, n, obs, act, 3, noise, 7, 0, 1, rew, done, succ, &plain, nullptr));
    REFUSED("hx_sac_act_step", hx_sac_act_step(policy, F, nullptr, nullptr, state, n, n, obs, act, 1, nullptr, 7, 0, 1, rew, done, succ, &plain, nullptr));
    // check_step_args, through both act_step entry points
    HxStepOpts no_ctr = plain; no_ctr.episode_ctr = nullptr;
    HxStepOpts small_cap = ringed; small_cap.cap = 511;
    HxStepOpts huge_cap = ringed; huge_cap.cap = (int64_t)1 << 31;
    HxStepOpts no_total = ringed; no_total.total = nullptr;
    HxStepOpts off_ring = ringed; off_ring.ring = ring + 1;
#define STEP_REFUSED(state_, n_, stride_, obs_, act_, rew_, done_, succ_, o_) do { \
    REFUSED("hx_actor_act_step", hx_actor_act_step(actor, F, nullptr, nullptr, state_, n_, stride_, obs_, act_, 0, nullptr, 0.0f, 7, 0, 1, 0.0f, rew_, done_, succ_, o_, nullptr)); \
    REFUSED("hx_sac_act_step", hx_sac_act_step(policy, F, nullptr, nullptr, state_, n_, stride_, obs_, act_, 0, nullptr, 7, 0, 1, rew_, done_, succ_, o_, nullptr)); } while (0)
    STEP_REFUSED(nullptr, n, n, obs, act, rew, done, succ, &plain);
    STEP_REFUSED(state, n, n, nullptr, act, rew, done, succ, &plain);
    STEP_REFUSED(state, n, n, obs, nullptr, rew, done, succ, &plain);
    STEP_REFUSED(state, n, n, obs, act, nullptr, done, succ, &plain);
    STEP_REFUSED(state, n, n, obs, act, rew, nullptr, succ, &plain);
    STEP_REFUSED(state, n, n, obs, act, rew, done, nullptr, &plain);
    STEP_REFUSED(state, 0, n, obs, act, rew, done, succ, &plain);
    STEP_REFUSED(state, n, n - 1, obs, act, rew, done, succ, &plain);
    STEP_REFUSED(state, (int64_t)1 << 31, (int64_t)1 << 31, obs, act, rew, done, succ, &plain);
    STEP_REFUSED(state, n, (int64_t)1 << 25, obs, act, rew, done, succ, &plain);
    STEP_REFUSED(state, n, n, obs, act, rew, done, succ, &no_ctr);
    STEP_REFUSED(state, n, n, obs, act, rew, done, succ, &small_cap);
    STEP_REFUSED(state, n, n, obs, act, rew, done, succ, &huge_cap);
    STEP_REFUSED(state, n, n, obs, act, rew, done, succ, &no_total);
    STEP_REFUSED(state, n, n, obs, act, rew, done, succ, &off_ring);
    printf(fails ? "FAILED: %d (%d calls, %d refusals)\n" : "acting entry points ran their host paths under the sanitizer (%d failures, %d calls, %d refusals refused)\n", fails, ran,
           refusals);
    return fails ? 1 : 0;
}
