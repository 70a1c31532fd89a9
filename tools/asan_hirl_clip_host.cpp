// tools/asan_hirl_clip_host.cpp — the host paths of HIRL's gradient-norm clipping (hx_hirl_clip_floats, hx_hirl_clip_shape, hx_hirl_grad_norm,
// hx_adam_clipped) under AddressSanitizer, as a stand-alone program on a box WITHOUT a GPU: sizes, every argument refusal, the filling of the two
// launches' arguments in every form (critic, actor, merged message, TD3, each acting format, the bf16 update's images; dry runs in the asan-host
// build), and hx_adam / hx_adam_mixed through the argument filling they now share with the clipped step.  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_hirl_clip_host.cpp -o /tmp/asan_hirl_clip_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_hirl_clip_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ != HX_ERR_ARG) { printf("NOT REFUSED (rc %d): %s\n", rc_, #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
#define CHECK(x) do { if (!(x)) { printf("CHECK FAILED: %s\n", #x); ++fails; } } while (0)
int main() {
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 130) ++fails;
    const int64_t na = hx_actor_param_count(), nc = hx_critic_param_count(), nmsg = hx_actor_message_floats(), nws = hx_hirl_clip_floats();
    int32_t shape[8] = {0};
    OK(hx_hirl_clip_shape(shape));
    REFUSED(hx_hirl_clip_shape(nullptr));
    printf("actor %lld critic %lld message %lld clip_ws %lld; shape %d %d %d %d %d depth %d %d partials at %d\n", (long long)na, (long long)nc, (long long)nmsg,
           (long long)nws, shape[0], shape[1], shape[2], shape[3], shape[4], shape[5], shape[6], shape[7]);
    const int64_t pa = (na + 3) & ~(int64_t)3;
    CHECK(shape[1] == 256 * 4 * shape[0] && shape[2] <= 64 && nws == shape[7] + 3 * shape[2] && nmsg == 2 * pa + 64);
    CHECK((int64_t)shape[3] * shape[1] >= nc / 2 && (int64_t)(shape[3] - 1) * shape[1] < nc / 2 && shape[3] <= shape[2]);
    CHECK((int64_t)shape[4] * shape[1] >= na && (int64_t)(shape[4] - 1) * shape[1] < na && shape[4] <= shape[2]);
    CHECK(shape[5] == shape[6] + 1 && shape[6] == 1 + 2 + (shape[0] - 1) + 6 + 2 + 6);
    auto f = [](int64_t n) { return (float*)dev((size_t)n * 4); };
    HxNets N;
    memset(&N, 0, sizeof N);
    N.actor = f(na); N.critic = f(nc); N.target_actor = f(na); N.target_critic = f(nc); N.bc_actor = f(na);
    N.grad_actor = f(na); N.grad_critic = f(nc); N.m_actor = f(na); N.v_actor = f(na); N.m_critic = f(nc); N.v_critic = f(nc);
    N.losses = f(8); N.soft_count = (int32_t*)dev(64); N.wstate = f(1); N.actor_w2_f32i = f(512 * 256);
    HxHyper Hy;
    memset(&Hy, 0, sizeof Hy);
    Hy.gamma = 0.99f; Hy.tau = 0.005f; Hy.lr_actor = 1e-3f; Hy.lr_critic = 1e-3f; Hy.noise_clamp = 0.5f; Hy.loss_lambda = 1e4f; Hy.use_bc = 1;
    float* ws = f(nws);   // (sized exactly: the sanitizer sees any host write behind it)
    float* msg = f(nmsg);
    uint32_t* word = (uint32_t*)dev(64);
    for (int pass = 0; pass < 5; ++pass) {  // fp32 image; + bf16 acting image; exact split; bf16 update's images; TD3 behind a status word
        uint16_t* extra = nullptr;
        if (pass == 1) { N.actor_w2_bf16 = extra = (uint16_t*)dev(512 * 256 * 2); }
        if (pass == 2) { N.actor_w2_x9 = extra = (uint16_t*)dev(3 * 512 * 256 * 2); }
        if (pass == 3) { N.w2_bf16_all = extra = (uint16_t*)dev((size_t)hx_bf16_images_elems() * 2); N.actor_w2_bf16 = extra; }
        if (pass == 4) { Hy.use_bc = 0; N.xchg_status = word; }
        for (int which = 0; which < 2; ++which)
            for (int pk = 0; pk <= 16; pk += 16) {
                OK(hx_hirl_grad_norm(&N, &Hy, which, 1, 0.0f, 0.05f, 128, nullptr, ws, nullptr));
                OK(hx_adam_clipped(&N, &Hy, which | pk, 1, 1.0f, 1, 0.0f, 0.05f, 128, nullptr, 1.0f, ws, nullptr));
                OK(hx_adam_clipped(&N, &Hy, which | pk, 1 << 30, 0.125f, 2, 0.0f, 0.0f, 1024, nullptr, 1e30f, ws, nullptr));
                OK(hx_adam(&N, &Hy, which | pk, 7, 0.5f, 0, 0.3f, 0.0f, 128, nullptr));
            }
        for (int kind = 0; kind < 3; ++kind) {
            OK(hx_hirl_grad_norm(&N, &Hy, 1, kind, 0.3f, 0.05f, 1024, msg, ws, nullptr));
            OK(hx_adam_clipped(&N, &Hy, 1 | 16, 3, 0.125f, kind, 0.3f, 0.05f, 1024, msg, 0.5f, ws, nullptr));
            OK(hx_adam_mixed(&N, &Hy, 1, 3, 0.125f, kind, 0.3f, 0.05f, 1024, msg, nullptr));
        }
        N.actor_w2_bf16 = nullptr; N.actor_w2_x9 = nullptr; N.w2_bf16_all = nullptr;
        free(extra);
    }
    Hy.use_bc = 1; N.xchg_status = nullptr;
    // refusals: every argument error of the two launching entry points
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 0.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, -1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, NAN, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, 0.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, -0.5f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, NAN, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 0, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 2, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 2 | 16, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 3, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 0, 1, 1.0f, 0, 0.0f, 0.0f, 128, msg, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, msg + 1, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws + 1, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, nullptr, nullptr));
    REFUSED(hx_adam_clipped(nullptr, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, nullptr, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 2, 0, 0.0f, 0.0f, 128, nullptr, ws, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, &Hy, -1, 0, 0.0f, 0.0f, 128, nullptr, ws, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 0, 0, 0.0f, 0.0f, 128, msg, ws, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 1, 0, 0.0f, 0.0f, 128, msg + 2, ws, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 1, 0, 0.0f, 0.0f, 128, nullptr, ws + 3, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 1, 0, 0.0f, 0.0f, 128, nullptr, nullptr, nullptr));
    REFUSED(hx_hirl_grad_norm(nullptr, &Hy, 1, 0, 0.0f, 0.0f, 128, nullptr, ws, nullptr));
    REFUSED(hx_hirl_grad_norm(&N, nullptr, 1, 0, 0.0f, 0.0f, 128, nullptr, ws, nullptr));
    float* own = N.grad_actor;
    N.grad_actor = own + 1;
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 1, 0, 0.0f, 0.0f, 128, nullptr, ws, nullptr));
    REFUSED(hx_adam_clipped(&N, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    N.grad_actor = nullptr;
    REFUSED(hx_hirl_grad_norm(&N, &Hy, 1, 0, 0.0f, 0.0f, 128, nullptr, ws, nullptr));
    N.grad_actor = own;
    N.actor_w2_x9 = (uint16_t*)dev(64); N.actor_w2_bf16 = N.actor_w2_x9;  // two acting formats at once
    REFUSED(hx_adam_clipped(&N, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, 1.0f, ws, nullptr));
    REFUSED(hx_adam(&N, &Hy, 1, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr));
    N.actor_w2_x9 = nullptr; N.actor_w2_bf16 = nullptr;
    // the older entry points keep their refusals (and their words) behind the shared filling
    REFUSED(hx_adam(&N, &Hy, 3, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr));
    CHECK(strstr(hx_last_error(), "hx_adam: bad arguments") != nullptr);
    REFUSED(hx_adam_mixed(&N, &Hy, 0, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr, nullptr));
    CHECK(strstr(hx_last_error(), "hx_adam_mixed: null message") != nullptr);
    REFUSED(hx_adam_mixed(&N, &Hy, 0, 1, 1.0f, 0, 0.0f, 0.0f, 128, msg + 1, nullptr));
    CHECK(strstr(hx_last_error(), "hx_adam_mixed: actor step only, 16-byte aligned message") != nullptr);
    OK(hx_adam(&N, &Hy, 2, 1, 1.0f, 0, 0.0f, 0.0f, 128, nullptr));
    printf(fails ? "FAILED: %d\n" : "HIRL's clip entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
