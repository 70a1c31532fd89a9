// tools/asan_clip_host.cpp — the host paths of the gradient-clipping entry points (hx_sac_grad_norm, hx_sac_adam_clipped, hx_sac_learn_weighted_clipped,
// hx_sac_clip_floats / _shape) and of the fixed entropy coefficient (target_entropy = HX_SAC_FIXED_ALPHA) under AddressSanitizer, as a stand-alone
// program on a box WITHOUT a GPU: argument checks, the refusals, the argument packing of the launches (dry runs in the asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_clip_host.cpp -o /tmp/asan_clip_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_clip_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int B = 48;
    const size_t P = (size_t)hx_sac_policy_param_count(), C = (size_t)hx_critic_param_count();
    int32_t shape[6];
    OK(hx_sac_clip_shape(shape));
    REFUSED(hx_sac_clip_shape(nullptr));
    printf("clip_ws floats %lld; shape %d %d %d %d %d %d\n", (long long)hx_sac_clip_floats(), shape[0], shape[1], shape[2], shape[3], shape[4], shape[5]);
    if (hx_sac_clip_floats() < 8 + 3 * shape[2] || shape[3] > shape[2] || shape[4] > shape[2]) ++fails;
    if ((size_t)shape[3] * shape[1] < C / 2 || (size_t)shape[4] * shape[1] < P) ++fails;  // every word of a segment lies in one of its chunks
    auto F = [](size_t n) { return (float*)dev(n * 4); };
    HxSacNets N{};
    N.policy = F(P); N.critic = F(C); N.target_critic = F(C); N.grad_policy = F(P); N.grad_critic = F(C);
    N.m_policy = F(P); N.v_policy = F(P); N.m_critic = F(C); N.v_critic = F(C); N.losses = F(8); N.alpha_state = F(4);
    N.ws = F((size_t)hx_sac_workspace_floats(B));
    N.policy_w2_f32i = F(512 * 256);
    HxHyper H{};
    H.gamma = 0.99f; H.tau = 0.005f; H.lr_critic = 1e-3f; H.lr_actor = 1e-3f;
    float* ws = F((size_t)hx_sac_clip_floats());
    HxSacBatch Bt{F(B * 32), B, nullptr, nullptr, 5, 1};
    float* w = F(B); float* err = F(B);
    for (int which = 0; which < 2; ++which) {
        OK(hx_sac_grad_norm(&N, which, ws, nullptr));
        OK(hx_sac_adam_clipped(&N, &H, which, 3, 1.0f, -4.0f, 1.0f, ws, nullptr));
        OK(hx_sac_adam_clipped(&N, &H, which, 3, 1.0f, HX_SAC_FIXED_ALPHA, 1e30f, ws, nullptr));
        OK(hx_sac_adam(&N, &H, which, 3, 1.0f, HX_SAC_FIXED_ALPHA, nullptr));
    }
    OK(hx_sac_learn_weighted_clipped(&N, &Bt, &H, w, err, 1, 3, -4.0f, 1.0f, ws, nullptr));
    OK(hx_sac_learn_weighted_clipped(&N, &Bt, &H, w, err, 0, 3, HX_SAC_FIXED_ALPHA, 0.5f, ws, nullptr));
    OK(hx_sac_learn_weighted(&N, &Bt, &H, w, err, 0, 3, HX_SAC_FIXED_ALPHA, nullptr));
    OK(hx_sac_learn(&N, &Bt, &H, nullptr, 0, 3, HX_SAC_FIXED_ALPHA, nullptr));
    REFUSED(hx_sac_grad_norm(nullptr, 0, ws, nullptr));
    REFUSED(hx_sac_grad_norm(&N, 2, ws, nullptr));
    REFUSED(hx_sac_grad_norm(&N, 0, nullptr, nullptr));
    REFUSED(hx_sac_grad_norm(&N, 0, ws + 1, nullptr));  // not 16-byte aligned
    HxSacNets hole = N; hole.grad_policy = nullptr;
    REFUSED(hx_sac_grad_norm(&hole, 1, ws, nullptr));
    REFUSED(hx_sac_adam_clipped(&N, &H, 0, 0, 1.0f, -4.0f, 1.0f, ws, nullptr));           // step is 1-based
    REFUSED(hx_sac_adam_clipped(&N, &H, 0, 3, 1.0f, -4.0f, 0.0f, ws, nullptr));           // max_norm must be positive
    REFUSED(hx_sac_adam_clipped(&N, &H, 0, 3, 1.0f, -4.0f, -1.0f, ws, nullptr));
    REFUSED(hx_sac_adam_clipped(&N, &H, 0, 3, 1.0f, -4.0f, std::nanf(""), ws, nullptr));
    REFUSED(hx_sac_adam_clipped(&N, &H, 0, 3, 0.0f, -4.0f, 1.0f, ws, nullptr));           // grad_scale must be positive
    REFUSED(hx_sac_adam_clipped(&N, &H, 2, 3, 1.0f, -4.0f, 1.0f, ws, nullptr));
    REFUSED(hx_sac_adam_clipped(&N, nullptr, 0, 3, 1.0f, -4.0f, 1.0f, ws, nullptr));
    REFUSED(hx_sac_adam_clipped(&N, &H, 0, 3, 1.0f, -4.0f, 1.0f, nullptr, nullptr));
    HxSacNets odd = N; odd.m_policy = N.m_policy + 1;
    REFUSED(hx_sac_adam_clipped(&odd, &H, 1, 3, 1.0f, -4.0f, 1.0f, ws, nullptr));         // buffers must be 16-byte aligned
    REFUSED(hx_sac_learn_weighted_clipped(&N, &Bt, &H, w, err, 0, 3, -4.0f, 1.0f, nullptr, nullptr));
    REFUSED(hx_sac_learn_weighted_clipped(&N, &Bt, &H, w, err, 0, 3, -4.0f, 0.0f, ws, nullptr));
    REFUSED(hx_sac_learn_weighted_clipped(&N, &Bt, &H, nullptr, err, 0, 3, -4.0f, 1.0f, ws, nullptr));
    REFUSED(hx_sac_learn_weighted_clipped(&N, &Bt, &H, w, err, 0, 0, -4.0f, 1.0f, ws, nullptr));
    printf(fails ? "asan_clip_host: %d FAILURES\n" : "asan_clip_host: ok\n", fails);
    return fails ? 1 : 0;
}
