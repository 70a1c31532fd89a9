// tools/asan_hirl_per_host.cpp — the host path of HIRL's / TD3's weighted critic stage (hx_hirl_critic_grads_weighted) under AddressSanitizer, as a
// stand-alone program on a box WITHOUT a GPU: every argument refusal, n_weighted = 0 (weights NULL and given) and = batch, and the filling of its five
// launches' arguments (launches A and B with the actor call's riding forwards, the weighted TD head, bwd_l2<3>'s two BM_GIVEN jobs, launch D with the
// head riders) in every form — critic-only and actor calls, HIRL soft / TD3 / no LayerNorm, the bf16 update's images, ragged batches; dry runs in the
// asan-host build.  The unweighted stage runs beside it through the arguments they share.  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_hirl_per_host.cpp -o /tmp/asan_hirl_per_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_hirl_per_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x, word) do { int rc_ = (x); if (rc_ != HX_ERR_ARG || !strstr(hx_last_error(), word)) { printf("NOT REFUSED as expected (rc %d, %s): %s\n", rc_, hx_last_error(), #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 131) ++fails;
    const int64_t na = hx_actor_param_count(), nc = hx_critic_param_count();
    auto f = [](int64_t n) { return (float*)dev((size_t)n * 4); };
    HxNets N;
    memset(&N, 0, sizeof N);
    N.actor = f(na); N.critic = f(nc); N.target_actor = f(na); N.target_critic = f(nc); N.bc_actor = f(na);
    N.grad_actor = f(na); N.grad_critic = f(nc); N.m_actor = f(na); N.v_actor = f(na); N.m_critic = f(nc); N.v_critic = f(nc);
    N.losses = f(8); N.soft_count = (int32_t*)dev(64); N.wstate = f(1); N.actor_w2_f32i = f(512 * 256);
    HxHyper Hy;
    memset(&Hy, 0, sizeof Hy);
    Hy.gamma = 0.99f; Hy.tau = 0.005f; Hy.lr_actor = 1e-3f; Hy.lr_critic = 1e-3f; Hy.noise_clamp = 0.5f; Hy.loss_lambda = 1e4f; Hy.use_bc = 1;
    uint16_t* images = (uint16_t*)dev((size_t)hx_bf16_images_elems() * 2);
    const int batches[4] = {16, 48, 144, 1024};
    for (int bi = 0; bi < 4; ++bi) {
        const int B = batches[bi];
        N.ws = f(hx_hirl_workspace_floats(B));  // (sized exactly: the sanitizer sees any host write behind it)
        float* rows = f((int64_t)B * 32); float* bc_rows = f((int64_t)B * 32); float* noise = f(4);
        float* w = f(B); float* err = f(B);     // (exactly batch words each)
        for (int pass = 0; pass < 4; ++pass) {  // HIRL fp32; the bf16 update's images; TD3 (leaky, no BC batch); no LayerNorm
            N.w2_bf16_all = pass == 1 ? images : nullptr;
            Hy.use_bc = pass == 2 ? 0 : 1; Hy.slope = pass == 2 ? 0.01f : 0.0f; Hy.no_layernorm = pass == 3 ? 1 : 0;
            HxBatch Bt;
            memset(&Bt, 0, sizeof Bt);
            Bt.rows = rows; Bt.bc_rows = Hy.use_bc ? bc_rows : nullptr; Bt.batch = B; Bt.noise = noise;
            for (int actor_fwd = 0; actor_fwd <= 2; ++actor_fwd) {
                OK(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, B, err, actor_fwd, nullptr));        // every row weighted
                OK(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, B - 5, err, actor_fwd, nullptr));    // expert rows behind
                OK(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, 1, err, actor_fwd, nullptr));
                OK(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, 0, err, actor_fwd, nullptr));        // none weighted, weights given
                OK(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, nullptr, 0, err, actor_fwd, nullptr));  // ... and NULL
                OK(hx_hirl_critic_grads(&N, &Bt, &Hy, actor_fwd, nullptr));
            }
            if (bi == 0 && pass == 0) {  // every argument error
                REFUSED(hx_hirl_critic_grads_weighted(nullptr, &Bt, &Hy, w, B, err, 0, nullptr), "batch must be a positive multiple of 16");
                REFUSED(hx_hirl_critic_grads_weighted(&N, nullptr, &Hy, w, B, err, 0, nullptr), "batch must be a positive multiple of 16");
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, nullptr, w, B, err, 0, nullptr), "batch must be a positive multiple of 16");
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, -1, err, 0, nullptr), "n_weighted -1 is not in 0..batch");
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, B + 1, err, 0, nullptr), "n_weighted 17 is not in 0..batch");
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, nullptr, 1, err, 0, nullptr), "weights may be NULL only with n_weighted == 0");
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, nullptr, B, err, 0, nullptr), "weights may be NULL only with n_weighted == 0");
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, B, nullptr, 0, nullptr), "errors_out[batch] is required");
                HxBatch bad = Bt;
                bad.batch = 0;
                REFUSED(hx_hirl_critic_grads_weighted(&N, &bad, &Hy, w, 0, err, 0, nullptr), "batch must be a positive multiple of 16");
                bad.batch = 24;
                REFUSED(hx_hirl_critic_grads_weighted(&N, &bad, &Hy, w, 8, err, 0, nullptr), "batch must be a positive multiple of 16");
                bad.batch = -16;
                REFUSED(hx_hirl_critic_grads_weighted(&N, &bad, &Hy, w, 0, err, 0, nullptr), "batch must be a positive multiple of 16");
                bad = Bt;
                bad.rows = nullptr;
                REFUSED(hx_hirl_critic_grads_weighted(&N, &bad, &Hy, w, B, err, 0, nullptr), "null rows, workspace or losses");
                float* own = N.ws;
                N.ws = nullptr;
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, B, err, 0, nullptr), "null rows, workspace or losses");
                N.ws = own;
                own = N.losses;
                N.losses = nullptr;
                REFUSED(hx_hirl_critic_grads_weighted(&N, &Bt, &Hy, w, B, err, 0, nullptr), "null rows, workspace or losses");
                N.losses = own;
            }
        }
        free(N.ws); free(rows); free(bc_rows); free(noise); free(w); free(err);
        N.ws = nullptr;
    }
    printf(fails ? "FAILED: %d\n" : "hx_hirl_critic_grads_weighted ran its host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
