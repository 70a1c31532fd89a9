// tools/asan_per_host.cpp — the host paths of the prioritized-replay entry points (hx_per_*, hx_sac_learn_weighted) under AddressSanitizer, as a
// stand-alone program on a box WITHOUT a GPU: argument checks, the refusals, the job packing of the 13 launches (which are dry runs in the
// asan-host build).  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_per_host.cpp -o /tmp/asan_per_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_per_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ == 0) { printf("NOT REFUSED: %s\n", #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t cap = 2500;
    const int B = 48;
    printf("sizeof(HxPer) %d / %zu, prio floats %lld\n", hx_per_sizeof(), sizeof(HxPer), (long long)hx_per_prio_floats(cap));
    if (hx_per_sizeof() != (int)sizeof(HxPer) || hx_per_prio_floats(cap) != 3072) ++fails;
    HxPer P{(float*)dev(3072 * 4), (float*)dev(3 * 4), (float*)dev(8), (uint64_t*)dev(8), (uint32_t*)dev(8), (const uint64_t*)dev(8), cap};
    int32_t* idx = (int32_t*)dev(B * 4); float* f = (float*)dev(B * 4); float* rows = (float*)dev(B * 128); float* ring = (float*)dev(cap * 128);
    OK(hx_per_mark_new(&P, 48, nullptr));
    OK(hx_per_mark_new(&P, 1 << 20, nullptr));
    OK(hx_per_set(&P, idx, f, B, nullptr));
    OK(hx_per_update(&P, idx, f, B, 0.6f, nullptr));
    OK(hx_per_resum(&P, nullptr));
    OK(hx_per_sample(&P, ring, B, nullptr, 7, 1, 0.4f, idx, f, rows, nullptr));
    OK(hx_per_sample(&P, ring, B, f, 7, 1, 1.0f, idx, f, rows, nullptr));
    REFUSED(hx_per_mark_new(nullptr, 48, nullptr));
    REFUSED(hx_per_mark_new(&P, 0, nullptr));
    HxPer big = P; big.cap = ((int64_t)1 << 24) + 1;
    REFUSED(hx_per_mark_new(&big, 48, nullptr));
    REFUSED(hx_per_sample(&big, ring, B, nullptr, 7, 1, 0.4f, idx, f, rows, nullptr));
    HxPer hole = P; hole.bsum = nullptr;
    REFUSED(hx_per_update(&hole, idx, f, B, 0.6f, nullptr));
    REFUSED(hx_per_set(&P, nullptr, f, B, nullptr));
    REFUSED(hx_per_update(&P, idx, f, 0, 0.6f, nullptr));
    REFUSED(hx_per_sample(&P, ring, 2000, nullptr, 7, 1, 0.4f, idx, f, rows, nullptr));
    REFUSED(hx_per_sample(&P, ring, B, nullptr, 7, 1, -1.0f, idx, f, rows, nullptr));
    // the weighted update
    const size_t np_ = hx_sac_policy_param_count(), nq = hx_critic_param_count();
    HxSacNets N{};
    N.policy = (float*)dev(np_ * 4); N.critic = (float*)dev(nq * 4); N.target_critic = (float*)dev(nq * 4);
    N.grad_policy = (float*)dev(np_ * 4); N.grad_critic = (float*)dev(nq * 4);
    N.m_policy = (float*)dev(np_ * 4); N.v_policy = (float*)dev(np_ * 4); N.m_critic = (float*)dev(nq * 4); N.v_critic = (float*)dev(nq * 4);
    N.losses = (float*)dev(32); N.alpha_state = (float*)dev(16); N.ws = (float*)dev(hx_sac_workspace_floats(B) * 4);
    N.policy_w2_f32i = (float*)dev(512 * 256 * 4);
    HxSacBatch Bt{rows, B, nullptr, nullptr, 5, 1};
    HxHyper Hy{0.99f, 0.005f, 1e-3f, 1e-3f, 0.0f, 0.5f, 0.0f, 0, 0};
    OK(hx_sac_learn_weighted(&N, &Bt, &Hy, f, f, 1, 3, -4.0f, nullptr));
    OK(hx_sac_learn_weighted(&N, &Bt, &Hy, f, f, 0, 1, -4.0f, nullptr));
    OK(hx_sac_learn(&N, &Bt, &Hy, nullptr, 1, 3, -4.0f, nullptr));
    REFUSED(hx_sac_learn_weighted(&N, &Bt, &Hy, nullptr, f, 1, 3, -4.0f, nullptr));
    REFUSED(hx_sac_learn_weighted(&N, &Bt, &Hy, f, nullptr, 1, 3, -4.0f, nullptr));
    REFUSED(hx_sac_learn_weighted(&N, &Bt, &Hy, f, f, 1, 0, -4.0f, nullptr));
    HxSacNets N16 = N; N16.w2_bf16_all = (uint16_t*)dev(16); N16.policy_w2_f32i = nullptr;
    REFUSED(hx_sac_learn_weighted(&N16, &Bt, &Hy, f, f, 1, 3, -4.0f, nullptr));
    HxSacBatch odd = Bt; odd.batch = 40;
    REFUSED(hx_sac_learn_weighted(&N, &odd, &Hy, f, f, 1, 3, -4.0f, nullptr));
    // priorities at insert: 40 new rows in chunks of 16
    float* sws = (float*)dev(hx_per_score_workspace_floats(16) * 4); float* serr = (float*)dev(40 * 4); float* seps = (float*)dev(40 * 16);
    OK(hx_per_score_new(&P, ring, &N, &Hy, 40, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    OK(hx_per_score_new(&P, ring, &N, &Hy, 40, 16, 0.6f, seps, 7, 2, sws, nullptr, nullptr));
    REFUSED(hx_per_score_new(nullptr, ring, &N, &Hy, 40, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&hole, ring, &N, &Hy, 40, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&big, ring, &N, &Hy, 40, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&P, nullptr, &N, &Hy, 40, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&P, ring, &N16, &Hy, 40, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&P, ring, &N, &Hy, 40, 10, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&P, ring, &N, &Hy, 0, 16, 0.6f, nullptr, 7, 1, sws, serr, nullptr));
    REFUSED(hx_per_score_new(&P, ring, &N, &Hy, 40, 16, 1.5f, nullptr, 7, 1, sws, serr, nullptr));
    printf(fails ? "FAILED: %d\n" : "per entry points ran their host paths under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
