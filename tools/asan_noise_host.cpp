// tools/asan_noise_host.cpp — the host path of hx_noise_init / hx_noise_fill (correlated exploration noise) under AddressSanitizer, as a stand-alone program
// on a box WITHOUT a GPU: the argument checks and refusals, the reading of the host coefficient table, the packing of the launch (a dry run in the asan-host
// build).  The coefficient table is allocated at its exact size, so a read beyond a | b | w [3][8] would be reported.  CPU only.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_noise_host.cpp -o /tmp/asan_noise_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_noise_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ != HX_ERR_ARG) { printf("NOT REFUSED (rc %d): %s\n", rc_, #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
int main() {
    const int64_t n = 300;
    const int K = HX_NOISE_MAX_POLES, S = HX_NOISE_MAX_STEPS;
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 134) ++fails;
    if (hx_noise_workspace_floats(n, K) != 4 * K * n || hx_noise_workspace_floats(n, 0) != 0 || hx_noise_workspace_floats(n, K + 1) != 0 ||
        hx_noise_workspace_floats(0, 1) != 0 || hx_noise_workspace_floats((int64_t)1 << 31, 1) != 0) ++fails;
    float* z = (float*)dev(4 * K * n * 4);
    float* sig = (float*)dev(n * 4);
    float* out = (float*)dev((size_t)S * n * 16);
    float* eps = (float*)dev((size_t)S * K * n * 16);
    float* coef = (float*)malloc(3 * K * sizeof(float));  // exactly a | b | w
    for (int k = 0; k < K; ++k) { const double a = exp(-pow(2.0, -k)); coef[k] = (float)a; coef[K + k] = (float)sqrt(1.0 - a * a); coef[2 * K + k] = (float)(1.0 / sqrt((double)K)); }
    for (int p = 1; p <= K; ++p) {
        OK(hx_noise_init(z, n, p, 7, 0xFFFFFFF0u, nullptr));
        OK(hx_noise_fill(z, nullptr, n, p, 0.1f, coef, 7, 0, 0, 1, out, nullptr, nullptr, nullptr));
        OK(hx_noise_fill(z, sig, n, p, 0.0f, coef, ~0ull, 0xFFFFFFFFu, ~0ull, S, out, eps, eps, nullptr));
    }
    float* bad = (float*)malloc(3 * K * sizeof(float));
    auto with = [&](int row, int k, float v) { memcpy(bad, coef, 3 * K * sizeof(float)); bad[row * K + k] = v; return bad; };
    OK(hx_noise_fill(z, nullptr, n, 2, 0.1f, with(0, 2, 5.0f), 7, 0, 0, 4, out, nullptr, eps, nullptr));  // (a coefficient beyond `poles` is not read)
    REFUSED(hx_noise_fill(z, nullptr, n, 0, 0.1f, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, K + 1, 0.1f, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, coef, 7, 0, 0, 0, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, coef, 7, 0, 0, S + 1, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, 0, 2, 0.1f, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, -1, 2, 0.1f, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, (int64_t)1 << 31, 2, 0.1f, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(nullptr, nullptr, n, 2, 0.1f, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, coef, 7, 0, 0, 4, nullptr, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, nullptr, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, coef, 7, 0, 0, 4, out + 1, nullptr, nullptr, nullptr));  // misaligned
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, coef, 7, 0, 0, 4, out, eps + 2, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, coef, 7, 0, 0, 4, out, nullptr, eps + 3, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, with(0, 0, 1.0f), 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, with(0, 1, -0.5f), 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, with(0, 1, NAN), 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, with(1, 0, INFINITY), 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, 0.1f, with(2, 1, NAN), 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, NAN, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_fill(z, nullptr, n, 2, INFINITY, coef, 7, 0, 0, 4, out, nullptr, nullptr, nullptr));
    REFUSED(hx_noise_init(nullptr, n, 2, 7, 0, nullptr));
    REFUSED(hx_noise_init(z, 0, 2, 7, 0, nullptr));
    REFUSED(hx_noise_init(z, n, 0, 7, 0, nullptr));
    REFUSED(hx_noise_init(z, n, K + 1, 7, 0, nullptr));
    free(bad); free(coef);
    printf(fails ? "FAILED: %d\n" : "hx_noise_* ran its host path under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
