// tools/asan_branch_steps_host.cpp — the host path of hx_pilot_branch_steps and hx_branch_workspace_bytes (expert branches of up to H steps,
// hx_branch_steps.hip) under AddressSanitizer, as a stand-alone program on a box WITHOUT a GPU: the argument checks and refusals, the workspace size, the
// host path at 64-bit call counts (2^32 - 1, 2^32, 2^40, 2^64 - 1), the packing of the launch (a dry run in the asan-host build).  CPU only.  The asan-host
// build of hx_branch_steps.hip keeps the four words the last call packed for its kernel — floor(n / k), call mod n, (call * k) mod M, max_steps — and
// hands them out (hx_pilot_branch_steps_last_packed: that build only, not in the public header): packed() below compares what the LIBRARY computed with
// 128-bit arithmetic.  On the GPU the same residues are held to the model by tests/test_branch_steps_gpu.py.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_branch_steps_host.cpp -o /tmp/asan_branch_steps_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_branch_steps_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ != HX_ERR_ARG) { printf("NOT REFUSED (rc %d): %s\n", rc_, #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
#define EQ(a, b) do { long long a_ = (long long)(a), b_ = (long long)(b); if (a_ != b_) { printf("%s = %lld, expected %lld\n", #a, a_, b_); ++fails; } } while (0)
extern "C" void hx_pilot_branch_steps_last_packed(uint32_t out[4]);
// what the last hx_pilot_branch_steps(.., n, .., M, k, H, call, ..) packed, against the rule in 128-bit arithmetic
static void packed(uint64_t call, uint64_t n, uint64_t m, uint64_t k, uint32_t h) {
    uint32_t got[4];
    hx_pilot_branch_steps_last_packed(got);
    const unsigned __int128 wide = (unsigned __int128)call * k;
    if (got[0] != (uint32_t)(n / k) || got[1] != (uint32_t)(call % n) || got[2] != (uint32_t)(wide % m) || got[3] != h) {
        printf("PACKED: call %llu n %llu k %llu M %llu H %u -> %u %u %u %u\n", (unsigned long long)call, (unsigned long long)n, (unsigned long long)k,
               (unsigned long long)m, h, got[0], got[1], got[2], got[3]);
        ++fails;
    }
}
int main() {
    const int64_t N = 300, stride = 320, E0 = 40, M = 50;
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 129) ++fails;
    // the workspace: 37 + 13 + 1 32-bit words and three 64-bit counters per column, k rounded up to 64 columns
    EQ(hx_branch_workspace_bytes(-5), 0); EQ(hx_branch_workspace_bytes(0), 0);
    EQ(hx_branch_workspace_bytes(1), 64 * 228); EQ(hx_branch_workspace_bytes(64), 64 * 228); EQ(hx_branch_workspace_bytes(65), 128 * 228);
    EQ(hx_branch_workspace_bytes(300), 320 * 228); EQ(hx_branch_workspace_bytes(2147483647), 2147483648ll * 228);
    float* state = (float*)dev(37 * stride * 4); float* obs = (float*)dev(N * 13 * 4);
    float* ring = (float*)dev((E0 + M) * 32 * 4); int8_t* succ = (int8_t*)dev(E0 + M);
    char* work = (char*)dev((size_t)hx_branch_workspace_bytes(50) + 16);
    const uint64_t calls[] = {0, 1, 299, 300, 0xFFFFFFFFull, 0x100000000ull, 1ull << 40, ~0ull};
    for (uint64_t c : calls) {
        OK(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 1500, c, work, 64, nullptr)); packed(c, N, M, 7, 1500);
        OK(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 50, 1, c, work, 64, nullptr)); packed(c, N, M, 50, 1);
        OK(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, 49, 48, 65535, c, work, 64, nullptr)); packed(c, N, 49, 48, 65535);
    }
    OK(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, 0, M, 1, 2, 3, work, 64, nullptr));
    OK(hx_pilot_branch_steps(state, 1, 1, obs, ring, succ, 3, 1, 1, 8, 1ull << 40, work, 64, nullptr));
    OK(hx_pilot_branch_steps(state, N, N, obs, ring, succ, E0, M, 50, 400, 0xFFFFFFFFull, work + 16, 64, nullptr));
    {
        char* big = (char*)dev((size_t)hx_branch_workspace_bytes(89));
        OK(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, 1, 89, 89, 8, 5, big, 128, nullptr));
        REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, 1, 89, 89, 8, 5, big, 64, nullptr));
        free(big);
    }
    // hx_pilot_branch's refusals
    REFUSED(hx_pilot_branch_steps(nullptr, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, nullptr, ring, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, nullptr, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, nullptr, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring + 1, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring + 16, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, 0, stride, obs, ring, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, -1, stride, obs, ring, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, N - 1, obs, ring, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, (int64_t)1 << 31, (int64_t)1 << 31, obs, ring, succ, E0, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, -1, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, 0, 1, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 0, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, -4, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 51, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, 40, stride, obs, ring, succ, E0, M, 41, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, (int64_t)1 << 31, M, 7, 8, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, ((int64_t)1 << 31) - M, M, 7, 8, 0, work, 64, nullptr));
    // its own: max_steps, the workspace and its stride
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 0, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, -1, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 65536, 0, work, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, nullptr, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work + 4, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work + 8, 64, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work, 0, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work, 7, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work, 128, nullptr));
    REFUSED(hx_pilot_branch_steps(state, N, stride, obs, ring, succ, E0, M, 7, 8, 0, work, -64, nullptr));
    printf(fails ? "FAILED: %d\n" : "hx_pilot_branch_steps ran its host path under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
