// tools/asan_branch_host.cpp — the host path of hx_pilot_branch (expert branches, hx_branch.hip) under AddressSanitizer, as a stand-alone program on
// a box WITHOUT a GPU: the argument checks and refusals, the host path at 64-bit call counts (2^32 - 1, 2^32, 2^40, 2^64 - 1), the packing of the launch
// (a dry run in the asan-host build).  CPU only.  The asan-host build of hx_branch.hip keeps the three words the last call packed for its kernel —
// floor(n / k), call mod n, (call * k) mod M — and hands them out (hx_pilot_branch_last_packed: that build only, not in the public header): packed()
// below compares what the LIBRARY computed with 128-bit arithmetic.  On the GPU the same residues are held to the model by tests/test_branch_gpu.py.
//   make -C hirl4ucav_amd/csrc asan-host
//   RT=$(dirname $(find /opt/rocm/lib/llvm/lib/clang -name 'libclang_rt.asan-x86_64.so' | head -1))
//   hipcc -x c++ -std=c++17 -g -O1 -fsanitize=address -shared-libsan -Iinclude tools/asan_branch_host.cpp -o /tmp/asan_branch_host \
//         -Lhirl4ucav_amd -l:libhx_mi355_asanhost.so -Wl,-rpath,$PWD/hirl4ucav_amd -Wl,-rpath,$RT
//   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 /tmp/asan_branch_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hirl4ucav.h"
static void* dev(size_t n) { void* p = nullptr; if (posix_memalign(&p, 256, n ? n : 256)) abort(); memset(p, 0, n ? n : 256); return p; }
static int fails = 0;
#define OK(x) do { int rc_ = (x); if (rc_ != 0) { printf("UNEXPECTED rc %d: %s -> %s\n", rc_, #x, hx_last_error()); ++fails; } } while (0)
#define REFUSED(x) do { int rc_ = (x); if (rc_ != HX_ERR_ARG) { printf("NOT REFUSED (rc %d): %s\n", rc_, #x); ++fails; } else printf("refused ok: %s\n", hx_last_error()); } while (0)
extern "C" void hx_pilot_branch_last_packed(uint32_t out[3]);
// what the last hx_pilot_branch(.., n, .., M, k, call) packed, against the rule in 128-bit arithmetic
static void packed(uint64_t call, uint64_t n, uint64_t m, uint64_t k) {
    uint32_t got[3];
    hx_pilot_branch_last_packed(got);
    const unsigned __int128 wide = (unsigned __int128)call * k;
    if (got[0] != (uint32_t)(n / k) || got[1] != (uint32_t)(call % n) || got[2] != (uint32_t)(wide % m)) {
        printf("PACKED: call %llu n %llu k %llu M %llu -> %u %u %u\n", (unsigned long long)call, (unsigned long long)n, (unsigned long long)k, (unsigned long long)m, got[0], got[1], got[2]);
        ++fails;
    }
}
int main() {
    const int64_t N = 300, stride = 320, E0 = 40, M = 50;
    if (hx_version() != HX_ABI_VERSION || HX_ABI_VERSION < 128) ++fails;
    float* state = (float*)dev(37 * stride * 4); float* obs = (float*)dev(N * 13 * 4);
    float* ring = (float*)dev((E0 + M) * 32 * 4); int8_t* succ = (int8_t*)dev(E0 + M);
    const uint64_t calls[] = {0, 1, 299, 300, 0xFFFFFFFFull, 0x100000000ull, 1ull << 40, ~0ull};
    for (uint64_t c : calls) {
        OK(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, M, 7, c, nullptr)); packed(c, N, M, 7);
        OK(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, M, 50, c, nullptr)); packed(c, N, M, 50);
        OK(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, 49, 48, c, nullptr)); packed(c, N, 49, 48);
    }
    OK(hx_pilot_branch(state, N, stride, obs, ring, succ, 0, M, 1, 3, nullptr));
    OK(hx_pilot_branch(state, 1, 1, obs, ring, succ, 3, 1, 1, 1ull << 40, nullptr));
    OK(hx_pilot_branch(state, N, stride, obs, ring, succ, 1, 89, 89, 5, nullptr));
    OK(hx_pilot_branch(state, N, N, obs, ring, succ, E0, M, 50, 0xFFFFFFFFull, nullptr));
    REFUSED(hx_pilot_branch(nullptr, N, stride, obs, ring, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, nullptr, ring, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, nullptr, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, nullptr, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring + 1, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring + 16, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, 0, stride, obs, ring, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, -1, stride, obs, ring, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, N - 1, obs, ring, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, (int64_t)1 << 31, (int64_t)1 << 31, obs, ring, succ, E0, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, -1, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, 0, 1, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, M, 0, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, M, -4, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, E0, M, 51, 0, nullptr));
    REFUSED(hx_pilot_branch(state, 40, stride, obs, ring, succ, E0, M, 41, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, (int64_t)1 << 31, M, 7, 0, nullptr));
    REFUSED(hx_pilot_branch(state, N, stride, obs, ring, succ, ((int64_t)1 << 31) - M, M, 7, 0, nullptr));
    printf(fails ? "FAILED: %d\n" : "hx_pilot_branch ran its host path under the sanitizer (%d failures)\n", fails);
    return fails ? 1 : 0;
}
