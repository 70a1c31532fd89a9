// hx_noise.hip — temporally correlated exploration noise (gfx950): per env and action component a bank of K (1..8) stationary AR(1) processes,
//     z[k] <- a[k] z[k] + b[k] eps[k]        x = ((w[0] z[0]) + w[1] z[1]) + ...        out[t][i][c] = s_i x
// with every coefficient from the host: K = 1 is Ornstein-Uhlenbeck noise, K octave-spaced poles approximate a 1/f spectrum, a = 0 is white noise.  The
// rule is stated in include/hirl4ucav.h ("Exploration noise") and, in numpy, in tests/_noise_model.py; the colours are host recipes (utils/noise.py).
//
// One env per lane, 64 per workgroup = one wave, one instantiation per K so that the 4 K <= 32 state words of an env stay in registers over the `steps`
// iterations of a launch.  z is struct-of-arrays over envs ([K][4][n]: every load and store of a wave is one contiguous run); a step's draws come in and go
// out as one 16-byte access per lane and pole, its output as one 16-byte store per lane: out[t] is the [n, 4] tensor noise_mode 2 and the Gaussian head's
// eps take.  The process does not depend on the env's state, so ONE launch produces `steps` vector steps.  No atomics, no LDS, no workgroup waits for
// another, no lane reads a word another lane writes: the same inputs give the same bits.  Tiny: per env and launch 32 K B of state traffic and 16 B per step.
#include "hx_update.h"

#pragma clang fp contract(off)
namespace {

constexpr int kEnvs = 64;                  // envs per workgroup = one wave
constexpr uint32_t kTagStep = 0x4E4F4900u;  // Philox counter word 3 of a step's draw: | k.  (The acting kernels' draws have 0 there: no collision.)
constexpr uint32_t kTagInit = 0x4E4F4980u;  // ... of the stationary starting draw: | k
typedef float nz_v4f __attribute__((ext_vector_type(4)));

struct Coef {
    float a[HX_NOISE_MAX_POLES], b[HX_NOISE_MAX_POLES], w[HX_NOISE_MAX_POLES];
};

struct FillArgs {
    float* z;
    const float* sigma_env;
    int64_t n;
    float sigma;
    Coef c;
    uint64_t seed, step0;
    uint32_t row0;
    int steps;
    nz_v4f* out;
    const nz_v4f* eps_in;
    nz_v4f* eps_out;
};

// one Philox call -> the four standard-normal draws of one pole: u01 and Box-Muller as hx_act.h's philox_normal forms them, cos / sin per pair
__device__ __forceinline__ nz_v4f normal4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint64_t seed) {
    uint32_t u[4];
    hxu::philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32), u);
    nz_v4f e;
#pragma unroll
    for (int p = 0; p < 4; p += 2) {
        const float ua = hxu::u01(u[p]), ub = hxu::u01(u[p + 1]);
        const float rad = sqrtf(-2.0f * logf(ua)), ang = 6.28318530717958647692f * ub;
        e[p] = rad * cosf(ang);
        e[p + 1] = rad * sinf(ang);
    }
    return e;
}

__global__ __launch_bounds__(kEnvs) void noise_init_kernel(float* __restrict__ z, int64_t n, int poles, uint64_t seed, uint32_t row0) {
    const int64_t i = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < poles; ++k) {
        const nz_v4f e = normal4(row0 + (uint32_t)i, 0u, 0u, kTagInit | (uint32_t)k, seed);
#pragma unroll
        for (int c = 0; c < 4; ++c) z[(int64_t)(k * 4 + c) * n + i] = e[c];
    }
}

template <int K>
__global__ __launch_bounds__(kEnvs) void noise_fill_kernel(FillArgs A) {
    const int64_t n = A.n, i = (int64_t)blockIdx.x * kEnvs + threadIdx.x;
    if (i >= n) return;
    float z[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) z[k][c] = A.z[(int64_t)(k * 4 + c) * n + i];
    const float s = A.sigma_env ? A.sigma_env[i] : A.sigma;
    const uint32_t row = A.row0 + (uint32_t)i;
    for (int t = 0; t < A.steps; ++t) {
        const uint64_t step = A.step0 + (uint64_t)t;
        nz_v4f x = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t at = ((int64_t)t * K + k) * n + i;  // eps [steps][K][n][4]
            const nz_v4f e = A.eps_in ? A.eps_in[at] : normal4(row, (uint32_t)step, (uint32_t)(step >> 32), kTagStep | (uint32_t)k, A.seed);
            if (A.eps_out) A.eps_out[at] = e;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float az = A.c.a[k] * z[k][c], be = A.c.b[k] * e[c];  // two rounded products, one rounded sum: no FMA
                z[k][c] = az + be;
                const float wz = A.c.w[k] * z[k][c];
                x[c] = k == 0 ? wz : x[c] + wz;
            }
        }
        const nz_v4f o = {s * x[0], s * x[1], s * x[2], s * x[3]};
        A.out[(int64_t)t * n + i] = o;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) A.z[(int64_t)(k * 4 + c) * n + i] = z[k][c];
}

int check_shape(const float* z, int64_t n_envs, int32_t poles, const char* who) {
    HX_REQUIRE(poles >= 1 && poles <= HX_NOISE_MAX_POLES, "%s: poles is 1..%d, got %d", who, HX_NOISE_MAX_POLES, poles);
    HX_REQUIRE(n_envs > 0 && n_envs < (1ll << 31), "%s: 0 < n_envs < 2^31, got %lld", who, (long long)n_envs);
    HX_REQUIRE(z, "%s: z [poles][4][n_envs] (hx_noise_workspace_floats)", who);
    return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int K>
void launch_fill(const FillArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(noise_fill_kernel<K>, dim3((unsigned)((A.n + kEnvs - 1) / kEnvs)), dim3(kEnvs), 0, stream, A);
}

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

int64_t hx_noise_workspace_floats(int64_t n_envs, int32_t poles) {
    if (n_envs <= 0 || n_envs >= (1ll << 31) || poles < 1 || poles > HX_NOISE_MAX_POLES) return 0;
    return (int64_t)poles * 4 * n_envs;
}

int hx_noise_init(float* z, int64_t n_envs, int32_t poles, uint64_t seed, uint32_t row0, void* stream) {
    if (int rc = check_shape(z, n_envs, poles, "hx_noise_init")) return rc;
    hipLaunchKernelGGL(noise_init_kernel, dim3((unsigned)((n_envs + kEnvs - 1) / kEnvs)), dim3(kEnvs), 0, (hipStream_t)stream, z, n_envs, (int)poles, seed, row0);
    HX_CHECK_LAUNCH("hx_noise_init");
    return 0;
}

int hx_noise_fill(float* z, const float* sigma_env, int64_t n_envs, int32_t poles, float sigma, const float* coef, uint64_t seed, uint32_t row0, uint64_t step0,
                  int32_t steps, float* out, const float* eps_in, float* eps_out, void* stream) {
    if (int rc = check_shape(z, n_envs, poles, "hx_noise_fill")) return rc;
    HX_REQUIRE(steps >= 1 && steps <= HX_NOISE_MAX_STEPS, "hx_noise_fill: steps is 1..%d, got %d", HX_NOISE_MAX_STEPS, steps);
    HX_REQUIRE(out, "hx_noise_fill: out [steps][n_envs][4]");
    HX_REQUIRE(aligned16(out), "hx_noise_fill: out is 16-byte aligned (a step's four components leave as one store)");
    HX_REQUIRE(aligned16(eps_in), "hx_noise_fill: eps_in is 16-byte aligned");
    HX_REQUIRE(aligned16(eps_out), "hx_noise_fill: eps_out is 16-byte aligned");
    HX_REQUIRE(coef, "hx_noise_fill: coef [3][%d] on the host: a | b | w", HX_NOISE_MAX_POLES);
    HX_REQUIRE(std::isfinite(sigma), "hx_noise_fill: sigma is finite");
    FillArgs A{z, sigma_env, n_envs, sigma, {}, seed, step0, row0, (int)steps, reinterpret_cast<nz_v4f*>(out), reinterpret_cast<const nz_v4f*>(eps_in),
               reinterpret_cast<nz_v4f*>(eps_out)};
    for (int k = 0; k < poles; ++k) {
        const float a = coef[k], b = coef[HX_NOISE_MAX_POLES + k], w = coef[2 * HX_NOISE_MAX_POLES + k];
        HX_REQUIRE(a >= 0.0f && a < 1.0f, "hx_noise_fill: a[%d] = %g: every pole lies in [0, 1) (a stationary AR(1) process)", k, (double)a);
        HX_REQUIRE(std::isfinite(b) && std::isfinite(w), "hx_noise_fill: b[%d] and w[%d] are finite", k, k);
        A.c.a[k] = a; A.c.b[k] = b; A.c.w[k] = w;
    }
    hipStream_t st = (hipStream_t)stream;
    switch (poles) {
        case 1: launch_fill<1>(A, st); break;
        case 2: launch_fill<2>(A, st); break;
        case 3: launch_fill<3>(A, st); break;
        case 4: launch_fill<4>(A, st); break;
        case 5: launch_fill<5>(A, st); break;
        case 6: launch_fill<6>(A, st); break;
        case 7: launch_fill<7>(A, st); break;
        default: launch_fill<8>(A, st); break;
    }
    HX_CHECK_LAUNCH("hx_noise_fill");
    return 0;
}

}  // extern "C"
