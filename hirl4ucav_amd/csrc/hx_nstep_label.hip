// hx_nstep_label.hip — truncated n-step returns for a LABELLED expert table (gfx950): the rows hx_label_transitions produced, one transition each and in
// recording order, become rows of up to n steps in the ordinary 32-word format — r = sum_k gamma^k r_k, the row's discount folded into the done column — by
// the fold a head performs in hx_nstep_push (include/hirl4ucav.h "n-step returns for a labelled expert table").  Row j stays row j.
//
// One row per lane, 64 rows per workgroup = one wave.  The workgroup's own rows enter LDS as whole 128-B lines; per row the reward, done and `last` words of
// rows j .. j + m - 1 and the 13 words of s' of row j + m - 1 are gathers (they may reach n - 1 rows past the workgroup's last row: never past E, never past a
// `last` row); the finished rows leave as whole 128-B lines, eight lanes of 16 B each.  Run once per expert table: memory-bound, about 128 B in, 128 B out
// and up to 8 x 9 + 52 B of gathers per row, most of them the workgroup's own lines again.
#include "hx_common.h"

#pragma clang fp contract(off)
namespace {

constexpr int kRows = 64;                      // rows per workgroup = one wave
constexpr int kRowPitch = HX_ROW_WORDS + 1;    // +1: conflict-free per-lane row accesses
constexpr int kQuads = HX_ROW_WORDS / 4;       // 16-B pieces of a row
enum { W_S2 = HX_OBS_DIM + HX_ACT_DIM, W_R = HX_ROW_WORDS - 2, W_D = HX_ROW_WORDS - 1 };  // s' | r | done
static_assert(HX_ROW_WORDS == 32 && W_S2 + HX_OBS_DIM == W_R, "the row format: s[13] a[4] s'[13] r done");
typedef float nl_v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kRows) void nstep_label_kernel(const float* __restrict__ rows_in, const uint8_t* __restrict__ last, int64_t E, int n, float gamma,
                                                            float* __restrict__ rows_out) {
    __shared__ float s_row[kRows * kRowPitch];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * kRows, j = j0 + tid;
    const int nblk = (int)((E - j0) < kRows ? (E - j0) : kRows);

    // the workgroup's rows: 8 lanes per row, 16 B each
    const nl_v4f* in4 = reinterpret_cast<const nl_v4f*>(rows_in);
#pragma unroll
    for (int it = 0; it < kQuads; ++it) {
        const int k = tid + it * kRows;
        const int rr = k >> 3, c = (k & 7) * 4;
        if (rr < nblk) {
            const nl_v4f v = in4[(size_t)(j0 + rr) * kQuads + (k & 7)];
            float* dst = s_row + rr * kRowPitch + c;
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
    }
    __syncthreads();

    if (tid < nblk) {
        float acc = 0.f, boot = 1.0f;
        int64_t end = j;  // the row the fold stops at: j + m - 1
        for (int k = 0; k < n; ++k) {
            end = j + k;  // (< E, and no `last` row lies in [j, end): checked before every advance)
            const float w = k == 0 ? 1.0f : boot * gamma;
            acc = acc + w * rows_in[end * HX_ROW_WORDS + W_R];
            boot = w;
            if (last[end] != 0 || end + 1 >= E) break;
        }
        float* row = s_row + tid * kRowPitch;
        const float* src = rows_in + end * HX_ROW_WORDS;
#pragma unroll
        for (int f = 0; f < HX_OBS_DIM; ++f) row[W_S2 + f] = src[W_S2 + f];
        row[W_R] = acc;
        row[W_D] = src[W_D] != 0.f ? 1.0f : 1.0f - boot;
    }
    __syncthreads();

    nl_v4f* out4 = reinterpret_cast<nl_v4f*>(rows_out);
#pragma unroll
    for (int it = 0; it < kQuads; ++it) {
        const int k = tid + it * kRows;
        const int rr = k >> 3, c = (k & 7) * 4;
        if (rr < nblk) {
            const float* src = s_row + rr * kRowPitch + c;
            const nl_v4f v = {src[0], src[1], src[2], src[3]};
            __builtin_nontemporal_store(v, out4 + (size_t)(j0 + rr) * kQuads + (k & 7));
        }
    }
}

}  // namespace
#pragma clang fp contract(fast)

extern "C" {

int hx_nstep_label(const float* rows_in, const uint8_t* last, int64_t E, int32_t n, float gamma, float* rows_out, void* stream) {
    HX_REQUIRE(n >= 1 && n <= HX_NSTEP_MAX, "hx_nstep_label: n is 1..%d, got %d", HX_NSTEP_MAX, n);
    HX_REQUIRE(E > 0 && E < (1ll << 31), "hx_nstep_label: 0 < E < 2^31 rows, got %lld", (long long)E);
    HX_REQUIRE(gamma >= 0.0f && gamma <= 1.0f, "hx_nstep_label: gamma in [0, 1]");
    HX_REQUIRE(rows_in && last && rows_out, "hx_nstep_label: rows_in [E][32], last [E] and rows_out [E][32]");
    HX_REQUIRE(((reinterpret_cast<uintptr_t>(rows_in) | reinterpret_cast<uintptr_t>(rows_out)) & 15u) == 0,
               "hx_nstep_label: rows_in and rows_out are 16-byte aligned (rows move as whole 128-byte lines)");
    const uintptr_t a = reinterpret_cast<uintptr_t>(rows_in), b = reinterpret_cast<uintptr_t>(rows_out), bytes = (uintptr_t)E * HX_ROW_WORDS * sizeof(float);
    HX_REQUIRE(a + bytes <= b || b + bytes <= a, "hx_nstep_label: rows_out must not overlap rows_in (a row reads up to n - 1 rows behind it, which another "
                                                 "workgroup may already have rewritten)");
    const unsigned grid = (unsigned)((E + kRows - 1) / kRows);
    hipLaunchKernelGGL(nstep_label_kernel, dim3(grid), dim3(kRows), 0, (hipStream_t)stream, rows_in, last, E, (int)n, gamma, rows_out);
    HX_CHECK_LAUNCH("hx_nstep_label");
    return 0;
}

}  // extern "C"
