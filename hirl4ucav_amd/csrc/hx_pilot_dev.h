// hx_pilot_dev.h — the pursuit pilot's law as device functions (gfx950), shared by hx_pilot.hip (hx_pilot_act, hx_pilot_refresh) and hx_branch.hip
// (hx_pilot_branch) so that the pilot's text exists once, and, on register operands, by hx_branch_steps.hip (hx_pilot_branch_steps).  The rule is
// stated in include/hirl4ucav.h ("The pilot as a kernel") and, in numpy, in tests/_pilot_model.py.  fp32 without contraction whatever the including translation unit uses, correctly rounded divide and square root.
#pragma once
#include "hx_common.h"

#pragma clang fp contract(off)
namespace hxpilot {

constexpr int kObs = 13, kRow = HX_ROW_WORDS;
constexpr int kAllyPos = 0, kAllyQuat = 6, kOppoPos = 13;  // state words (hirl4ucav.h "Env state layout")
static_assert(kRow == 32, "a table row is one 128-byte line");

// (pitch, roll, yaw) levels BEFORE noise and clamp, in the header's order of operations
__device__ __forceinline__ void pursuit_levels(const float* __restrict__ state, int64_t stride, int64_t i, float& l0, float& l1, float& l2) {
    const float w = state[(kAllyQuat + 0) * stride + i], x = state[(kAllyQuat + 1) * stride + i];
    const float y = state[(kAllyQuat + 2) * stride + i], z = state[(kAllyQuat + 3) * stride + i];
    const float d0 = state[(kOppoPos + 0) * stride + i] - state[(kAllyPos + 0) * stride + i];
    const float d1 = state[(kOppoPos + 1) * stride + i] - state[(kAllyPos + 1) * stride + i];
    const float d2 = state[(kOppoPos + 2) * stride + i] - state[(kAllyPos + 2) * stride + i];
    const float ax0 = 1.f - 2.f * (y * y + z * z), ax1 = 2.f * (x * y + w * z), ax2 = 2.f * (x * z - w * y);
    const float ay0 = 2.f * (x * y - w * z), ay1 = 1.f - 2.f * (x * x + z * z), ay2 = 2.f * (y * z + w * x);
    const float az0 = 2.f * (x * z + w * y), az1 = 2.f * (y * z - w * x), az2 = 1.f - 2.f * (x * x + y * y);
    const float b0 = (ax0 * d0 + ax1 * d1) + ax2 * d2;
    const float b1 = (ay0 * d0 + ay1 * d1) + ay2 * d2;
    const float b2 = (az0 * d0 + az1 * d1) + az2 * d2;
    float nrm = sqrtf((b0 * b0 + b1 * b1) + b2 * b2);
    if (nrm < 1e-6f) nrm = 1e-6f;  // (a comparison: a NaN stays a NaN)
    l0 = -4.f * (b1 / nrm);
    l1 = -2.f * (b0 / nrm);
    l2 = 4.f * (b0 / nrm);
}

// The same law on register operands — the ally's quaternion and d = p_opp - p_ally, what hxenv::Stepper holds (hx_branch_steps.hip) — BESIDE the
// memory form, not under it: with the memory form calling this one, the compiler swapped the operands of packed multiplies in pilot_act_kernel,
// pilot_refresh_kernel and pilot_branch_kernel (the same bits, another instruction stream), and those three kernels are to stay as they were.  The
// operations and their order are the memory form's, line for line; tests/test_branch_steps_gpu.py holds the two to each other bit for bit.
__device__ __forceinline__ void pursuit_levels(float w, float x, float y, float z, float d0, float d1, float d2, float& l0, float& l1, float& l2) {
    const float ax0 = 1.f - 2.f * (y * y + z * z), ax1 = 2.f * (x * y + w * z), ax2 = 2.f * (x * z - w * y);
    const float ay0 = 2.f * (x * y - w * z), ay1 = 1.f - 2.f * (x * x + z * z), ay2 = 2.f * (y * z + w * x);
    const float az0 = 2.f * (x * z + w * y), az1 = 2.f * (y * z - w * x), az2 = 1.f - 2.f * (x * x + y * y);
    const float b0 = (ax0 * d0 + ax1 * d1) + ax2 * d2;
    const float b1 = (ay0 * d0 + ay1 * d1) + ay2 * d2;
    const float b2 = (az0 * d0 + az1 * d1) + az2 * d2;
    float nrm = sqrtf((b0 * b0 + b1 * b1) + b2 * b2);
    if (nrm < 1e-6f) nrm = 1e-6f;  // (a comparison: a NaN stays a NaN)
    l0 = -4.f * (b1 / nrm);
    l1 = -2.f * (b0 / nrm);
    l2 = 4.f * (b0 / nrm);
}

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }  // (comparisons: a NaN stays a NaN)

__device__ __forceinline__ bool finite_word(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

}  // namespace hxpilot
#pragma clang fp contract(fast)
