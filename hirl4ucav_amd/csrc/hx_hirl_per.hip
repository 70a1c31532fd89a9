// hx_hirl_per.hip — prioritized replay for HIRL and TD3 (gfx950): the twin deterministic critics' TD head as a per-row kernel with importance
// weights.  The reference's HIRL.py / TD3.py draw uniformly (hirl/utils/buffer.py ships a SumTree that HIRL.py:236,283 never reaches): a declared
// extension (include/hirl4ucav.h "Prioritized replay for HIRL / TD3").
//   hirl_td_head_weighted   y = r + gamma min(Q1', Q2') (1 - d) (HIRL.py:270-274), errors = |Q1(s, a) - y|, critic_loss += w ((Q1 - y)^2 + (Q2 - y)^2) / B,
//                           head gradients 2 w (Q_h - y) / B: what bwd_l2<0>'s prologue (BM_CRITIC_TD) computes, per row and with the weight.  The
//                           critics' backward then runs with the head gradient given (bwd_l2<3>, BM_GIVEN) — the move td_head_weighted_kernel made for SAC
//                           (hx_sac.hip), with the engine's leaky slope, its layerNorm switch, and ONE loss slot (HIRL logs the sum).
// Rows [0, n_weighted) carry weights[r], the rows behind them (the expert rows of the minibatch, HIRL.py:226-227) the weight 1; weights is not read there.
#include <cmath>

#include "hx_update.h"

using namespace hxnn;
using namespace hxu;

namespace {

// sac_td_heads<true> (hx_update.h) with the activation slope as an argument (SAC's critics are plain ReLU stacks, HIRL's leaky with the engine's slope;
// m.no_ln travels in m): the two target critics on (s', a') -> their minimum, Q1 and Q2 on (s, a), each critic's LayerNorm stats stored for bwd_l2<3>
template <bool RELU>
__device__ __forceinline__ void hirl_td_heads(const Mlp m, float slope, int r, const QHeadIn t1, const QHeadIn t2, const QHeadIn c1, const QHeadIn c2, float& qmin,
                                              float& q1, float& q2) {
    const int lane = threadIdx.x & 63;
    RowReg<H2> xh, y;
    float mean_, rstd_, a[1], b[1], o[1];
    head_row<1, RELU>(t1.z2 + (size_t)r * H2, t1.net, m, slope, xh, y, mean_, rstd_, a);
    head_row<1, RELU>(t2.z2 + (size_t)r * H2, t2.net, m, slope, xh, y, mean_, rstd_, b);
    head_row<1, RELU>(c1.z2 + (size_t)r * H2, c1.net, m, slope, xh, y, mean_, rstd_, o);
    q1 = o[0];
    if (lane == 0) { c1.st2[r * 2] = mean_; c1.st2[r * 2 + 1] = rstd_; }
    head_row<1, RELU>(c2.z2 + (size_t)r * H2, c2.net, m, slope, xh, y, mean_, rstd_, o);
    q2 = o[0];
    if (lane == 0) { c2.st2[r * 2] = mean_; c2.st2[r * 2 + 1] = rstd_; }
    qmin = fminf(a[0], b[0]);
}

// One wave per row, four rows per workgroup; no LDS, no barrier, no workgroup waits for another.  fp32 in both update dtypes (the z2 rows and the heads
// are fp32 on the bf16 path too).
template <bool RELU>
__global__ __launch_bounds__(kThreads) void hirl_td_head_weighted_kernel(HirlTdHead A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= A.nrows) return;
    float qmin, q1, q2;
    hirl_td_heads<RELU>(A.m, A.slope, r, {A.t1net, A.z2_t1, nullptr}, {A.t2net, A.z2_t2, nullptr}, {A.q1net, A.s1.z2, A.s1.st2}, {A.q2net, A.s2.z2, A.s2.st2}, qmin,
                        q1, q2);
    if (lane == 0) {
        const float lab0 = A.rows[(size_t)r * 32 + 30], lab1 = A.rows[(size_t)r * 32 + 31];
        const float target = lab0 + (A.gamma * qmin) * (1.0f - lab1);  // bwd_l2<0>'s expression (HIRL.py:270-274)
        const float w = r < A.n_weighted ? A.weights[r] : 1.0f;        // (expert rows: exactly 1, nothing read)
        const float wb = w * A.inv_batch;
        const float d1 = q1 - target, d2 = q2 - target;
        A.errors[r] = fabsf(d1);
        A.s1.dout[(size_t)r * OW] = 2.0f * d1 * wb;
        A.s2.dout[(size_t)r * OW] = 2.0f * d2 * wb;
        atomicAdd(&A.losses[0], d1 * d1 * wb);
        atomicAdd(&A.losses[0], d2 * d2 * wb);
    }
}

}  // namespace

namespace hxu {

void launch_hirl_td_head(const HirlTdHead& T, hipStream_t st) {
    const dim3 grid((unsigned)((T.nrows + 3) / 4));
    if (T.slope == 0.0f) hipLaunchKernelGGL((hirl_td_head_weighted_kernel<true>), grid, dim3(kThreads), 0, st, T);
    else hipLaunchKernelGGL((hirl_td_head_weighted_kernel<false>), grid, dim3(kThreads), 0, st, T);
}

}  // namespace hxu
