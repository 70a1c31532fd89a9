// hx_sac.hip — SacAgent.learn (hirl/agents/SAC/agent.py:276-414: the non-imitative branch train_sac.py uses, and the imitative one — "SAC, imitative
// branch" below) on the shared fwd_l2 / bwd_l2<3> / wgrad machinery, plus the small per-row kernels around it (gfx950).
#include <cmath>

#include "hx_act.h"

using namespace hxnn;
using namespace hxu;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// SAC (hirl/agents/SAC): small per-row kernels around the shared fwd_l2 / bwd_l2<3> / wgrad machinery.  One wave per row.
// ---------------------------------------------------------------------------------------------------------------
// GaussianPolicy.sample (SAC/model.py:69-82) from the policy's z2 rows: mean, log_std = chunk(head), clamp(log_std, -20, 2),
// x = mean + exp(log_std) eps, a = tanh(x), entropy = -sum_j (log N(x_j) - log(1 - a_j^2 + 1e-6)).
struct GaussArgs {
    const float* net;
    Mlp m;
    const float* z2;
    const float* eps;  // [rows][4] standard-normal draws; nullptr with mode 2 -> Philox; mode 0 ignores it
    int rows, mode;    // 0: exploit tanh(mean) (agent.py:191-196), 1: sample with eps, 2: sample with Philox(seed; row, call)
    float* act;        // [rows][4]
    float* ent;        // [rows] or nullptr
    float* aux;        // [rows][16] or nullptr: a[4], sigma*eps[4], clamp pass-through mask[4], entropy
    uint64_t seed;
    uint32_t row0, call;
};
// One launch serves up to TWO evaluations (policy.sample(s') for the TD target and policy.sample(s) for the policy loss: both read z2 rows of
// the first forward launch and the policy as it is before this learn()'s steps) and, behind them, the soft_update of the target critics
// that SacAgent.learn does first on every target_update_interval-th call (agent.py:278-279): nothing reads the targets before the NEXT launch.
struct GaussLaunch {
    GaussArgs g[2];
    int nb0;       // workgroups of g[0]; g[1] follows (rows 0: none)
    int nb_gauss;  // workgroups of g[0] + g[1]; Polyak blocks follow
    float* target; const float* source; int n; float tau;  // soft_update (n = 0: none)
    // SAC bf16 path: the bf16 images of the targets' W2 follow the step (element e of segment s = W2 of head s: [seg_lo[s], + 512 x 256) of target)
    uint16_t* img[2]; int seg_lo[2];
};
// the bf16 image element(s) of the target weight(s) at flat index i (four consecutive k of one column when `four`)
__device__ __forceinline__ void polyak_image(const GaussLaunch& L, int i, const float* t, bool four) {
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        if (!L.img[sg] || i < L.seg_lo[sg] || i >= L.seg_lo[sg] + H2 * H1) continue;
        const uint32_t e = (uint32_t)(i - L.seg_lo[sg]), col = e / H1, k = e % H1;
        if (four) {
            *reinterpret_cast<uint2*>(L.img[sg] + w2_image_index(col, k)) = pack4_bf16(t[0], t[1], t[2], t[3]);
        } else {
            L.img[sg][w2_image_index(col, k)] = __builtin_bit_cast(uint16_t, (__bf16)t[0]);
        }
    }
}
__device__ __forceinline__ void gauss_head_rows(const GaussArgs& A, int block);
__global__ __launch_bounds__(kThreads) void gauss_head_kernel(GaussLaunch L) {
    const int b = blockIdx.x;
    if (b >= L.nb_gauss) {  // target <- (1 - tau) target + tau source, 16 B per lane (the arithmetic of polyak_kernel)
        const int i = ((b - L.nb_gauss) * kThreads + threadIdx.x) * 4;
        if (i + 4 <= L.n) {
            float4 t4 = *reinterpret_cast<const float4*>(L.target + i);
            const float4 s4 = *reinterpret_cast<const float4*>(L.source + i);
            t4.x = polyak_update(t4.x, s4.x, L.tau); t4.y = polyak_update(t4.y, s4.y, L.tau);
            t4.z = polyak_update(t4.z, s4.z, L.tau); t4.w = polyak_update(t4.w, s4.w, L.tau);
            *reinterpret_cast<float4*>(L.target + i) = t4;
            const float tv[4] = {t4.x, t4.y, t4.z, t4.w};
            polyak_image(L, i, tv, true);  // (W2 starts at a multiple of 4 floats: the float4 is inside or outside)
        } else {
            for (int c = 0; i + c < L.n; ++c) {
                const float tv = polyak_update(L.target[i + c], L.source[i + c], L.tau);
                L.target[i + c] = tv;
                polyak_image(L, i + c, &tv, false);
            }
        }
        return;
    }
    if (b < L.nb0) gauss_head_rows(L.g[0], b);
    else gauss_head_rows(L.g[1], b - L.nb0);
}
__device__ __forceinline__ void gauss_head_rows(const GaussArgs& A, int block) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = block * 4 + wave;
    if (r >= A.rows) return;
    RowReg<H2> xh, y;
    float mean_, rstd_, o[8];
    head_row<8, true>(A.z2 + (size_t)r * H2, A.net, A.m, 0.0f, xh, y, mean_, rstd_, o);
    const int j = lane & 3;
    const float mu = pick8(o, j), ls_raw = pick8(o, 4 + j);
    const float ls = fminf(fmaxf(ls_raw, -20.0f), 2.0f);  // model.py:65-66
    const float sd = expf(ls);
    float e = 0.0f;
    if (A.mode == 1) e = A.eps[(size_t)r * 4 + j];
    if (A.mode == 2) {
        uint32_t u[4];
        philox4x32_10(A.row0 + (uint32_t)r, A.call, 0x53414331u, 0u, (uint32_t)A.seed, (uint32_t)(A.seed >> 32), u);
        const float ua = u01(u[j & 2]), ub = u01(u[(j & 2) + 1]);
        const float rad = sqrtf(-2.0f * logf(ua)), ang = 6.28318530717958647692f * ub;
        e = (j & 1) ? rad * sinf(ang) : rad * cosf(ang);
    }
    const float se = sd * e;
    const float a = tanhf(A.mode == 0 ? mu : mu + se);
    // Normal(mean, std).log_prob(x) with x - mean = sd * eps, minus the tanh correction   model.py:77-78
    const float logp = (-(se * se) / (2.0f * (sd * sd)) - ls - 0.91893853320467274f) - logf(1.0f - a * a + 1e-6f);
    float h = lane < 4 ? -logp : 0.0f;
    h = sum16(h);  // lanes 0..3 sit in the first 16-lane row
    if (lane < 4) {
        A.act[(size_t)r * 4 + j] = a;
        if (A.aux) {
            float* x = A.aux + (size_t)r * 16;
            x[j] = a;
            x[4 + j] = se;
            x[8 + j] = (ls_raw >= -20.0f && ls_raw <= 2.0f) ? 1.0f : 0.0f;
            if (lane == 0) x[12] = h;
        }
    }
    if (lane == 0 && A.ent) A.ent[r] = h;
}

// min(Q1, Q2)(s, a~) for the policy loss (SAC/agent.py:380-383): writes each head's output gradient -w/B (w = 1 for the smaller
// head, 1/2 each on a tie: torch.min's subgradient) and accumulates the -min(Q)/B part of the policy loss.
struct QSelArgs {
    const float* net1;
    const float* net2;
    Mlp m;
    Slot s1, s2;
    int rows;
    float inv_batch;
    float* losses;
    const float* weights;  // WEIGHTED: [rows] importance weights (prioritized replay): inv_batch becomes w_r / B
};
template <bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void q_select_kernel(QSelArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= A.rows) return;
    const float inv_batch = WEIGHTED ? A.weights[r] * A.inv_batch : A.inv_batch;
    RowReg<H2> xh, y;
    float mean_, rstd_, q1[1], q2[1];
    head_row<1, true>(A.s1.z2 + (size_t)r * H2, A.net1, A.m, 0.0f, xh, y, mean_, rstd_, q1);
    if (lane == 0) { A.s1.st2[r * 2] = mean_; A.s1.st2[r * 2 + 1] = rstd_; }
    head_row<1, true>(A.s2.z2 + (size_t)r * H2, A.net2, A.m, 0.0f, xh, y, mean_, rstd_, q2);
    if (lane == 0) {
        A.s2.st2[r * 2] = mean_; A.s2.st2[r * 2 + 1] = rstd_;
        const float w1 = q1[0] < q2[0] ? 1.0f : (q1[0] == q2[0] ? 0.5f : 0.0f);
        A.s1.dout[(size_t)r * OW] = -w1 * inv_batch;
        A.s2.dout[(size_t)r * OW] = -(1.0f - w1) * inv_batch;
        atomicAdd(&A.losses[2], -fminf(q1[0], q2[0]) * inv_batch);
    }
}

// Gradient of the policy loss mean(-min Q - alpha H) (SAC/agent.py:404-406) wrt the policy head's 8 pre-activations: the
// critics' input gradients wrt the action (both heads; the unselected one carries zeros) chained through a = tanh(mean + sigma eps),
// plus the entropy term.  Also accumulates -alpha H / B (policy loss) and stores mean H (for the alpha step).
struct PDoutArgs {
    const float* q1net;
    const float* q2net;
    Mlp mq;
    Slot c1, c2, pol;
    const float* aux;
    const float* alpha_state;  // [4]: log_alpha, m, v, alpha
    int rows;
    float inv_batch;
    float* losses;
    const float* weights;  // WEIGHTED: [rows] importance weights (SAC/agent.py:405): inv_batch becomes w_r / B in the gradient and in the logged loss
    float* wsum;           // WEIGHTED: [2] <- mean(w H), mean(w) in a fixed order: what the weighted log-alpha step consumes (agent.py:408-414)
};
template <bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void policy_dout_kernel(PDoutArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= A.rows) return;
    const float inv_batch = WEIGHTED ? A.weights[r] * A.inv_batch : A.inv_batch;
    float da[4] = {0.f, 0.f, 0.f, 0.f};
    for (int hsel = 0; hsel < 2; ++hsel) {
        const Slot& C = hsel ? A.c2 : A.c1;
        const float* net = hsel ? A.q2net : A.q1net;
        RowReg<H1> dh, z;
        dh.load(C.dh1 + (size_t)r * H1);
        z.load(C.z1 + (size_t)r * H1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // hidden unit k = lane*4 + c; plain stack: dz1 = dh1 * relu'(z1)
            const int k = lane * 4 + c;
            const float dz1 = act_bwd<true>(dh.v[c], z.v[c], 0.0f);
            const float* w = net + A.mq.W1() + k * A.mq.in + 13;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) da[jj] += dz1 * w[jj];
        }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) da[jj] = wave_sum(da[jj]);
    const float alpha = A.alpha_state[3];
    if (lane < 4) {
        const float* x = A.aux + (size_t)r * 16;
        float d_mean, d_logstd;
        sac_policy_dout(lane == 0 ? da[0] : lane == 1 ? da[1] : lane == 2 ? da[2] : da[3], x[lane], x[4 + lane], x[8 + lane], alpha * inv_batch, d_mean, d_logstd);
        A.pol.dout[(size_t)r * OW + lane] = d_mean;
        A.pol.dout[(size_t)r * OW + 4 + lane] = d_logstd;
        if (lane == 0) atomicAdd(&A.losses[2], -alpha * x[12] * inv_batch);  // logged only
    }
    // The mean entropy feeds the log-alpha step, so it must not depend on arrival order: the per-row entropies were written by
    // the head kernel before this launch, one wave adds them in a fixed order.
    if (blockIdx.x == 0 && wave == 0) {
        float s = 0.0f;
        for (int rr = lane; rr < A.rows; rr += 64) s += A.aux[(size_t)rr * 16 + 12];
        s = wave_sum(s);
        if (lane == 0) A.losses[4] = s * A.inv_batch;  // (the UNWEIGHTED mean with weights too: stats/entropy, agent.py:351)
        if (WEIGHTED) {  // the same order, with the weights: at w == 1 mean(w H) has the bits of the mean entropy and mean(w) is exactly 1
            float sh = 0.0f, sw = 0.0f;
            for (int rr = lane; rr < A.rows; rr += 64) {
                sh += A.weights[rr] * A.aux[(size_t)rr * 16 + 12];
                sw += A.weights[rr];
            }
            sh = wave_sum(sh);
            sw = wave_sum(sw);
            if (lane == 0) { A.wsum[0] = sh * A.inv_batch; A.wsum[1] = sw / (float)A.rows; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// SAC with importance weights (prioritized replay; SAC/agent.py:361-374, 408-414): the critics' TD head and the log-alpha step as kernels of their
// own.  One wave per row.
// ---------------------------------------------------------------------------------------------------------------
// y = r + (1 - d) gamma (min Q_target(s', a') + alpha H'), errors = |Q1(s, a) - y|, q_h_loss += w (Q_h - y)^2 / B, head gradients 2 w (Q_h - y) / B:
// what bwd_l2<0>'s prologue (BM_CRITIC_TD) computes, per row and with the weight; the critics' backward then runs with the head gradient given.
struct TdHeadArgs {
    const float* q1net; const float* q2net; const float* t1net; const float* t2net;
    Mlp m;
    Slot s1, s2;                              // Q1 / Q2 (s, a): z2 read; st2 and dout written
    const float* z2_t1; const float* z2_t2;   // target Q1 / Q2 (s', a')
    const float* rows;                        // [rows][32]: reward, done in columns 30, 31
    const float* ent_next;                    // [rows] H'
    const float* alpha_state;
    const float* weights;
    int nrows;
    float gamma, inv_batch;
    float* errors;                            // [rows] out
    float* losses;
};
__global__ __launch_bounds__(kThreads) void td_head_weighted_kernel(TdHeadArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= A.nrows) return;
    float qmin, q1, q2;
    sac_td_heads<true>(A.m, r, {A.t1net, A.z2_t1, nullptr}, {A.t2net, A.z2_t2, nullptr}, {A.q1net, A.s1.z2, A.s1.st2}, {A.q2net, A.s2.z2, A.s2.st2}, qmin, q1, q2);
    if (lane == 0) {
        const float lab0 = A.rows[(size_t)r * 32 + 30], lab1 = A.rows[(size_t)r * 32 + 31];
        const float target = sac_td_target(lab0, lab1, A.gamma, qmin, A.ent_next[r], A.alpha_state[3]);
        const float wb = A.weights[r] * A.inv_batch;
        const float d1 = q1 - target, d2 = q2 - target;
        A.errors[r] = fabsf(d1);
        A.s1.dout[(size_t)r * OW] = 2.0f * d1 * wb;
        A.s2.dout[(size_t)r * OW] = 2.0f * d2 * wb;
        atomicAdd(&A.losses[0], d1 * d1 * wb);
        atomicAdd(&A.losses[1], d2 * d2 * wb);
    }
}
// entropy_loss = -mean(log_alpha (target_entropy - H) w) and alpha_optim.step() (agent.py:322-325, 408-414): sac_alpha_step on mean(w H) and
// target_entropy mean(w) (wsum[0], wsum[1]: policy_dout_kernel<true>'s).  One thread.
struct AlphaStepArgs {
    float* alpha_state; float* losses; const float* wsum;
    float target_entropy, b1, b2, eps, step_size, bc2_sqrt;
};
__global__ __launch_bounds__(64) void alpha_step_weighted_kernel(AlphaStepArgs A) {
    if (threadIdx.x != 0) return;
    sac_alpha_step(A.alpha_state, A.losses, A.wsum[0], A.target_entropy * A.wsum[1], A.b1, A.b2, A.eps, A.step_size, A.bc2_sqrt);
}

// ---------------------------------------------------------------------------------------------------------------
// SAC, imitative branch (SAC/agent.py:385-403): the per-row kernels of the BC-gated policy loss.  One wave per row.
// ---------------------------------------------------------------------------------------------------------------
// a_bc = bc_actor(s): the frozen LayerNorm actor's tanh head from its z2 rows (leaky slope = a parameter; SAC's own launches run as ReLU,
// so the bc_actor has a forward launch and this head kernel of its own)
struct BcHeadArgs {
    const float* net;
    Mlp m;
    const float* z2;
    float slope;
    int rows;
    float* act;  // [rows][4]
};
__global__ __launch_bounds__(kThreads) void bc_head_kernel(BcHeadArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= A.rows) return;
    RowReg<H2> xh, y;
    float mean_, rstd_, o[4];
    head_row4<false>(A.z2 + (size_t)r * H2, A.net, A.m, A.slope, xh, y, mean_, rstd_, o);
    if (lane < 4) A.act[(size_t)r * 4 + lane] = tanhf(lane == 0 ? o[0] : lane == 1 ? o[1] : lane == 2 ? o[2] : o[3]);
}

// bc_loss = mse(ae, tanh(mean)) * 10000 (agent.py:395-398) for ONE action component: the squared error and the gradient wrt the head's
// pre-activation mean_j, scale = 2 * 10000 / (4 B).  Contraction off, the products spelled out: whoever evaluates it rounds alike.
#pragma clang fp contract(off)
__device__ __forceinline__ void isac_bc_dout(float mean, float ae, float scale, float& d_mean, float& sq) {
    const float t = tanhf(mean);
    const float diff = t - ae;
    sq = diff * diff;
    d_mean = (scale * diff) * (1.0f - t * t);
}
#pragma clang fp contract(fast)

// Per minibatch row: the gate min(Q1, Q2)(s, a_bc) > min(Q1, Q2)(s, a~) (agent.py:390-393; strict >) counted as an INTEGER, so that
// bc_weight = count / B does not depend on arrival order; per expert row: the BC head gradient of the 8-wide Gaussian head — the four
// log_std outputs get exactly zero — and the row's squared error (summed in a fixed order by isac_finish_kernel).
struct IsacRowsArgs {
    const float* q1net;
    const float* q2net;
    Mlp mq;
    const float* z2_q1p; const float* z2_q2p;  // Q1 / Q2 (s, a~)
    const float* z2_q1b; const float* z2_q2b;  // Q1 / Q2 (s, a_bc)
    const float* policy;
    Mlp mp;
    Slot pe;                   // policy(s_e): z2 read, dout written
    const float* expert_rows;  // [rows][32]: the expert action in columns 13..16
    int rows;
    float scale;               // 2 * 10000 / (4 B)
    int* count;
    float* row_sq;             // [rows]
};
__global__ __launch_bounds__(kThreads) void isac_rows_kernel(IsacRowsArgs A) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= A.rows) return;
    RowReg<H2> xh, y;
    float mean_, rstd_, qa[1], qb[1];
    head_row<1, true>(A.z2_q1p + (size_t)r * H2, A.q1net, A.mq, 0.0f, xh, y, mean_, rstd_, qa);
    head_row<1, true>(A.z2_q2p + (size_t)r * H2, A.q2net, A.mq, 0.0f, xh, y, mean_, rstd_, qb);
    const float q = fminf(qa[0], qb[0]);
    head_row<1, true>(A.z2_q1b + (size_t)r * H2, A.q1net, A.mq, 0.0f, xh, y, mean_, rstd_, qa);
    head_row<1, true>(A.z2_q2b + (size_t)r * H2, A.q2net, A.mq, 0.0f, xh, y, mean_, rstd_, qb);
    const float bc_q = fminf(qa[0], qb[0]);
    if (lane == 0 && bc_q > q) atomicAdd(A.count, 1);
    float o[8];
    head_row<8, true>(A.pe.z2 + (size_t)r * H2, A.policy, A.mp, 0.0f, xh, y, mean_, rstd_, o);
    const int j = lane & 3;
    float d_mean, sq;
    isac_bc_dout(pick8(o, j), A.expert_rows[(size_t)r * 32 + 13 + j], A.scale, d_mean, sq);
    const float row_sq = sum16(lane < 4 ? sq : 0.0f);  // lanes 0..3 sit in the first 16-lane row
    if (lane < 4) {
        A.pe.dout[(size_t)r * OW + lane] = d_mean;
        A.pe.dout[(size_t)r * OW + 4 + lane] = 0.0f;
    }
    if (lane == 0) A.row_sq[r] = row_sq;
}

// One wave, after every part of the policy loss is complete: bc_loss (fixed-order sum) -> losses[6], bc_weight -> losses[7], and
// policy_loss = mean(-q - alpha H) (1 - w) + bc_loss w -> losses[2] (agent.py:400-403).  Contraction off: plain products and sums.
#pragma clang fp contract(off)
__global__ __launch_bounds__(64) void isac_finish_kernel(const float* row_sq, const int* count, int rows, float inv_batch, float* losses) {
    const int lane = threadIdx.x;
    float s = 0.0f;
    for (int rr = lane; rr < rows; rr += 64) s += row_sq[rr];
    s = wave_sum(s);
    if (lane == 0) {
        const float bc_loss = s * (2500.0f * inv_batch);  // 10000 * mean over B * 4 elements
        const float w = (float)(*count) * inv_batch;
        losses[6] = bc_loss;
        losses[7] = w;
        losses[2] = losses[2] * (1.0f - w) + bc_loss * w;
    }
}
#pragma clang fp contract(fast)

}  // namespace

extern "C" {

/* ------------------------------------------------------------------------------------------------------------------
 * SAC (hirl/agents/SAC/agent.py, the non-imitative branch train_sac.py uses).
 * Slots: 0 policy(s'), 1 policy(s), 2/3 Q1/Q2(s, a), 4/5 target Q1/Q2(s', a'), 6/7 Q1/Q2(s, a~)
 * ------------------------------------------------------------------------------------------------------------------ */
enum { SS_PN = 0, SS_PC, SS_Q1, SS_Q2, SS_T1, SS_T2, SS_Q1P, SS_Q2P };

int hx_sac_policy_param_count(void) { return kPolicy.padded(); }
int64_t hx_sac_workspace_floats(int32_t batch) { return hx_hirl_workspace_floats(batch) + 32 * (int64_t)batch; }

struct SacAux {
    float* act_n; float* ent_n; float* act_c; float* aux_c;
};
static SacAux sac_aux(const HxSacNets* N, int B) {
    float* p = N->ws + (size_t)S_COUNT * kSlotFloats * B;
    return SacAux{p, p + 4 * B, p + 5 * B, p + 9 * B};  // [B][4], [B], [B][4], [B][16]
}
static void launch_gauss(const GaussArgs& g0, const GaussArgs* g1, float* target, const float* source, int n, float tau, hipStream_t st,
                         uint16_t* images = nullptr) {
    GaussLaunch L{};
    if (images && n > 0) {  // SAC bf16 path: IM_TC1 / IM_TC2 follow the Polyak step of the target critics
        for (int h = 0; h < 2; ++h) { L.img[h] = images + (IM_TC1 + h) * kImgElems; L.seg_lo[h] = h * kQs.padded() + kQs.W2(); }
    }
    L.g[0] = g0;
    L.nb0 = (g0.rows + 3) / 4;
    L.nb_gauss = L.nb0;
    if (g1) { L.g[1] = *g1; L.nb_gauss += (g1->rows + 3) / 4; }
    L.target = target; L.source = source; L.n = n; L.tau = tau;
    const int nbp = n > 0 ? (n / 4 + kThreads) / kThreads : 0;
    hipLaunchKernelGGL(gauss_head_kernel, dim3((unsigned)(L.nb_gauss + nbp)), dim3(kThreads), 0, st, L);
}
static void sac_slots(const HxSacNets* N, int B, Slot* s) {
    for (int i = 0; i < S_COUNT; ++i) s[i] = carve_slot(N->ws + (size_t)i * kSlotFloats * B, B);
}
// what the launches of one learn() share: the workspace slots, the Gaussian heads' row buffers, the minibatch and the two critics
struct SacCtx {
    const HxSacNets* N;
    const HxSacBatch* Bt;
    int B;
    hipStream_t st;
    uint16_t* im;  // the SAC bf16 path's images (include/hirl4ucav.h), or NULL
    Slot s[S_COUNT];
    SacAux X;
    RowSrc src;
    const float* q1; const float* q2;
    SacCtx(const HxSacNets* N_, const HxSacBatch* Bt_, void* stream)
        : N(N_), Bt(Bt_), B(Bt_->batch), st((hipStream_t)stream), im(N_->w2_bf16_all), X(sac_aux(N_, Bt_->batch)), src{Bt_->rows, nullptr, nullptr, 0, 32},
          q1(N_->critic), q2(N_->critic + kQs.padded()) {
        sac_slots(N, B, s);
    }
};

/* Critic half of SacAgent.learn (SAC/agent.py:278-313): [Polyak of the target critics first when polyak_first], a', H' =
 * policy.sample(s') with eps_next, y = r + (1 - d) gamma (min Q_target(s', a') + alpha H'), q1_loss / q2_loss -> losses[0..1],
 * grad_critic.  Also evaluates policy(s) for the policy half.  Follow with hx_sac_adam(which = 0). */
// one_call (hx_sac_learn): the Polyak step rides behind the Gaussian heads' workgroups instead of in a launch of its own, and policy.sample(s)
// of the policy half is evaluated beside policy.sample(s') — the same arithmetic on the same values, two launches less
// launch 1 of SacAgent.learn: policy(s'), policy(s), Q1/Q2(s, a)
static void sac_launch_1(const SacCtx& C, FwdArgs& F) {
    const int B = C.B;
    F = FwdArgs{};
    F.njobs = 4; F.slope = 0.0f;
    F.zero_f = C.N->losses; F.zero_nf = 5;
    F.job[0] = FwdJob{C.N->policy, kPolicy, C.src, 17, 0, Head{}, nullptr, 0.f, C.s[SS_PN], B, 0, IM_ACTOR};
    F.job[1] = FwdJob{C.N->policy, kPolicy, C.src, 0, 0, Head{}, nullptr, 0.f, C.s[SS_PC], B, 1, IM_ACTOR};
    F.job[2] = FwdJob{C.q1, kQs, C.src, 0, 0, Head{}, nullptr, 0.f, C.s[SS_Q1], B, 1, IM_C1};
    F.job[3] = FwdJob{C.q2, kQs, C.src, 0, 0, Head{}, nullptr, 0.f, C.s[SS_Q2], B, 1, IM_C2};
    F.images = C.im;  // (NULL: fp32)
}
// a~, H = policy.sample(s) for the policy loss: beside policy.sample(s') in the one call, a launch of its own in the staged form
static GaussArgs gauss_cur(const SacCtx& C) {
    return GaussArgs{C.N->policy, kPolicy, C.s[SS_PC].z2, C.Bt->eps_cur, C.B, C.Bt->eps_cur ? 1 : 2, C.X.act_c, nullptr, C.X.aux_c, C.Bt->seed, 0x80000000u, C.Bt->call};
}
// a', H' = policy.sample(s') for the TD target
static GaussArgs gauss_next(const SacCtx& C) {
    return GaussArgs{C.N->policy, kPolicy, C.s[SS_PN].z2, C.Bt->eps_next, C.B, C.Bt->eps_next ? 1 : 2, C.X.act_n, C.X.ent_n, nullptr, C.Bt->seed, 0x40000000u, C.Bt->call};
}
// the one call's Gaussian launch: policy.sample(s') and policy.sample(s) together, the Polyak step of the targets (and their bf16 images) behind them
static void launch_gauss_both(const SacCtx& C, const HxHyper* Hy, bool polyak) {
    const GaussArgs G2 = gauss_cur(C);
    launch_gauss(gauss_next(C), &G2, C.N->target_critic, C.N->critic, polyak ? 2 * kQs.padded() : 0, Hy->tau, C.st, C.im);
}
// Both critics' backward launch down to dh1 on slots s[slot0], s[slot0 + 1].  BM_CRITIC_TD (bwd_l2<0>): y, losses and the head gradient in the prologue,
// from the target slots and H'; BM_SAC_QMIN (<4>): the min(Q1, Q2) selection in the prologue; BM_GIVEN (<3>): a per-row kernel left the head gradient
static int launch_critics_bwd(const SacCtx& C, int slot0, int mode, const HxHyper* Hy = nullptr) {
    const float* t1 = C.N->target_critic; const float* t2 = C.N->target_critic + kQs.padded();
    BwdArgs G{};
    G.njobs = 2; G.slope = 0.0f; G.inv_batch = 1.0f / C.B; G.losses = C.N->losses;
    for (int h = 0; h < 2; ++h) {
        BwdJob& J = G.job[h];
        J = BwdJob{};
        J.net = h ? C.q2 : C.q1; J.m = kQs; J.ws = C.s[slot0 + h]; J.rows = C.B; J.mode = mode;
        if (mode == BM_CRITIC_TD) {
            J.t1 = Head{t1, kQs, C.s[SS_T1]}; J.t2 = Head{t2, kQs, C.s[SS_T2]}; J.src = C.src; J.gamma = Hy->gamma;
            J.bonus = C.X.ent_n; J.bonus_scale = C.N->alpha_state + 3; J.loss_slot = h;
        }
        if (mode == BM_SAC_QMIN) { J.t1 = Head{h ? C.q1 : C.q2, kQs, C.s[slot0 + (1 - h)]}; J.loss_slot = h; }
        J.img_t = IM_C1_T + h;
    }
    G.images = C.im;
    return launch_bwd(mode == BM_CRITIC_TD ? 0 : mode == BM_SAC_QMIN ? 4 : 3, G, C.st);
}
// grad_critic from the slots of Q1 / Q2 (s, a).  adam_step > 0 (one GPU): q1_optim.step() / q2_optim.step() ride in the launch — the thread that
// produced a gradient steps it, and the critic's images follow its step
static void launch_critics_wg(const SacCtx& C, const HxHyper* Hy, int adam_step) {
    const HxSacNets* N = C.N;
    WgArgs W{};
    W.njobs = 2; W.slope = 0.0f; W.w_kind = 0; W.inv_batch = 1.0f / C.B;
    W.bf16 = C.im != nullptr;
    for (int h = 0; h < 2; ++h) {
        WgJob& J = W.job[h];
        J = WgJob{};
        J.net = h ? C.q2 : C.q1; J.grad = N->grad_critic + h * kQs.padded(); J.m = kQs;
        J.ws[0] = C.s[SS_Q1 + h]; J.rows[0] = C.B; J.nslots = 1; J.wmode[0] = 0;
        if (adam_step > 0) {
            J.p = N->critic + h * kQs.padded();
            J.mom = N->m_critic + h * kQs.padded(); J.var = N->v_critic + h * kQs.padded();
            if (C.im) { J.w2b = C.im + (IM_C1 + h) * kImgElems; J.w2tb = C.im + (IM_C1_T + h) * kImgElems; }
        }
    }
    if (adam_step > 0) {
        set_adam_scalars(W.ad, Hy->lr_critic, adam_step);
        W.ad.losses = N->losses;
    }
    launch_wg(W, adam_step > 0, C.st);
}
// hx_sac_learn_weighted[_clipped]'s departures from the critic half: the TD head as a per-row kernel with the importance weights (the critics'
// backward then runs with the head gradient given), and with clip_ws the weight-gradient launch without Adam, then the norm and the clipped step
struct SacWeighted {
    const float* weights; float* errors_out;
    float* clip_ws; float max_norm, target_entropy;
};
// skip_first: launch 1 has run already (as workgroups of hx_sac_front's launch)
static int sac_critic_grads_impl(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSample* S, int32_t polyak_first, void* stream,
                                 int adam_step = 0, bool one_call = false, bool skip_first = false, const SacWeighted* Wt = nullptr) {
    HX_REQUIRE(N && Bt && Hy && Bt->rows && Bt->batch > 0 && Bt->batch % 16 == 0, "hx_sac_critic_grads: bad arguments");
    if (int rc = sac_check_formats(N, "hx_sac_critic_grads")) return rc;
    const SacCtx C(N, Bt, stream);
    uint16_t* const im = C.im;
    hipStream_t st = C.st;
    const int B = C.B;
    SampleDev SD{};
    bool fused = false;
    if (S) {  // memory.sample(batch_size) inside the first forward launch (or, batch > 256, by the sampling launch right here)
        HX_REQUIRE(!S->bc_table && !S->idx_bc, "hx_sac_critic_grads_sampled: SAC has no BC minibatch");
        if (int rc = prepare_draw(S, B, const_cast<float*>(Bt->rows), nullptr, nullptr, stream, &SD, &fused)) return rc;
    }
    if (polyak_first && !one_call) {  // soft_update(critic_target, critic) BEFORE the update, agent.py:278-279
        launch_polyak(N->target_critic, N->critic, 2 * kQs.padded(), Hy->tau, nullptr, nullptr, 0, st);
        if (im)  // ... and the targets' bf16 images follow it
            for (int h = 0; h < 2; ++h) launch_pack_bf16(N->target_critic + h * kQs.padded() + kQs.W2(), im + (IM_TC1 + h) * kImgElems, false, st);
    }
    if (!skip_first) {   // policy(s'), policy(s), Q1/Q2(s, a)
        FwdArgs F;
        sac_launch_1(C, F);
        F.sample = fused ? &SD : nullptr;
        launch_fwd(F, st);
    }
    if (one_call) launch_gauss_both(C, Hy, polyak_first != 0);
    else launch_gauss(gauss_next(C), nullptr, nullptr, nullptr, 0, 0.0f, st);
    launch_target_q(C.s + SS_T1, N->target_critic, C.src, C.X.act_n, B, im, st);
    if (Wt) {  // y, errors, losses and the head gradients per row, with the weights; then both critics backward from them
        const TdHeadArgs T{C.q1, C.q2, N->target_critic, N->target_critic + kQs.padded(), kQs, C.s[SS_Q1], C.s[SS_Q2], C.s[SS_T1].z2, C.s[SS_T2].z2, Bt->rows,
                           C.X.ent_n, N->alpha_state, Wt->weights, B, Hy->gamma, 1.0f / B, Wt->errors_out, N->losses};
        hipLaunchKernelGGL(td_head_weighted_kernel, dim3((unsigned)((B + 3) / 4)), dim3(kThreads), 0, st, T);
    }
    if (int rc = launch_critics_bwd(C, SS_Q1, Wt ? BM_GIVEN : BM_CRITIC_TD, Hy)) return rc;  // (BM_CRITIC_TD: y, losses, dq in its prologue)
    const bool clip = Wt && Wt->clip_ws;
    launch_critics_wg(C, Hy, clip ? 0 : adam_step);
    if (clip) {
        if (int rc = sac_grad_norm(N, 0, Wt->clip_ws, st, "hx_sac_learn_weighted_clipped")) return rc;
        if (int rc = sac_clipped_step(N, Hy, 0, adam_step, 1.0f, Wt->target_entropy, Wt->max_norm, Wt->clip_ws, false, st, "hx_sac_learn_weighted_clipped")) return rc;
    }
    HX_CHECK_LAUNCH(Wt ? "hx_sac_learn_weighted" : "hx_sac_critic_grads");
    return 0;
}
int hx_sac_critic_grads(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, int32_t polyak_first, void* stream) {
    return sac_critic_grads_impl(N, Bt, Hy, nullptr, polyak_first, stream);
}
/* The same with memory.sample (SAC/agent.py:286-296) drawn and gathered inside its first launch (HxSample without a BC table; Bt->rows is
 * the output tile): bit-identical to hx_sample_batch followed by hx_sac_critic_grads. */
int hx_sac_critic_grads_sampled(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSample* S, int32_t polyak_first, void* stream) {
    HX_REQUIRE(S, "hx_sac_critic_grads_sampled: null sample description");
    return sac_critic_grads_impl(N, Bt, Hy, S, polyak_first, stream);
}

/* Policy half (SAC/agent.py:315-319, 376-406): a~, H = policy.sample(s) with eps_cur, Q1/Q2(s, a~) with the UPDATED critics,
 * policy_loss = mean(-min Q - alpha H) -> losses[2], mean entropy -> losses[4], grad_policy.  Follow with hx_sac_adam(which = 1). */
/* One GPU: hx_sac_critic_grads[_sampled] + hx_sac_adam(which = 0, grad_scale 1) as ONE call with the optimizer step inside the weight-gradient
 * launch (sample may be null: the minibatch was assembled by the caller).  Same Adam on the same gradients: bit-identical to the two calls. */
int hx_sac_critic_step(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSample* S, int32_t polyak_first, int32_t step, void* stream) {
    HX_REQUIRE(step >= 1, "hx_sac_critic_step: step is 1-based");
    return sac_critic_grads_impl(N, Bt, Hy, S, polyak_first, stream, step);
}

// ---- the pieces of the policy half: the plain sequence (sac_policy_grads_impl) runs them back to back, the imitative one (sac_policy_grads_imit_impl)
// ---- with its own launches in between.  The imitative branch is fp32 only: C.im is NULL there.
// staged form: a~, H = policy.sample(s) as a launch of its own (the one call evaluated it in the critic half's Gaussian launch)
static void launch_sample_cur(const SacCtx& C) { launch_gauss(gauss_cur(C), nullptr, nullptr, nullptr, 0, 0.0f, C.st); }
// Q1 / Q2 (s, a~) with the UPDATED critics, saved for their backward pass
static void launch_q_pi(const SacCtx& C) {
    FwdArgs F{};
    F.njobs = 2; F.slope = 0.0f;
    F.job[0] = FwdJob{C.q1, kQs, C.src, 0, 3, Head{}, C.X.act_c, 0.f, C.s[SS_Q1P], C.B, 1, IM_C1};
    F.job[1] = FwdJob{C.q2, kQs, C.src, 0, 3, Head{}, C.X.act_c, 0.f, C.s[SS_Q2P], C.B, 1, IM_C2};
    F.images = C.im;
    launch_fwd(F, C.st);
}
// [q_select] -> both critics backward down to dh1 -> [policy_dout] -> policy(s) backward.
// one call: min(Q1, Q2) is selected in the critics' backward prologue and the policy's head gradient is formed in the policy's backward
// prologue (bwd_l2<4> / <5>) — q_select_kernel and policy_dout_kernel as launches of their own are the staged form
// weights / wsum (hx_sac_learn_weighted): the staged form with the weighted per-row kernels
static int launch_policy_tail(const SacCtx& C, bool one_call, const float* weights = nullptr, float* wsum = nullptr) {
    const int B = C.B;
    const Slot* s = C.s;
    const HxSacNets* N = C.N;
    static const bool fold_env = !(getenv("HX_SAC_FOLD") && getenv("HX_SAC_FOLD")[0] == '0');  // A/B knob
    // The SAC bf16 path keeps the staged form: built in bf16, the folded one call gave policy b2 gradients that differ from the staged sequence's in
    // the last bit (77 of 512 entries at the first call; dW2 and every other gradient equal), so the fold has no bf16 instantiation (launch_bwd refuses).
    const bool fold = one_call && fold_env && !C.im && !weights;
    const unsigned nb = (unsigned)((B + 3) / 4);
    if (!fold) {
        QSelArgs Q{C.q1, C.q2, kQs, s[SS_Q1P], s[SS_Q2P], B, 1.0f / B, N->losses, weights};
        if (weights) hipLaunchKernelGGL(q_select_kernel<true>, dim3(nb), dim3(kThreads), 0, C.st, Q);
        else hipLaunchKernelGGL(q_select_kernel<false>, dim3(nb), dim3(kThreads), 0, C.st, Q);
    }
    if (int rc = launch_critics_bwd(C, SS_Q1P, fold ? BM_SAC_QMIN : BM_GIVEN)) return rc;  // both critics backward down to dh1
    if (!fold) {
        PDoutArgs P{C.q1, C.q2, kQs, s[SS_Q1P], s[SS_Q2P], s[SS_PC], C.X.aux_c, N->alpha_state, B, 1.0f / B, N->losses, weights, wsum};
        if (weights) hipLaunchKernelGGL(policy_dout_kernel<true>, dim3(nb), dim3(kThreads), 0, C.st, P);
        else hipLaunchKernelGGL(policy_dout_kernel<false>, dim3(nb), dim3(kThreads), 0, C.st, P);
    }
    BwdArgs G{};
    G.njobs = 1; G.slope = 0.0f; G.inv_batch = 1.0f / B; G.losses = N->losses;
    BwdJob& J = G.job[0];
    J = BwdJob{};
    J.net = N->policy; J.m = kPolicy; J.ws = s[SS_PC]; J.rows = B; J.mode = fold ? BM_SAC_POLICY : BM_GIVEN;
    if (fold) {
        J.t1 = Head{C.q1, kQs, s[SS_Q1P]}; J.t2 = Head{C.q2, kQs, s[SS_Q2P]};
        J.bonus = C.X.aux_c; J.bonus_scale = N->alpha_state + 3;
    }
    J.img_t = IM_ACTOR_T;
    G.images = C.im;
    return launch_bwd(fold ? 5 : 3, G, C.st);
}
// The policy's weight-gradient launch: W carries the caller's slots, weights and predraw; slot 0 is policy(s).  adam_step > 0 (the one call):
// policy_optim.step() + the log-alpha step ride in it (the thread that produced a gradient steps it; thread 0 of the launch steps log_alpha)
// alpha_step = false (hx_sac_learn_weighted): the log-alpha step is a launch of its own behind this one
static void launch_policy_wg(WgArgs& W, const SacCtx& C, const HxHyper* Hy, int adam_step, float target_entropy, bool alpha_step = true) {
    const HxSacNets* N = C.N;
    W.njobs = 1; W.slope = 0.0f; W.inv_batch = 1.0f / C.B;
    WgJob& J = W.job[0];
    J.net = N->policy; J.grad = N->grad_policy; J.m = kPolicy; J.ws[0] = C.s[SS_PC]; J.rows[0] = C.B;
    if (adam_step > 0) {
        J.p = N->policy; J.mom = N->m_policy; J.var = N->v_policy;
        J.w2f = N->policy_w2_f32i;  // the acting kernels' images of the policy's W2 follow its optimizer step
        if (N->policy_w2_x9) { J.w2b = N->policy_w2_x9; J.w2b_x9 = 1; }
        if (N->policy_w2_bf16) J.w2b = N->policy_w2_bf16;  // bf16 acting beside an fp32 update
        if (C.im) { J.w2b = C.im + IM_ACTOR * kImgElems; J.w2tb = C.im + IM_ACTOR_T * kImgElems; }  // the bf16 path: forward (= acting) and transposed images
        set_adam_scalars(W.ad, Hy->lr_actor, adam_step);
        W.ad.losses = N->losses;
        if (alpha_step && !std::isnan(target_entropy)) { W.ad.alpha_state = N->alpha_state; W.ad.target_entropy = target_entropy; W.ad.alpha_step_size = W.ad.step_size; }  // (alpha_optim: the policy's learning rate)
    }
    launch_wg(W, adam_step > 0, C.st);
}

// adam_step > 0 (hx_sac_learn): policy.sample(s) was evaluated in the critic half's launch, and the optimizer steps ride in the weight-gradient launch
static int sac_policy_grads_impl(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, void* stream, int adam_step, float target_entropy,
                                 const SampleDev* predraw = nullptr) {
    HX_REQUIRE(N && Bt && Hy && Bt->rows && Bt->batch > 0 && Bt->batch % 16 == 0, "hx_sac_policy_grads: bad arguments");
    if (int rc = sac_check_formats(N, "hx_sac_policy_grads")) return rc;
    const SacCtx C(N, Bt, stream);
    if (adam_step == 0) launch_sample_cur(C);
    launch_q_pi(C);
    if (int rc = launch_policy_tail(C, adam_step > 0)) return rc;
    WgArgs W{};
    W.bf16 = C.im != nullptr;
    W.job[0].nslots = 1;
    W.predraw = predraw; W.predraw_batch = C.B;  // hx_sac_learn_back: one more workgroup assembles the next front launch's minibatch (112 workgroups: CUs to spare)
    launch_policy_wg(W, C, Hy, adam_step, target_entropy);
    HX_CHECK_LAUNCH("hx_sac_policy_grads");
    return 0;
}
int hx_sac_policy_grads(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, void* stream) {
    return sac_policy_grads_impl(N, Bt, Hy, stream, 0, 0.0f);
}
/* One GPU: the whole SacAgent.learn (SAC/agent.py:276-327) in ONE call and 9 launches (the staged sequence takes 14): the Polyak step and
 * policy.sample(s) ride in the launch of policy.sample(s'), both optimizers' steps (and the log-alpha step) in their weight-gradient launches,
 * the min(Q1, Q2) selection and the policy's head gradient in the prologues of the backward launches that consume them.
 * Bit-identical to hx_sac_critic_step + hx_sac_policy_grads + hx_sac_adam(which = 1).  sample may be NULL; step is 1-based. */
int hx_sac_learn(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSample* S, int32_t polyak_first, int32_t step, float target_entropy,
                 void* stream) {
    HX_REQUIRE(step >= 1, "hx_sac_learn: step is 1-based");
    if (int rc = sac_critic_grads_impl(N, Bt, Hy, S, polyak_first, stream, step, true)) return rc;
    return sac_policy_grads_impl(N, Bt, Hy, stream, step, target_entropy);
}

/* SacAgent.learn with per-row importance weights (prioritized replay: SAC/agent.py:306-331, 361-374, 405, 408-414).  One GPU, fp32.  hx_sac_learn's
 * staged helpers with the weighted per-row kernels in between (+), 13 launches (the one call: 9):
 *     fwd_l2      policy(s'), policy(s), Q1 / Q2 (s, a); clears the loss sums
 *     gauss       a', H' = policy.sample(s') and a~, H = policy.sample(s)  [+ the Polyak step of the targets behind them]
 *     fwd_l2      target Q1 / Q2 (s', a')
 *   + td_head     y, errors_out = |Q1 - y|, q_h_loss += w (Q_h - y)^2 / B, head gradients 2 w (Q_h - y) / B
 *     bwd_l2<3>   both critics, head gradient given (instead of BM_CRITIC_TD's own TD head)
 *     wgrad       critics + q1_optim / q2_optim steps
 *     fwd_l2      Q1 / Q2 (s, a~) with the updated critics
 *   + q_select<weighted>, bwd_l2<3> (critics), + policy_dout<weighted> (also mean(w H), mean(w)), bwd_l2<3> (policy)
 *     wgrad       policy + policy_optim step (WITHOUT the log-alpha step)
 *   + alpha_step  entropy_loss and alpha_optim.step() from mean(w H) - target_entropy mean(w) */
// clip_ws != NULL (hx_sac_learn_weighted_clipped): both weight-gradient launches run without Adam, each followed by the norm and the clipped step
static int sac_learn_weighted_impl(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const float* weights, float* errors_out, int32_t polyak_first,
                                   int32_t step, float target_entropy, float max_norm, float* clip_ws, void* stream) {
    HX_REQUIRE(step >= 1, "hx_sac_learn_weighted: step is 1-based");
    HX_REQUIRE(N && Bt && Hy && Bt->rows && Bt->batch > 0 && Bt->batch % 16 == 0 && weights && errors_out, "hx_sac_learn_weighted: bad arguments (nets, batch, hyper, weights, errors_out)");
    HX_REQUIRE(!N->w2_bf16_all, "hx_sac_learn_weighted: the weighted update is fp32 only (nets->w2_bf16_all must be NULL)");
    if (int rc = sac_check_formats(N, "hx_sac_learn_weighted")) return rc;
    const SacWeighted Wt{weights, errors_out, clip_ws, max_norm, target_entropy};
    if (int rc = sac_critic_grads_impl(N, Bt, Hy, nullptr, polyak_first, stream, step, /*one_call=*/true, /*skip_first=*/false, &Wt)) return rc;
    const SacCtx C(N, Bt, stream);
    hipStream_t st = C.st;
    float* const wsum = C.X.aux_c + 16 * (size_t)C.B;  // two of the workspace's spare words behind the Gaussian heads' row buffers
    launch_q_pi(C);
    if (int rc = launch_policy_tail(C, false, weights, wsum)) return rc;
    {
        WgArgs W{};
        W.job[0].nslots = 1;
        launch_policy_wg(W, C, Hy, clip_ws ? 0 : step, target_entropy, /*alpha_step=*/false);
        if (clip_ws) {
            if (int rc = sac_grad_norm(N, 1, clip_ws, st, "hx_sac_learn_weighted_clipped")) return rc;
            if (int rc = sac_clipped_step(N, Hy, 1, step, 1.0f, target_entropy, max_norm, clip_ws, false, st, "hx_sac_learn_weighted_clipped")) return rc;
        }
    }
    if (!std::isnan(target_entropy)) {  // (NaN = HX_SAC_FIXED_ALPHA: no log-alpha optimiser)
        AlphaStepArgs A{N->alpha_state, N->losses, wsum, target_entropy, 0.f, 0.f, 0.f, 0.f, 0.f};
        set_adam_scalars(A, Hy->lr_actor, step);  // (alpha_optim: the policy's learning rate)
        hipLaunchKernelGGL(alpha_step_weighted_kernel, dim3(1), dim3(64), 0, st, A);
    }
    HX_CHECK_LAUNCH("hx_sac_learn_weighted");
    return 0;
}
int hx_sac_learn_weighted(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const float* weights, float* errors_out, int32_t polyak_first,
                          int32_t step, float target_entropy, void* stream) {
    return sac_learn_weighted_impl(N, Bt, Hy, weights, errors_out, polyak_first, step, target_entropy, 0.0f, nullptr, stream);
}
int hx_sac_learn_weighted_clipped(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const float* weights, float* errors_out, int32_t polyak_first,
                                  int32_t step, float target_entropy, float max_norm, float* clip_ws, void* stream) {
    HX_REQUIRE(clip_ws && max_norm > 0.0f, "hx_sac_learn_weighted_clipped: clip_ws (hx_sac_clip_floats() floats) and a positive max_norm");
    return sac_learn_weighted_impl(N, Bt, Hy, weights, errors_out, polyak_first, step, target_entropy, max_norm, clip_ws, stream);
}

/* ------------------------------------------------------------------------------------------------------------------
 * SAC, imitative branch (SAC/agent.py:315-318, 353-359, 385-403; imitative=True).  The critic half is the code above, unchanged.  The policy half
 * is sac_policy_grads_impl's sequence — the same helpers — with the BC-gated loss around it (new launches marked +):
 *     [gauss        a~, H = policy.sample(s)                                     staged form only]
 *   + fwd_l2        bc_actor(s): LayerNorm actor, leaky slope = imit->bc_slope (a launch of its own: the activation is per launch); clears count
 *   + bc_head       a_bc = tanh(head(bc_actor))
 *     fwd_l2        Q1 / Q2 (s, a~), saved                                       (the launch of the plain call, same tiling: same bits)
 *   + fwd_l2        Q1 / Q2 (s, a_bc) values only, policy(s_e) saved on the B expert rows
 *   + isac_rows     count += min Q(s, a_bc) > min Q(s, a~) per row (integer); the BC head gradient of policy(s_e), log_std outputs exactly 0
 *   + bwd_l2<3>     policy(s_e) down to dh1
 *     [q_select] bwd_l2 (critics) [policy_dout] bwd_l2 (policy(s))               as in the plain call (folded prologues in the one call)
 *   + isac_finish   losses[6] = bc_loss, losses[7] = bc_weight = count / B, losses[2] = policy_loss (1 - w) + bc_loss w
 *     wgrad         ONE launch over both policy slots: slot 0 = policy(s) scaled (1 - w), slot 1 = policy(s_e) scaled w, w read from the count
 *                   (+ Adam and the log-alpha step in the one call)
 * Departures from the reference: bc_actor is the 13-input LayerNorm actor this project's BC agent writes (the reference builds a 14-input one
 * against a 13-wide observation and crashes); WHICH expert rows are drawn is not claimed (Philox on the device, as hx_sample_batch).
 * Imitative workspace: slots 0 bc_actor(s), 1 / 2 Q1 / Q2 (s, a_bc), 3 policy(s_e); then a_bc [B][4] and the per-row squared errors [B].
 * ------------------------------------------------------------------------------------------------------------------ */
enum { IS_BCA = 0, IS_Q1B, IS_Q2B, IS_PE, IS_COUNT };
int hx_sac_imit_sizeof(void) { return (int)sizeof(HxSacImit); }
int64_t hx_sac_imit_workspace_floats(int32_t batch) { return (int64_t)IS_COUNT * (int64_t)kSlotFloats * batch + 8 * (int64_t)batch; }

static int sac_policy_grads_imit_impl(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSacImit* I, void* stream, int adam_step,
                                      float target_entropy, const char* who) {
    HX_REQUIRE(N && Bt && Hy && Bt->rows && Bt->batch > 0 && Bt->batch % 16 == 0, "%s: bad arguments", who);
    HX_REQUIRE(I && I->bc_actor && I->expert_rows && I->ws && I->count, "%s: imit needs bc_actor, expert_rows, ws and count", who);
    HX_REQUIRE(I->bc_slope >= 0.0f && I->bc_slope < 1.0f, "%s: imit->bc_slope is the bc_actor's leaky slope, in [0, 1)", who);
    HX_REQUIRE(!N->w2_bf16_all, "%s: the imitative branch is fp32 only (nets->w2_bf16_all must be NULL)", who);
    if (int rc = sac_check_formats(N, who)) return rc;
    const SacCtx C(N, Bt, stream);
    hipStream_t st = C.st;
    const int B = C.B;
    Slot si[IS_COUNT];
    for (int i = 0; i < IS_COUNT; ++i) si[i] = carve_slot(I->ws + (size_t)i * kSlotFloats * B, B);
    float* const a_bc = I->ws + (size_t)IS_COUNT * kSlotFloats * B;
    float* const row_sq = a_bc + 4 * (size_t)B;
    const RowSrc esrc{I->expert_rows, nullptr, nullptr, 0, 32};
    const unsigned nb = (unsigned)((B + 3) / 4);
    if (adam_step == 0) launch_sample_cur(C);
    {   // bc_actor(s), no gradient
        FwdArgs F{};
        F.njobs = 1; F.slope = I->bc_slope;
        F.zero_i = I->count;
        F.job[0] = FwdJob{I->bc_actor, kActor, C.src, 0, 0, Head{}, nullptr, 0.f, si[IS_BCA], B, 0, IM_BC};
        launch_fwd(F, st);
        BcHeadArgs H{I->bc_actor, kActor, si[IS_BCA].z2, I->bc_slope, B, a_bc};
        hipLaunchKernelGGL(bc_head_kernel, dim3(nb), dim3(kThreads), 0, st, H);
    }
    launch_q_pi(C);
    {   // Q1 / Q2 (s, a_bc): values only; policy(s_e), saved for its backward pass
        FwdArgs F{};
        F.njobs = 3; F.slope = 0.0f;
        F.job[0] = FwdJob{C.q1, kQs, C.src, 0, 3, Head{}, a_bc, 0.f, si[IS_Q1B], B, 0, IM_C1};
        F.job[1] = FwdJob{C.q2, kQs, C.src, 0, 3, Head{}, a_bc, 0.f, si[IS_Q2B], B, 0, IM_C2};
        F.job[2] = FwdJob{N->policy, kPolicy, esrc, 0, 0, Head{}, nullptr, 0.f, si[IS_PE], B, 1, IM_ACTOR};
        launch_fwd(F, st);
    }
    {   // the gate's count, the BC head gradient
        IsacRowsArgs R{C.q1, C.q2, kQs, C.s[SS_Q1P].z2, C.s[SS_Q2P].z2, si[IS_Q1B].z2, si[IS_Q2B].z2, N->policy, kPolicy, si[IS_PE], I->expert_rows, B,
                       (2.0f * 10000.0f * 0.25f) / B, I->count, row_sq};
        hipLaunchKernelGGL(isac_rows_kernel, dim3(nb), dim3(kThreads), 0, st, R);
    }
    {   // policy(s_e) backward down to dh1
        BwdArgs G{};
        G.njobs = 1; G.slope = 0.0f; G.inv_batch = 1.0f / B; G.losses = N->losses;
        BwdJob& J = G.job[0];
        J = BwdJob{};
        J.net = N->policy; J.m = kPolicy; J.ws = si[IS_PE]; J.rows = B; J.mode = BM_GIVEN; J.img_t = IM_ACTOR_T;
        if (int rc = launch_bwd(3, G, st)) return rc;
    }
    if (int rc = launch_policy_tail(C, adam_step > 0)) return rc;
    // both parts of the policy loss are complete: combine them (a launch of its own rather than thread 0 of the weight-gradient launch, whose
    // SAC step already carries the log-alpha state in the fields HIRL's finish_actor uses — and whose register figures stay what they were)
    hipLaunchKernelGGL(isac_finish_kernel, dim3(1), dim3(64), 0, st, row_sq, I->count, B, 1.0f / B, N->losses);
    WgArgs W{};
    W.w_kind = 1; W.warm = 0.0f; W.soft_count = I->count;
    WgJob& J = W.job[0];
    J.nslots = 2;
    J.wmode[0] = 1;                                        // policy(s):   (1 - w)
    J.ws[1] = si[IS_PE]; J.rows[1] = B; J.wmode[1] = 2;    // policy(s_e): w
    launch_policy_wg(W, C, Hy, adam_step, target_entropy);
    HX_CHECK_LAUNCH(who);
    return 0;
}
/* Staged form, gradients only: follow with hx_sac_adam(which = 1). */
int hx_sac_policy_grads_imitative(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSacImit* I, void* stream) {
    return sac_policy_grads_imit_impl(N, Bt, Hy, I, stream, 0, 0.0f, "hx_sac_policy_grads_imitative");
}
/* One GPU: the whole imitative SacAgent.learn in one call.  Bit-identical to hx_sac_critic_step + hx_sac_policy_grads_imitative +
 * hx_sac_adam(which = 1).  expert_sample NULL: the expert rows are in imit->expert_rows already; else the B rows are drawn from the expert
 * memory it describes (total / cap / ring: the expert ring as the main ring, n_main = batch) as hx_sample_batch draws them. */
int hx_sac_learn_imitative(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, const HxSample* S, const HxSacImit* I, const HxSample* ES,
                           int32_t polyak_first, int32_t step, float target_entropy, void* stream) {
    HX_REQUIRE(step >= 1, "hx_sac_learn_imitative: step is 1-based");
    HX_REQUIRE(N && Bt && I && I->bc_actor && I->expert_rows && I->ws && I->count, "hx_sac_learn_imitative: imit needs bc_actor, expert_rows, ws and count");
    HX_REQUIRE(!N->w2_bf16_all, "hx_sac_learn_imitative: the imitative branch is fp32 only (nets->w2_bf16_all must be NULL)");
    if (ES) {
        HX_REQUIRE(ES->n_main == Bt->batch && !ES->expert_ring && !ES->bc_table && !ES->idx_bc && !ES->guard && ES->idx,
                   "hx_sac_learn_imitative: expert_sample describes the expert memory as the main ring (n_main = batch, idx; no expert ring, BC table or guard)");
        if (int rc = hx_sample_batch(ES->total, ES->cap, ES->ring, nullptr, 0, nullptr, 0, Bt->batch, Bt->batch, 1, ES->seed, ES->call, 0.0f, ES->idx,
                                     nullptr, nullptr, I->expert_rows, nullptr, stream)) return rc;
    }
    if (int rc = sac_critic_grads_impl(N, Bt, Hy, S, polyak_first, stream, step, true)) return rc;
    return sac_policy_grads_imit_impl(N, Bt, Hy, I, stream, step, target_entropy, "hx_sac_learn_imitative");
}

/* hx_sac_learn in two parts around an env step (include/hirl4ucav.h "SAC front launch"): hx_sac_front = hx_sac_act_step for n envs AND the first
 * forward launch of the learn() call behind it as workgroups of ONE launch, on the minibatch tiles a predraw left in `batch`; hx_sac_learn_back = the rest. */
int hx_sac_front(const float* policy, const uint16_t* w2_x9, const float* w2_f32i, float* state, int64_t n, int64_t stride, float* obs_io, float* actions, int32_t mode,
                 const float* eps, uint64_t seed, uint32_t row0, uint32_t call, float* reward, uint8_t* done, int8_t* success, const HxStepOpts* opts,
                 const HxSacNets* N, const HxSacBatch* Bt, void* stream) {
    HX_REQUIRE(N && opts && Bt && Bt->rows && Bt->batch > 0 && Bt->batch % 16 == 0 && Bt->batch <= kFusedBatchMax && mode >= 0 && mode <= 2 &&
               (mode != 1 || eps), "hx_sac_front: bad arguments");
    if (int rc = sac_check_formats(N, "hx_sac_front")) return rc;
    HX_REQUIRE(N->w2_bf16_all || !N->policy_w2_bf16,
               "hx_sac_front: bf16 acting beside the fp32 update (policy_w2_bf16 without w2_bf16_all) has no front form: hx_sac_act_step + hx_sac_learn");
    // the acting format follows nets: the bf16 path acts from its first image (the image arguments must be NULL), the fp32 update from w2_x9 / w2_f32i
    const uint16_t* w2b = N->w2_bf16_all ? sac_act_image(N) : nullptr;
    HX_REQUIRE(policy && (w2b ? (!w2_x9 && !w2_f32i) : (w2_x9 || w2_f32i)),
               "hx_sac_front: with nets->w2_bf16_all the acting image is its first one (w2_x9, w2_f32i NULL); else w2_x9 or w2_f32i");
    const hxact::ActEnv E{state, stride, reward, done, success, *opts};
    if (int rc = hxact::check_step_args(obs_io, n, actions, E, "hx_sac_front")) return rc;
    // up to 8,192 envs the exact-split image plays no part (as in hx_sac_act_step: the per-tile workgroups act from the fp32 image, which must then be given)
    if (n <= hxact::kFuseEnvMax) w2_x9 = nullptr;
    HX_REQUIRE(w2b || w2_x9 || w2_f32i, "hx_sac_front: up to 8,192 envs the fp32 policy acts from the fp32 image: w2_f32i must be given");
    if (int rc = hxact::check_images16("hx_sac_front", "the acting image of W2 must be 16-byte aligned", {w2b ? (const void*)w2b : w2_x9 ? (const void*)w2_x9 : (const void*)w2_f32i})) return rc;
    const hxact::ActFusedArgs H = hxact::act_args_gauss(policy, obs_io, n, actions, mode, eps, seed, row0, call, hxact::ActImages{w2_f32i, w2_x9, w2b}, &E);
    FwdArgs F;
    sac_launch_1(SacCtx(N, Bt, stream), F);
    return launch_front_sac(H, F, (hipStream_t)stream);
}
/* Rebuild every bf16 image of the SAC bf16 path from the fp32 networks (after parameters were loaded or written directly), and the bf16 acting
 * image policy_w2_bf16 when it is a buffer of its own. */
int hx_sac_pack_update_images(const HxSacNets* N, void* stream) {
    HX_REQUIRE(N && N->policy && (N->w2_bf16_all || N->policy_w2_bf16), "hx_sac_pack_update_images: the policy and w2_bf16_all or policy_w2_bf16");
    if (int rc = sac_check_formats(N, "hx_sac_pack_update_images")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (uint16_t* im = N->w2_bf16_all) {
        HX_REQUIRE(N->critic && N->target_critic, "hx_sac_pack_update_images: null critic");
        launch_pack_bf16(N->policy + kPolicy.W2(), im + IM_ACTOR * kImgElems, false, st);
        launch_pack_bf16(N->policy + kPolicy.W2(), im + IM_ACTOR_T * kImgElems, true, st);
        for (int h = 0; h < 2; ++h) {
            launch_pack_bf16(N->critic + h * kQs.padded() + kQs.W2(), im + (IM_C1 + h) * kImgElems, false, st);
            launch_pack_bf16(N->critic + h * kQs.padded() + kQs.W2(), im + (IM_C1_T + h) * kImgElems, true, st);
            launch_pack_bf16(N->target_critic + h * kQs.padded() + kQs.W2(), im + (IM_TC1 + h) * kImgElems, false, st);
        }
    } else {
        launch_pack_bf16(N->policy + kPolicy.W2(), N->policy_w2_bf16, false, st);
    }
    HX_CHECK_LAUNCH("hx_sac_pack_update_images");
    return 0;
}

int hx_sac_learn_back(const HxSacNets* N, const HxSacBatch* Bt, const HxHyper* Hy, int32_t polyak_first, int32_t step, float target_entropy, const HxSample* next,
                      float* next_rows, void* stream) {
    HX_REQUIRE(step >= 1 && N && Bt && Hy, "hx_sac_learn_back: step is 1-based");
    SampleDev SD{};
    if (next) {
        HX_REQUIRE(next_rows && next_rows != Bt->rows && !next->bc_table && !next->idx_bc, "hx_sac_learn_back: the next minibatch needs a tile of its own; SAC has no BC minibatch");
        bool fused = false;
        if (int rc = prepare_draw(next, Bt->batch, next_rows, nullptr, nullptr, stream, &SD, &fused, /*launch_now=*/false)) return rc;
        HX_REQUIRE(fused, "hx_sac_learn_back: the predraw covers minibatches of at most 256 rows");
    }
    if (int rc = sac_critic_grads_impl(N, Bt, Hy, nullptr, polyak_first, stream, step, true, /*skip_first=*/true)) return rc;
    return sac_policy_grads_impl(N, Bt, Hy, stream, step, target_entropy, next ? &SD : nullptr);
}

}  // extern "C"

namespace hxu {
// (host code only)
void launch_target_q(const Slot* slots, const float* target_critic, const RowSrc& src, const float* act, int rows, const uint16_t* images, hipStream_t st) {
    FwdArgs F{};
    F.njobs = 2; F.slope = 0.0f;
    for (int h = 0; h < 2; ++h) F.job[h] = FwdJob{target_critic + h * kQs.padded(), kQs, src, 17, 3, Head{}, act, 0.f, slots[h], rows, 0, IM_TC1 + h};
    F.images = images;
    launch_fwd(F, st);
}
void launch_sac_gauss_rows(const float* policy, const float* z2, const float* eps, int rows, float* act, float* ent, uint64_t seed, uint32_t row0,
                           uint32_t call, hipStream_t st) {
    launch_gauss(GaussArgs{policy, kPolicy, z2, eps, rows, eps ? 1 : 2, act, ent, nullptr, seed, row0, call}, nullptr, nullptr, nullptr, 0, 0.0f, st);
}
}  // namespace hxu
