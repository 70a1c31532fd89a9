// hx_wgrad.hip — parameter gradients and optimizer steps (gfx950).
//   wgrad    all parameter gradients of one MLP block into the flat gradient buffer; on one GPU the same threads apply Adam, the Polyak step of
//            the target and refresh the W2 images                                   (loss.backward() + optimizer.step(), HIRL.py:284-288,322-330)
//   wgrad2   the same for ONE job with TWO slots of at most 256 rows together (the actor step, SAC's imitative policy step; fp32): each slot on
//            its own threads, 224 workgroups instead of 112, bit-identical (launch_wg chooses; HX_WGRAD_TWO_SLOT=0 keeps wgrad)
//   head riders  (wgrad only) workgroups beyond the jobs' own evaluate the head of up to two nets the launch does not change, once per row: the actor
//            call's actor(s) [and bc_actor(s)] in the critics' launch, for launch G to read instead of repeating it per column workgroup (HX_HEAD_RIDER=0: off)
//   adam     torch.optim.Adam defaults over a flat buffer (sharded path, SAC, BC)   (HIRL.py:50,123; SAC/agent.py:310-325)
//   polyak   soft_update                                                             (HIRL.py:11-13)
#include <cmath>

#include "hx_update.h"

using namespace hxnn;
using namespace hxu;

namespace {

// compact kernel argument (see FwdJobC): 128 bytes per job; everything a workgroup needs before its first vector load is in its own job
struct WgJobC {
    const float* net; float* grad;
    float* ws0; float* ws1;
    float* mom; float* var; float* target; uint16_t* w2b; float* w2f;
    uint32_t cfg;  // m:10 | nslots:2 | wmode0:2 | wmode1:2 | w_kind:2 | adam.finish_actor:1 | adam.use_bc:1 | w2b_x9:1 | sac_alpha:1
                   // (sac_alpha: a SAC policy step — wstate holds alpha_state, w_given the target entropy, warm the log-alpha step size)
    int32_t rows0, rows1;
    float slope, w_given, warm, inv_batch;
    float b1, b2, eps, step_size, bc2_sqrt, tau;
    uint32_t pad_;
    const int* soft_count; float* wstate; float* losses;
    uint16_t* w2tb; uint16_t* tgt_w2b;  // bf16 update path: the transposed image of W2 and the image of the target's W2
    float* count_out;                    // job 0 only: (float)*soft_count goes here (the merged actor message of a sharded run)
};
static_assert(sizeof(WgJobC) == 176, "WgJobC layout");
// a head rider's job: the net, the slot that holds its z2 rows, and how many
struct HeadJobC {
    const float* net; float* ws;
    int32_t rows;     // 0: no such job
    uint32_t cfg;     // m:10
};
struct WgArgsC {
    WgJobC job[2];
    HeadJobC head[2];
    // hx_hirl_learn_back: workgroup (kWgPerJob, 0) — one beyond the jobs' own, on a CU this launch leaves idle — assembles the next front launch's minibatch
    int has_pre, pre_batch;
    SampleDev pre;
};

// One parameter of the fused step: Adam with the gradient just produced, then (optionally) Polyak of the target and the bf16 image.
// p/m/v/t are this element's values requested at kernel entry (their latency hides under the gradient's own operand loads).
struct AdamElem {
    float p, m, v, t;
    __device__ __forceinline__ void fetch(const WgJob& J, unsigned idx) {
        p = J.p[idx];
        m = J.mom[idx];
        v = J.var[idx];
        t = J.target ? J.target[idx] : 0.0f;
    }
    __device__ __forceinline__ void apply(const WgJob& J, const WgAdam& a, unsigned idx, float g) {
        adam_update(p, m, v, g, a.b1, a.b2, a.eps, a.step_size, a.bc2_sqrt);
        J.p[idx] = p;
        J.mom[idx] = m;
        J.var[idx] = v;
        if (J.target) {
            t = polyak_update(t, p, a.tau);
            J.target[idx] = t;
        }
    }
};

// 112 workgroups per job: the critic launch (two jobs) is 224 of the 256 CUs, ONE round.  Half the rows per thread of the 56-workgroup
// partition before it: a workgroup's time is its operands' round trip plus rows-per-thread of arithmetic, and the launch is as long as
// its slowest workgroup.
constexpr int kWgTilesPerBlock = 2 * (H2 / 16);          // 64 workgroups: 16 (n) x 128 (k) of dW2; a 16 x 16 tile per wave PAIR, each half of the rows
constexpr int kWgCols = 16;                              // columns per vector / layer-1 workgroup (a quarter wave)
constexpr int kWgVecWgs = H2 / kWgCols;                  // 32 workgroups: 16 columns x 64 row groups, 512-wide vector gradients
constexpr int kWgL1Wgs = H1 / kWgCols;                   // 16 workgroups: layer-1 gradients, 16 units x 64 row groups
constexpr int kWgRG = kWide / kWgCols;                   // row groups = quarter waves: the batch rows of a column are split 64 ways
constexpr int kWgPerJob = kWgTilesPerBlock + kWgVecWgs + kWgL1Wgs;
constexpr int kWgRowChunk = 256;                         // rows whose per-row scalars are staged in LDS at a time

// fixed-order sum of the 16 row groups' partial results of one (column, item): red[group][64][kRedP]; the odd pitch keeps the 64 lanes of a
// wave on 64 different banks (pitch 20: 16 banks, every read and write of the reduction four-way conflicted)
constexpr int kRedP = 21;
// two threads per (column, item): each sums 32 of the 64 row groups (tree) — the even groups / the odd groups: one group apart is 16 banks
// apart, so the pair's reads never meet on a bank (groups 0..31 / 32..63 would: 32 groups are a multiple of 32 banks) — the even lane
// adds its neighbour's sum (one DPP move)
template <int COLS = kWgCols>
__device__ __forceinline__ float sum_groups(const float* p, int half) {
    constexpr int N = kWgRG / 2;
    float v[N];
#pragma unroll
    for (int g = 0; g < N; ++g) v[g] = p[(2 * g + half) * COLS * kRedP];
#pragma unroll
    for (int w = 1; w < N; w *= 2)
#pragma unroll
        for (int g = 0; g < N; g += 2 * w) v[g] += v[g + w];
    const float other = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v[0]), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
    return half ? other + v[0] : v[0] + other;  // (even groups) + (odd groups) on both lanes
}

// ADAM: each thread applies the optimizer step to the gradient elements it has just produced (every parameter's gradient is
// produced by exactly one thread), so a single-GPU learn() has no separate Adam / Polyak launch.  Same adam_update on the same
// gradient values as adam_kernel: the one-call and the staged (sharded) paths stay bit-identical.
__device__ __forceinline__ void expand_wg(const WgJobC& c, WgJob& J, WgArgs& A) {
    J.net = c.net; J.grad = c.grad; J.m = mlp_of(c.cfg & 1023u);
    J.nslots = (int)((c.cfg >> 10) & 3u);
    J.wmode[0] = (int)((c.cfg >> 12) & 3u); J.wmode[1] = (int)((c.cfg >> 14) & 3u);
    J.ws[0] = carve_slot(c.ws0, c.rows0); J.ws[1] = carve_slot(c.ws1, c.rows1);
    J.rows[0] = c.rows0; J.rows[1] = c.rows1;
    J.p = const_cast<float*>(c.net); J.mom = c.mom; J.var = c.var; J.target = c.target; J.w2b = c.w2b; J.w2f = c.w2f;
    J.w2tb = c.w2tb; J.tgt_w2b = c.tgt_w2b; J.w2b_x9 = (int)((c.cfg >> 20) & 1u);
    A.slope = c.slope; A.w_kind = (int)((c.cfg >> 16) & 3u); A.w_given = c.w_given; A.warm = c.warm; A.inv_batch = c.inv_batch;
    A.soft_count = c.soft_count; A.wstate = c.wstate;
    A.ad.b1 = c.b1; A.ad.b2 = c.b2; A.ad.eps = c.eps; A.ad.step_size = c.step_size; A.ad.bc2_sqrt = c.bc2_sqrt; A.ad.tau = c.tau;
    A.ad.finish_actor = (int)((c.cfg >> 18) & 1u); A.ad.use_bc = (int)((c.cfg >> 19) & 1u);
    A.ad.losses = c.losses; A.ad.wstate = c.wstate;
    A.count_out = c.count_out;
    A.ad.alpha_state = nullptr; A.ad.target_entropy = 0.0f; A.ad.alpha_step_size = 0.0f;
    if ((c.cfg >> 21) & 1u) {  // the three fields a SAC policy step does not use otherwise carry its log-alpha step
        A.ad.alpha_state = c.wstate; A.ad.target_entropy = c.w_given; A.ad.alpha_step_size = c.warm;
        A.ad.wstate = nullptr; A.wstate = nullptr; A.w_given = 0.0f; A.warm = 0.0f;
    }
}
inline WgJobC pack_wg(const WgJob& J, const WgArgs& A) {
    WgJobC c{};
    c.net = J.net; c.grad = J.grad; c.ws0 = J.ws[0].x; c.ws1 = J.nslots > 1 ? J.ws[1].x : J.ws[0].x;
    c.mom = J.mom; c.var = J.var; c.target = J.target; c.w2b = J.w2b; c.w2f = J.w2f; c.w2tb = J.w2tb; c.tgt_w2b = J.tgt_w2b;
    c.cfg = mlp_bits(J.m) | ((uint32_t)J.nslots << 10) | ((uint32_t)J.wmode[0] << 12) | ((uint32_t)J.wmode[1] << 14) | ((uint32_t)A.w_kind << 16) |
            ((uint32_t)(A.ad.finish_actor ? 1 : 0) << 18) | ((uint32_t)(A.ad.use_bc ? 1 : 0) << 19) | ((uint32_t)(J.w2b_x9 ? 1 : 0) << 20) |
            ((uint32_t)(A.ad.alpha_state ? 1 : 0) << 21);
    c.rows0 = J.rows[0]; c.rows1 = J.nslots > 1 ? J.rows[1] : J.rows[0];
    c.slope = A.slope; c.w_given = A.w_given; c.warm = A.warm; c.inv_batch = A.inv_batch;
    c.b1 = A.ad.b1; c.b2 = A.ad.b2; c.eps = A.ad.eps; c.step_size = A.ad.step_size; c.bc2_sqrt = A.ad.bc2_sqrt; c.tau = A.ad.tau;
    c.soft_count = A.soft_count; c.wstate = const_cast<float*>(A.wstate); c.losses = A.ad.losses; c.count_out = A.count_out;
    if (A.ad.alpha_state) { c.wstate = A.ad.alpha_state; c.w_given = A.ad.target_entropy; c.warm = A.ad.alpha_step_size; }
    return c;
}

// ---- what both partitions of the launch (wgrad_kernel, wgrad2_kernel) share: every gradient element is ONE accumulation chain — per thread slot
// 0's rows in order, then slot 1's in the same accumulator, then the fixed-order sums across row halves / row groups — whichever threads run it
// what thread 0 of the launch does besides its gradients
template <bool ADAM>
__device__ __forceinline__ void wg_thread0(const WgArgs& A, float w) {
    if (A.count_out) {  // word 0: the count itself; words 1..kCountDigits: its base-32 digits, what adam_w reads (count_from_digits)
        const int c = A.soft_count ? *A.soft_count : 0;
        A.count_out[0] = (float)c;
        uint32_t u = (uint32_t)c;
#pragma unroll
        for (int k = 0; k < kCountDigits; ++k, u >>= 5) A.count_out[1 + k] = (float)(u & 31u);
    }
    if (ADAM && A.ad.finish_actor) {  // what adam_kernel's thread 0 does on an actor step
        if (A.ad.use_bc) {
            A.ad.losses[1] = A.ad.losses[2] * w + A.ad.losses[3] * (1.0f - w);  // HIRL.py:321
            A.ad.losses[5] = w;
            *A.ad.wstate = w;
        } else {
            A.ad.losses[1] = A.ad.losses[3];  // TD3.py:236
        }
    }
    if (ADAM && A.ad.alpha_state)  // a SAC policy step: the log-alpha step with the mean entropy
        sac_alpha_step(A.ad.alpha_state, A.ad.losses, A.ad.losses[4], A.ad.target_entropy, A.ad.b1, A.ad.b2, A.ad.eps, A.ad.alpha_step_size, A.ad.bc2_sqrt);
}
// dW2 tile, fp32: the operands of the 64-row chunk at c0 (16 + 16 dwords per lane), and its 16 MFMAs on the accumulator
__device__ __forceinline__ void tile_load(const float* dz, const float* h1, unsigned dzo, unsigned h1o, int c0, int g, int rows, float (&av)[16], float (&hv)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = c0 + 4 * i + g;  // MFMA i reduces over rows c0+4i .. c0+4i+3 (one per lane group)
        const unsigned rc = (unsigned)(row < rows ? row : rows - 1);  // unconditional loads (clamped); rows past the end get scale 0
        av[i] = dz[rc * (unsigned)H2 + dzo];
        hv[i] = h1[rc * (unsigned)H1 + h1o];
    }
}
__device__ __forceinline__ void tile_mfma(const float (&av)[16], const float (&hv)[16], int c0, int g, int rend, float sc, v4f& acc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc = mfma16(av[i] * (c0 + 4 * i + g < rend ? sc : 0.0f), hv[i], acc);
}
// The end of a dW2 tile.  The two waves that hold the sums over the two halves of the rows swap half of their accumulators through LDS (xch:
// [pairs][2 halves][64 lanes]): the half-0 wave finishes (and steps) elements 0, 1 of every lane, the half-1 wave elements 2, 3 — two parameters
// per lane.  Every wave of the workgroup calls it (one barrier inside); a wave that is not `live` holds no sum and only meets the barrier.
template <bool ADAM>
__device__ __forceinline__ void tile_finish(const WgJob& J, const WgAdam& ad, const v4f acc, int n0, int k0, int r, int g, int half, int pair, bool live,
                                            float2* xch, int lane) {
    // ADAM: this lane's two parameters are requested only now — the operand registers of the reduction above are dead; the round trip
    // (L2-resident: touched once per learn()) hides under the pair's exchange
    const int q0 = 2 * half;  // this wave finishes elements q0, q0 + 1
    AdamElem ae[2];
    if (ADAM && live) {
#pragma unroll
        for (int q = 0; q < 2; ++q) ae[q].fetch(J, J.m.W2() + (n0 + 4 * g + q0 + q) * H1 + k0 + r);
    }
    if (live) xch[(pair * 2 + half) * 64 + lane] = half ? make_float2(acc[0], acc[1]) : make_float2(acc[2], acc[3]);
    __syncthreads();
    if (!live) return;
    const float2 got = xch[(pair * 2 + (half ^ 1)) * 64 + lane];
    // (first half of the rows) + (second half), whoever adds them
    const float fin[2] = {half ? got.x + acc[2] : acc[0] + got.x, half ? got.y + acc[3] : acc[1] + got.y};
    float* out = J.grad + J.m.W2();
#pragma unroll
    for (int q = 0; q < 2; ++q) out[(unsigned)((n0 + 4 * g + q0 + q) * H1 + k0 + r)] = fin[q];
    if (ADAM) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = J.m.W2() + (n0 + 4 * g + q0 + q) * H1 + k0 + r;
            ae[q].apply(J, ad, idx, fin[q]);
            if (J.w2b) {
                const uint32_t ix = w2_image_index((uint32_t)(n0 + 4 * g + q0 + q), (uint32_t)(k0 + r));
                uint16_t hi, mid, lo;
                split3_bf16(ae[q].p, hi, mid, lo);  // hi = the weight rounded to bf16 (the plain image); mid | lo only for the x9 images
                J.w2b[ix] = hi;
                if (J.w2b_x9) { J.w2b[kImgElems + ix] = mid; J.w2b[2 * kImgElems + ix] = lo; }
            }
            if (J.w2f) J.w2f[w2f_image_index((uint32_t)(n0 + 4 * g + q0 + q), (uint32_t)(k0 + r))] = ae[q].p;
            if (J.w2tb) {
                const __bf16 bv = (__bf16)ae[q].p;
                J.w2tb[w2t_image_index((uint32_t)(k0 + r), (uint32_t)(n0 + 4 * g + q0 + q))] = __builtin_bit_cast(uint16_t, bv);
            }
            if (J.target && J.tgt_w2b) {
                const __bf16 bv = (__bf16)ae[q].t;
                J.tgt_w2b[w2_image_index((uint32_t)(n0 + 4 * g + q0 + q), (uint32_t)(k0 + r))] = __builtin_bit_cast(uint16_t, bv);
            }
        }
    }
}
// one batch row of a vector workgroup's column: db2, dg2, dbe2, dW3[j][n] (+ db3 by the columns of the first workgroup: b3col)
struct VecAcc {
    float db2, dg, dbe, dw3[OW], db3;
};
constexpr int kVecRP = 12;  // rinfo pitch of the vector workgroups: mean, rstd, dout[0..7], pad
template <bool RELU>
__device__ __forceinline__ void vec_row(VecAcc& a, const float* rrow, float z, float d, float g2, float be2, const float (&w3)[OW], int out, float slope, float sc,
                                        bool b3col, int cl) {
    // the row's scalars in three 16-byte LDS reads (one address per half wave: broadcast)
    float ri[kVecRP];
    {
        const float4* r4 = reinterpret_cast<const float4*>(rrow);
        const float4 a4 = r4[0], b4 = r4[1], c4 = r4[2];
        ri[0] = a4.x; ri[1] = a4.y; ri[2] = a4.z; ri[3] = a4.w; ri[4] = b4.x; ri[5] = b4.y; ri[6] = b4.z; ri[7] = b4.w;
        ri[8] = c4.x; ri[9] = c4.y; ri[10] = c4.z; ri[11] = c4.w;
    }
    const float xh = (z - ri[0]) * ri[1];
    const float y = g2 * xh + be2;
    float dh2 = (ri[2] * w3[0] + ri[3] * w3[1]) + (ri[4] * w3[2] + ri[5] * w3[3]);
    if (out > 4) dh2 += (ri[6] * w3[4] + ri[7] * w3[5]) + (ri[8] * w3[6] + ri[9] * w3[7]);
    const float dy = act_bwd<RELU>(dh2, y, slope);
    const float h2 = act_f<RELU>(y, slope);
    a.db2 += sc * d;
    a.dbe += sc * dy;
    a.dg += sc * dy * xh;
#pragma unroll
    for (int jj = 0; jj < OW; ++jj) a.dw3[jj] += sc * ri[2 + jj] * h2;
    // db3[j] = sum_r dout[r][j]: columns 0..out-1 of the first column block, over this row group's rows
    if (b3col) a.db3 += sc * rrow[2 + cl];
}
// one batch row of a layer-1 workgroup's hidden unit: db1, dg1, dbe1, dW1[k][0..16]; rrow: mean, rstd, the two LN1-backward row means
struct L1Acc {
    float db1, dg, dbe, dw1[17];
};
template <bool RELU>
__device__ __forceinline__ void l1_row(L1Acc& a, const float* rrow, const float* xrow, float z, float d, float g1, float be1, float slope, float sc) {
    const float4 ri = *reinterpret_cast<const float4*>(rrow);
    const float xh = (z - ri.x) * ri.y;
    const float dy = act_bwd<RELU>(d, g1 * xh + be1, slope);
    const float dz = sc * (ri.y * (dy * g1 - ri.z - xh * ri.w));
    a.db1 += dz;
    a.dbe += sc * dy;
    a.dg += sc * dy * xh;
    // the input row in five 16-byte LDS reads (one address per half wave: broadcast), not seventeen 4-byte ones
    const float4* xr4 = reinterpret_cast<const float4*>(xrow);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 x4 = xr4[q];
        a.dw1[4 * q] += dz * x4.x; a.dw1[4 * q + 1] += dz * x4.y; a.dw1[4 * q + 2] += dz * x4.z; a.dw1[4 * q + 3] += dz * x4.w;
    }
    a.dw1[16] += dz * xrow[16];
}

// The workgroups of wgrad_kernel's columns beyond the jobs' own (blockIdx.x >= kWgPerJob) are numbered so that slot s sits on XCD s % 8: column
// group c / 8 first, then the job row, then c % 8.  Slot 0 is the predraw's when there is one; the head riders' tiles follow from slot 8 then (a row
// tile t on XCD t % 8, where launch G's workgroups of that tile run), else from slot 0.
__device__ __forceinline__ int extra_slot() {
    const int c = (int)blockIdx.x - kWgPerJob;
    return ((c >> 3) * (int)gridDim.y + (int)blockIdx.y) * 8 + (c & 7);
}
inline int extra_columns(int slots, int njobs) { return 8 * ((slots + 8 * njobs - 1) / (8 * njobs)); }
// Head rider: row tile t of the launch's head jobs (job 0's tiles, then job 1's) — one wave per row evaluates the net's head exactly as a forward
// workgroup with act_mode 1 does in its prologue (hx_fwd_body.h: the same head_row4 / head_row, the same fast_tanh, no smoothing noise) and writes what
// that job's first column workgroups write: outv[row][0..3] and st2[row].  No LDS, no barrier; a slot beyond the tiles exits.
template <bool RELU>
__device__ __forceinline__ void head_rider_wg(const WgArgsC& AC, int t) {
    if (t < 0) return;
    const float slope = AC.job[0].slope;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const HeadJobC& hj = AC.head[h];
        const int tiles = (hj.rows + RT - 1) / RT;
        if (t < tiles) {
            const int r = t * RT + wave;
            if (r >= hj.rows) return;
            const Mlp m = mlp_of(hj.cfg & 1023u);
            const Slot S = carve_slot(hj.ws, hj.rows);
            RowReg<H2> xh, y;
            float mean, rstd, o[4];
            if (m.out == 4) head_row4<RELU, false, true>(S.z2 + (size_t)r * H2, hj.net, m, slope, xh, y, mean, rstd, o);
            else head_row<4, RELU>(S.z2 + (size_t)r * H2, hj.net, m, slope, xh, y, mean, rstd, o);
            if (lane < 4) S.outv[(size_t)r * OW + lane] = fast_tanh(lane == 0 ? o[0] : lane == 1 ? o[1] : lane == 2 ? o[2] : o[3]);  // Actor.forward's tanh, HIRL.py:140
            if (lane == 0) {
                S.st2[(size_t)r * 2] = mean;
                S.st2[(size_t)r * 2 + 1] = rstd;
            }
            return;
        }
        t -= tiles;
    }
}

// BF16 (the bf16 update path): dW2 = dz2^T h1 on v_mfma_f32_16x16x32_bf16 — both operands rounded to bf16 as they are loaded (32 batch rows
// per MFMA instead of 4), fp32 accumulation per slot, the slot's BC weight applied to the fp32 sum; every other gradient (biases, LayerNorm,
// layer 1, the head) is fp32 arithmetic on fp32 values.  With ADAM the step also refreshes the bf16 images of W2 (forward, transposed,
// target).
// the layer-1 workgroups' inner stamps (a dozen, each an s_waitcnt lgkmcnt(0)) lengthen that path: only with -DHX_STAMPS_L1 (tools/ubench/stamps.py's
// layer-1 line); the default stamps build keeps the workgroup's life span alone, so that tools/ubench/wgrad_blocks.py compares like with like
#ifdef HX_STAMPS_L1
#define STAMP_L1() STAMP()
#else
#define STAMP_L1()
#endif
template <bool ADAM, bool RELU, bool BF16 = false>
__global__ __launch_bounds__(kWide) void wgrad_kernel(WgArgsC AC) {
    __shared__ __attribute__((aligned(16))) float lds[kWgRowChunk * XP + kWgRowChunk * 12 + kWgRG * kWgCols * kRedP];
    float* xs = lds;                          // [chunk][XP]   inputs (layer-1 job)
    float* rinfo = lds + kWgRowChunk * XP;    // [chunk][<=12] per-row scalars
    float* red = rinfo + kWgRowChunk * 12;    // [16][64][kRedP]  cross-row-group reduction

    {
        static_assert(sizeof(lds) >= (4 * kFusedSlots + 2 * kFusedBatchMax) * 4, "predraw_wg's tables fit");
        if (blockIdx.x >= kWgPerJob) {  // (columns beyond the jobs' own, eight at a time: the XCD of every other workgroup stays what it was)
            const int s = extra_slot();
            if (AC.has_pre && s == 0) predraw_wg(AC.pre, AC.pre_batch, lds);
            else head_rider_wg<RELU>(AC, s - (AC.has_pre ? 8 : 0));
            return;
        }
    }
    const int j = blockIdx.y, b = blockIdx.x;
    WgJob J;
    WgArgs A;
    expand_wg(AC.job[j], J, A);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float slope = A.slope;
    STAMP_DECL;
    STAMP();
    const float w = effective_w(A.w_kind, A.w_given, A.warm, A.inv_batch, A.soft_count, A.wstate);
    float scale[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) scale[s] = J.wmode[s] == 0 ? 1.0f : (J.wmode[s] == 1 ? 1.0f - w : w);
#ifdef HX_STAMPS
    asm volatile("" ::"v"(w));
    STAMP();
#endif
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) wg_thread0<ADAM>(A, w);

    if (b < kWgTilesPerBlock) {
        // dW2[n][k] = sum_r scale dz2[r][n] h1[r][k].  Tile 16 (n) x 16 (k) per wave PAIR (w, w + 8): each wave reduces over half of the
        // batch rows, 16 per MFMA group; all operands of a 64-row chunk (16 + 16 dwords per lane) are requested before the first MFMA.
        // The pair then swaps half of its accumulator through LDS: wave w finishes (and steps) elements 0, 1 of every lane, wave w + 8
        // elements 2, 3 — two parameters per lane.
        const int n0 = (b >> 1) * 16, k0 = (b & 1) * (H1 / 2) + (wave & 7) * 16, half = wave >> 3;
        const int r = lane & 15, g = lane >> 4;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int s = 0; s < 2; ++s) if (s < J.nslots) {  // compile-time slot index: J lives in registers, not in scratch
            const float sc = scale[s];
            const float* dz = J.ws[s].dz2;  // uniform bases + 32-bit lane offsets: no 64-bit address arithmetic per load
            const float* h1 = J.ws[s].h1;
            const unsigned dzo = (unsigned)(n0 + r), h1o = (unsigned)(k0 + r);
            const int rows = J.rows[s];
            const int hr = ((rows + 7) >> 3) << 2;  // rows per half, a multiple of the MFMA's 4
            const int rbeg = half * hr, rend = min(rows, rbeg + hr);
            if constexpr (BF16) {
                // MFMA m reduces over rows c0 + 32 m .. + 31: lane (r, g) feeds rows + 8 g .. + 7 of column n0 + r (A) / k0 + r (B)
                v4f accs = {0.f, 0.f, 0.f, 0.f};
                for (int c0 = rbeg; c0 < rend; c0 += 64) {
                    float av[2][8], hv[2][8];
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int row = c0 + 32 * m + 8 * g + j;
                            const unsigned rc = (unsigned)(row < rows ? row : rows - 1);  // unconditional loads (clamped)
                            av[m][j] = dz[rc * (unsigned)H2 + dzo];
                            hv[m][j] = h1[rc * (unsigned)H1 + h1o];
                        }
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (c0 + 32 * m + 8 * g + j >= rend) av[m][j] = 0.0f;  // rows past this half's end contribute nothing
                        accs = mfma16_bf16(pack8_bf16(av[m]), pack8_bf16(hv[m]), accs);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_fmaf(sc, accs[q], acc[q]);
            } else {
                for (int c0 = rbeg; c0 < rend; c0 += 64) {
                    float av[16], hv[16];
                    tile_load(dz, h1, dzo, h1o, c0, g, rows, av, hv);
                    tile_mfma(av, hv, c0, g, rend, sc, acc);
                }
            }
        }
        STAMP();
        tile_finish<ADAM>(J, A.ad, acc, n0, k0, r, g, half, wave & 7, true, reinterpret_cast<float2*>(red), lane);  // [8 pairs][2 halves][64 lanes]
        STAMP();
        STAMP_FLUSH(32, blockIdx.x == 0 && blockIdx.y == 0 && tid == 0);
        SPAN_LOG(HX_SPAN_WGRAD);
        return;
    }
    // Vector and layer-1 workgroups: 16 columns x 64 row groups (a quarter wave per row group): two batch rows per thread at B = 128.
    // (64 columns x 16 row groups put eight rows on every thread, 32 x 32 four: these workgroups, not the MFMA tiles, set the launch's duration.)
    const int cl = lane & (kWgCols - 1);           // column inside the workgroup
    const int rg = tid / kWgCols;                  // row group: rows rg, rg + 64, ...
    // after the reduction: thread pair -> (item, column); each thread of the pair sums half of the row groups
    const int ohalf = tid & 1, oitem = (tid >> 1) / kWgCols, ocol = (tid >> 1) % kWgCols;
    if (b < kWgTilesPerBlock + kWgVecWgs) {
        // column n: db2, dg2, dbe2, dW3[j][n] (+ db3 by the first workgroup)
        constexpr int RP = kVecRP;
        const int vb = b - kWgTilesPerBlock;
        const int n = vb * kWgCols + cl;
        const float g2 = J.net[J.m.g2() + n], be2 = J.net[J.m.be2() + n];
        float w3[OW];
#pragma unroll
        for (int jj = 0; jj < OW; ++jj) w3[jj] = jj < J.m.out ? J.net[J.m.W3() + jj * H2 + n] : 0.0f;
        VecAcc a = {};
        // ADAM: the parameter this thread will step after the reduction (item oitem of column ocol; the last items: b3), requested now
        const int on = vb * kWgCols + ocol;
        const unsigned vidx = (unsigned)(oitem == 0 ? J.m.b2() + on : oitem == 1 ? J.m.g2() + on : oitem == 2 ? J.m.be2() + on : J.m.W3() + (oitem - 3) * H2 + on);
        const bool vlive = oitem < 3 + J.m.out;
        const bool b3live = vb == 0 && oitem == 3 + OW && ocol < J.m.out;  // (item 3 + OW of the reduction tile carries db3)
        const unsigned b3idx = (unsigned)(J.m.b3() + (ocol < J.m.out ? ocol : 0));
        AdamElem vae;
        bool vae_pending = ADAM && (vlive || b3live) && ohalf == 0;  // its operands are needed last: requested behind the first chunk's loads
        #pragma unroll
        for (int s = 0; s < 2; ++s) if (s < J.nslots) {  // compile-time slot index: J lives in registers, not in scratch
            const Slot& S = J.ws[s];
            const float sc = scale[s];
            for (int c0 = 0; c0 < J.rows[s]; c0 += kWgRowChunk) {
                const int nr = min(kWgRowChunk, J.rows[s] - c0);
                // this thread's first 4 rows are requested before the per-row scalars are staged: one round trip, not two
                float zv[4], dv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) if (kWgRG * i < nr) {  // (scalar: at B = 128 row blocks 2, 3 are past the end for every thread)
                    const int r = rg + kWgRG * i;
                    const unsigned o = (unsigned)(c0 + (r < nr ? r : nr - 1)) * (unsigned)H2 + (unsigned)n;  // unconditional inside a block, clamped
                    zv[i] = S.z2[o];
                    dv[i] = S.dz2[o];
                }
                // the per-row scalars are requested BEFORE the barrier that frees the LDS tile: one round trip with the loads above
                static_assert(kWgRowChunk <= kWide, "staging: one row per thread");
                // (whole waves without a row skip theirs behind a scalar branch: 2 of the 16 waves have rows at B = 128, and the address
                //  pipeline takes 16 lanes per clock whatever they ask for)
                const int er = tid < nr ? tid : 0;
                v2f st2v;  // (unset in a skipping wave, which never stores it: see HeadImage::fetch)
                v4f d4, d5;
                if (__builtin_amdgcn_readfirstlane(tid) < nr) {
                    st2v = *reinterpret_cast<const v2f*>(S.st2 + (size_t)(c0 + er) * 2);
                    d4 = *reinterpret_cast<const v4f*>(S.dout + (size_t)(c0 + er) * OW);
                    d5 = *reinterpret_cast<const v4f*>(S.dout + (size_t)(c0 + er) * OW + 4);
                }
                if (vae_pending) {
                    vae.fetch(J, b3live ? b3idx : vidx);
                    vae_pending = false;
                }
                __syncthreads();
                if (tid < nr) {
                    float4* r4 = reinterpret_cast<float4*>(rinfo + tid * RP);
                    r4[0] = make_float4(st2v[0], st2v[1], d4[0], d4[1]);
                    r4[1] = make_float4(d4[2], d4[3], d5[0], d5[1]);
                    r4[2] = make_float4(d5[2], d5[3], 0.0f, 0.0f);
                }
                __syncthreads();
                for (int rb0 = 0; rb0 < nr; rb0 += kWgRG * 4) {  // 4 rows per thread per block, all loads in flight together
                    const int rb = rg + rb0;
                    if (rb0 != 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (rb0 + kWgRG * i < nr) {
                            const int r = rb + kWgRG * i;
                            const unsigned o = (unsigned)(c0 + (r < nr ? r : nr - 1)) * (unsigned)H2 + (unsigned)n;
                            zv[i] = S.z2[o];
                            dv[i] = S.dz2[o];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = rb + kWgRG * i;
                        if (r < nr) vec_row<RELU>(a, rinfo + r * RP, zv[i], dv[i], g2, be2, w3, J.m.out, slope, sc, vb == 0 && cl < J.m.out, cl);
                    }
                }
            }
        }
        STAMP();
        float* my = red + (rg * kWgCols + cl) * kRedP;
        my[0] = a.db2; my[1] = a.dg; my[2] = a.dbe;
#pragma unroll
        for (int jj = 0; jj < OW; ++jj) my[3 + jj] = a.dw3[jj];
        my[3 + OW] = a.db3;
        __syncthreads();
        if (vlive || b3live) {  // thread pair -> (item, column): 32 partial sums each, the even thread finishes
            float v = sum_groups(red + ocol * kRedP + oitem, ohalf);
            if ((oitem == 1 || oitem == 2) && J.m.no_ln) v = 0.0f;
            const unsigned idx = b3live ? b3idx : vidx;
            if (ohalf == 0) {
                J.grad[idx] = v;
                if (ADAM) vae.apply(J, A.ad, idx, v);
            }
        }
        STAMP();
        STAMP_FLUSH(40, b == kWgTilesPerBlock && j == 0 && tid == 0);
        SPAN_LOG(HX_SPAN_WGRAD);
        return;
    }
    // layer 1: hidden unit k; dz1 = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) with the row means taken from the
    // per-workgroup partial sums bwd_l2 left in lnp -> no cross-column work here.
    {
        const int kb = (b - kWgTilesPerBlock - kWgVecWgs) * kWgCols;
        const int k = kb + cl;
        const int in = J.m.in;
        const float g1 = J.net[J.m.g1() + k], be1 = J.net[J.m.be1() + k];
        STAMP_L1();
        L1Acc a = {};
        // ADAM: the parameter this thread will step (item oitem of unit kb + ocol; 3 + in <= 20 items x 16 units, two threads each), requested now
        const int ok = kb + ocol;
        const unsigned lidx = (unsigned)(oitem == 0 ? J.m.b1() + ok : oitem == 1 ? J.m.g1() + ok : oitem == 2 ? J.m.be1() + ok : J.m.W1() + ok * in + (oitem - 3));
        const bool llive = oitem < 3 + in;
        AdamElem lae;
        bool lae_pending = ADAM && llive && ohalf == 0;  // needed last: requested behind the first chunk's loads
        #pragma unroll
        for (int s = 0; s < 2; ++s) if (s < J.nslots) {  // compile-time slot index: J lives in registers, not in scratch
            const Slot& S = J.ws[s];
            const float sc = scale[s];
            for (int c0 = 0; c0 < J.rows[s]; c0 += kWgRowChunk) {
                const int nr = min(kWgRowChunk, J.rows[s] - c0);
                float zv[4], dv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) if (kWgRG * i < nr) {  // (scalar: at B = 128 row blocks 2, 3 are past the end for every thread)
                    const int r = rg + kWgRG * i;
                    const unsigned o = (unsigned)(c0 + (r < nr ? r : nr - 1)) * (unsigned)H1 + (unsigned)k;  // unconditional inside a block, clamped
                    zv[i] = S.z1[o];
                    dv[i] = S.dh1[o];
                }
                STAMP_L1();
                // the chunk's shared operands are requested BEFORE the barrier that frees the LDS tiles: one round trip with the loads above
                static_assert(kWgRowChunk * XP <= 5 * kWide && kWgRowChunk <= kWide && kColWgB == 8, "staging: five words + one row per thread");
                // (whole waves past the end of a tile skip their loads behind a scalar branch: at B = 128 the input tile is 2.5 of the 5
                //  passes and 2 of the 16 waves have a row; the address pipeline takes 16 lanes per clock whatever they ask for)
                const int w0 = __builtin_amdgcn_readfirstlane(tid);
                float xst[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const int e = tid + q * kWide;
                    if (w0 + q * kWide < nr * XP) xst[q] = S.x[(size_t)c0 * XP + (e < nr * XP ? e : 0)];
                }
                STAMP_L1();
                const int er = tid < nr ? tid : 0;
                v2f st1v;  // (unset in a skipping wave, which never stores it)
                v4f l0, l1, l2, l3;
                if (w0 < nr) {
                    st1v = *reinterpret_cast<const v2f*>(S.st1 + (size_t)(c0 + er) * 2);
                    const v4f* lp4 = reinterpret_cast<const v4f*>(S.lnp + (size_t)(c0 + er) * (2 * kColWgB));  // [8 column workgroups][2]
                    l0 = lp4[0]; l1 = lp4[1]; l2 = lp4[2]; l3 = lp4[3];
                }
                STAMP_L1();
                if (lae_pending) {
                    lae.fetch(J, lidx);
                    lae_pending = false;
                }
                STAMP_L1();
                __syncthreads();
                STAMP_L1();
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const int e = tid + q * kWide;
                    if (e < nr * XP) xs[e] = xst[q];
                }
                if (tid < nr) {  // lnp_sum's fixed-order tree over the eight partials of each of the two row sums
                    const float s1 = ((l0[0] + l0[2]) + (l1[0] + l1[2])) + ((l2[0] + l2[2]) + (l3[0] + l3[2]));
                    const float s2 = ((l0[1] + l0[3]) + (l1[1] + l1[3])) + ((l2[1] + l2[3]) + (l3[1] + l3[3]));
                    *reinterpret_cast<float4*>(rinfo + tid * 8) = make_float4(st1v[0], st1v[1], s1 * (1.0f / H1), s2 * (1.0f / H1));
                }
                __syncthreads();
                STAMP_L1();
                for (int rb0 = 0; rb0 < nr; rb0 += kWgRG * 4) {
                    const int rb = rg + rb0;
                    if (rb0 != 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (rb0 + kWgRG * i < nr) {
                            const int r = rb + kWgRG * i;
                            const unsigned o = (unsigned)(c0 + (r < nr ? r : nr - 1)) * (unsigned)H1 + (unsigned)k;
                            zv[i] = S.z1[o];
                            dv[i] = S.dh1[o];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = rb + kWgRG * i;
                        if (r < nr) l1_row<RELU>(a, rinfo + r * 8, xs + r * XP, zv[i], dv[i], g1, be1, slope, sc);
                    }
                }
            }
        }
        STAMP_L1();
        float* my = red + (rg * kWgCols + cl) * kRedP;
        my[0] = a.db1; my[1] = a.dg; my[2] = a.dbe;
#pragma unroll
        for (int i = 0; i < 17; ++i) my[3 + i] = a.dw1[i];
        STAMP_L1();
        __syncthreads();
        STAMP_L1();
        if (llive) {
            float v = sum_groups(red + ocol * kRedP + oitem, ohalf);
            if ((oitem == 1 || oitem == 2) && J.m.no_ln) v = 0.0f;
#ifdef HX_STAMPS
            asm volatile("" ::"v"(v));
            STAMP_L1();
#endif
            if (ohalf == 0) {
                J.grad[lidx] = v;
                if (ADAM) lae.apply(J, A.ad, lidx, v);
            }
        }
        STAMP_L1();
        STAMP_FLUSH(48, b == kWgTilesPerBlock + kWgVecWgs && j == 0 && tid == 0);
        SPAN_LOG(HX_SPAN_WGRAD);
    }
}

// The partition for ONE job with TWO slots whose rows fit the LDS tiles together (rows0 + rows1 <= kWgRowChunk: the actor step of HIRL, the imitative
// policy step of SAC), fp32.  wgrad_kernel runs such a job on 112 workgroups, every thread walking slot 0 and then slot 1: slot 1's operands are
// requested after slot 0's arithmetic — a second round trip (and in the vector / layer-1 workgroups a second barrier pair) in a launch whose life is
// one round trip and a little arithmetic, beside 144 idle CUs.  Here each slot has its OWN threads — waves 0..7 of a workgroup are stage 0 (slot 0),
// waves 8..15 stage 1 (slot 1) — on half the columns per workgroup: 128 + 64 + 32 = 224 workgroups, every operand of both slots requested at entry.
// Each accumulation chain keeps its order: the stage-0 thread runs slot 0's rows from zero and leaves its running sums in LDS, the stage-1 thread of
// the same chain starts from them and continues with slot 1's rows; then the same fixed-order sums as in wgrad_kernel.  Same bits.
constexpr int kWg2Cols = kWgCols / 2;                    // columns per vector / layer-1 workgroup: 8 columns x 64 row groups x 2 stages
constexpr int kWg2Tiles = 4 * (H2 / 16);                 // 128 workgroups: 16 (n) x 64 (k) of dW2; a 16 x 16 tile per wave QUAD (stage, half of the rows)
constexpr int kWg2VecWgs = H2 / kWg2Cols;                // 64
constexpr int kWg2L1Wgs = H1 / kWg2Cols;                 // 32
constexpr int kWg2PerJob = kWg2Tiles + kWg2VecWgs + kWg2L1Wgs;
static_assert(kWide / 2 / kWg2Cols == kWgRG && kWg2PerJob == 2 * kWgPerJob, "two stages of 64 row groups; as many workgroups as the critics' two jobs");
template <bool ADAM, bool RELU>
__global__ __launch_bounds__(kWide) void wgrad2_kernel(WgArgsC AC) {
    __shared__ __attribute__((aligned(16))) float lds[kWgRowChunk * XP + kWgRowChunk * 12 + kWgRG * kWgCols * kRedP];
    float* xs = lds;                                  // [rows0 + rows1][XP]   inputs (layer-1 workgroups): slot 0's rows, then slot 1's
    float* rinfo = lds + kWgRowChunk * XP;            // [rows0 + rows1][<=12] per-row scalars, likewise
    float* red = rinfo + kWgRowChunk * 12;            // [64][8][kRedP]  cross-row-group reduction (tile workgroups: the half exchange)
    float* hand = red + kWgRG * kWg2Cols * kRedP;     // [64][8][kRedP]  stage 0 -> stage 1: the running sums (tile workgroups: [4 tiles][2 halves][64 lanes] v4f)
    static_assert((kWgRG * kWg2Cols * kRedP) % 4 == 0 && 8 * 64 * 4 <= kWgRG * kWg2Cols * kRedP, "the tile hand-off is 16-byte aligned and fits");

    if (AC.has_pre && blockIdx.x >= kWg2PerJob) {  // (as in wgrad_kernel)
        if (blockIdx.x == kWg2PerJob) predraw_wg(AC.pre, AC.pre_batch, lds);
        return;
    }
    const int b = blockIdx.x;
    WgJob J;
    WgArgs A;
    expand_wg(AC.job[0], J, A);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int stage = __builtin_amdgcn_readfirstlane(tid) >> 9;  // scalar: which slot this wave works on
    const float slope = A.slope;
    STAMP_DECL;
    STAMP();
    const float w = effective_w(A.w_kind, A.w_given, A.warm, A.inv_batch, A.soft_count, A.wstate);
    float scale[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) scale[s] = J.wmode[s] == 0 ? 1.0f : (J.wmode[s] == 1 ? 1.0f - w : w);
    if (blockIdx.x == 0 && tid == 0) wg_thread0<ADAM>(A, w);
    // this wave's slot: scalar selects between the two slots' (scalar) fields — J stays in registers
    const float sc = stage ? scale[1] : scale[0];
    const int rows0 = J.rows[0], rows1 = J.rows[1], nrt = rows0 + rows1;  // both > 0, nrt <= kWgRowChunk (launch_wg)
    const int nr = stage ? rows1 : rows0, roff = stage ? rows0 : 0;      // this slot's rows, and where they begin in xs / rinfo

    if (b < kWg2Tiles) {
        // a 16 x 16 tile of dW2 per wave quad: wave (stage, half, tile) reduces over one half of the rows of its slot.  The stage-0 wave's accumulator
        // is the stage-1 wave's starting value: the same MFMA sequence on the accumulator as wgrad_kernel's wave that takes both slots in turn.
        const int tile = wave & 3, half = (wave >> 2) & 1;
        const int n0 = (b >> 2) * 16, k0 = (b & 3) * (H1 / 4) + tile * 16;
        const int r = lane & 15, g = lane >> 4;
        const float* dz = stage ? J.ws[1].dz2 : J.ws[0].dz2;
        const float* h1 = stage ? J.ws[1].h1 : J.ws[0].h1;
        const unsigned dzo = (unsigned)(n0 + r), h1o = (unsigned)(k0 + r);
        const int hr = ((nr + 7) >> 3) << 2;  // rows per half, a multiple of the MFMA's 4
        const int rbeg = half * hr, rend = min(nr, rbeg + hr);
        float av[16], hv[16];
        if (rbeg < rend) tile_load(dz, h1, dzo, h1o, rbeg, g, nr, av, hv);  // both stages' first chunks are in flight together
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        v4f* hnd = reinterpret_cast<v4f*>(hand) + (tile * 2 + half) * 64 + lane;
        if (stage == 0) {
            for (int c0 = rbeg; c0 < rend; c0 += 64) {
                if (c0 != rbeg) tile_load(dz, h1, dzo, h1o, c0, g, nr, av, hv);
                tile_mfma(av, hv, c0, g, rend, sc, acc);
            }
            *hnd = acc;
        }
        __syncthreads();
        if (stage == 1) {
            acc = *hnd;
            for (int c0 = rbeg; c0 < rend; c0 += 64) {
                if (c0 != rbeg) tile_load(dz, h1, dzo, h1o, c0, g, nr, av, hv);
                tile_mfma(av, hv, c0, g, rend, sc, acc);
            }
        }
        tile_finish<ADAM>(J, A.ad, acc, n0, k0, r, g, half, tile, stage == 1, reinterpret_cast<float2*>(red), lane);  // [4 tiles][2 halves][64 lanes]
        SPAN_LOG(HX_SPAN_WGRAD);
        return;
    }
    // Vector and layer-1 workgroups: 8 columns x 64 row groups per stage (an eighth of a wave per row group): two batch rows per thread at B = 128.
    const int cl = lane & (kWg2Cols - 1);          // column inside the workgroup
    const int rg = (tid & (kWide / 2 - 1)) / kWg2Cols;  // row group: rows rg, rg + 64, ... of this stage's slot
    // after the reduction: thread pair -> (item, column); each thread of the pair sums half of the row groups
    const int ohalf = tid & 1, oitem = (tid >> 1) / kWg2Cols, ocol = (tid >> 1) % kWg2Cols;
    // staging: thread t < nrt stages row t of the combined tiles — of slot 0 below rows0, of slot 1 from there
    const int w0 = __builtin_amdgcn_readfirstlane(tid);
    const bool mine0 = tid < rows0;
    const int er = tid < nrt ? (mine0 ? tid : tid - rows0) : 0;  // (a lane past the end asks for row 0 of slot 1)
    float* hnd = hand + (rg * kWg2Cols + cl) * kRedP;
    float* my = red + (rg * kWg2Cols + cl) * kRedP;
    if (b < kWg2Tiles + kWg2VecWgs) {
        // column n: db2, dg2, dbe2, dW3[j][n] (+ db3 by the first workgroup)
        constexpr int RP = kVecRP;
        const int vb = b - kWg2Tiles;
        const int n = vb * kWg2Cols + cl;
        const float g2 = J.net[J.m.g2() + n], be2 = J.net[J.m.be2() + n];
        float w3[OW];
#pragma unroll
        for (int jj = 0; jj < OW; ++jj) w3[jj] = jj < J.m.out ? J.net[J.m.W3() + jj * H2 + n] : 0.0f;
        static_assert(OW <= kWg2Cols, "db3's columns are in the first column block");
        // ADAM: the parameter this thread will step after the reduction (item oitem of column ocol; the last items: b3), requested at entry
        const int on = vb * kWg2Cols + ocol;
        const unsigned vidx = (unsigned)(oitem == 0 ? J.m.b2() + on : oitem == 1 ? J.m.g2() + on : oitem == 2 ? J.m.be2() + on : J.m.W3() + (oitem - 3) * H2 + on);
        const bool vlive = oitem < 3 + J.m.out;
        const bool b3live = vb == 0 && oitem == 3 + OW && ocol < J.m.out;  // (item 3 + OW of the reduction tile carries db3)
        const unsigned b3idx = (unsigned)(J.m.b3() + (ocol < J.m.out ? ocol : 0));
        // this thread's rows (up to 4: nr < kWgRowChunk) and the row scalars it stages, all requested before the first barrier: one round trip
        const float* z2 = stage ? J.ws[1].z2 : J.ws[0].z2;
        const float* dz2 = stage ? J.ws[1].dz2 : J.ws[0].dz2;
        float zv[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) if (kWgRG * i < nr) {
            const int r = rg + kWgRG * i;
            const unsigned o = (unsigned)(r < nr ? r : nr - 1) * (unsigned)H2 + (unsigned)n;  // unconditional inside a block, clamped
            zv[i] = z2[o];
            dv[i] = dz2[o];
        }
        v2f st2v;  // (unset in a skipping wave, which never stores it: see HeadImage::fetch)
        v4f d4, d5;
        if (w0 < nrt) {
            const float* st2 = mine0 ? J.ws[0].st2 : J.ws[1].st2;
            const float* dout = mine0 ? J.ws[0].dout : J.ws[1].dout;
            st2v = *reinterpret_cast<const v2f*>(st2 + (size_t)er * 2);
            d4 = *reinterpret_cast<const v4f*>(dout + (size_t)er * OW);
            d5 = *reinterpret_cast<const v4f*>(dout + (size_t)er * OW + 4);
        }
        AdamElem vae;
        if (ADAM && (vlive || b3live) && ohalf == 0) vae.fetch(J, b3live ? b3idx : vidx);
        if (tid < nrt) {
            float4* r4 = reinterpret_cast<float4*>(rinfo + tid * RP);
            r4[0] = make_float4(st2v[0], st2v[1], d4[0], d4[1]);
            r4[1] = make_float4(d4[2], d4[3], d5[0], d5[1]);
            r4[2] = make_float4(d5[2], d5[3], 0.0f, 0.0f);
        }
        __syncthreads();
        VecAcc a = {};
        const bool b3col = vb == 0 && cl < J.m.out;
        if (stage == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rg + kWgRG * i;
                if (r < nr) vec_row<RELU>(a, rinfo + (roff + r) * RP, zv[i], dv[i], g2, be2, w3, J.m.out, slope, sc, b3col, cl);
            }
            hnd[0] = a.db2; hnd[1] = a.dg; hnd[2] = a.dbe;
#pragma unroll
            for (int jj = 0; jj < OW; ++jj) hnd[3 + jj] = a.dw3[jj];
            hnd[3 + OW] = a.db3;
        }
        __syncthreads();
        if (stage == 1) {
            a.db2 = hnd[0]; a.dg = hnd[1]; a.dbe = hnd[2];
#pragma unroll
            for (int jj = 0; jj < OW; ++jj) a.dw3[jj] = hnd[3 + jj];
            a.db3 = hnd[3 + OW];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rg + kWgRG * i;
                if (r < nr) vec_row<RELU>(a, rinfo + (roff + r) * RP, zv[i], dv[i], g2, be2, w3, J.m.out, slope, sc, b3col, cl);
            }
            my[0] = a.db2; my[1] = a.dg; my[2] = a.dbe;
#pragma unroll
            for (int jj = 0; jj < OW; ++jj) my[3 + jj] = a.dw3[jj];
            my[3 + OW] = a.db3;
        }
        __syncthreads();
        if (vlive || b3live) {  // thread pair -> (item, column): 32 partial sums each, the even thread finishes
            float v = sum_groups<kWg2Cols>(red + ocol * kRedP + oitem, ohalf);
            if ((oitem == 1 || oitem == 2) && J.m.no_ln) v = 0.0f;
            const unsigned idx = b3live ? b3idx : vidx;
            if (ohalf == 0) {
                J.grad[idx] = v;
                if (ADAM) vae.apply(J, A.ad, idx, v);
            }
        }
        SPAN_LOG(HX_SPAN_WGRAD);
        return;
    }
    // layer 1: hidden unit k (see wgrad_kernel)
    {
        const int kb = (b - kWg2Tiles - kWg2VecWgs) * kWg2Cols;
        const int k = kb + cl;
        const int in = J.m.in;
        const float g1 = J.net[J.m.g1() + k], be1 = J.net[J.m.be1() + k];
        // ADAM: the parameter this thread will step (item oitem of unit kb + ocol; 3 + in <= 20 items x 8 units, two threads each), requested at entry
        const int ok = kb + ocol;
        const unsigned lidx = (unsigned)(oitem == 0 ? J.m.b1() + ok : oitem == 1 ? J.m.g1() + ok : oitem == 2 ? J.m.be1() + ok : J.m.W1() + ok * in + (oitem - 3));
        const bool llive = oitem < 3 + in;
        const float* z1 = stage ? J.ws[1].z1 : J.ws[0].z1;
        const float* dh1 = stage ? J.ws[1].dh1 : J.ws[0].dh1;
        float zv[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) if (kWgRG * i < nr) {
            const int r = rg + kWgRG * i;
            const unsigned o = (unsigned)(r < nr ? r : nr - 1) * (unsigned)H1 + (unsigned)k;  // unconditional inside a block, clamped
            zv[i] = z1[o];
            dv[i] = dh1[o];
        }
        // the input tiles of both slots, one behind the other: five words per thread (whole waves past the end skip theirs behind a scalar branch)
        static_assert(kWgRowChunk * XP <= 5 * kWide && kWgRowChunk <= kWide && kColWgB == 8, "staging: five words + one row per thread");
        const int nx0 = rows0 * XP, nxt = nrt * XP;
        float xst[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int e = tid + q * kWide;
            if (w0 + q * kWide < nxt) {
                const float* xp = e < nx0 ? J.ws[0].x : J.ws[1].x;
                xst[q] = xp[e < nxt ? (e < nx0 ? e : e - nx0) : 0];
            }
        }
        v2f st1v;  // (unset in a skipping wave, which never stores it)
        v4f l0, l1, l2, l3;
        if (w0 < nrt) {
            const float* st1 = mine0 ? J.ws[0].st1 : J.ws[1].st1;
            const float* lnp = mine0 ? J.ws[0].lnp : J.ws[1].lnp;
            st1v = *reinterpret_cast<const v2f*>(st1 + (size_t)er * 2);
            const v4f* lp4 = reinterpret_cast<const v4f*>(lnp + (size_t)er * (2 * kColWgB));  // [8 column workgroups][2]
            l0 = lp4[0]; l1 = lp4[1]; l2 = lp4[2]; l3 = lp4[3];
        }
        AdamElem lae;
        if (ADAM && llive && ohalf == 0) lae.fetch(J, lidx);
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int e = tid + q * kWide;
            if (e < nxt) xs[e] = xst[q];
        }
        if (tid < nrt) {  // lnp_sum's fixed-order tree over the eight partials of each of the two row sums
            const float s1 = ((l0[0] + l0[2]) + (l1[0] + l1[2])) + ((l2[0] + l2[2]) + (l3[0] + l3[2]));
            const float s2 = ((l0[1] + l0[3]) + (l1[1] + l1[3])) + ((l2[1] + l2[3]) + (l3[1] + l3[3]));
            *reinterpret_cast<float4*>(rinfo + tid * 8) = make_float4(st1v[0], st1v[1], s1 * (1.0f / H1), s2 * (1.0f / H1));
        }
        __syncthreads();
        L1Acc a = {};
        if (stage == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rg + kWgRG * i;
                if (r < nr) l1_row<RELU>(a, rinfo + (roff + r) * 8, xs + (roff + r) * XP, zv[i], dv[i], g1, be1, slope, sc);
            }
            hnd[0] = a.db1; hnd[1] = a.dg; hnd[2] = a.dbe;
#pragma unroll
            for (int i = 0; i < 17; ++i) hnd[3 + i] = a.dw1[i];
        }
        __syncthreads();
        if (stage == 1) {
            a.db1 = hnd[0]; a.dg = hnd[1]; a.dbe = hnd[2];
#pragma unroll
            for (int i = 0; i < 17; ++i) a.dw1[i] = hnd[3 + i];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rg + kWgRG * i;
                if (r < nr) l1_row<RELU>(a, rinfo + (roff + r) * 8, xs + (roff + r) * XP, zv[i], dv[i], g1, be1, slope, sc);
            }
            my[0] = a.db1; my[1] = a.dg; my[2] = a.dbe;
#pragma unroll
            for (int i = 0; i < 17; ++i) my[3 + i] = a.dw1[i];
        }
        __syncthreads();
        if (llive) {
            float v = sum_groups<kWg2Cols>(red + ocol * kRedP + oitem, ohalf);
            if ((oitem == 1 || oitem == 2) && J.m.no_ln) v = 0.0f;
            if (ohalf == 0) {
                J.grad[lidx] = v;
                if (ADAM) lae.apply(J, A.ad, lidx, v);
            }
        }
        SPAN_LOG(HX_SPAN_WGRAD);
    }
}

// (the BC weight of the call: adam_w, hx_update.h)
__global__ __launch_bounds__(kThreads) void adam_kernel(AdamArgs A) {
    if (A.guard && __hip_atomic_load(A.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;  // failed exchange: fail-stop
    if (A.alpha_state && blockIdx.x == 0 && threadIdx.x == 0)  // a SAC policy step: the log-alpha step with the mean entropy
        sac_alpha_step(A.alpha_state, A.losses, A.losses[4], A.target_entropy, A.b1, A.b2, A.eps, A.alpha_step_size, A.bc2_sqrt);
    const float wmix = A.g2 ? adam_w(A) : 0.0f;  // (read before thread 0 of block 0 may store the new weight: same value either way)
    if (A.finish_actor && blockIdx.x == 0 && threadIdx.x == 0) {
        if (A.use_bc) {
            const float w = adam_w(A);
            A.losses[1] = A.losses[2] * w + A.losses[3] * (1.0f - w);  // HIRL.py:321
            A.losses[5] = w;
            *A.wstate = w;
        } else {
            A.losses[1] = A.losses[3];  // TD3.py:236
        }
    }
    const int i = (blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i >= A.n) return;
    if (i + 4 <= A.n) {  // the flat buffers are 16-B aligned and a multiple of 4 floats long: one 16-B access per array
        float4 g4 = *reinterpret_cast<const float4*>(A.g + i);
        if (A.g2) {  // g = w dL_bc + (1 - w) dL_rl  (HIRL.py:321), combined AFTER the exchange
            const float4 b4 = *reinterpret_cast<const float4*>(A.g2 + i);
            g4.x = wmix * b4.x + (1.0f - wmix) * g4.x;
            g4.y = wmix * b4.y + (1.0f - wmix) * g4.y;
            g4.z = wmix * b4.z + (1.0f - wmix) * g4.z;
            g4.w = wmix * b4.w + (1.0f - wmix) * g4.w;
        }
        adam_step4(A, i, make_float4(g4.x * A.gscale, g4.y * A.gscale, g4.z * A.gscale, g4.w * A.gscale));
        return;
    }
    for (int c = 0; c < A.n - i; ++c) {  // ragged tail
        float pv = A.p[i + c], mv = A.m[i + c], vv = A.v[i + c];
        const float gv = A.g2 ? wmix * A.g2[i + c] + (1.0f - wmix) * A.g[i + c] : A.g[i + c];
        adam_update(pv, mv, vv, gv * A.gscale, A.b1, A.b2, A.eps, A.step_size, A.bc2_sqrt);
        A.p[i + c] = pv; A.m[i + c] = mv; A.v[i + c] = vv;
        if (A.target) A.target[i + c] = polyak_update(A.target[i + c], pv, A.tau);
    }
}

// up to two (target, source) segments in one launch: blocks [0, nb1) walk the first, the rest the second
// guard: nullptr, or a word that must be 0 for the step to happen (HxNets.xchg_status: after a failed exchange no target moves either)
__global__ __launch_bounds__(kThreads) void polyak_kernel(float* target, const float* source, int n, float tau, float* target2 = nullptr,
                                                          const float* source2 = nullptr, int n2 = 0, const uint32_t* guard = nullptr) {
    if (guard && *guard != 0u) return;
    const int nb1 = (n / 4 + kThreads) / kThreads;
    int blk = blockIdx.x;
    if (blk >= nb1) {
        blk -= nb1; target = target2; source = source2; n = n2;
    }
    const int i = (blk * kThreads + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        float4 t4 = *reinterpret_cast<const float4*>(target + i);
        const float4 s4 = *reinterpret_cast<const float4*>(source + i);
        t4.x = polyak_update(t4.x, s4.x, tau);
        t4.y = polyak_update(t4.y, s4.y, tau);
        t4.z = polyak_update(t4.z, s4.z, tau);
        t4.w = polyak_update(t4.w, s4.w, tau);
        *reinterpret_cast<float4*>(target + i) = t4;
        return;
    }
    for (int c = 0; c < n - i; ++c) target[i + c] = polyak_update(target[i + c], source[i + c], tau);
}

}  // namespace

namespace hxu {

// HX_HEAD_RIDER=0 (read once): launch G evaluates the heads it feeds on itself, in every column workgroup — for A/B timing and the bit-for-bit test
bool head_rider_on() {
    static const bool on = !(getenv("HX_HEAD_RIDER") && atoi(getenv("HX_HEAD_RIDER")) == 0);
    return on;
}

void launch_wg(const WgArgs& W, bool adam, hipStream_t st) {
    WgArgsC C{};
    for (int j = 0; j < W.njobs; ++j) C.job[j] = pack_wg(W.job[j], W);
    const bool pre = W.predraw != nullptr;
    C.has_pre = pre ? 1 : 0;
    if (pre) { C.pre = *W.predraw; C.pre_batch = W.predraw_batch; }
    // head riders: the tiles take the slots the predraw's eight columns leave free, and as many more columns (eight at a time) as they need
    int head_tiles = 0;
    for (int h = 0; h < W.nhead && h < 2; ++h) {
        C.head[h] = HeadJobC{W.head[h].net, W.head[h].ws.x, W.head_rows[h], mlp_bits(W.head[h].m)};
        head_tiles += (W.head_rows[h] + RT - 1) / RT;
    }
    const int extra = (pre || head_tiles) ? extra_columns((pre ? 8 : 0) + head_tiles, W.njobs) : 0;
    const dim3 grid(kWgPerJob + extra, W.njobs);
    const bool relu = W.slope == 0.0f;
#define HX_WG(ADAM_, RELU_, BF16_) hipLaunchKernelGGL((wgrad_kernel<ADAM_, RELU_, BF16_>), grid, dim3(kWide), 0, st, C)
    static const int dbg_off = getenv("HX_DBG_BF16_OFF") ? atoi(getenv("HX_DBG_BF16_OFF")) : 0;
    // HX_WGRAD_TWO_SLOT=0 (read once): a two-slot job stays on wgrad_kernel's 112 workgroups too — for A/B timing and the bit-for-bit test
    static const bool two_on = !(getenv("HX_WGRAD_TWO_SLOT") && atoi(getenv("HX_WGRAD_TWO_SLOT")) == 0);
    const WgJob& J0 = W.job[0];
    if (W.bf16 && !(dbg_off & 4)) {
        if (adam) { if (relu) HX_WG(true, true, true); else HX_WG(true, false, true); }
        else { if (relu) HX_WG(false, true, true); else HX_WG(false, false, true); }
    } else if (two_on && head_tiles == 0 && W.njobs == 1 && J0.nslots == 2 && J0.rows[0] > 0 && J0.rows[1] > 0 && J0.rows[0] + J0.rows[1] <= kWgRowChunk) {
        // one job, two slots whose rows fit the LDS tiles together: each slot on its own threads, 224 workgroups (wgrad2_kernel)
        const dim3 grid2(kWg2PerJob + (pre ? 8 : 0), 1);
#define HX_WG2(ADAM_, RELU_) hipLaunchKernelGGL((wgrad2_kernel<ADAM_, RELU_>), grid2, dim3(kWide), 0, st, C)
        if (adam) { if (relu) HX_WG2(true, true); else HX_WG2(true, false); }
        else { if (relu) HX_WG2(false, true); else HX_WG2(false, false); }
#undef HX_WG2
    } else {
        if (adam) { if (relu) HX_WG(true, true, false); else HX_WG(true, false, false); }
        else { if (relu) HX_WG(false, true, false); else HX_WG(false, false, false); }
    }
#undef HX_WG
}
void launch_adam(const AdamArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(adam_kernel, dim3((A.n / 4 + kThreads) / kThreads), dim3(kThreads), 0, st, A);
}
void launch_polyak(float* target, const float* source, int n, float tau, float* target2, const float* source2, int n2, hipStream_t st, const uint32_t* guard) {
    const int nb = (n / 4 + kThreads) / kThreads + (target2 ? (n2 / 4 + kThreads) / kThreads : 0);
    hipLaunchKernelGGL(polyak_kernel, dim3(nb), dim3(kThreads), 0, st, target, source, n, tau, target2, source2, n2, guard);
}

}  // namespace hxu

extern "C" {

/* Adam step over a flat buffer (torch.optim.Adam defaults; step = 1-based step count; grad is multiplied by
 * grad_scale first — 1/world_size after a SUM all-reduce).  which: 0 critic, 1 actor (also finishes actor_loss /
 * bc_weight bookkeeping: w_kind 0 given, 1 estimate from soft_count, 2 reuse stored). */
static int adam_impl(const HxNets* N, const HxHyper* Hy, int32_t which, int32_t step, float grad_scale, int32_t w_kind, float w_given,
                     float warm, int32_t batch, const float* msg, void* stream) {
    const bool polyak = (which & 16) != 0;  // + 16: soft_update of this network's target in the same launch
    which &= 15;
    HX_REQUIRE(N && Hy && step >= 1 && which >= 0 && which <= 2, "hx_adam: bad arguments");
    AdamArgs A{};
    if (int rc = hirl_adam_fill(A, N, Hy, which, polyak, step, grad_scale, w_kind, w_given, warm, batch, msg, "hx_adam", "hx_adam_mixed")) return rc;
    launch_adam(A, (hipStream_t)stream);
    HX_CHECK_LAUNCH("hx_adam");
    return 0;
}
int hx_adam(const HxNets* N, const HxHyper* Hy, int32_t which, int32_t step, float grad_scale, int32_t w_kind, float w_given,
            float warm, int32_t batch, void* stream) {
    return adam_impl(N, Hy, which, step, grad_scale, w_kind, w_given, warm, batch, nullptr, stream);
}
/* The actor's optimizer step from the MERGED message of a sharded run (one collective for the whole actor phase):
 * msg = [dL_rl (hx_actor_param_count() floats, padded to 4) | dL_bc (same) | soft count as a float | ...], already summed over the
 * ranks; w = count / batch + warm (w_kind 1), the given or the stored weight otherwise; g = w dL_bc + (1 - w) dL_rl (HIRL.py:321). */
int hx_adam_mixed(const HxNets* N, const HxHyper* Hy, int32_t polyak, int32_t step, float grad_scale, int32_t w_kind, float w_given,
                  float warm, int32_t batch, const float* msg, void* stream) {
    HX_REQUIRE(msg, "hx_adam_mixed: null message");
    return adam_impl(N, Hy, 1 | (polyak ? 16 : 0), step, grad_scale, w_kind, w_given, warm, batch, msg, stream);
}

/* soft_update of both targets (HIRL.py:327-330) */
int hx_polyak(const HxNets* N, const HxHyper* Hy, void* stream) {
    HX_REQUIRE(N && Hy, "hx_polyak: bad arguments");
    const int nc = 2 * kQ.padded(), na = kActor.size();
    // (HxNets.xchg_status non-zero — a failed one-shot exchange: the targets stay where they are, like everything hx_adam* guards; the image
    //  refresh below then re-derives the same images from the unchanged targets)
    launch_polyak(N->target_critic, N->critic, nc, Hy->tau, N->target_actor, N->actor, na, (hipStream_t)stream, N->xchg_status);
    if (uint16_t* im = N->w2_bf16_all) {  // bf16 update path: the targets' images follow
        launch_pack_bf16(N->target_actor + kActor.W2(), im + IM_TA * kImgElems, false, (hipStream_t)stream);
        for (int h = 0; h < 2; ++h)
            launch_pack_bf16(N->target_critic + h * kQ.padded() + kQ.W2(), im + (IM_TC1 + h) * kImgElems, false, (hipStream_t)stream);
    }
    HX_CHECK_LAUNCH("hx_polyak");
    return 0;
}

/* Adam (torch defaults) for SAC.  which 0: q1_optim + q2_optim over the flat critic (SAC/agent.py:310-313); which 1:
 * policy_optim, followed in the same launch by the log-alpha step of alpha_optim with the mean entropy in losses[4]
 * (SAC/agent.py:318-325).  step: 1-based (all four optimisers step once per learn()).  grad_scale: 1/world after a SUM. */
int hx_sac_adam(const HxSacNets* N, const HxHyper* Hy, int32_t which, int32_t step, float grad_scale, float target_entropy, void* stream) {
    HX_REQUIRE(N && Hy && step >= 1 && (which == 0 || which == 1), "hx_sac_adam: bad arguments");
    AdamArgs A{};
    if (int rc = sac_adam_fill(A, N, Hy, which, step, grad_scale, target_entropy, /*alpha_step=*/true, "hx_sac_adam")) return rc;
    launch_adam(A, (hipStream_t)stream);
    HX_CHECK_LAUNCH("hx_sac_adam");
    return 0;
}

}  // extern "C"

HX_DEFINE_DEBUG_COLLECTORS(wgrad, 32, 56)
