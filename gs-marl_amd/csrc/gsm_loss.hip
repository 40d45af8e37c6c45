// gsm_loss.hip — the clipped PPO / Lagrangian loss: logp, entropy and the twin
// values of the heads -> the loss, eight statistics and the row gradients
// (gsm_ppo_loss). The contract is in include/gsm.h.
//
// Mapping: an item is four consecutive rows, one item per thread, 256 threads a
// workgroup, a capped grid with a grid-stride loop over the items. With R % 4
// == 0 and every pointer 16-byte aligned an item is one 16-byte load per input
// (kVec); otherwise the same four rows by scalar loads. Either way a thread
// adds the same rows in the same order, so the sums do not depend on the path.
// A row of weight 0 is never loaded by the scalar path and never used by
// either: its inputs may hold NaN.
//
// Pass 1 (gsm_ppo_loss_partial_kernel): every thread adds its rows' eight
// weighted terms, the wave adds its 64 lanes (a shuffle tree), the workgroup
// its four waves through LDS, and one [8] partial per workgroup goes to `work`.
// When the gradients are wanted it also writes w_r * d_r of its rows.
// Pass 2 (gsm_ppo_loss_finish_kernel): every workgroup adds the partials' W in
// one fixed order (loss_block_sum, the same code in every workgroup, so the
// same bits) and multiplies its rows' w_r * d_r by 1.0f / W in place;
// workgroup 0 also adds the other seven partials and writes loss and stats.
// Without gradients pass 2 is one workgroup. No float atomics.
#include "gsm.h"
#include "gsm_internal.h"

namespace gsm {

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 256;      // one per CU: the size of `work`, in partials
constexpr int kLossSums = 8;             // loss, policy, entropy, value 0, value 1, KL, clip fraction, W

// a row's terms and the derivatives of its term with respect to logp and v
struct LossRow {
    float t, pol, kl, out, val[2], d_logp, d_v[2];
};

// Every line one correctly rounded fp32 operation; the selects are written as
// comparisons so that a NaN stays a NaN (fminf / fmaxf would drop it).
__device__ __forceinline__ LossRow loss_row(const LossParams &p, float lam, float lo, float hi, float logp, float ent,
                                            float logp_old, const float (&v)[2], const float (&adv)[2],
                                            const float (&v_old)[2], const float (&ret)[2]) {
    LossRow o;
    const float A = p.nO == 2 ? adv[0] - lam * adv[1] : adv[0];
    const float ratio = expf(logp - logp_old);
    const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
    const float s1 = ratio * A, s2 = rc * A;
    const bool inside = ratio >= lo && ratio <= hi;
    o.pol = -(s1 < s2 ? s1 : s2);
    o.d_logp = (inside || s1 < s2) ? -s1 : 0.0f;
    o.kl = logp_old - logp;
    o.out = inside ? 0.0f : 1.0f;
    float vsum = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        o.val[h] = 0.0f, o.d_v[h] = 0.0f;
        if (h < p.nO) {
            const float d = v[h] - v_old[h];
            const float dc = d < -p.value_clip ? -p.value_clip : (d > p.value_clip ? p.value_clip : d);
            const float vc = v_old[h] + dc;
            const float e1 = v[h] - ret[h], e2 = vc - ret[h];
            const float q1 = e1 * e1, q2 = e2 * e2;
            o.val[h] = q1 > q2 ? q1 : q2;
            o.d_v[h] = (fabsf(d) <= p.value_clip || q1 > q2) ? (2.0f * e1) * p.value_coef : 0.0f;
            vsum = h == 0 ? o.val[h] : vsum + o.val[h];
        }
    }
    o.t = (o.pol - p.ent_coef * ent) + p.value_coef * vsum;
    return o;
}

// four consecutive floats from row r0 on: one 16-byte load (kVec, when any of
// them is needed), else a scalar load for each needed one; 0.0f elsewhere
template <bool kVec>
__device__ __forceinline__ void loss_load4(const float *__restrict__ src, int64_t r0, const bool (&need)[4],
                                           float (&out)[4]) {
    if constexpr (kVec) {
        const float4 q = *reinterpret_cast<const float4 *>(src + r0);
        out[0] = need[0] ? q.x : 0.0f, out[1] = need[1] ? q.y : 0.0f;
        out[2] = need[2] ? q.z : 0.0f, out[3] = need[3] ? q.w : 0.0f;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = need[k] ? src[r0 + k] : 0.0f;
    }
}

template <bool kVec>
__device__ __forceinline__ void loss_store4(float *__restrict__ dst, int64_t r0, int64_t R, const float (&v)[4]) {
    if constexpr (kVec) {
        *reinterpret_cast<float4 *>(dst + r0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (r0 + k < R) dst[r0 + k] = v[k];
    }
}

// the 64 lanes of a wave added by a shuffle tree; lane 0 holds the sum
__device__ __forceinline__ float loss_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// The workgroup's sum of v, returned to every thread: the wave tree, then the
// waves in ascending order. red: kLossThreads / 64 floats of LDS. The one
// order every total of pass 2 is formed in.
__device__ __forceinline__ float loss_block_sum(float v, float *red) {
    const int tid = threadIdx.x;
    v = loss_wave_sum(v);
    __syncthreads();   // the readers of the previous call are done
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float tot = red[0];
#pragma unroll
    for (int w = 1; w < kLossThreads / 64; ++w) tot = tot + red[w];
    return tot;
}

template <bool kVec>
__global__ __launch_bounds__(kLossThreads) void gsm_ppo_loss_partial_kernel(const LossParams p) {
    __shared__ float red[kLossThreads / 64][kLossSums];
    const int tid = threadIdx.x, N = p.n_agents;
    const int64_t R = p.R, n_items = (R + 3) >> 2;
    const float lam = p.nO == 2 ? *p.lam : 0.0f;
    float acc[kLossSums];
#pragma unroll
    for (int c = 0; c < kLossSums; ++c) acc[c] = 0.0f;
    int flags = 0;
    for (int64_t item = (int64_t)blockIdx.x * kLossThreads + tid; item < n_items;
         item += (int64_t)gridDim.x * kLossThreads) {
        const int64_t r0 = item << 2;
        // the rows' weights: the agent mask first (a padded row's weight is not looked at)
        bool valid[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t r = r0 + k;
            valid[k] = r < R;
            if (valid[k] && p.n_valid) {
                const int64_t b = r / N;
                const int i = (int)(r - b * N);
                int n = p.n_valid[b];
                if (n < 0 || n > N) {
                    flags |= GSM_LOSS_BAD_COUNT;
                    n = n < 0 ? 0 : N;
                }
                valid[k] = i < n;
            }
        }
        float w[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (p.weight && (valid[0] || valid[1] || valid[2] || valid[3])) loss_load4<kVec>(p.weight, r0, valid, w);
        bool on[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (valid[k] && !(w[k] >= 0.0f && __builtin_isfinite(w[k]))) {
                flags |= GSM_LOSS_BAD_WEIGHT;
                w[k] = 0.0f;
            }
            if (!valid[k]) w[k] = 0.0f;
            on[k] = w[k] != 0.0f;
            any = any || on[k];
        }
        float gl[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ge[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float gv[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
        if (any) {
            float logp[4], ent[4], logp_old[4], v[2][4], adv[2][4], v_old[2][4], ret[2][4];
            loss_load4<kVec>(p.logp, r0, on, logp);
            loss_load4<kVec>(p.ent, r0, on, ent);
            loss_load4<kVec>(p.logp_old, r0, on, logp_old);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h < p.nO) {
                    loss_load4<kVec>(p.values + h * R, r0, on, v[h]);
                    loss_load4<kVec>(p.adv + h * R, r0, on, adv[h]);
                    loss_load4<kVec>(p.v_old + h * R, r0, on, v_old[h]);
                    loss_load4<kVec>(p.ret + h * R, r0, on, ret[h]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[h][k] = adv[h][k] = v_old[h][k] = ret[h][k] = 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!on[k]) continue;
                const float vk[2] = {v[0][k], v[1][k]}, ak[2] = {adv[0][k], adv[1][k]};
                const float ok[2] = {v_old[0][k], v_old[1][k]}, rk[2] = {ret[0][k], ret[1][k]};
                const LossRow o = loss_row(p, lam, p.ratio_lo, p.ratio_hi, logp[k], ent[k], logp_old[k], vk, ak, ok,
                                           rk);
                if (!__builtin_isfinite(o.t)) flags |= GSM_LOSS_NONFINITE;
                const float wk = w[k];
                acc[0] = acc[0] + wk * o.t;
                acc[1] = acc[1] + wk * o.pol;
                acc[2] = acc[2] + wk * ent[k];
                acc[3] = acc[3] + wk * o.val[0];
                acc[4] = acc[4] + wk * o.val[1];
                acc[5] = acc[5] + wk * o.kl;
                acc[6] = acc[6] + wk * o.out;
                acc[7] = acc[7] + wk;
                gl[k] = wk * o.d_logp;
                ge[k] = wk * -p.ent_coef;
                gv[0][k] = wk * o.d_v[0];
                gv[1][k] = wk * o.d_v[1];
            }
        }
        if (p.g_logp) {
            loss_store4<kVec>(p.g_logp, r0, R, gl);
            loss_store4<kVec>(p.g_ent, r0, R, ge);
            loss_store4<kVec>(p.g_values, r0, R, gv[0]);
            if (p.nO == 2) loss_store4<kVec>(p.g_values + R, r0, R, gv[1]);
        }
    }
    if (flags && p.status) atomicOr(p.status, flags);
#pragma unroll
    for (int c = 0; c < kLossSums; ++c) {
        const float s = loss_wave_sum(acc[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = s;
    }
    __syncthreads();
    if (tid < kLossSums) {
        float tot = red[0][tid];
#pragma unroll
        for (int wv = 1; wv < kLossThreads / 64; ++wv) tot = tot + red[wv][tid];
        p.work[(int64_t)blockIdx.x * kLossSums + tid] = tot;
    }
}

// the sum of component c over the n_part partials: a thread adds partials tid,
// tid + 256, .. in ascending order, then loss_block_sum
__device__ __forceinline__ float loss_total(const float *__restrict__ part, int n_part, int c, float *red) {
    float s = 0.0f;
    for (int j = threadIdx.x; j < n_part; j += kLossThreads) s = s + part[(int64_t)j * kLossSums + c];
    return loss_block_sum(s, red);
}

template <bool kVec>
__global__ __launch_bounds__(kLossThreads) void gsm_ppo_loss_finish_kernel(const LossParams p, int n_part) {
    __shared__ float red[kLossThreads / 64];
    const int tid = threadIdx.x;
    const float W = loss_total(p.work, n_part, kLossSums - 1, red);
    const bool some = W > 0.0f;
    if (blockIdx.x == 0) {
        float tot[kLossSums - 1];
#pragma unroll
        for (int c = 0; c < kLossSums - 1; ++c) tot[c] = loss_total(p.work, n_part, c, red);
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < kLossSums - 1; ++c) p.stats[c] = some ? tot[c] / W : 0.0f;
            p.stats[kLossSums - 1] = some ? W : 0.0f;
            p.loss[0] = some ? tot[0] / W : 0.0f;
        }
    }
    if (!p.g_logp) return;
    const float inv = some ? 1.0f / W : 0.0f;
    const int64_t R = p.R, n_items = (R + 3) >> 2;
    for (int64_t item = (int64_t)blockIdx.x * kLossThreads + tid; item < n_items;
         item += (int64_t)gridDim.x * kLossThreads) {
        const int64_t r0 = item << 2;
        float *dst[4] = {p.g_logp, p.g_ent, p.g_values, p.nO == 2 ? p.g_values + R : nullptr};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (!dst[a]) continue;
            if constexpr (kVec) {
                float4 q = *reinterpret_cast<float4 *>(dst[a] + r0);
                q.x = q.x * inv, q.y = q.y * inv, q.z = q.z * inv, q.w = q.w * inv;
                *reinterpret_cast<float4 *>(dst[a] + r0) = q;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (r0 + k < R) dst[a][r0 + k] = dst[a][r0 + k] * inv;
            }
        }
    }
}

int64_t ppo_loss_work_floats() { return (int64_t)kLossMaxBlocks * kLossSums; }

static bool loss_aligned(const void *q) { return ((uintptr_t)q & 15) == 0; }

hipError_t launch_ppo_loss(const LossParams &p, hipStream_t s) {
    const int64_t n_items = (p.R + 3) >> 2;
    const int64_t want = (n_items + kLossThreads - 1) / kLossThreads;
    const unsigned blocks = (unsigned)(want < kLossMaxBlocks ? want : kLossMaxBlocks);
    // null pointers count as aligned: they are not read
    const bool vec = p.R % 4 == 0 && loss_aligned(p.logp) && loss_aligned(p.ent) && loss_aligned(p.values) &&
                     loss_aligned(p.logp_old) && loss_aligned(p.adv) && loss_aligned(p.v_old) &&
                     loss_aligned(p.ret) && loss_aligned(p.weight) && loss_aligned(p.g_logp) &&
                     loss_aligned(p.g_ent) && loss_aligned(p.g_values);
    (void)hipGetLastError();
    if (blocks) {
        if (vec) gsm_ppo_loss_partial_kernel<true><<<blocks, kLossThreads, 0, s>>>(p);
        else gsm_ppo_loss_partial_kernel<false><<<blocks, kLossThreads, 0, s>>>(p);
    }
    const unsigned blocks2 = (p.g_logp && blocks) ? blocks : 1u;
    if (vec) gsm_ppo_loss_finish_kernel<true><<<blocks2, kLossThreads, 0, s>>>(p, (int)blocks);
    else gsm_ppo_loss_finish_kernel<false><<<blocks2, kLossThreads, 0, s>>>(p, (int)blocks);
    return hipGetLastError();
}

}  // namespace gsm
