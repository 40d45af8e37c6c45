// gsm_mlp.h — the device pieces the MLP heads share (gsm_actor.hip, gsm_critic.hip):
// a workgroup of kMlpThreads threads, one row of a tile per thread, the weights
// in LDS with W1 transposed to [cols][kH], a row's hidden units in registers.
//
// Every function keeps one written sequence of fp32 operations (the library is
// built with -ffp-contract=off), so a head's forward and backward, and two
// heads that share a chain, agree bit for bit.
#pragma once
#include <type_traits>

#include "gsm.h"
#include "gsm_device.h"

namespace gsm {

constexpr int kMlpThreads = 128;   // = rows of a tile
// both heads' names for the workgroup size and their dynamic-LDS ceiling (the actor head had them first)
constexpr int kActorThreads = kMlpThreads;
constexpr int kActorLdsMax = 160 * 1024;

// The weights into LDS (scalar loads: no alignment asked of them). W1
// [kH][cols] is transposed to [cols][kH]; W2 [n_out][KW] and b2 are padded with
// zero rows up to kO (b2 to at least four floats). kH == 0: no first layer.
template <int kH, int kO>
__device__ __forceinline__ void mlp_load_weights(const float *w1, const float *b1, const float *w2, const float *b2,
                                                 int cols, int KW, int n_out, float *s_w1, float *s_b1, float *s_w2,
                                                 float *s_b2) {
    const int tid = threadIdx.x;
    if (kH) {
        for (int i = tid; i < kH * cols; i += kMlpThreads) {
            const int j = i / cols, k = i - j * cols;
            s_w1[k * kH + j] = w1[i];
        }
        for (int i = tid; i < kH; i += kMlpThreads) s_b1[i] = b1[i];
    }
    for (int i = tid; i < kO * KW; i += kMlpThreads) s_w2[i] = i < n_out * KW ? w2[i] : 0.0f;
    for (int i = tid; i < (kO < 4 ? 4 : kO); i += kMlpThreads) s_b2[i] = i < n_out ? b2[i] : 0.0f;
}

// Rows [row0, row0 + 128) of x into the tile, a row padded by (1, 0, 0, 0);
// a row that on(row) rejects is staged as zeros and never read from memory.
template <class Pred>
__device__ __forceinline__ void mlp_load_tile(const float *__restrict__ x, int64_t x_stride, int64_t row0, int n4,
                                              float *xs, int XS, const Pred &on) {
    const int per = n4 + 1;
    for (int i = threadIdx.x; i < kMlpThreads * per; i += kMlpThreads) {
        const int row = i / per, c4 = i - row * per;
        float4 v = make_float4(c4 < n4 ? 0.0f : 1.0f, 0.0f, 0.0f, 0.0f);
        if (c4 < n4 && on(row)) v = *reinterpret_cast<const float4 *>(x + (row0 + row) * x_stride + 4 * c4);
        *reinterpret_cast<float4 *>(xs + row * XS + 4 * c4) = v;
    }
}

// h[0..kH) continued over n4 groups of four inputs of the row xr, w1t the
// [.][kH] rows of W1^T that belong to them, in ascending input order; then
// relu. The caller preloads h (the bias, or a prefix of the chain).
template <int kH>
__device__ __forceinline__ void mlp_hidden(const float *__restrict__ xr, const float *__restrict__ w1t, int n4,
                                           float (&h)[kH]) {
#pragma unroll 1
    for (int k4 = 0; k4 < n4; ++k4) {
        const float4 xv = *reinterpret_cast<const float4 *>(xr + 4 * k4);
        const float xk[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {   // input 4 k4 + kk into every h[j]: 16-byte reads of four j
            const float *wk = w1t + (4 * k4 + kk) * kH;
#pragma unroll
            for (int j4 = 0; j4 < kH / 4; ++j4) {
                const float4 w = *reinterpret_cast<const float4 *>(wk + 4 * j4);
                h[4 * j4] = fmaf(w.x, xk[kk], h[4 * j4]);
                h[4 * j4 + 1] = fmaf(w.y, xk[kk], h[4 * j4 + 1]);
                h[4 * j4 + 2] = fmaf(w.z, xk[kk], h[4 * j4 + 2]);
                h[4 * j4 + 3] = fmaf(w.w, xk[kk], h[4 * j4 + 3]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kH; ++j) h[j] = h[j] < 0.0f ? 0.0f : h[j];   // a NaN stays a NaN
}

// out[o] = b2[o] + <W2[o], h>, all kO chains side by side (the padded rows of
// W2 are zeros and their outputs are never looked at)
template <int kH, int kO>
__device__ __forceinline__ void mlp_output(const float *__restrict__ w2, const float *__restrict__ b2,
                                           const float (&h)[kH], float (&out)[kO]) {
#pragma unroll
    for (int o = 0; o < kO; ++o) out[o] = b2[o];
#pragma unroll
    for (int j4 = 0; j4 < kH / 4; ++j4) {
#pragma unroll
        for (int o = 0; o < kO; ++o) {
            const float4 w = *reinterpret_cast<const float4 *>(w2 + o * kH + 4 * j4);
            out[o] = fmaf(w.x, h[4 * j4], out[o]);
            out[o] = fmaf(w.y, h[4 * j4 + 1], out[o]);
            out[o] = fmaf(w.z, h[4 * j4 + 2], out[o]);
            out[o] = fmaf(w.w, h[4 * j4 + 3], out[o]);
        }
    }
}

// dh = W2^T d over the first n outputs where h > 0, in h's registers
template <int kH, int kO>
__device__ __forceinline__ void mlp_hidden_grad(const float *__restrict__ w2, const float (&d)[kO], int n,
                                                float (&h)[kH]) {
#pragma unroll
    for (int j4 = 0; j4 < kH / 4; ++j4) {
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int o = 0; o < kO; ++o)
            if (o < n) {
                const float4 w = *reinterpret_cast<const float4 *>(w2 + o * kH + 4 * j4);
                g.x = fmaf(w.x, d[o], g.x), g.y = fmaf(w.y, d[o], g.y);
                g.z = fmaf(w.z, d[o], g.z), g.w = fmaf(w.w, d[o], g.w);
            }
        h[4 * j4] = h[4 * j4] > 0.0f ? g.x : 0.0f;
        h[4 * j4 + 1] = h[4 * j4 + 1] > 0.0f ? g.y : 0.0f;
        h[4 * j4 + 2] = h[4 * j4 + 2] > 0.0f ? g.z : 0.0f;
        h[4 * j4 + 3] = h[4 * j4 + 3] > 0.0f ? g.w : 0.0f;
    }
}

// the row's h (or dh) into its LDS row; kPad: with the pad (1, 0, 0, 0), the
// column of ones whose product is the bias gradient, which is written once
template <int kH, bool kPad>
__device__ __forceinline__ void mlp_store_row(float *hr, const float (&h)[kH]) {
#pragma unroll
    for (int j4 = 0; j4 < kH / 4; ++j4)
        *reinterpret_cast<float4 *>(hr + 4 * j4) = make_float4(h[4 * j4], h[4 * j4 + 1], h[4 * j4 + 2], h[4 * j4 + 3]);
    if (kPad) *reinterpret_cast<float4 *>(hr + kH) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
}

// Four components of W1^T g: w1t the four [kH] rows of W1^T, g a pointer into
// LDS (the thread's own stores, or an env's sum): read back from there so that
// the caller's loop is not unrolled over registers.
template <int kH>
__device__ __forceinline__ float4 mlp_dx_group(const float *w1t, const float *gs) {
    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int j4 = 0; j4 < kH / 4; ++j4) {
        const float4 g = *reinterpret_cast<const float4 *>(gs + 4 * j4);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float4 w = *reinterpret_cast<const float4 *>(w1t + kk * kH + 4 * j4);
            d[kk] = fmaf(w.x, g.x, d[kk]);
            d[kk] = fmaf(w.y, g.y, d[kk]);
            d[kk] = fmaf(w.z, g.z, d[kk]);
            d[kk] = fmaf(w.w, g.w, d[kk]);
        }
    }
    return make_float4(d[0], d[1], d[2], d[3]);
}

// acc[i][.] += a[i] * b[.]: one row's contribution to a 4x4 tile of A^T B
__device__ __forceinline__ void mlp_outer(float4 (&acc)[4], const float4 a, const float4 b) {
    acc[0].x = fmaf(a.x, b.x, acc[0].x), acc[0].y = fmaf(a.x, b.y, acc[0].y);
    acc[0].z = fmaf(a.x, b.z, acc[0].z), acc[0].w = fmaf(a.x, b.w, acc[0].w);
    acc[1].x = fmaf(a.y, b.x, acc[1].x), acc[1].y = fmaf(a.y, b.y, acc[1].y);
    acc[1].z = fmaf(a.y, b.z, acc[1].z), acc[1].w = fmaf(a.y, b.w, acc[1].w);
    acc[2].x = fmaf(a.z, b.x, acc[2].x), acc[2].y = fmaf(a.z, b.y, acc[2].y);
    acc[2].z = fmaf(a.z, b.z, acc[2].z), acc[2].w = fmaf(a.z, b.w, acc[2].w);
    acc[3].x = fmaf(a.w, b.x, acc[3].x), acc[3].y = fmaf(a.w, b.y, acc[3].y);
    acc[3].z = fmaf(a.w, b.z, acc[3].z), acc[3].w = fmaf(a.w, b.w, acc[3].w);
}

// One 4x4 tile of A^T B over n rows of LDS: four columns of A at sa (row
// stride SA), four of B at sb (row stride SB), the rows in ascending order
__device__ __forceinline__ void mlp_gemm_tile(float4 (&acc)[4], const float *sa, int SA, const float *sb, int SB,
                                              int n) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
    for (int row = 0; row < n; ++row)
        mlp_outer(acc, *reinterpret_cast<const float4 *>(sa + row * SA),
                  *reinterpret_cast<const float4 *>(sb + row * SB));
}

// One 4x4 tile of a gradient block into the workgroup's partial: rows
// m0..m0+3 (< n_rows), columns c4*4.. of `mat` ([n_rows][n_cols]) or, for the
// pad column block (c4 == n_cols / 4), its first column into `bias`. The first
// tile of rows sets the partial, the later ones add to it (the same thread
// owns the same entries every time). One branch on `first` per row, not a
// select per element: behind mlp_gemm_tile the selects are vectorised with the
// accumulators and cost gsm_actor_bwd_kernel<0> a wave of occupancy (85 -> 109
// VGPRs).
__device__ __forceinline__ void mlp_add_tile(const float4 (&acc)[4], int m0, int c4, int n_rows, int n_cols,
                                             float *mat, float *bias, bool first) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + i;
        if (m >= n_rows) continue;
        if (4 * c4 < n_cols) {
            float *d = mat + m * n_cols + 4 * c4;
            if (first) {
                d[0] = acc[i].x, d[1] = acc[i].y, d[2] = acc[i].z, d[3] = acc[i].w;
            } else {
                d[0] = d[0] + acc[i].x, d[1] = d[1] + acc[i].y, d[2] = d[2] + acc[i].z, d[3] = d[3] + acc[i].w;
            }
        } else {
            bias[m] = first ? acc[i].x : bias[m] + acc[i].x;
        }
    }
}

template <class K>
static hipError_t actor_lds_attr(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds);
}

// one head kernel on `blocks` workgroups with `lds` bytes of dynamic LDS
template <class K, class P>
static hipError_t mlp_launch(K kernel, unsigned blocks, size_t lds, const P &p, hipStream_t s) {
    const hipError_t e = actor_lds_attr(kernel, lds);
    if (e != hipSuccess) return e;
    kernel<<<blocks, kMlpThreads, lds, s>>>(p);
    return hipSuccess;
}

// f(std::integral_constant<int, hidden>) for the hidden sizes the heads are
// built for; kLinear: 0 (no hidden layer) is one of them
template <bool kLinear, class F>
static hipError_t mlp_dispatch_hidden(int hidden, const F &f) {
    switch (hidden) {
        case 0:
            if constexpr (kLinear) return f(std::integral_constant<int, 0>{});
            else return hipErrorInvalidValue;
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gsm
