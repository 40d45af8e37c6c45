// gsm_actor.h — the actor head (included by gsm_gnn.hip): features -> MLP ->
// categorical distribution -> Philox-sampled action, log-probability, entropy
// (gsm_actor_sample), the same head on stored actions (gsm_actor_eval) and its
// gradients (gsm_actor_eval_bwd). The contract is in include/gsm.h.
//
// Mapping: a workgroup of 128 threads takes tiles of 128 rows, one row per
// thread. The weights sit in LDS for the workgroup's life, W1 transposed to
// [in][hidden] (read as 16-byte broadcasts: every lane wants the same four
// W1[j..j+3][k], which go into four independent chains); a tile's x rows are
// staged into LDS by coalesced 16-byte loads, a row padded by four floats
// (1, 0, 0, 0): the pad spreads the rows over the banks and, in the backward,
// is the column of ones whose product with dh is db1. A row's hidden
// activations and logits live in registers; nothing per-row goes to global
// memory but the outputs.
//
// Every dot product is an explicit fmaf chain from the bias in ascending input
// index (actor_head, the one function all three kernels form the logits and
// the softmax statistics with), so sample and eval agree bit for bit.
//
// Backward: the per-row part (dlogit, dh, dx) runs a row per thread; the
// weight gradients are two small GEMMs over the tile's rows, dW2|db2 = dlogit^T
// [h | 1] and dW1|db1 = dh^T [x | 1], from LDS with a 4x4 register tile per
// thread, each tile's products added by their owning thread to the workgroup's
// partial in `work` (a few KB that stay in L2, so no accumulator is held over
// the per-row part); gsm_actor_bwd_sum_kernel adds the partials in a fixed
// order. No float atomics.
#pragma once
#include "gsm.h"
#include "gsm_device.h"
#include "gsm_philox.h"

namespace gsm {

constexpr int kActorThreads = 128;       // = rows of a tile
constexpr int kActorMaxActions = 8;
constexpr int kActorFwdMaxBlocks = 2048;
constexpr int kActorBwdMaxBlocks = 512;  // two per CU: the size of `work`
constexpr int kActorLdsMax = 160 * 1024;

// LDS, in floats; every block starts on a 16-byte boundary (in % 4 == 0, kH % 16 == 0)
struct ActorLds {
    int xs, w1, b1, w2, b2, hs, ds, total;
    int XS, KW, HS;   // row strides of the x tile, of w2 and of the h tile
};

__host__ __device__ inline ActorLds actor_lds(int in, int kH, bool bwd) {
    ActorLds L;
    L.XS = in + 4;
    L.KW = kH ? kH : in;
    L.HS = kH + 4;
    int o = 0;
    L.xs = o, o += kActorThreads * L.XS;
    L.w1 = o, o += kH * in;
    L.b1 = o, o += kH;
    L.w2 = o, o += kActorMaxActions * L.KW;
    L.b2 = o, o += kActorMaxActions;
    L.hs = o, o += (bwd && kH) ? kActorThreads * L.HS : 0;
    L.ds = o, o += bwd ? kActorThreads * kActorMaxActions : 0;
    L.total = o;
    return L;
}

// the weights into LDS (scalar loads: no alignment asked of them); the rows of
// w2 / b2 past n_actions are zeros
template <int kH>
__device__ __forceinline__ void actor_load_weights(const ActorParams &p, const ActorLds &L, float *sm) {
    const int tid = threadIdx.x;
    if (kH) {
        for (int i = tid; i < kH * p.in; i += kActorThreads) {   // transposed: [in][kH]
            const int j = i / p.in, k = i - j * p.in;
            sm[L.w1 + k * kH + j] = p.w1[i];
        }
        for (int i = tid; i < kH; i += kActorThreads) sm[L.b1 + i] = p.b1[i];
    }
    for (int i = tid; i < kActorMaxActions * L.KW; i += kActorThreads)
        sm[L.w2 + i] = i < p.nA * L.KW ? p.w2[i] : 0.0f;
    for (int i = tid; i < kActorMaxActions; i += kActorThreads) sm[L.b2 + i] = i < p.nA ? p.b2[i] : 0.0f;
}

// rows [row0, row0 + 128) of x into the tile, zeros past R, the pad (1, 0, 0, 0)
__device__ __forceinline__ void actor_load_tile(const ActorParams &p, const ActorLds &L, float *sm, int64_t row0) {
    const int n4 = p.in >> 2, per = n4 + 1;
    for (int i = threadIdx.x; i < kActorThreads * per; i += kActorThreads) {
        const int row = i / per, c4 = i - row * per;
        float4 v = make_float4(c4 < n4 ? 0.0f : 1.0f, 0.0f, 0.0f, 0.0f);
        if (c4 < n4 && row0 + row < p.R)
            v = *reinterpret_cast<const float4 *>(p.x + (row0 + row) * p.x_stride + 4 * c4);
        *reinterpret_cast<float4 *>(sm + L.xs + row * L.XS + 4 * c4) = v;
    }
}

struct ActorRow {
    float l[kActorMaxActions];   // logits (0 past n_actions)
    float e[kActorMaxActions];   // exp(l - m)
    float m, s, logs;
    bool finite;
};

// The head of one row, from the row's x in LDS: h (kH > 0), the logits and the
// softmax statistics, each line one fp32 operation in the documented order.
template <int kH>
__device__ __forceinline__ void actor_head(const float *__restrict__ xr, const float *__restrict__ sm,
                                           const ActorLds &L, int in, int nA, float (&h)[kH ? kH : 1],
                                           ActorRow &o) {
    const int n4 = in >> 2;
    if constexpr (kH > 0) {
#pragma unroll
        for (int j = 0; j < kH; ++j) h[j] = sm[L.b1 + j];
#pragma unroll 1
        for (int k4 = 0; k4 < n4; ++k4) {
            const float4 xv = *reinterpret_cast<const float4 *>(xr + 4 * k4);
            const float xk[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {   // input 4 k4 + kk into every h[j]: 16-byte reads of four j
                const float *wk = sm + L.w1 + (4 * k4 + kk) * kH;
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
        // all eight chains side by side (the rows of w2 past n_actions are zeros and their
        // logits are never looked at)
#pragma unroll
        for (int a = 0; a < kActorMaxActions; ++a) o.l[a] = sm[L.b2 + a];
#pragma unroll
        for (int j4 = 0; j4 < kH / 4; ++j4) {
#pragma unroll
            for (int a = 0; a < kActorMaxActions; ++a) {
                const float4 w = *reinterpret_cast<const float4 *>(sm + L.w2 + a * kH + 4 * j4);
                o.l[a] = fmaf(w.x, h[4 * j4], o.l[a]);
                o.l[a] = fmaf(w.y, h[4 * j4 + 1], o.l[a]);
                o.l[a] = fmaf(w.z, h[4 * j4 + 2], o.l[a]);
                o.l[a] = fmaf(w.w, h[4 * j4 + 3], o.l[a]);
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < kActorMaxActions; ++a) o.l[a] = sm[L.b2 + a];
        for (int k4 = 0; k4 < n4; ++k4) {
            const float4 xv = *reinterpret_cast<const float4 *>(xr + 4 * k4);
#pragma unroll
            for (int a = 0; a < kActorMaxActions; ++a) {
                const float4 w = *reinterpret_cast<const float4 *>(sm + L.w2 + a * in + 4 * k4);
                o.l[a] = fmaf(w.x, xv.x, o.l[a]);
                o.l[a] = fmaf(w.y, xv.y, o.l[a]);
                o.l[a] = fmaf(w.z, xv.z, o.l[a]);
                o.l[a] = fmaf(w.w, xv.w, o.l[a]);
            }
        }
    }
    bool fin = true;
    float m = o.l[0];
#pragma unroll
    for (int a = 0; a < kActorMaxActions; ++a)
        if (a < nA) {
            fin = fin && __builtin_isfinite(o.l[a]);
            m = o.l[a] > m ? o.l[a] : m;
        }
    float s = 0.0f;
#pragma unroll
    for (int a = 0; a < kActorMaxActions; ++a) {
        o.e[a] = a < nA ? expf(o.l[a] - m) : 0.0f;
        s = a == 0 ? o.e[0] : (a < nA ? s + o.e[a] : s);
    }
    o.m = m;
    o.s = s;
    o.logs = logf(s);
    o.finite = fin;
}

// entropy = log s - (sum_a e_a (l_a - m)) / s, the sum ascending
__device__ __forceinline__ float actor_entropy(const ActorRow &o, int nA) {
    float t = 0.0f;
#pragma unroll
    for (int a = 0; a < kActorMaxActions; ++a) {
        const float term = o.e[a] * (o.l[a] - o.m);
        t = a == 0 ? term : (a < nA ? t + term : t);
    }
    return o.logs - t / o.s;
}

// v[a] without a dynamic register index: the one matching element's bits (0.0f
// for an a out of range). Not a chain of selects between the elements, which
// the compiler turns into an indexed load from a stack copy of v.
__device__ __forceinline__ float actor_pick(const float (&v)[kActorMaxActions], int a) {
    uint32_t bits = 0u;
#pragma unroll
    for (int i = 0; i < kActorMaxActions; ++i) bits |= a == i ? __float_as_uint(v[i]) : 0u;
    return __uint_as_float(bits);
}

// kEval = false: gsm_actor_sample; true: gsm_actor_eval
template <int kH, bool kEval>
__global__ __launch_bounds__(kActorThreads) void gsm_actor_fwd_kernel(const ActorParams p) {
    extern __shared__ __align__(16) float actor_sm[];
    float *sm = actor_sm;
    const ActorLds L = actor_lds(p.in, kH, false);
    const int tid = threadIdx.x;
    actor_load_weights<kH>(p, L, sm);
    uint32_t draw = 0;
    if (!kEval && !p.deterministic) draw = (uint32_t)(p.draw_host + (p.draw_dev ? *p.draw_dev : 0));
    const int n_tiles = (p.R + kActorThreads - 1) / kActorThreads;
    const float qnan = __builtin_nanf("");
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = (int64_t)tile * kActorThreads;
        __syncthreads();   // the previous tile's readers are done (and, first, the weights are in)
        actor_load_tile(p, L, sm, row0);
        __syncthreads();
        float h[kH ? kH : 1];
        ActorRow o;
        actor_head<kH>(sm + L.xs + tid * L.XS, sm, L, p.in, p.nA, h, o);
        const int64_t r = row0 + tid;
        if (r >= p.R) continue;   // no barrier below
        int act = 0, flag = 0;
        if (kEval) {
            act = p.actions_in[r];
            if (act < 0 || act >= p.nA) flag |= GSM_ACTOR_BAD_ACTION;
        } else if (o.finite) {
            if (p.deterministic) {
                act = p.nA - 1;
#pragma unroll
                for (int a = kActorMaxActions - 1; a >= 0; --a)
                    if (a < p.nA && o.l[a] == o.m) act = a;
            } else {
                const int b = (int)(r / p.n_agents), i = (int)(r - (int64_t)b * p.n_agents);
                const Philox4 ph = philox4x32_10((uint32_t)i, draw, (uint32_t)(p.env_base + b), kTagPolicy, p.k0,
                                                 p.k1);
                const float t = u01(ph.x0) * o.s;
                float c = 0.0f;
                bool found = false;
                act = p.nA - 1;
#pragma unroll
                for (int a = 0; a < kActorMaxActions; ++a)
                    if (a < p.nA) {
                        c = c + o.e[a];
                        if (!found && t < c) act = a, found = true;
                    }
            }
        }
        if (!o.finite) flag |= GSM_ACTOR_NONFINITE;
        float lp = (actor_pick(o.l, act) - o.m) - o.logs;
        float ent = actor_entropy(o, p.nA);
        if (flag) {
            lp = qnan;
            if (!kEval) act = 0;
            if (!o.finite) ent = qnan;
            if (p.status) atomicOr(p.status, flag);
        }
        if (!kEval) p.actions_out[r] = act;
        p.logp[r] = lp;
        if (p.entropy) p.entropy[r] = ent;
        if (!kEval && p.logits_out) {
#pragma unroll
            for (int a = 0; a < kActorMaxActions; ++a)
                if (a < p.nA) p.logits_out[r * p.nA + a] = o.l[a];
        }
    }
}

// acc[i][.] += a[i] * b[.]: one row's contribution to a 4x4 tile of A^T B
__device__ __forceinline__ void actor_outer(float4 (&acc)[4], const float4 a, const float4 b) {
    acc[0].x = fmaf(a.x, b.x, acc[0].x), acc[0].y = fmaf(a.x, b.y, acc[0].y);
    acc[0].z = fmaf(a.x, b.z, acc[0].z), acc[0].w = fmaf(a.x, b.w, acc[0].w);
    acc[1].x = fmaf(a.y, b.x, acc[1].x), acc[1].y = fmaf(a.y, b.y, acc[1].y);
    acc[1].z = fmaf(a.y, b.z, acc[1].z), acc[1].w = fmaf(a.y, b.w, acc[1].w);
    acc[2].x = fmaf(a.z, b.x, acc[2].x), acc[2].y = fmaf(a.z, b.y, acc[2].y);
    acc[2].z = fmaf(a.z, b.z, acc[2].z), acc[2].w = fmaf(a.z, b.w, acc[2].w);
    acc[3].x = fmaf(a.w, b.x, acc[3].x), acc[3].y = fmaf(a.w, b.y, acc[3].y);
    acc[3].z = fmaf(a.w, b.z, acc[3].z), acc[3].w = fmaf(a.w, b.w, acc[3].w);
}

// One 4x4 tile of a gradient block into the workgroup's partial: rows
// m0..m0+3 (< n_rows), columns c4*4.. of `mat` ([n_rows][n_cols]) or, for the
// pad column block (c4 == n_cols / 4), its first column into `bias`. The first
// tile of rows sets the partial, the later ones add to it (the same thread
// owns the same entries every time).
__device__ __forceinline__ void actor_add_tile(const float4 (&acc)[4], int m0, int c4, int n_rows, int n_cols,
                                               float *mat, float *bias, bool first) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + i;
        if (m >= n_rows) continue;
        if (4 * c4 < n_cols) {
            float *d = mat + m * n_cols + 4 * c4;
            d[0] = first ? acc[i].x : d[0] + acc[i].x;
            d[1] = first ? acc[i].y : d[1] + acc[i].y;
            d[2] = first ? acc[i].z : d[2] + acc[i].z;
            d[3] = first ? acc[i].w : d[3] + acc[i].w;
        } else {
            bias[m] = first ? acc[i].x : bias[m] + acc[i].x;
        }
    }
}

// a partial: dw1 [kH][in], db1 [kH], dw2 [nA][KW], db2 [nA]
__host__ __device__ inline int actor_partial_floats(int in, int kH, int nA) {
    return kH * in + kH + nA * (kH ? kH : in) + nA;
}

template <int kH>
__global__ __launch_bounds__(kActorThreads) void gsm_actor_bwd_kernel(const ActorParams p) {
    extern __shared__ __align__(16) float actor_sm[];
    float *sm = actor_sm;
    const ActorLds L = actor_lds(p.in, kH, true);
    const int tid = threadIdx.x, in = p.in, nA = p.nA, n4 = in >> 2;
    actor_load_weights<kH>(p, L, sm);
    // this thread's tiles of the two products: (a4, c4) of dlogit^T [B | 1], (j4, c4) of dh^T [x | 1]
    const int per2 = (kH ? kH : in) / 4 + 1, n_items2 = 2 * per2;
    const int per1 = n4 + 1, n_items1 = (kH / 4) * per1;
    // the workgroup's partial: every tile of rows adds its products to it
    float *part = p.part + (int64_t)blockIdx.x * actor_partial_floats(in, kH, nA);
    float *pw1 = part, *pb1 = pw1 + kH * in, *pw2 = pb1 + kH, *pb2 = pw2 + nA * (kH ? kH : in);
    const int n_tiles = (p.R + kActorThreads - 1) / kActorThreads;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = (int64_t)tile * kActorThreads;
        __syncthreads();
        actor_load_tile(p, L, sm, row0);
        __syncthreads();
        const float *xr = sm + L.xs + tid * L.XS;
        float h[kH ? kH : 1];
        float dl[kActorMaxActions];
        {
            ActorRow o;
            actor_head<kH>(xr, sm, L, in, nA, h, o);
            const int64_t r = row0 + tid;
            const bool valid = r < p.R;
            int act = -1, flag = 0;
            float gl = 0.0f, ge = 0.0f;
            if (valid) {
                act = p.actions_in[r];
                gl = p.g_logp[r];
                if (p.g_ent) ge = p.g_ent[r];
                if (act < 0 || act >= nA) flag |= GSM_ACTOR_BAD_ACTION;
                if (!o.finite) flag |= GSM_ACTOR_NONFINITE;
                if (flag && p.status) atomicOr(p.status, flag);
            }
            const float H = actor_entropy(o, nA);
#pragma unroll
            for (int a = 0; a < kActorMaxActions; ++a) {
                const float pa = o.e[a] / o.s, lpa = (o.l[a] - o.m) - o.logs;
                float d = gl * ((a == act ? 1.0f : 0.0f) - pa);
                if (p.g_ent) d = d - ge * (pa * (lpa + H));
                dl[a] = (valid && a < nA) ? d : 0.0f;
            }
        }
        *reinterpret_cast<float4 *>(sm + L.ds + tid * 8) = make_float4(dl[0], dl[1], dl[2], dl[3]);
        *reinterpret_cast<float4 *>(sm + L.ds + tid * 8 + 4) = make_float4(dl[4], dl[5], dl[6], dl[7]);
        const int64_t r = row0 + tid;
        if constexpr (kH > 0) {
            float *hr = sm + L.hs + tid * L.HS;
#pragma unroll
            for (int j4 = 0; j4 < kH / 4; ++j4)
                *reinterpret_cast<float4 *>(hr + 4 * j4) = make_float4(h[4 * j4], h[4 * j4 + 1], h[4 * j4 + 2],
                                                                       h[4 * j4 + 3]);
            *reinterpret_cast<float4 *>(hr + kH) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
            // dh = W2^T dlogit where h > 0, in h's registers
#pragma unroll
            for (int j4 = 0; j4 < kH / 4; ++j4) {
                float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int a = 0; a < kActorMaxActions; ++a)
                    if (a < nA) {
                        const float4 w = *reinterpret_cast<const float4 *>(sm + L.w2 + a * kH + 4 * j4);
                        d.x = fmaf(w.x, dl[a], d.x), d.y = fmaf(w.y, dl[a], d.y);
                        d.z = fmaf(w.z, dl[a], d.z), d.w = fmaf(w.w, dl[a], d.w);
                    }
                h[4 * j4] = h[4 * j4] > 0.0f ? d.x : 0.0f;
                h[4 * j4 + 1] = h[4 * j4 + 1] > 0.0f ? d.y : 0.0f;
                h[4 * j4 + 2] = h[4 * j4 + 2] > 0.0f ? d.z : 0.0f;
                h[4 * j4 + 3] = h[4 * j4 + 3] > 0.0f ? d.w : 0.0f;
            }
        } else {
            if (p.dx && r < p.R)
                for (int k4 = 0; k4 < n4; ++k4) {
                    float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                    for (int a = 0; a < kActorMaxActions; ++a) {
                        const float4 w = *reinterpret_cast<const float4 *>(sm + L.w2 + a * in + 4 * k4);
                        d.x = fmaf(w.x, dl[a], d.x), d.y = fmaf(w.y, dl[a], d.y);
                        d.z = fmaf(w.z, dl[a], d.z), d.w = fmaf(w.w, dl[a], d.w);
                    }
                    *reinterpret_cast<float4 *>(p.dx + r * in + 4 * k4) = d;
                }
        }
        __syncthreads();   // dlogit and h (or x) of every row are in LDS
        const bool first = tile == (int)blockIdx.x;
        if (tid < n_items2) {
            const int a4 = tid / per2, c4 = tid - a4 * per2;
            const float *sa = sm + L.ds + 4 * a4;
            const float *sb = kH ? sm + L.hs + 4 * c4 : sm + L.xs + 4 * c4;
            const int SB = kH ? L.HS : L.XS;
            float4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
            for (int row = 0; row < kActorThreads; ++row)
                actor_outer(acc, *reinterpret_cast<const float4 *>(sa + row * 8),
                            *reinterpret_cast<const float4 *>(sb + row * SB));
            actor_add_tile(acc, 4 * a4, c4, nA, kH ? kH : in, pw2, pb2, first);
        }
        if constexpr (kH > 0) {
            __syncthreads();   // h has been read: dh takes its place
            float *hr = sm + L.hs + tid * L.HS;
#pragma unroll
            for (int j4 = 0; j4 < kH / 4; ++j4)
                *reinterpret_cast<float4 *>(hr + 4 * j4) = make_float4(h[4 * j4], h[4 * j4 + 1], h[4 * j4 + 2],
                                                                       h[4 * j4 + 3]);
            // dx = W1^T dh, the row's dh read back from LDS (the thread's own stores) so that
            // this loop is not unrolled over h's registers
            if (p.dx && r < p.R)
                for (int k4 = 0; k4 < n4; ++k4) {
                    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
                    for (int j4 = 0; j4 < kH / 4; ++j4) {
                        const float4 g = *reinterpret_cast<const float4 *>(hr + 4 * j4);
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            const float4 w =
                                *reinterpret_cast<const float4 *>(sm + L.w1 + (4 * k4 + kk) * kH + 4 * j4);
                            d[kk] = fmaf(w.x, g.x, d[kk]);
                            d[kk] = fmaf(w.y, g.y, d[kk]);
                            d[kk] = fmaf(w.z, g.z, d[kk]);
                            d[kk] = fmaf(w.w, g.w, d[kk]);
                        }
                    }
                    *reinterpret_cast<float4 *>(p.dx + r * in + 4 * k4) = make_float4(d[0], d[1], d[2], d[3]);
                }
            __syncthreads();
            for (int item = tid; item < n_items1; item += kActorThreads) {
                const int j4 = item / per1, c4 = item - j4 * per1;
                const float *sa = sm + L.hs + 4 * j4, *sb = sm + L.xs + 4 * c4;
                float4 acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
                for (int row = 0; row < kActorThreads; ++row)
                    actor_outer(acc, *reinterpret_cast<const float4 *>(sa + row * L.HS),
                                *reinterpret_cast<const float4 *>(sb + row * L.XS));
                actor_add_tile(acc, 4 * j4, c4, kH, in, pw1, pb1, first);
            }
        }
    }
}
// partials -> dw1 | db1 | dw2 | db2 (contiguous in a partial, four outputs):
// gsm_env_conv_bwd_sum_kernel's scheme, a fixed order for a given shape
__global__ __launch_bounds__(64 * kBwdSumRows) void gsm_actor_bwd_sum_kernel(const float *__restrict__ part,
                                                                             int n_part, int P, int o_b1, int o_w2,
                                                                             int o_b2, float *__restrict__ dw1,
                                                                             float *__restrict__ db1,
                                                                             float *__restrict__ dw2,
                                                                             float *__restrict__ db2) {
    __shared__ float red[kBwdSumRows][64];
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float sum = 0.0f;
    if (c < P)
        for (int b = r; b < n_part; b += 8 * kBwdSumRows) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int bu = b + u * kBwdSumRows;
                x[u] = bu < n_part ? part[(int64_t)bu * P + c] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += x[u];
        }
    red[r][lane] = sum;
    __syncthreads();
    if (r == 0 && c < P) {
        float tot = 0.0f;
        for (int i = 0; i < kBwdSumRows; ++i) tot += red[i][lane];
        if (c < o_b1) dw1[c] = tot;
        else if (c < o_w2) db1[c - o_b1] = tot;
        else if (c < o_b2) dw2[c - o_w2] = tot;
        else db2[c - o_b2] = tot;
    }
}

int64_t actor_backward_work_floats(int in, int hidden, int nA) {
    return (int64_t)kActorBwdMaxBlocks * actor_partial_floats(in, hidden, nA);
}

template <class K>
static hipError_t actor_lds_attr(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds);
}

hipError_t launch_actor_forward(const ActorParams &p, int hidden, bool eval, hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)actor_lds(p.in, hidden, false).total;
    if (lds > (size_t)kActorLdsMax) return hipErrorInvalidValue;
    const int n_tiles = (p.R + kActorThreads - 1) / kActorThreads;
    const unsigned blocks = (unsigned)(n_tiles < kActorFwdMaxBlocks ? n_tiles : kActorFwdMaxBlocks);
    (void)hipGetLastError();
#define GSM_ACTOR_FWD(H)                                                                   \
    do {                                                                                   \
        hipError_t e = eval ? actor_lds_attr(gsm_actor_fwd_kernel<H, true>, lds)           \
                            : actor_lds_attr(gsm_actor_fwd_kernel<H, false>, lds);         \
        if (e != hipSuccess) return e;                                                     \
        if (eval) gsm_actor_fwd_kernel<H, true><<<blocks, kActorThreads, lds, s>>>(p);     \
        else gsm_actor_fwd_kernel<H, false><<<blocks, kActorThreads, lds, s>>>(p);         \
    } while (0)
    switch (hidden) {
        case 0: GSM_ACTOR_FWD(0); break;
        case 16: GSM_ACTOR_FWD(16); break;
        case 32: GSM_ACTOR_FWD(32); break;
        case 64: GSM_ACTOR_FWD(64); break;
        default: return hipErrorInvalidValue;
    }
#undef GSM_ACTOR_FWD
    return hipGetLastError();
}

hipError_t launch_actor_backward(const ActorParams &p, int hidden, float *dw1, float *db1, float *dw2, float *db2,
                                 hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)actor_lds(p.in, hidden, true).total;
    if (lds > (size_t)kActorLdsMax) return hipErrorInvalidValue;
    const int n_tiles = (p.R + kActorThreads - 1) / kActorThreads;
    const unsigned blocks = (unsigned)(n_tiles < kActorBwdMaxBlocks ? n_tiles : kActorBwdMaxBlocks);
    (void)hipGetLastError();
#define GSM_ACTOR_BWD(H)                                                          \
    do {                                                                          \
        const hipError_t e = actor_lds_attr(gsm_actor_bwd_kernel<H>, lds);        \
        if (e != hipSuccess) return e;                                            \
        gsm_actor_bwd_kernel<H><<<blocks, kActorThreads, lds, s>>>(p);            \
    } while (0)
    switch (hidden) {
        case 0: GSM_ACTOR_BWD(0); break;
        case 16: GSM_ACTOR_BWD(16); break;
        case 32: GSM_ACTOR_BWD(32); break;
        case 64: GSM_ACTOR_BWD(64); break;
        default: return hipErrorInvalidValue;
    }
#undef GSM_ACTOR_BWD
    const int P = actor_partial_floats(p.in, hidden, p.nA);
    const int o_b1 = hidden * p.in, o_w2 = o_b1 + hidden, o_b2 = o_w2 + p.nA * (hidden ? hidden : p.in);
    gsm_actor_bwd_sum_kernel<<<(unsigned)((P + 63) / 64), 64 * kBwdSumRows, 0, s>>>(p.part, (int)blocks, P, o_b1,
                                                                                   o_w2, o_b2, dw1, db1, dw2, db2);
    return hipGetLastError();
}

}  // namespace gsm
