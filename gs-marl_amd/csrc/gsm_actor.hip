// gsm_actor.hip — the actor head: features -> MLP -> categorical
// distribution -> Philox-sampled action, log-probability, entropy
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
// the per-row part); gsm_partial_sum_kernel (gsm_gnn.hip) adds the partials in
// a fixed order. No float atomics. The MLP pieces are gsm_mlp.h's, shared with
// the critic head.
#include "gsm_mlp.h"
#include "gsm_philox.h"

namespace gsm {

constexpr int kActorMaxActions = 8;
constexpr int kActorFwdMaxBlocks = 2048;
constexpr int kActorBwdMaxBlocks = 512;  // two per CU: the size of `work`

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

// the weights into LDS: W1^T [in][kH], w2 / b2 padded to eight rows
template <int kH>
__device__ __forceinline__ void actor_load_weights(const ActorParams &p, const ActorLds &L, float *sm) {
    mlp_load_weights<kH, kActorMaxActions>(p.w1, p.b1, p.w2, p.b2, p.in, L.KW, p.nA, sm + L.w1, sm + L.b1, sm + L.w2,
                                           sm + L.b2);
}

// rows [row0, row0 + 128) of x into the tile, zeros past R
__device__ __forceinline__ void actor_load_tile(const ActorParams &p, const ActorLds &L, float *sm, int64_t row0) {
    mlp_load_tile(p.x, p.x_stride, row0, p.in >> 2, sm + L.xs, L.XS, [&](int row) { return row0 + row < p.R; });
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
        mlp_hidden<kH>(xr, sm + L.w1, n4, h);
        mlp_output<kH, kActorMaxActions>(sm + L.w2, sm + L.b2, h, o.l);
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
            mlp_store_row<kH, true>(sm + L.hs + tid * L.HS, h);
            mlp_hidden_grad<kH, kActorMaxActions>(sm + L.w2, dl, nA, h);
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
            mlp_gemm_tile(acc, sa, 8, sb, SB, kActorThreads);
            mlp_add_tile(acc, 4 * a4, c4, nA, kH ? kH : in, pw2, pb2, first);
        }
        if constexpr (kH > 0) {
            __syncthreads();   // h has been read: dh takes its place
            float *hr = sm + L.hs + tid * L.HS;
            mlp_store_row<kH, false>(hr, h);
            // dx = W1^T dh, the row's dh read back from LDS (the thread's own stores) so that
            // this loop is not unrolled over h's registers
            if (p.dx && r < p.R)
                for (int k4 = 0; k4 < n4; ++k4)
                    *reinterpret_cast<float4 *>(p.dx + r * in + 4 * k4) =
                        mlp_dx_group<kH>(sm + L.w1 + 4 * k4 * kH, hr);
            __syncthreads();
            for (int item = tid; item < n_items1; item += kActorThreads) {
                const int j4 = item / per1, c4 = item - j4 * per1;
                const float *sa = sm + L.hs + 4 * j4, *sb = sm + L.xs + 4 * c4;
                float4 acc[4];
                mlp_gemm_tile(acc, sa, L.HS, sb, L.XS, kActorThreads);
                mlp_add_tile(acc, 4 * j4, c4, kH, in, pw1, pb1, first);
            }
        }
    }
}

int64_t actor_backward_work_floats(int in, int hidden, int nA) {
    return (int64_t)kActorBwdMaxBlocks * actor_partial_floats(in, hidden, nA);
}

hipError_t launch_actor_forward(const ActorParams &p, int hidden, bool eval, hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)actor_lds(p.in, hidden, false).total;
    if (lds > (size_t)kActorLdsMax) return hipErrorInvalidValue;
    const int n_tiles = (p.R + kActorThreads - 1) / kActorThreads;
    const unsigned blocks = (unsigned)(n_tiles < kActorFwdMaxBlocks ? n_tiles : kActorFwdMaxBlocks);
    (void)hipGetLastError();
    const hipError_t e = mlp_dispatch_hidden<true>(hidden, [&](auto H) {
        constexpr int kH = decltype(H)::value;
        return eval ? mlp_launch(gsm_actor_fwd_kernel<kH, true>, blocks, lds, p, s)
                    : mlp_launch(gsm_actor_fwd_kernel<kH, false>, blocks, lds, p, s);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_actor_backward(const ActorParams &p, int hidden, float *dw1, float *db1, float *dw2, float *db2,
                                 hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)actor_lds(p.in, hidden, true).total;
    if (lds > (size_t)kActorLdsMax) return hipErrorInvalidValue;
    const int n_tiles = (p.R + kActorThreads - 1) / kActorThreads;
    const unsigned blocks = (unsigned)(n_tiles < kActorBwdMaxBlocks ? n_tiles : kActorBwdMaxBlocks);
    (void)hipGetLastError();
    const hipError_t e = mlp_dispatch_hidden<true>(hidden, [&](auto H) {
        return mlp_launch(gsm_actor_bwd_kernel<decltype(H)::value>, blocks, lds, p, s);
    });
    if (e != hipSuccess) return e;
    // a partial is dw1 | db1 | dw2 | db2, contiguous
    launch_partial_sum(p.part, (int)blocks, {{hidden * p.in, dw1},
                                            {hidden, db1},
                                            {p.nA * (hidden ? hidden : p.in), dw2},
                                            {p.nA, db2}}, s);
    return hipGetLastError();
}

}  // namespace gsm
