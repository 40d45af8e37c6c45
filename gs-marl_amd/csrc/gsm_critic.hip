// gsm_critic.hip — the critic head: features -> mean over an env's valid
// agents -> MLP on [pool | x] -> one or two values a row (gsm_critic_eval) and
// their gradients (gsm_critic_eval_bwd).
// The contract is in include/gsm.h.
//
// Mapping: a workgroup of 128 threads takes tiles of whole envs, ept =
// min(128 / n_agents, 64) envs and ept * n_agents <= 128 rows, one row per
// thread (thread t: env t / n_agents of the tile, agent t % n_agents). As in
// gsm_actor.hip the weights sit in LDS for the workgroup's life, W1 transposed to
// [2 in][hidden] (16-byte broadcast reads that feed four chains), and a tile's
// x rows are staged by coalesced 16-byte loads, a row padded by (1, 0, 0, 0);
// padded agents (i >= n_valid[b]) and the rows past the tile's envs are staged
// as zeros and never read from memory.
//
// The readout runs on per-env tasks spread over the threads: pool_b (task =
// env x four columns: the valid rows added in ascending agent order, then one
// division), then the env's prefix c_b (task = env x four hidden units: the
// chain from b1 over the pool half of W1). A row's chain continues from c_b
// over the x half, so a row's result depends on its env's rows alone, bit for
// bit, wherever the env falls in a tile, in the grid or in the batch.
//
// Backward: dv, h and then dh go through LDS; dW2|db2 = dv^T [h | 1] and
// dW1[:, in:]|db1 = dh^T [x | 1] are the actor's small GEMMs over the tile's
// rows (mlp_gemm_tile / mlp_add_tile, a 4x4 register tile per thread added to
// the workgroup's partial in `work` tile by tile, so no accumulator is held
// over the per-row part); the pool path adds s_b = sum_i dh_{b,i} (env task,
// ascending agent), dW1[:, :in] = s^T pool (a GEMM over the tile's envs) and
// dpool_b = W1[:, :in]^T s_b, whose quotient by n_b every row of the env adds
// to its dx. gsm_partial_sum_kernel adds the partials in a fixed order. No
// float atomics. The MLP pieces are gsm_mlp.h's, shared with the actor head.
#include "gsm_mlp.h"

namespace gsm {

constexpr int kCriticMaxEnvs = 64;       // envs of a tile: the n_agents <= 2 shapes, set by the LDS budget
constexpr int kCriticMaxOut = 2;
constexpr int kCriticFwdMaxBlocks = 2048;
constexpr int kCriticBwdMaxBlocks = 512;  // the size of `work`

__host__ __device__ inline int critic_envs_per_tile(int n_agents) {
    const int e = kActorThreads / n_agents;
    return e < kCriticMaxEnvs ? e : kCriticMaxEnvs;
}

// LDS, in floats; every block starts on a 16-byte boundary
struct CriticLds {
    int xs, w1, b1, w2, b2, cnt, pool, c, hs, ds, s, total;
    int XS, HS, CS;   // row strides of the x tile (and of pool), of the h tile, of c (dpool / n_b in the backward)
};

// the one place the dynamic-LDS size is formed: the kernels and the launchers call it
__host__ __device__ inline CriticLds critic_lds(int in, int kH, int ept, bool bwd) {
    CriticLds L;
    L.XS = in + 4;
    L.HS = kH + 4;
    L.CS = (kH > in ? kH : in) + 4;   // the pad spreads the envs' rows over the banks
    int o = 0;
    L.xs = o, o += kActorThreads * L.XS;
    L.w1 = o, o += 2 * in * kH;
    L.b1 = o, o += kH;
    L.w2 = o, o += kCriticMaxOut * kH;
    L.b2 = o, o += 4;
    L.cnt = o, o += (ept + 3) & ~3;
    L.pool = o, o += ept * L.XS;
    L.c = o, o += ept * L.CS;
    L.hs = o, o += bwd ? kActorThreads * L.HS : 0;
    L.ds = o, o += bwd ? kActorThreads * 4 : 0;
    L.s = o, o += bwd ? ept * kH : 0;
    L.total = o;
    return L;
}

// the weights into LDS: W1^T [2 in][kH], w2 / b2 padded to two rows
template <int kH>
__device__ __forceinline__ void critic_load_weights(const CriticParams &p, const CriticLds &L, float *sm) {
    mlp_load_weights<kH, kCriticMaxOut>(p.w1, p.b1, p.w2, p.b2, 2 * p.in, kH, p.nO, sm + L.w1, sm + L.b1, sm + L.w2,
                                        sm + L.b2);
}

// The tile of envs [env0, env0 + ept): the clamped agent counts, the x rows
// (zeros for padded agents and past the tile's envs, the pad (1, 0, 0, 0)),
// pool and the prefix c. Ends with a barrier; starts with the one that lets
// the previous tile's readers finish.
template <int kH>
__device__ __forceinline__ void critic_load_tile(const CriticParams &p, const CriticLds &L, float *sm, int ept,
                                                 int64_t env0) {
    const int tid = threadIdx.x, N = p.n_agents, in = p.in, n4 = in >> 2;
    int *cnt = reinterpret_cast<int *>(sm + L.cnt);
    __syncthreads();
    if (tid < ept) {
        int n = 0;
        if (env0 + tid < p.n_envs) {
            n = p.n_valid ? p.n_valid[env0 + tid] : N;
            if (n < 0 || n > N) {
                if (p.status) atomicOr(p.status, GSM_CRITIC_BAD_COUNT);
                n = n < 0 ? 0 : N;
            }
        }
        cnt[tid] = n;
    }
    __syncthreads();
    mlp_load_tile(p.x, p.x_stride, env0 * N, n4, sm + L.xs, L.XS, [&](int row) {
        const int e = row / N, a = row - e * N;
        return e < ept && a < cnt[e];
    });
    __syncthreads();
    // pool_b = (x_{b,0} + x_{b,1} + ..) / n_b over the valid agents, ascending
    for (int t = tid; t < ept * n4; t += kActorThreads) {
        const int e = t / n4, c4 = t - e * n4, n = cnt[e];
        const float *xe = sm + L.xs + e * N * L.XS + 4 * c4;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int i = 0; i < n; ++i) {
            const float4 v = *reinterpret_cast<const float4 *>(xe + i * L.XS);
            if (i == 0) a = v;
            else a.x = a.x + v.x, a.y = a.y + v.y, a.z = a.z + v.z, a.w = a.w + v.w;
        }
        if (n > 0) {
            const float d = (float)n;
            a.x = a.x / d, a.y = a.y / d, a.z = a.z / d, a.w = a.w / d;
        }
        *reinterpret_cast<float4 *>(sm + L.pool + e * L.XS + 4 * c4) = a;
    }
    __syncthreads();
    // c_b[h] = the chain from b1[h] over the pool half of W1, once per env
    for (int t = tid; t < ept * (kH / 4); t += kActorThreads) {
        const int e = t / (kH / 4), j4 = t - e * (kH / 4);
        const float *pe = sm + L.pool + e * L.XS;
        float4 a = *reinterpret_cast<const float4 *>(sm + L.b1 + 4 * j4);
#pragma unroll 4
        for (int k = 0; k < in; ++k) {
            const float4 w = *reinterpret_cast<const float4 *>(sm + L.w1 + k * kH + 4 * j4);
            const float pk = pe[k];
            a.x = fmaf(w.x, pk, a.x), a.y = fmaf(w.y, pk, a.y);
            a.z = fmaf(w.z, pk, a.z), a.w = fmaf(w.w, pk, a.w);
        }
        *reinterpret_cast<float4 *>(sm + L.c + e * L.CS + 4 * j4) = a;
    }
    __syncthreads();
}

// h of one row: the chain continued from its env's prefix cb over the x half
// of W1 (the actor's loop), then relu
template <int kH>
__device__ __forceinline__ void critic_hidden(const float *__restrict__ xr, const float *__restrict__ cb,
                                              const float *__restrict__ sm, const CriticLds &L, int in,
                                              float (&h)[kH]) {
#pragma unroll
    for (int j4 = 0; j4 < kH / 4; ++j4) {
        const float4 c = *reinterpret_cast<const float4 *>(cb + 4 * j4);
        h[4 * j4] = c.x, h[4 * j4 + 1] = c.y, h[4 * j4 + 2] = c.z, h[4 * j4 + 3] = c.w;
    }
    mlp_hidden<kH>(xr, sm + L.w1 + in * kH, in >> 2, h);
}

template <int kH>
__global__ __launch_bounds__(kActorThreads) void gsm_critic_fwd_kernel(const CriticParams p) {
    extern __shared__ __align__(16) float actor_sm[];
    float *sm = actor_sm;
    const int N = p.n_agents, ept = critic_envs_per_tile(N);
    const CriticLds L = critic_lds(p.in, kH, ept, false);
    const int tid = threadIdx.x, e = tid / N, a = tid - e * N;
    const int *cnt = reinterpret_cast<const int *>(sm + L.cnt);
    critic_load_weights<kH>(p, L, sm);
    float mean[kCriticMaxOut], sd[kCriticMaxOut];
#pragma unroll
    for (int o = 0; o < kCriticMaxOut; ++o) {
        const bool on = p.denorm && o < p.nO;
        mean[o] = on ? p.denorm[2 * o] : 0.0f;
        sd[o] = on ? p.denorm[2 * o + 1] : 1.0f;
    }
    const int64_t n_tiles = (p.n_envs + ept - 1) / ept;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t env0 = tile * ept;
        critic_load_tile<kH>(p, L, sm, ept, env0);
        if (e >= ept || env0 + e >= p.n_envs) continue;   // no barrier below
        float h[kH];
        critic_hidden<kH>(sm + L.xs + tid * L.XS, sm + L.c + e * L.CS, sm, L, p.in, h);
        float v[kCriticMaxOut];
        mlp_output<kH, kCriticMaxOut>(sm + L.w2, sm + L.b2, h, v);
        const bool valid = a < cnt[e];
        const int64_t r = (env0 + e) * N + a;
        bool fin = true;
#pragma unroll
        for (int o = 0; o < kCriticMaxOut; ++o)
            if (o < p.nO) {
                fin = fin && __builtin_isfinite(v[o]);
                float out = v[o];
                if (p.denorm) {
                    out = out * sd[o];
                    out = out + mean[o];
                }
                p.values[(int64_t)o * p.R + r] = valid ? out : 0.0f;
            }
        if (valid && !fin && p.status) atomicOr(p.status, GSM_CRITIC_NONFINITE);
    }
}

// a partial: dw1 [kH][2 in], db1 [kH], dw2 [n_out][kH], db2 [n_out]
__host__ __device__ inline int critic_partial_floats(int in, int kH, int nO) {
    return kH * 2 * in + kH + nO * kH + nO;
}

template <int kH>
__global__ __launch_bounds__(kActorThreads) void gsm_critic_bwd_kernel(const CriticParams p) {
    extern __shared__ __align__(16) float actor_sm[];
    float *sm = actor_sm;
    const int N = p.n_agents, ept = critic_envs_per_tile(N);
    const CriticLds L = critic_lds(p.in, kH, ept, true);
    const int tid = threadIdx.x, in = p.in, nO = p.nO, n4 = in >> 2;
    const int e = tid / N, a = tid - e * N;
    const int *cnt = reinterpret_cast<const int *>(sm + L.cnt);
    critic_load_weights<kH>(p, L, sm);
    // this thread's tiles of the products: c4 of dv^T [h | 1]; (j4, c4) of dh^T [x | 1] and of s^T pool
    const int per2 = kH / 4 + 1;
    const int per1 = n4 + 1, n_items1 = (kH / 4) * per1, n_items0 = (kH / 4) * n4;
    float *part = p.part + (int64_t)blockIdx.x * critic_partial_floats(in, kH, nO);
    float *pw1 = part, *pb1 = pw1 + kH * 2 * in, *pw2 = pb1 + kH, *pb2 = pw2 + nO * kH;
    const int64_t n_tiles = (p.n_envs + ept - 1) / ept;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t env0 = tile * ept;
        critic_load_tile<kH>(p, L, sm, ept, env0);
        const bool active = e < ept && env0 + e < p.n_envs;
        const bool valid = active && a < cnt[e];
        const int64_t r = (env0 + e) * N + a;
        float h[kH];
        critic_hidden<kH>(sm + L.xs + tid * L.XS, sm + L.c + (active ? e : 0) * L.CS, sm, L, in, h);
        float dv[kCriticMaxOut];
#pragma unroll
        for (int o = 0; o < kCriticMaxOut; ++o) dv[o] = (valid && o < nO) ? p.g[(int64_t)o * p.R + r] : 0.0f;
        *reinterpret_cast<float4 *>(sm + L.ds + tid * 4) = make_float4(dv[0], dv[1], 0.0f, 0.0f);
        float *hr = sm + L.hs + tid * L.HS;
        // a row that is no valid agent's takes no part: h = 0, dh = 0
        if (!valid) {
#pragma unroll
            for (int j = 0; j < kH; ++j) h[j] = 0.0f;
        }
        mlp_store_row<kH, true>(hr, h);
        mlp_hidden_grad<kH, kCriticMaxOut>(sm + L.w2, dv, nO, h);
        __syncthreads();   // dv and h of every row are in LDS
        const bool first = tile == (int64_t)blockIdx.x;
        if (tid < per2) {
            float4 acc[4];
            mlp_gemm_tile(acc, sm + L.ds, 4, sm + L.hs + 4 * tid, L.HS, kActorThreads);
            mlp_add_tile(acc, 0, tid, nO, kH, pw2, pb2, first);
        }
        __syncthreads();   // h has been read: dh takes its place
        mlp_store_row<kH, false>(hr, h);
        __syncthreads();
        // s_b = dh_{b,0} + dh_{b,1} + .. over the env's valid agents, ascending
        for (int t = tid; t < ept * (kH / 4); t += kActorThreads) {
            const int eb = t / (kH / 4), j4 = t - eb * (kH / 4), n = cnt[eb];
            const float *de = sm + L.hs + eb * N * L.HS + 4 * j4;
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int i = 0; i < n; ++i) {
                const float4 v = *reinterpret_cast<const float4 *>(de + i * L.HS);
                if (i == 0) s = v;
                else s.x = s.x + v.x, s.y = s.y + v.y, s.z = s.z + v.z, s.w = s.w + v.w;
            }
            *reinterpret_cast<float4 *>(sm + L.s + eb * kH + 4 * j4) = s;
        }
        __syncthreads();
        // dpool_b = W1[:, :in]^T s_b; what every row of the env adds to its dx, dpool_b / n_b, over c
        if (p.dx)
            for (int t = tid; t < ept * n4; t += kActorThreads) {
                const int eb = t / n4, k4 = t - eb * n4, n = cnt[eb];
                const float4 d = mlp_dx_group<kH>(sm + L.w1 + 4 * k4 * kH, sm + L.s + eb * kH);
                const float dn = n > 0 ? (float)n : 1.0f;
                *reinterpret_cast<float4 *>(sm + L.c + eb * L.CS + 4 * k4) =
                    make_float4(d.x / dn, d.y / dn, d.z / dn, d.w / dn);
            }
        __syncthreads();
        // dx = W1[:, in:]^T dh + dpool / n_b, the row's dh read back from LDS (the thread's own
        // stores) so that this loop is not unrolled over h's registers; a padded row gets zeros
        if (p.dx && active)
            for (int k4 = 0; k4 < n4; ++k4) {
                const float4 d = mlp_dx_group<kH>(sm + L.w1 + (in + 4 * k4) * kH, hr);
                const float4 q = *reinterpret_cast<const float4 *>(sm + L.c + e * L.CS + 4 * k4);
                float4 out = make_float4(d.x + q.x, d.y + q.y, d.z + q.z, d.w + q.w);
                if (!valid) out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                *reinterpret_cast<float4 *>(p.dx + r * in + 4 * k4) = out;
            }
        // dW1[:, in:] | db1 = dh^T [x | 1] over the tile's rows, into columns in.. of the partial's rows
        for (int item = tid; item < n_items1; item += kActorThreads) {
            const int j4 = item / per1, c4 = item - j4 * per1;
            float4 acc[4];
            mlp_gemm_tile(acc, sm + L.hs + 4 * j4, L.HS, sm + L.xs + 4 * c4, L.XS, kActorThreads);
            mlp_add_tile(acc, 4 * j4, c4 < n4 ? c4 : 2 * n4, kH, 2 * in, pw1 + in, pb1, first);
        }
        // dW1[:, :in] = s^T pool over the tile's envs
        for (int item = tid; item < n_items0; item += kActorThreads) {
            const int j4 = item / n4, c4 = item - j4 * n4;
            float4 acc[4];
            mlp_gemm_tile(acc, sm + L.s + 4 * j4, kH, sm + L.pool + 4 * c4, L.XS, ept);
            mlp_add_tile(acc, 4 * j4, c4, kH, 2 * in, pw1, pb1, first);
        }
    }
}

int64_t critic_backward_work_floats(int in, int hidden, int nO) {
    return (int64_t)kCriticBwdMaxBlocks * critic_partial_floats(in, hidden, nO);
}

size_t critic_lds_bytes(int in, int hidden, int n_agents, bool bwd) {
    return sizeof(float) * (size_t)critic_lds(in, hidden, critic_envs_per_tile(n_agents), bwd).total;
}

static unsigned critic_blocks(const CriticParams &p, int cap) {
    const int ept = critic_envs_per_tile(p.n_agents);
    const int64_t n_tiles = (p.n_envs + ept - 1) / ept;
    return (unsigned)(n_tiles < cap ? n_tiles : cap);
}

hipError_t launch_critic_forward(const CriticParams &p, int hidden, hipStream_t s) {
    const size_t lds = critic_lds_bytes(p.in, hidden, p.n_agents, false);
    if (lds > (size_t)kActorLdsMax) return hipErrorInvalidValue;
    const unsigned blocks = critic_blocks(p, kCriticFwdMaxBlocks);
    (void)hipGetLastError();
    const hipError_t e = mlp_dispatch_hidden<false>(hidden, [&](auto H) {
        return mlp_launch(gsm_critic_fwd_kernel<decltype(H)::value>, blocks, lds, p, s);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_critic_backward(const CriticParams &p, int hidden, float *dw1, float *db1, float *dw2, float *db2,
                                  hipStream_t s) {
    const size_t lds = critic_lds_bytes(p.in, hidden, p.n_agents, true);
    if (lds > (size_t)kActorLdsMax) return hipErrorInvalidValue;
    const unsigned blocks = critic_blocks(p, kCriticBwdMaxBlocks);
    (void)hipGetLastError();
    const hipError_t e = mlp_dispatch_hidden<false>(hidden, [&](auto H) {
        return mlp_launch(gsm_critic_bwd_kernel<decltype(H)::value>, blocks, lds, p, s);
    });
    if (e != hipSuccess) return e;
    // a partial is dw1 | db1 | dw2 | db2, contiguous
    launch_partial_sum(p.part, (int)blocks, {{hidden * 2 * p.in, dw1}, {hidden, db1}, {p.nO * hidden, dw2}, {p.nO, db2}},
                       s);
    return hipGetLastError();
}

}  // namespace gsm
