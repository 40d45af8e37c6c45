// gsm_adam.hip — the optimizer step: the global gradient norm of a list of
// tensors, the clip coefficient and one Adam update of every tensor in two
// passes (gsm_adam_step). The contract is in include/gsm_optim.h.
//
// Mapping: a chunk is kOptChunk = 1024 consecutive elements of one tensor, an
// item four consecutive elements, one item per thread, 256 threads a workgroup,
// one chunk per workgroup at a time, a capped grid with a grid-stride loop over
// the chunks of the launch. The tensors are scattered allocations, so a launch
// gets a table of up to kOptTable of them {p, g, m, v, n, first chunk} by value
// in its kernel arguments; a workgroup finds its chunk's tensor by a search
// whose index is the same in every lane, so the table is read by scalar loads.
// A call on more tensors is several launches of either pass; chunks are
// numbered through the whole call, so the launches' partials are disjoint.
// With the tensor's pointers 16-byte aligned a whole item is one 16-byte access
// per array (a chunk starts at a multiple of 1024 elements, so the base decides);
// otherwise, and for the item the tensor ends in, the same four elements by
// scalar accesses. Either way a thread handles the same elements in the same
// order, so the bits do not depend on the path.
//
// Pass 1 (gsm_adam_norm_kernel): a thread adds the squares of its item in fp64
// (the product of two floats is exact there), the wave adds its 64 lanes (a
// shuffle tree), the workgroup its four waves through LDS, and one fp64 partial
// per chunk goes to `work`. Workgroup 0 of the call's first launch copies the
// step word + 1 into the workspace header.
// Pass 2 (gsm_adam_update_kernel): every workgroup adds all partials in one
// fixed order (opt_block_sum, the same code in every workgroup, so the same
// bits), forms norm, coef, the skip decision and the bias corrections (fp64,
// from the header's step count), then updates its chunks of p, m, v. Workgroup 0
// of the call's first launch writes stats, the status and the step word: no
// workgroup of pass 2 reads the step word. No float atomics.
#include <vector>

#include "gsm_internal.h"

namespace gsm {

constexpr int kOptThreads = 256;
constexpr int kOptChunk = 4 * kOptThreads;   // elements of a chunk: one item of four per thread
constexpr int kOptMaxBlocks = 1024;          // four workgroups per CU
constexpr int kOptHeader = 2;                // the workspace header, in doubles: [0] the step count after the call

// the 64 lanes of a wave added by a shuffle tree; lane 0 holds the sum
__device__ __forceinline__ double opt_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// The workgroup's sum of v, returned to every thread: the wave tree, then the
// waves in ascending order. red: kOptThreads / 64 doubles of LDS.
__device__ __forceinline__ double opt_block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    v = opt_wave_sum(v);
    __syncthreads();   // the readers of the previous call are done
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double tot = red[0];
#pragma unroll
    for (int w = 1; w < kOptThreads / 64; ++w) tot = tot + red[w];
    return tot;
}

// the table entry chunk c lies in: the last one whose first chunk is <= c. c is
// the same in every lane, so is the result (held in a scalar register)
__device__ __forceinline__ int opt_find(const OptTable &tab, int64_t c) {
    int k = 0;
    for (int j = 1; j < tab.n_tensors; ++j)
        if (tab.t[j].first_chunk <= c) k = j;
    return __builtin_amdgcn_readfirstlane(k);
}

__device__ __forceinline__ bool opt_aligned(const void *q) { return ((uintptr_t)q & 15) == 0; }

// four consecutive floats from e0 on: one 16-byte load when `vec` and all four
// lie inside [0, n), else a scalar load for each that does; 0.0f elsewhere
__device__ __forceinline__ void opt_load4(const float *__restrict__ src, int64_t e0, int64_t n, bool vec,
                                          float (&out)[4]) {
    if (vec && e0 + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4 *>(src + e0);
        out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = e0 + k < n ? src[e0 + k] : 0.0f;
    }
}

__device__ __forceinline__ void opt_store4(float *__restrict__ dst, int64_t e0, int64_t n, bool vec,
                                           const float (&v)[4]) {
    if (vec && e0 + 4 <= n) {
        *reinterpret_cast<float4 *>(dst + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e0 + k < n) dst[e0 + k] = v[k];
    }
}

__global__ __launch_bounds__(kOptThreads) void gsm_adam_norm_kernel(const OptTable tab, const int32_t *step,
                                                                    double *work, int lead) {
    __shared__ double red[kOptThreads / 64];
    const int tid = threadIdx.x;
    if (lead && blockIdx.x == 0 && tid == 0) reinterpret_cast<int32_t *>(work)[0] = step[0] + 1;
    double *part = work + kOptHeader;
    for (int64_t c = tab.chunk_lo + blockIdx.x; c < tab.chunk_hi; c += gridDim.x) {
        const int k = opt_find(tab, c);
        const float *g = tab.t[k].g;
        const int64_t n = tab.t[k].n;
        const int64_t e0 = (c - tab.t[k].first_chunk) * kOptChunk + (int64_t)tid * 4;
        float x[4];
        opt_load4(g, e0, n, opt_aligned(g), x);
        double s = (double)x[0] * (double)x[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) s = s + (double)x[j] * (double)x[j];
        s = opt_block_sum(s, red);
        if (tid == 0) part[c] = s;
    }
}

// b^t for t >= 0 by squaring, in fp64
__device__ __forceinline__ double opt_powi(double b, int t) {
    double r = 1.0;
    for (; t > 0; t >>= 1) {
        if (t & 1) r = r * b;
        b = b * b;
    }
    return r;
}

__global__ __launch_bounds__(kOptThreads) void gsm_adam_update_kernel(const OptTable tab, const OptScalars sc,
                                                                      const double *work, int64_t n_part,
                                                                      const float *lr, int32_t *step, float *stats,
                                                                      int32_t *status, int lead) {
    __shared__ double red[kOptThreads / 64];
    const int tid = threadIdx.x;
    const double *part = work + kOptHeader;
    // a thread adds partials tid, tid + 256, .. in ascending order, then opt_block_sum
    double s = 0.0;
    for (int64_t j = tid; j < n_part; j += kOptThreads) s = s + part[j];
    const double total = opt_block_sum(s, red);
    const float norm = (float)sqrt(total);
    const bool skip = !__builtin_isfinite(norm);
    const float ratio = sc.max_norm / (norm + 1e-6f);
    const float coef = ratio < 1.0f ? ratio : 1.0f;      // max_norm = inf: 1
    const int32_t t = reinterpret_cast<const int32_t *>(work)[0];
    if (lead && blockIdx.x == 0 && tid == 0) {
        stats[0] = norm, stats[1] = skip ? 0.0f : coef;
        stats[2] = (float)(skip ? t - 1 : t), stats[3] = skip ? 1.0f : 0.0f;
        if (skip) {
            if (status) atomicOr(status, kOptNonfinite);
        } else {
            step[0] = t;
        }
    }
    if (skip) return;
    const double bc1 = 1.0 - opt_powi(sc.beta1, t), bc2 = 1.0 - opt_powi(sc.beta2, t);
    const float step_size = (float)((double)lr[0] / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float b1 = (float)sc.beta1, b2 = (float)sc.beta2, eps = (float)sc.eps;
    const float omb1 = (float)(1.0 - sc.beta1), omb2 = (float)(1.0 - sc.beta2);
    for (int64_t c = tab.chunk_lo + blockIdx.x; c < tab.chunk_hi; c += gridDim.x) {
        const int k = opt_find(tab, c);
        float *p = tab.t[k].p, *m = tab.t[k].m, *v = tab.t[k].v;
        const float *g = tab.t[k].g;
        const int64_t n = tab.t[k].n;
        const int64_t e0 = (c - tab.t[k].first_chunk) * kOptChunk + (int64_t)tid * 4;
        if (e0 >= n) continue;
        const bool vec = opt_aligned(p) && opt_aligned(g) && opt_aligned(m) && opt_aligned(v);
        float xp[4], xg[4], xm[4], xv[4];
        opt_load4(p, e0, n, vec, xp);
        opt_load4(g, e0, n, vec, xg);
        opt_load4(m, e0, n, vec, xm);
        opt_load4(v, e0, n, vec, xv);
        // every line one correctly rounded fp32 operation at a time (-ffp-contract=off)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gc = xg[j] * coef;
            xm[j] = b1 * xm[j] + omb1 * gc;
            xv[j] = b2 * xv[j] + omb2 * (gc * gc);
            const float denom = sqrtf(xv[j]) / bc2_sqrt + eps;
            xp[j] = xp[j] - step_size * (xm[j] / denom);
        }
        opt_store4(p, e0, n, vec, xp);
        opt_store4(m, e0, n, vec, xm);
        opt_store4(v, e0, n, vec, xv);
    }
}

int64_t adam_chunks(int64_t n) { return (n + kOptChunk - 1) / kOptChunk; }

int64_t adam_work_floats(int64_t n_tensors, int64_t total_elements) {
    // a tensor of n elements has ceil(n / kOptChunk) <= n / kOptChunk + 1 chunks
    return 2 * (kOptHeader + total_elements / kOptChunk + n_tensors);
}

hipError_t launch_adam_step(float *const *p, const float *const *g, float *const *m, float *const *v,
                            const int64_t *n, int64_t n_tensors, const OptScalars &sc, const float *lr,
                            int32_t *step, float *work, float *stats, int32_t *status, hipStream_t s) {
    double *w = reinterpret_cast<double *>(work);
    // the tables of the call: tensors of no elements are left out
    std::vector<OptTable> tabs;
    int64_t chunk = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (n[i] == 0) continue;
        if (tabs.empty() || tabs.back().n_tensors == kOptTable) {
            tabs.emplace_back();
            tabs.back().n_tensors = 0, tabs.back().chunk_lo = chunk;
        }
        OptTable &tab = tabs.back();
        tab.t[tab.n_tensors++] = {p[i], g[i], m[i], v[i], n[i], chunk};
        chunk += adam_chunks(n[i]);
        tab.chunk_hi = chunk;
    }
    if (tabs.empty()) {                       // nothing to update: the header, stats and the step word all the same
        tabs.emplace_back();
        tabs.back().n_tensors = 0, tabs.back().chunk_lo = tabs.back().chunk_hi = 0;
    }
    auto blocks = [](const OptTable &tab) {
        const int64_t want = tab.chunk_hi - tab.chunk_lo;
        return (unsigned)(want < 1 ? 1 : (want < kOptMaxBlocks ? want : kOptMaxBlocks));
    };
    (void)hipGetLastError();
    for (size_t i = 0; i < tabs.size(); ++i)
        gsm_adam_norm_kernel<<<blocks(tabs[i]), kOptThreads, 0, s>>>(tabs[i], step, w, i == 0);
    for (size_t i = 0; i < tabs.size(); ++i)
        gsm_adam_update_kernel<<<blocks(tabs[i]), kOptThreads, 0, s>>>(tabs[i], sc, w, chunk, lr, step, stats,
                                                                      status, i == 0);
    return hipGetLastError();
}

}  // namespace gsm
