// gsm_gnn.hip — graph-attention message passing over the env graph
// (the GNN encoder that consumes node_feat /
// edge_index; reference: gsmarl/algorithms, SOURCES.txt:8, torch-geometric
// 2.3.1 requirements.txt:119 — the InforMARL lineage uses PyG TransformerConv).
//
// The dense projections (q = W_q x, k = W_k x, v = W_v x, skip = W_r x) are
// GEMMs and stay on hipBLASLt (torch.matmul), except for the first layer on an
// env-form graph, whose K = 7 projections gsm_env_conv (below) forms on chip
// together with the attention. This kernel is the part that is
// a gather / segmented softmax / scatter over the graph, for target node i with
// source neighbours j (CSR rows: row_ptr / col), per head h:
//
//   e_ij   = w_ij * w_e[h]                    (edge feature, edge_dim = 1)
//   s_ij   = scale * <q_i[h], k_j[h] + e_ij>
//   a_ij   = softmax_j(s_ij)                  (over the row; empty row -> 0)
//   out_i[h] = sum_j a_ij (v_j[h] + e_ij)  (+ skip_i[h])
//
// Layout: q, k, v, skip, out are [n_nodes][H*C] f32 (head-major channels).
// Mapping: four channels per lane (16-byte gathers of the k_j / v_j rows)
// when the heads allow, so a node takes pow2 >= H*C/4 lanes and a wave works
// on 64/that nodes at once (memory-level parallelism for the dependent
// row_ptr -> col -> k/v loads); a head's lanes reduce the score with xor
// shuffles; an online softmax keeps (max, denominator, accumulator) in
// registers while the row's edges stream through (the next edge's index one
// iteration ahead), so every k_j / v_j row is read once per edge.
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "gsm.h"
#include "gsm_device.h"

namespace gsm {

template <int kVec>
struct VecT;
template <>
struct VecT<1> {
    using T = float;
    static __device__ __forceinline__ float get(const T &x, int) { return x; }
    static __device__ __forceinline__ void set(T &x, int, float v) { x = v; }
};
template <>
struct VecT<4> {
    using T = float4;
    static __device__ __forceinline__ float get(const T &x, int i) {
        return i == 0 ? x.x : (i == 1 ? x.y : (i == 2 ? x.z : x.w));
    }
    static __device__ __forceinline__ void set(T &x, int i, float v) {
        if (i == 0) x.x = v;
        else if (i == 1) x.y = v;
        else if (i == 2) x.z = v;
        else x.w = v;
    }
};

// kLP lanes per node, kVec consecutive channels per lane (a lane's channels
// belong to one head: C % kVec == 0); 64 / kLP nodes per wave.
template <int kLP, int kVec>
__global__ __launch_bounds__(256) void gsm_attn_aggregate_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
    const float *__restrict__ edge_w, const float *__restrict__ w_e, const int64_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const float *__restrict__ skip, int64_t n_nodes, int HC, int C,
    float scale, float *__restrict__ out, float *__restrict__ lse) {
    using V = VecT<kVec>;
    using T = typename V::T;
    constexpr int kNPW = kWave / kLP;                       // nodes per wave
    const int lane = threadIdx.x & 63;
    const int sub = lane / kLP, ch = (lane % kLP) * kVec;
    const int64_t node = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kNPW + sub;
    const bool live = node < n_nodes && ch < HC;
    const int64_t nd = node < n_nodes ? node : 0;
    const int lanes_per_head = C / kVec;                    // power of two
    T qi, we, acc;
    for (int i = 0; i < kVec; ++i) {
        V::set(qi, i, 0.0f);
        V::set(we, i, 0.0f);
        V::set(acc, i, 0.0f);
    }
    if (live) {
        qi = *(const T *)(q + nd * HC + ch);
        if (w_e) we = *(const T *)(w_e + ch);
    }
    const int64_t r0 = node < n_nodes ? row_ptr[nd] : 0, r1 = node < n_nodes ? row_ptr[nd + 1] : 0;
    const int deg = (int)(r1 - r0);
    int wdeg = deg;                                          // the wave runs its longest row
#pragma unroll
    for (int o = kLP; o < kWave; o <<= 1) wdeg = max(wdeg, __shfl_xor(wdeg, o));
    float mx = -__builtin_inff(), den = 0.0f;
    // next edge's source and weight fetched one iteration ahead
    int64_t jn = (live && deg > 0) ? col[r0] : 0;
    float wn = (live && deg > 0 && edge_w) ? edge_w[r0] : 0.0f;
    for (int t = 0; t < wdeg; ++t) {
        const bool on = live && t < deg;
        const int64_t j = jn;
        const float w = wn;
        if (live && t + 1 < deg) {
            jn = col[r0 + t + 1];
            if (edge_w) wn = edge_w[r0 + t + 1];
        }
        T kj, vj;
        for (int i = 0; i < kVec; ++i) {
            V::set(kj, i, 0.0f);
            V::set(vj, i, 0.0f);
        }
        if (on) {
            kj = *(const T *)(k + j * HC + ch);
            vj = *(const T *)(v + j * HC + ch);
        }
        float sc = 0.0f;
#pragma unroll
        for (int i = 0; i < kVec; ++i) sc += V::get(qi, i) * (V::get(kj, i) + w * V::get(we, i));
#pragma unroll
        for (int o = 1; o < kLP; o <<= 1)
            if (o < lanes_per_head) sc += __shfl_xor(sc, o);   // sum over the head's lanes
        sc *= scale;
        if (on) {
            const float m2 = fmaxf(mx, sc);
            const float a = __expf(mx - m2), b = __expf(sc - m2);
            den = den * a + b;
#pragma unroll
            for (int i = 0; i < kVec; ++i)
                V::set(acc, i, V::get(acc, i) * a + b * (V::get(vj, i) + w * V::get(we, i)));
            mx = m2;
        }
    }
    if (live) {
        const float inv = den > 0.0f ? 1.0f / den : 0.0f;
        T r;
        T sk;
        if (skip) sk = *(const T *)(skip + nd * HC + ch);
#pragma unroll
        for (int i = 0; i < kVec; ++i)
            V::set(r, i, V::get(acc, i) * inv + (skip ? V::get(sk, i) : 0.0f));
        *(T *)(out + nd * HC + ch) = r;
        // softmax statistics for the backward: each head's first lane; an
        // empty row stores a finite value that is never read
        if (lse && ch % C == 0) lse[nd * (HC / C) + ch / C] = den > 0.0f ? mx + logf(den) : 0.0f;
    }
}

// The lanes of a node (or output row), for the four launchers below: four
// channels per lane (16-byte accesses) when every head spans whole lanes and
// the rows the launcher names are 16-byte aligned, one channel per lane
// otherwise; lp = the power of two >= HC / vec lanes. ok: a node fits a wave.
struct Lanes {
    int lp, vec;
    bool ok;
};

static bool aligned16(std::initializer_list<const void *> ptrs) {
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p;
    return bits % 16 == 0;
}

static Lanes select_lanes(int HC, int C, bool aligned) {
    const int vec = C % 4 == 0 && HC % 4 == 0 && aligned ? 4 : 1;
    int lp = 1;
    while (lp * vec < HC) lp <<= 1;
    return {lp, vec, lp <= kWave};
}

// f(integral_constant LP, integral_constant VEC) for the 12 legal pairs
template <class F>
static hipError_t dispatch_lanes(const Lanes &l, const F &f) {
#define GSM_LANES(LP, VEC) \
    case LP: f(std::integral_constant<int, LP>{}, std::integral_constant<int, VEC>{}); return hipSuccess
    if (l.vec == 4) {
        switch (l.lp) {
            GSM_LANES(1, 4);
            GSM_LANES(2, 4);
            GSM_LANES(4, 4);
            GSM_LANES(8, 4);
            GSM_LANES(16, 4);
        }
    } else {
        switch (l.lp) {
            GSM_LANES(1, 1);
            GSM_LANES(2, 1);
            GSM_LANES(4, 1);
            GSM_LANES(8, 1);
            GSM_LANES(16, 1);
            GSM_LANES(32, 1);
            GSM_LANES(64, 1);
        }
    }
#undef GSM_LANES
    return hipErrorInvalidValue;
}

hipError_t launch_attn_aggregate(const float *q, const float *k, const float *v, const float *edge_w,
                                 const float *w_e, const int64_t *row_ptr, const int32_t *col,
                                 const float *skip, int64_t n_nodes, int HC, int C, float scale, float *out,
                                 float *lse, hipStream_t s) {
    const Lanes l = select_lanes(HC, C, aligned16({q, k, v, out, skip, w_e}));
    if (!l.ok) return hipErrorInvalidValue;
    const int npw = kWave / l.lp;
    const int64_t waves = (n_nodes + npw - 1) / npw;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    (void)hipGetLastError();
    const hipError_t e = dispatch_lanes(l, [&](auto LP, auto VEC) {
        gsm_attn_aggregate_kernel<decltype(LP)::value, decltype(VEC)::value><<<blocks, 256, 0, s>>>(
            q, k, v, edge_w, w_e, row_ptr, col, skip, n_nodes, HC, C, scale, out, lse);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

// ---------------------------------------------------------------------------
// Backward. With m_ij = v_j + e_ij, g_i the upstream gradient of out_i:
//
//   D_i[h]   = <g_i[h], out_i[h] - skip_i[h]>       (= sum_j a_ij <g_i[h], m_ij[h]>)
//   ds_ij[h] = a_ij[h] * (<g_i[h], m_ij[h]> - D_i[h])
//            = a_ij[h] * <g_i[h], m_ij[h] - (out_i[h] - skip_i[h])>   (the form evaluated)
//   dq_i[h]  = scale * sum_j ds_ij[h] (k_j[h] + e_ij[h])
//   dk_j[h]  = scale * sum_{i: j in row i} ds_ij[h] q_i[h]
//   dv_j[h]  =         sum_{i: j in row i} a_ij[h]  g_i[h]
//   de_ij[c] = scale * ds_ij[h(c)] q_i[c] + a_ij[h(c)] g_i[c]
//   dw_e[c]  = sum_ij w_ij de_ij[c],   dedge_w_ij = sum_c de_ij[c] w_e[c]
//
// Two gather kernels and no float atomics, so every output is bitwise
// reproducible. The target kernel walks the CSR rows exactly as the forward
// does (same lanes-per-node mapping, one-edge-ahead index prefetch), rebuilds
// a_ij = exp(s_ij - lse_i) from the saved statistics, keeps dq_i in registers
// and stores a_ij, ds_ij per (entry, head). The source kernel walks the
// transposed lists (entries grouped by source) and sums dk_j, dv_j in
// registers from those two arrays and the q / g rows of the entries' targets.
// dw_e regroups to one [HC] row per node, scale*q_i*U_i + g_i*A_i with
// U_i = sum_j w_ij ds_ij and A_i = sum_j w_ij a_ij; a block sums the rows of
// its nodes in a fixed order (registers across its node groups, then LDS) to
// one partial, and a one-block launch sums the partials in index order.

// target-kernel grid cap = dw_e partial rows: 5 blocks (its occupancy at 93
// VGPRs) on each of the 256 CUs, so every block is resident from the start and
// the count, hence the summation order, is the same on every device
constexpr int kBwdMaxBlocks = 1280;
constexpr int kBwdSumRows = 16;       // row groups of the dw_e partial sum

template <int kLP, int kVec>
__global__ __launch_bounds__(256) void gsm_attn_bwd_target_kernel(
    const float *__restrict__ g, const float *__restrict__ q, const float *__restrict__ k,
    const float *__restrict__ v, const float *__restrict__ edge_w, const float *__restrict__ w_e,
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const float *__restrict__ out,
    const float *__restrict__ skip, const float *__restrict__ lse, int64_t n_nodes, int64_t n_groups, int HC,
    int C, float scale, float *__restrict__ wa, float *__restrict__ wds, float *__restrict__ part,
    float *__restrict__ dq, float *__restrict__ dedge_w) {
    using V = VecT<kVec>;
    using T = typename V::T;
    constexpr int kNPW = kWave / kLP;                       // nodes per wave
    __shared__ float red[256 * kVec];
    const int lane = threadIdx.x & 63;
    const int sub = lane / kLP, ch = (lane % kLP) * kVec;
    const int lanes_per_head = C / kVec;                    // power of two
    const int H = HC / C, head = ch < HC ? ch / C : 0;
    T we, dwe;
    for (int i = 0; i < kVec; ++i) {
        V::set(we, i, 0.0f);
        V::set(dwe, i, 0.0f);
    }
    if (ch < HC && w_e) we = *(const T *)(w_e + ch);
    for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int64_t node = (grp * 4 + (threadIdx.x >> 6)) * kNPW + sub;
        const bool live = node < n_nodes && ch < HC;
        const int64_t nd = node < n_nodes ? node : 0;
        T qi, gi, acc;
        for (int i = 0; i < kVec; ++i) {
            V::set(qi, i, 0.0f);
            V::set(gi, i, 0.0f);
            V::set(acc, i, 0.0f);
        }
        // gm_ij - D_i = <g_i, m_ij - (out_i - skip_i)>, formed per channel before the
        // dot product: where one entry dominates the row, m_ij is out_i - skip_i
        // to a few bits, the difference is small and so is its rounding, which dq
        // multiplies by k_j; subtracting two separately rounded dot products
        // would leave their full rounding there
        T om;
        for (int i = 0; i < kVec; ++i) V::set(om, i, 0.0f);
        float ls = 0.0f;
        if (live) {
            qi = *(const T *)(q + nd * HC + ch);
            gi = *(const T *)(g + nd * HC + ch);
            om = *(const T *)(out + nd * HC + ch);
            if (skip) {
                const T sk = *(const T *)(skip + nd * HC + ch);
                for (int i = 0; i < kVec; ++i) V::set(om, i, V::get(om, i) - V::get(sk, i));
            }
            ls = lse[nd * H + head];
        }
        // this lane's share of <q_i, w_e> and <g_i, w_e> (dedge_w)
        float pq = 0.0f, pg = 0.0f;
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            pq += V::get(qi, i) * V::get(we, i);
            pg += V::get(gi, i) * V::get(we, i);
        }
        const int64_t r0 = node < n_nodes ? row_ptr[nd] : 0, r1 = node < n_nodes ? row_ptr[nd + 1] : 0;
        const int deg = (int)(r1 - r0);
        int wdeg = deg;                                      // the wave runs its longest row
#pragma unroll
        for (int o = kLP; o < kWave; o <<= 1) wdeg = max(wdeg, __shfl_xor(wdeg, o));
        float U = 0.0f, A = 0.0f;
        int64_t jn = (live && deg > 0) ? col[r0] : 0;
        float wn = (live && deg > 0 && edge_w) ? edge_w[r0] : 0.0f;
        for (int t = 0; t < wdeg; ++t) {
            const bool on = live && t < deg;
            const int64_t j = jn;
            const float w = wn;
            if (live && t + 1 < deg) {
                jn = col[r0 + t + 1];
                if (edge_w) wn = edge_w[r0 + t + 1];
            }
            T kj, vj;
            for (int i = 0; i < kVec; ++i) {
                V::set(kj, i, 0.0f);
                V::set(vj, i, 0.0f);
            }
            if (on) {
                kj = *(const T *)(k + j * HC + ch);
                vj = *(const T *)(v + j * HC + ch);
            }
            float sc = 0.0f, gd = 0.0f;                      // gd = gm_ij - D_i
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                sc += V::get(qi, i) * (V::get(kj, i) + w * V::get(we, i));
                gd += V::get(gi, i) * ((V::get(vj, i) + w * V::get(we, i)) - V::get(om, i));
            }
#pragma unroll
            for (int o = 1; o < kLP; o <<= 1)
                if (o < lanes_per_head) {
                    sc += __shfl_xor(sc, o);
                    gd += __shfl_xor(gd, o);
                }
            sc *= scale;
            const float a = on ? __expf(sc - ls) : 0.0f;
            const float ds = a * gd;
#pragma unroll
            for (int i = 0; i < kVec; ++i)
                V::set(acc, i, V::get(acc, i) + ds * (V::get(kj, i) + w * V::get(we, i)));
            U += w * ds;
            A += w * a;
            if (on && ch % C == 0) {
                wa[(r0 + t) * H + head] = a;
                wds[(r0 + t) * H + head] = ds;
            }
            if (dedge_w) {
                float p = scale * ds * pq + a * pg;
#pragma unroll
                for (int o = 1; o < kLP; o <<= 1) p += __shfl_xor(p, o);
                if (on && ch == 0) dedge_w[r0 + t] = p;
            }
        }
        if (live) {
            T r;
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                V::set(r, i, V::get(acc, i) * scale);
                V::set(dwe, i, V::get(dwe, i) + (scale * V::get(qi, i) * U + V::get(gi, i) * A));
            }
            *(T *)(dq + nd * HC + ch) = r;
        }
    }
    if (part) {
        // the block's dw_e rows -> one partial, summed in slot order
#pragma unroll
        for (int i = 0; i < kVec; ++i) red[threadIdx.x * kVec + i] = V::get(dwe, i);
        __syncthreads();
        const int c = threadIdx.x;
        if (c < HC) {
            float sum = 0.0f;
            for (int s = 0; s < 256 / kLP; ++s) sum += red[(s * kLP + c / kVec) * kVec + c % kVec];
            part[(int64_t)blockIdx.x * HC + c] = sum;
        }
    }
}

// The sum of n_part partial rows of P floats, for every gradient that
// workgroups leave as one partial each: a workgroup of 64 * kBwdSumRows
// threads takes 64 of the columns; row group r sums partials r, r+R, .. in
// order, then the column's thread sums the R row groups in order.
__global__ __launch_bounds__(64 * kBwdSumRows) void gsm_partial_sum_kernel(const float *__restrict__ part,
                                                                           int n_part, int P,
                                                                           const SumSegments seg) {
    __shared__ float red[kBwdSumRows][64];
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float sum = 0.0f;
    if (c < P)
        for (int b = r; b < n_part; b += 8 * kBwdSumRows) {
            float x[8];                                    // eight loads in flight, added in order
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
        int lo = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (c >= lo && c < seg.end[i] && seg.ptr[i]) seg.ptr[i][c - lo] = tot;
            lo = seg.end[i];
        }
    }
}

// the partials' sum into the segments given as (length, pointer), in order
void launch_partial_sum(const float *part, int n_part, std::initializer_list<std::pair<int, float *>> segments,
                        hipStream_t s) {
    SumSegments seg;
    int P = 0, n = 0;
    for (const auto &sg : segments) {
        P += sg.first;
        seg.end[n] = P;
        seg.ptr[n++] = sg.second;
    }
    for (; n < 4; ++n) seg.end[n] = P, seg.ptr[n] = nullptr;
    gsm_partial_sum_kernel<<<(unsigned)((P + 63) / 64), 64 * kBwdSumRows, 0, s>>>(part, n_part, P, seg);
}

template <int kLP, int kVec>
__global__ __launch_bounds__(256) void gsm_attn_bwd_source_kernel(
    const float *__restrict__ g, const float *__restrict__ q, const float *__restrict__ wa,
    const float *__restrict__ wds, const int64_t *__restrict__ t_ptr, const int32_t *__restrict__ t_edge,
    const int32_t *__restrict__ t_tgt, int64_t n_nodes, int HC, int C, float scale, float *__restrict__ dk,
    float *__restrict__ dv) {
    using V = VecT<kVec>;
    using T = typename V::T;
    constexpr int kNPW = kWave / kLP;
    const int lane = threadIdx.x & 63;
    const int sub = lane / kLP, ch = (lane % kLP) * kVec;
    const int64_t node = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * kNPW + sub;
    if (node >= n_nodes || ch >= HC) return;                // no cross-lane traffic in this kernel
    const int H = HC / C, head = ch / C;
    T ak, av;
    for (int i = 0; i < kVec; ++i) {
        V::set(ak, i, 0.0f);
        V::set(av, i, 0.0f);
    }
    const int64_t p0 = t_ptr[node];
    const int deg = (int)(t_ptr[node + 1] - p0);            // a degree-0 source stores zeros
    // next entry's id and target fetched one iteration ahead
    int64_t en = deg > 0 ? t_edge[p0] : 0, in = deg > 0 ? t_tgt[p0] : 0;
    for (int t = 0; t < deg; ++t) {
        const int64_t e = en, i_t = in;
        if (t + 1 < deg) {
            en = t_edge[p0 + t + 1];
            in = t_tgt[p0 + t + 1];
        }
        const float a = wa[e * H + head], ds = wds[e * H + head];
        const T qi = *(const T *)(q + i_t * HC + ch);
        const T gi = *(const T *)(g + i_t * HC + ch);
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            V::set(ak, i, V::get(ak, i) + ds * V::get(qi, i));
            V::set(av, i, V::get(av, i) + a * V::get(gi, i));
        }
    }
#pragma unroll
    for (int i = 0; i < kVec; ++i) V::set(ak, i, V::get(ak, i) * scale);
    *(T *)(dk + node * HC + ch) = ak;
    *(T *)(dv + node * HC + ch) = av;
}

int64_t attn_backward_work_floats(int64_t n_edges, int heads, int HC) {
    return 2 * n_edges * heads + (int64_t)kBwdMaxBlocks * HC;
}

hipError_t launch_attn_backward(const float *g, const float *q, const float *k, const float *v,
                                const float *edge_w, const float *w_e, const int64_t *row_ptr,
                                const int32_t *col, const float *out, const float *skip, const float *lse,
                                const int64_t *t_ptr, const int32_t *t_edge, const int32_t *t_tgt,
                                int64_t n_nodes, int64_t n_edges, int HC, int C, float scale, float *work,
                                float *dq, float *dk, float *dv, float *dedge_w, float *dw_e, hipStream_t s) {
    const Lanes l = select_lanes(HC, C, aligned16({g, q, k, v, out, dq, dk, dv, skip, w_e}));
    if (!l.ok) return hipErrorInvalidValue;
    const int npw = kWave / l.lp;
    const int64_t waves = (n_nodes + npw - 1) / npw;
    const int64_t groups = (waves + 3) / 4;
    const unsigned blocks_a = (unsigned)(groups < kBwdMaxBlocks ? groups : kBwdMaxBlocks);
    const unsigned blocks_b = (unsigned)groups;
    const int H = HC / C;
    float *wa = work, *wds = work + n_edges * H, *part = dw_e ? work + 2 * n_edges * H : nullptr;
    (void)hipGetLastError();
    const hipError_t e = dispatch_lanes(l, [&](auto LP, auto VEC) {
        constexpr int kLP = decltype(LP)::value, kVec = decltype(VEC)::value;
        gsm_attn_bwd_target_kernel<kLP, kVec><<<blocks_a, 256, 0, s>>>(g, q, k, v, edge_w, w_e, row_ptr, col, out,
                                                                       skip, lse, n_nodes, groups, HC, C, scale, wa,
                                                                       wds, part, dq, dedge_w);
        gsm_attn_bwd_source_kernel<kLP, kVec><<<blocks_b, 256, 0, s>>>(g, q, wa, wds, t_ptr, t_edge, t_tgt, n_nodes,
                                                                       HC, C, scale, dk, dv);
    });
    if (e != hipSuccess) return e;
    if (dw_e) launch_partial_sum(part, (int)blocks_a, {{HC, dw_e}}, s);   // HC <= 64: one workgroup
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Minibatch assembly: K samples (slot t_k, env b_k) of a rollout buffer as one
// CSR batch with its transposed graph, for the kernels above. Two launches
// with the per-sample entry offsets handed over the kernel boundary:
//
//   ptr kernel     cnt_k = edge_ptr[t_k][b_k+1] - edge_ptr[t_k][b_k] (0 for a
//                  bad sample), sample_ptr = exclusive scan; one workgroup,
//                  kPtrItems consecutive samples per thread and chunk, their
//                  loads issued together
//   gather kernel  one wave per sample: node rows copied; a node's row offset
//                  is the lower bound of its id in the sample's (sorted)
//                  source list; columns relabelled b*E + e -> k*E + e; and,
//                  the env graph being symmetric with ascending rows and
//                  columns, the transposed CSR is (row_ptr, t_edge, col) with
//                  t_edge[p] = the position of row(p) inside row col(p): one
//                  more search
//
// Every offset read from memory is checked before it bounds a loop or forms an
// address: a sample's range must satisfy 0 <= start <= end <= capacity (else it
// counts no entries) and its output range must lie inside [0, n_edges) with the
// same length (else nothing is written for it); every search runs over the
// sample's own entries only. Bad data sets status bits and gets defined
// in-range values.

constexpr int kPtrThreads = 1024;
constexpr int kPtrItems = 8;          // samples per thread and chunk
constexpr int kStageEntries = 512;    // entries per wave staged in LDS (src and dst: 4 KiB a wave)

// the checked entry range of sample (t, b): false (and bits) when it is unusable
__device__ __forceinline__ bool sample_range(const int64_t *__restrict__ edge_ptr, int64_t S, int64_t B,
                                             int64_t cap, int64_t t, int64_t b, int64_t &start, int64_t &cnt,
                                             int &bits) {
    start = 0;
    cnt = 0;
    if (t < 0 || t >= S || b < 0 || b >= B) {
        bits |= GSM_BATCH_BAD_INDEX;
        return false;
    }
    const int64_t a = edge_ptr[t * (B + 1) + b], e = edge_ptr[t * (B + 1) + b + 1];
    if (e > cap) {
        bits |= GSM_BATCH_TRUNCATED;
        return false;
    }
    if (a < 0 || e < a) {
        bits |= GSM_BATCH_BAD_OFFSETS;
        return false;
    }
    start = a;
    cnt = e - a;
    return true;
}

__global__ __launch_bounds__(kPtrThreads) void gsm_graph_batch_ptr_kernel(
    const int64_t *__restrict__ edge_ptr, int64_t S, int64_t B, int64_t cap, const int64_t *__restrict__ t_idx,
    const int64_t *__restrict__ b_idx, int64_t K, int64_t *__restrict__ sample_ptr, int32_t *__restrict__ status) {
    __shared__ int64_t wsum[kPtrThreads / kWave];
    __shared__ int64_t chunk_total;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int bits = 0;
    int64_t carry = 0;
    if (tid == 0) sample_ptr[0] = 0;
    for (int64_t base = 0; base < K; base += (int64_t)kPtrThreads * kPtrItems) {
        const int64_t k0 = base + (int64_t)tid * kPtrItems;
        int64_t t[kPtrItems], b[kPtrItems], cnt[kPtrItems];
#pragma unroll
        for (int u = 0; u < kPtrItems; ++u) {
            const bool in = k0 + u < K;
            t[u] = in ? t_idx[k0 + u] : -1;
            b[u] = in ? b_idx[k0 + u] : -1;
        }
#pragma unroll
        for (int u = 0; u < kPtrItems; ++u) {
            int64_t start;
            cnt[u] = 0;
            if (k0 + u < K) sample_range(edge_ptr, S, B, cap, t[u], b[u], start, cnt[u], bits);
        }
        int64_t mine = 0;
#pragma unroll
        for (int u = 0; u < kPtrItems; ++u) mine += cnt[u];
        int64_t inc = mine;                                   // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int64_t up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == kWave - 1) wsum[wv] = inc;
        __syncthreads();
        int64_t before = 0;
        for (int w = 0; w < wv; ++w) before += wsum[w];
        if (tid == kPtrThreads - 1) chunk_total = before + inc;
        int64_t run = carry + before + inc - mine;            // entries before this thread's samples
#pragma unroll
        for (int u = 0; u < kPtrItems; ++u) {
            run += cnt[u];
            if (k0 + u < K) sample_ptr[k0 + u + 1] = run;
        }
        __syncthreads();
        carry += chunk_total;
    }
    if (bits) atomicOr(status, bits);
}

// first position in [0, n) whose value is >= x (n when none); the list ascends
template <class A>
__device__ __forceinline__ int lower_bound(const A &at, int lo, int n, int x) {
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (at(mid) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the sample's entries through src(p), dst(p): local ids (global id - b*E)
template <class FS, class FD>
__device__ __forceinline__ void batch_sample_entries(const FS &src, const FD &dst, int n, int E, int lane,
                                                     int64_t k, int64_t s0, const float *__restrict__ attr_in,
                                                     int64_t *__restrict__ row_ptr, int32_t *__restrict__ col,
                                                     float *__restrict__ attr_out, int32_t *__restrict__ t_edge,
                                                     int &bits) {
    for (int e = lane; e < E; e += kWave) row_ptr[k * E + e] = s0 + lower_bound(src, 0, n, e);
    for (int p = lane; p < n; p += kWave) {
        const int j = src(p), i = dst(p);
        const bool inside = i >= 0 && i < E && j >= 0 && j < E;
        if (!inside) bits |= GSM_BATCH_OUT_OF_ENV;
        col[s0 + p] = (int32_t)(k * E + min(max(i, 0), E - 1));
        attr_out[s0 + p] = attr_in[p];
        if (t_edge) {
            int q = p;
            if (inside) {
                // row i of the sample, then j's position among its columns
                const int r0 = lower_bound(src, 0, n, i);
                const int r1 = lower_bound(src, r0, n, i + 1);
                const int f = lower_bound(dst, r0, r1, j);
                if (f < r1 && dst(f) == j && src(f) == i) q = f;
                else bits |= GSM_BATCH_ASYMMETRIC;
            }
            t_edge[s0 + p] = (int32_t)(s0 + q);
        }
    }
}

__global__ __launch_bounds__(256) void gsm_graph_batch_gather_kernel(
    const float *__restrict__ node_feat, const int32_t *__restrict__ edge_index,
    const float *__restrict__ edge_attr, const int64_t *__restrict__ edge_ptr, int64_t S, int64_t B, int E,
    int64_t cap, const int64_t *__restrict__ t_idx, const int64_t *__restrict__ b_idx,
    const int64_t *__restrict__ sample_ptr, int64_t K, int64_t n_edges, float *__restrict__ node_feat_out,
    int64_t *__restrict__ row_ptr, int32_t *__restrict__ col, float *__restrict__ attr_out,
    int32_t *__restrict__ t_edge, int32_t *__restrict__ status) {
    __shared__ int32_t lsrc[4][kStageEntries], ldst[4][kStageEntries];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * 4 + wv;           // wave-uniform
    const bool have = k < K;
    int bits = 0, n = 0;
    int64_t t = 0, b = 0, start = 0, s0 = 0;
    bool valid = false;
    if (have) {
        int64_t cnt;
        t = t_idx[k];
        b = b_idx[k];
        valid = sample_range(edge_ptr, S, B, cap, t, b, start, cnt, bits);
        if (!valid) t = b = 0;
        s0 = sample_ptr[k];
        const int64_t s1 = sample_ptr[k + 1];
        // the scan's range must be this sample's count inside the outputs
        if (s0 < 0 || s1 < s0 || s1 > n_edges || s1 - s0 != cnt) {
            bits |= GSM_BATCH_BAD_OFFSETS;
            cnt = 0;
            s0 = min(max(s0, (int64_t)0), n_edges);
        }
        n = (int)cnt;                                         // <= n_edges < 2^31
    }
    const int32_t *gs = edge_index + (valid ? (t * 2 * cap + start) : 0), *gd = gs + cap;
    const int bE = (int)(b * E);                              // K*E and B*E < 2^31 (host-checked)
    const bool staged = n <= kStageEntries;
    if (staged)
        for (int p = lane; p < n; p += kWave) {
            lsrc[wv][p] = gs[p] - bE;
            ldst[wv][p] = gd[p] - bE;
        }
    __syncthreads();
    if (!have) return;
    // node rows: E*7 dwords, contiguous on both sides; 16-byte pieces when aligned
    {
        const int nd = E * 7;
        const float *in = node_feat + (valid ? (t * B + b) * nd : 0);
        float *out = node_feat_out + k * nd;
        if (!valid) {
            for (int x = lane; x < nd; x += kWave) out[x] = 0.0f;
        } else if (((uintptr_t)in | (uintptr_t)out) % 16 == 0 && nd % 4 == 0) {
            for (int x = lane; x < nd / 4; x += kWave) ((float4 *)out)[x] = ((const float4 *)in)[x];
        } else {
            for (int x = lane; x < nd; x += kWave) out[x] = in[x];
        }
    }
    if (k == K - 1 && lane == 0) row_ptr[K * E] = n_edges;
    const float *attr_in = edge_attr + (valid ? (t * cap + start) : 0);
    if (staged) {
        const int32_t *ls = lsrc[wv], *ld = ldst[wv];
        batch_sample_entries([ls](int p) { return ls[p]; }, [ld](int p) { return ld[p]; }, n, E, lane, k, s0,
                             attr_in, row_ptr, col, attr_out, t_edge, bits);
    } else {
        batch_sample_entries([gs, bE](int p) { return gs[p] - bE; }, [gd, bE](int p) { return gd[p] - bE; }, n, E,
                             lane, k, s0, attr_in, row_ptr, col, attr_out, t_edge, bits);
    }
    if (bits) atomicOr(status, bits);
}

hipError_t launch_graph_batch_ptr(const int64_t *edge_ptr, int64_t S, int64_t B, int64_t cap,
                                  const int64_t *t_idx, const int64_t *b_idx, int64_t K, int64_t *sample_ptr,
                                  int32_t *status, hipStream_t s) {
    (void)hipGetLastError();
    gsm_graph_batch_ptr_kernel<<<1, kPtrThreads, 0, s>>>(edge_ptr, S, B, cap, t_idx, b_idx, K, sample_ptr, status);
    return hipGetLastError();
}

hipError_t launch_graph_batch_gather(const float *node_feat, const int32_t *edge_index, const float *edge_attr,
                                     const int64_t *edge_ptr, int64_t S, int64_t B, int E, int64_t cap,
                                     const int64_t *t_idx, const int64_t *b_idx, const int64_t *sample_ptr,
                                     int64_t K, int64_t n_edges, float *node_feat_out, int64_t *row_ptr,
                                     int32_t *col, float *attr_out, int32_t *t_edge, int32_t *status,
                                     hipStream_t s) {
    (void)hipGetLastError();
    gsm_graph_batch_gather_kernel<<<(unsigned)((K + 3) / 4), 256, 0, s>>>(
        node_feat, edge_index, edge_attr, edge_ptr, S, B, E, cap, t_idx, b_idx, sample_ptr, K, n_edges,
        node_feat_out, row_ptr, col, attr_out, t_edge, status);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// GAE over a stored episode: one thread per (env, agent) walks the slots from
// the last to the first with the running advantage in a register; the loads
// of a slot are coalesced across (env, agent). Each operation below is one
// correctly rounded fp32 operation in the order of the torch loop it replaces
// (the library is built with -ffp-contract=off), so the returns are the same
// bit for bit.
__global__ __launch_bounds__(256) void gsm_gae_kernel(const float *__restrict__ reward,
                                                      const float *__restrict__ value,
                                                      const uint8_t *__restrict__ done, int64_t T, int64_t BN,
                                                      int N, float gamma, float gamma_lambda,
                                                      float *__restrict__ ret) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= BN) return;
    const int64_t B = (uint32_t)BN / (uint32_t)N, b = (uint32_t)x / (uint32_t)N;   // B*N < 2^31 (host-checked)
    float gae = 0.0f;
    float v1 = value[T * BN + x];
#pragma unroll 4
    for (int64_t t = T - 1; t >= 0; --t) {
        const float r = reward[t * BN + x], v0 = value[t * BN + x];
        const float m = 1.0f - (float)done[(t + 1) * B + b];
        const float delta = (r + (gamma * v1) * m) - v0;
        gae = delta + (gamma_lambda * m) * gae;
        ret[t * BN + x] = gae + v0;
        v1 = v0;
    }
}

hipError_t launch_gae(const float *reward, const float *value, const uint8_t *done, int64_t T, int64_t B, int N,
                      float gamma, float gamma_lambda, float *ret, hipStream_t s) {
    const int64_t BN = B * N;
    (void)hipGetLastError();
    gsm_gae_kernel<<<(unsigned)((BN + 255) / 256), 256, 0, s>>>(reward, value, done, T, BN, N, gamma,
                                                                gamma_lambda, ret);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fused first layer on env-form graphs (gsm_env_conv): the four K = 7
// projections and the attention of one TransformerConv(7, C, heads) layer in
// one launch, straight from node_feat [B][E][7] and the env's packed edge list.
// Edges never leave their env and an env's entries are contiguous and sorted
// by row, so a workgroup keeps whole envs on chip (max(1, 64 / E) of them, so
// that small envs fill the block's node slots):
//
//   ranges    thread g < envs: edge_ptr[b], edge_ptr[b+1] checked against
//             0 <= start <= end <= edge_limit (else the env counts 0 entries)
//   rows      the envs' 7-float rows -> LDS, 8 floats a row (two 16-byte reads)
//   entries   one coalesced pass over the envs' row and col ids: every id
//             checked against [bE, (b+1)E) and every row against its
//             predecessor; the first entry of a run of equal rows writes the
//             row starts of the rows it opens (row_start[r] = position, for r
//             in (previous row, row]), so the per-node offsets need neither a
//             bincount nor a search. An env that fails a check is edgeless.
//   table     k_j, v_j of every node once per env -> LDS (table form), when
//             rows + offsets + 2 * nodes * HC floats fit 64 KiB (two or more
//             workgroups a CU); else k_j, v_j are recomputed from the source's
//             row for every entry (recompute form: E = 288 with HC >= 24)
//   walk      kLP lanes per output row, kVec channels per lane, the online
//             softmax of gsm_attn_aggregate over the row's entries in ascending
//             order; q_i and skip_i formed from the row in LDS; the sources'
//             k_j, v_j come from the LDS table (or the LDS rows), the column
//             ids and distances from global memory one entry ahead
//
// A projection is acc = bias, then acc = acc + W[c][f] * x[f] for f = 0..6,
// one fp32 operation per step (no contraction), in both forms, so the two
// forms agree bit for bit; no atomics on floats: the output is reproducible.

constexpr int kConvThreads = 256;
constexpr int kConvLdsMax = 64 * 1024;

struct ConvParams {
    const float *node_feat;
    const int64_t *edge_ptr;
    const int32_t *erow, *ecol;
    const float *edge_attr;
    int64_t edge_limit;
    const float *w, *w_e;
    int B, E, epb, HC, C, skip, n_rows_out;
    float scale;
    float *out;
    float *lse;                                 // [B][n_rows_out][H] softmax statistics, or nullptr
    int64_t *row_ptr_out;
    int32_t *status;
};

// byte offsets of the workgroup's LDS regions
struct ConvLds {
    int xs, est, ecnt, ebad, rs, tab, total;
};
__host__ __device__ inline ConvLds conv_lds(int epb, int E, int HC, bool table) {
    ConvLds l;
    const int n = epb * E;
    l.xs = 0;                                   // f32 [n][8]
    l.est = l.xs + n * 32;                      // int64 [epb] checked start
    l.ecnt = l.est + epb * 8;                   // int [epb] checked entry count
    l.ebad = l.ecnt + epb * 4;                  // int [epb] an entry failed its check
    l.rs = l.ebad + epb * 4;                    // int [epb][E+1] row starts inside the env
    l.tab = (l.rs + epb * (E + 1) * 4 + 15) & ~15;   // f32 [2][n][HC] k, v
    l.total = l.tab + (table ? 2 * n * HC * 4 : 0);
    return l;
}

// rows c .. c+kVec-1 of weight block blk: [HC][8] = 7 weights and the bias
template <int kVec>
__device__ __forceinline__ void conv_load_w(const float *__restrict__ w, int blk, int HC, int ch, bool on,
                                            float (&r)[kVec][8]) {
#pragma unroll
    for (int i = 0; i < kVec; ++i) {
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (on) {
            const float4 *src = (const float4 *)(w + ((int64_t)blk * HC + ch + i) * 8);
            a = src[0];
            b = src[1];
        }
        r[i][0] = a.x, r[i][1] = a.y, r[i][2] = a.z, r[i][3] = a.w;
        r[i][4] = b.x, r[i][5] = b.y, r[i][6] = b.z, r[i][7] = b.w;
    }
}

template <int kVec>
__device__ __forceinline__ typename VecT<kVec>::T conv_project(const float (&wr)[kVec][8], const float4 &x0,
                                                               const float4 &x1) {
    typename VecT<kVec>::T r;
#pragma unroll
    for (int i = 0; i < kVec; ++i) {
        float acc = wr[i][7];
        acc = acc + wr[i][0] * x0.x;
        acc = acc + wr[i][1] * x0.y;
        acc = acc + wr[i][2] * x0.z;
        acc = acc + wr[i][3] * x0.w;
        acc = acc + wr[i][4] * x1.x;
        acc = acc + wr[i][5] * x1.y;
        acc = acc + wr[i][6] * x1.z;
        VecT<kVec>::set(r, i, acc);
    }
    return r;
}

// ranges, rows and entries of envs b0 .. b0+ne-1 -> LDS (est, ecnt, ebad, xs,
// rs), the checks' bits -> status; shared by the forward and the backward, so
// an env is edgeless in both or in neither. Ends on a barrier.
__device__ __forceinline__ void conv_stage_envs(const ConvParams &p, const ConvLds &L, char *sm, int b0, int ne,
                                                int tid) {
    const int E = p.E, n_loc = ne * E;
    float *xs = (float *)(sm + L.xs);
    int64_t *est = (int64_t *)(sm + L.est);
    int *ecnt = (int *)(sm + L.ecnt), *ebad = (int *)(sm + L.ebad), *rs = (int *)(sm + L.rs);
    int bits = 0;

    // ranges: every offset checked before it bounds a loop or forms an address
    if (tid < ne) {
        const int64_t a = p.edge_ptr[b0 + tid], e = p.edge_ptr[b0 + tid + 1];
        int cnt = 0;
        if (e > p.edge_limit) bits |= GSM_BATCH_TRUNCATED;
        else if (a < 0 || e < a) bits |= GSM_BATCH_BAD_OFFSETS;
        else cnt = (int)(e - a);                             // <= edge_limit < 2^31
        est[tid] = a < 0 ? 0 : (a > p.edge_limit ? p.edge_limit : a);
        ecnt[tid] = cnt;
        ebad[tid] = 0;
    }
    // rows: n_loc * 7 contiguous floats
    {
        const float *src = p.node_feat + (int64_t)b0 * E * 7;
        for (int x = tid; x < n_loc * 7; x += kConvThreads) {
            const int nd = x / 7;
            xs[nd * 8 + (x - nd * 7)] = src[x];
        }
    }
    __syncthreads();

    // entries: ids and order checked, row starts marked
    for (int g = 0; g < ne; ++g) {
        const int cnt = ecnt[g];
        int *r = rs + g * (E + 1);
        if (cnt == 0) {
            for (int x = tid; x <= E; x += kConvThreads) r[x] = 0;
            continue;
        }
        const int64_t s = est[g];
        const uint32_t bE = (uint32_t)(b0 + g) * (uint32_t)E;   // B * E < 2^31 (host-checked)
        for (int q = tid; q < cnt; q += kConvThreads) {
            const uint32_t ri = (uint32_t)p.erow[s + q] - bE, ci = (uint32_t)p.ecol[s + q] - bE;
            const uint32_t pr = q ? (uint32_t)p.erow[s + q - 1] - bE : 0u;
            // pr <= ri < E: both rows inside the env and ascending
            if (!(ri < (uint32_t)E && ci < (uint32_t)E && pr <= ri)) {
                ebad[g] = 1;
                continue;
            }
            for (int x = q ? (int)pr + 1 : 0; x <= (int)ri; ++x) r[x] = q;
            if (q == cnt - 1)
                for (int x = (int)ri + 1; x <= E; ++x) r[x] = cnt;
        }
    }
    __syncthreads();
    if (tid < ne && ebad[tid]) bits |= GSM_BATCH_OUT_OF_ENV;
    if (bits) atomicOr(p.status, bits);
}

// the table form is held to 128 VGPRs (four waves a SIMD); the recompute form
// keeps all four weight blocks in registers at two. kLse (gsm_env_conv_fwd) is
// the same kernel with one more store, the rows' softmax statistics; that
// store takes the table form to 132 VGPRs, three waves, so it is a template
// flag and the inference instantiations are untouched by it
template <int kLP, int kVec, bool kTable, bool kLse>
__global__ __launch_bounds__(kConvThreads, kTable ? (kLse ? 3 : 4) : 2) void gsm_env_conv_kernel(const ConvParams p) {
    using V = VecT<kVec>;
    using T = typename V::T;
    constexpr int kNPP = kConvThreads / kLP;                 // output rows per pass of the block
    extern __shared__ float4 conv_smem[];
    char *sm = (char *)conv_smem;
    const int E = p.E, HC = p.HC;
    const ConvLds L = conv_lds(p.epb, E, HC, kTable);
    float *xs = (float *)(sm + L.xs);
    int64_t *est = (int64_t *)(sm + L.est);
    int *ecnt = (int *)(sm + L.ecnt), *ebad = (int *)(sm + L.ebad), *rs = (int *)(sm + L.rs);
    float *ktab = (float *)(sm + L.tab), *vtab = ktab + p.epb * E * HC;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * p.epb;                       // grid = ceil(B / epb): b0 < B
    const int ne = min(p.epb, p.B - b0), n_loc = ne * E;

    conv_stage_envs(p, L, sm, b0, ne, tid);

    // the per-node offsets env_csr would give (a failed env repeats its start)
    if (p.row_ptr_out) {
        for (int x = tid; x < n_loc; x += kConvThreads) {
            const int g = x / E;
            p.row_ptr_out[(int64_t)b0 * E + x] = est[g] + (ebad[g] ? 0 : rs[g * (E + 1) + (x - g * E)]);
        }
        if (b0 + ne == p.B && tid == 0)
            p.row_ptr_out[(int64_t)p.B * E] = est[ne - 1] + (ebad[ne - 1] ? 0 : ecnt[ne - 1]);
    }

    const int slot = tid / kLP, ch = (tid % kLP) * kVec;
    const bool chon = ch < HC;
    if constexpr (kTable) {
        float wk[kVec][8], wv[kVec][8];
        conv_load_w<kVec>(p.w, 1, HC, ch, chon, wk);
        conv_load_w<kVec>(p.w, 2, HC, ch, chon, wv);
        if (chon)
            for (int x = slot; x < n_loc; x += kNPP) {
                const float4 x0 = *(const float4 *)(xs + x * 8), x1 = *(const float4 *)(xs + x * 8 + 4);
                *(T *)(ktab + x * HC + ch) = conv_project<kVec>(wk, x0, x1);
                *(T *)(vtab + x * HC + ch) = conv_project<kVec>(wv, x0, x1);
            }
        __syncthreads();
    }

    const int lanes_per_head = p.C / kVec;                   // power of two
    float wq[kVec][8], ws[kVec][8], wk[kVec][8], wv[kVec][8];
    conv_load_w<kVec>(p.w, 0, HC, ch, chon, wq);
    conv_load_w<kVec>(p.w, 3, HC, ch, chon && p.skip, ws);
    if constexpr (!kTable) {
        conv_load_w<kVec>(p.w, 1, HC, ch, chon, wk);
        conv_load_w<kVec>(p.w, 2, HC, ch, chon, wv);
    }
    T we;
    for (int i = 0; i < kVec; ++i) V::set(we, i, 0.0f);
    if (chon && p.w_e) we = *(const T *)(p.w_e + ch);
    const int R = p.n_rows_out, n_walk = ne * R;
    for (int base = 0; base < n_walk; base += kNPP) {        // block-uniform trip count
        const int idx = base + slot;
        const bool have = idx < n_walk, live = have && chon;
        const int id = have ? idx : 0;
        const int g = id / R, i = id - g * R, gE = g * E;
        const float4 x0 = *(const float4 *)(xs + (gE + i) * 8), x1 = *(const float4 *)(xs + (gE + i) * 8 + 4);
        const T qi = conv_project<kVec>(wq, x0, x1);
        const T sk = conv_project<kVec>(ws, x0, x1);
        const bool good = have && !ebad[g];
        const int r0 = good ? rs[g * (E + 1) + i] : 0;
        const int deg = good ? rs[g * (E + 1) + i + 1] - r0 : 0;
        const int32_t *colp = p.ecol + est[g] + r0;
        const float *attrp = p.edge_attr + est[g] + r0;
        const uint32_t bE = (uint32_t)(b0 + g) * (uint32_t)E;
        int wdeg = deg;                                      // the wave runs its longest row
#pragma unroll
        for (int o = kLP; o < kWave; o <<= 1) wdeg = max(wdeg, __shfl_xor(wdeg, o));
        T acc;
        for (int c = 0; c < kVec; ++c) V::set(acc, c, 0.0f);
        float mx = -__builtin_inff(), den = 0.0f;
        // next entry's source and distance fetched one iteration ahead
        int32_t jn = (live && deg > 0) ? colp[0] : 0;
        float wn = (live && deg > 0 && p.w_e) ? attrp[0] : 0.0f;
        for (int t = 0; t < wdeg; ++t) {
            const bool on = live && t < deg;
            const int jl = min(max((int)((uint32_t)jn - bE), 0), E - 1);   // checked above; clamped again
            const float w = wn;
            if (live && t + 1 < deg) {
                jn = colp[t + 1];
                if (p.w_e) wn = attrp[t + 1];
            }
            T kj, vj;
            for (int c = 0; c < kVec; ++c) {
                V::set(kj, c, 0.0f);
                V::set(vj, c, 0.0f);
            }
            if (on) {
                if constexpr (kTable) {
                    kj = *(const T *)(ktab + (gE + jl) * HC + ch);
                    vj = *(const T *)(vtab + (gE + jl) * HC + ch);
                } else {
                    const float4 y0 = *(const float4 *)(xs + (gE + jl) * 8),
                                 y1 = *(const float4 *)(xs + (gE + jl) * 8 + 4);
                    kj = conv_project<kVec>(wk, y0, y1);
                    vj = conv_project<kVec>(wv, y0, y1);
                }
            }
            float sc = 0.0f;
#pragma unroll
            for (int c = 0; c < kVec; ++c) sc += V::get(qi, c) * (V::get(kj, c) + w * V::get(we, c));
#pragma unroll
            for (int o = 1; o < kLP; o <<= 1)
                if (o < lanes_per_head) sc += __shfl_xor(sc, o);   // sum over the head's lanes
            sc *= p.scale;
            if (on) {
                const float m2 = fmaxf(mx, sc);
                const float a = __expf(mx - m2), b = __expf(sc - m2);
                den = den * a + b;
#pragma unroll
                for (int c = 0; c < kVec; ++c)
                    V::set(acc, c, V::get(acc, c) * a + b * (V::get(vj, c) + w * V::get(we, c)));
                mx = m2;
            }
        }
        if (live) {
            const float inv = den > 0.0f ? 1.0f / den : 0.0f;
            T r;
#pragma unroll
            for (int c = 0; c < kVec; ++c)
                V::set(r, c, V::get(acc, c) * inv + (p.skip ? V::get(sk, c) : 0.0f));
            *(T *)(p.out + ((int64_t)(b0 + g) * R + i) * HC + ch) = r;
            // softmax statistics for the backward: each head's first lane; an
            // empty row stores a finite value that is never read
            if constexpr (kLse)
                if (ch % p.C == 0)
                    p.lse[((int64_t)(b0 + g) * R + i) * (HC / p.C) + ch / p.C] =
                        den > 0.0f ? mx + logf(den) : 0.0f;
        }
    }
}

hipError_t launch_env_conv(const float *node_feat, const int64_t *edge_ptr, const int32_t *edge_index,
                           int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit, const float *w,
                           const float *w_e, int64_t B, int E, int HC, int C, float scale, bool skip,
                           int n_rows_out, float *out, float *lse, int64_t *row_ptr_out, int32_t *status,
                           hipStream_t s) {
    const Lanes l = select_lanes(HC, C, aligned16({out, w_e}));
    if (!l.ok) return hipErrorInvalidValue;
    ConvParams p;
    p.node_feat = node_feat;
    p.edge_ptr = edge_ptr;
    p.erow = edge_index;
    p.ecol = edge_index ? edge_index + edge_row_stride : nullptr;
    p.edge_attr = edge_attr;
    p.edge_limit = edge_limit;
    p.w = w;
    p.w_e = w_e;
    p.B = (int)B;
    p.E = E;
    p.epb = E >= 64 ? 1 : 64 / E;
    p.HC = HC;
    p.C = C;
    p.skip = skip;
    p.n_rows_out = n_rows_out;
    p.scale = scale;
    p.out = out;
    p.lse = lse;
    p.row_ptr_out = row_ptr_out;
    p.status = status;
    const bool table = conv_lds(p.epb, E, HC, true).total <= kConvLdsMax;
    const size_t lds = (size_t)conv_lds(p.epb, E, HC, table).total;
    if (lds > (size_t)kConvLdsMax) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((B + p.epb - 1) / p.epb);
    (void)hipGetLastError();
    const hipError_t e = dispatch_lanes(l, [&](auto LP, auto VEC) {
        constexpr int kLP = decltype(LP)::value, kVec = decltype(VEC)::value;
        if (table && lse) gsm_env_conv_kernel<kLP, kVec, true, true><<<blocks, kConvThreads, lds, s>>>(p);
        else if (table) gsm_env_conv_kernel<kLP, kVec, true, false><<<blocks, kConvThreads, lds, s>>>(p);
        else if (lse) gsm_env_conv_kernel<kLP, kVec, false, true><<<blocks, kConvThreads, lds, s>>>(p);
        else gsm_env_conv_kernel<kLP, kVec, false, false><<<blocks, kConvThreads, lds, s>>>(p);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

// ---------------------------------------------------------------------------
// Backward of the fused first layer (gsm_env_conv_bwd). node_feat and
// edge_attr are env data, so the gradients are those of the weights alone:
// with x_i the node's seven features and a trailing 1, g_i = grad_out of row i
// (0 for i >= n_rows_out) and dq, dk, dv of the aggregation's backward above,
//
//   dW_q[c][f] = sum_i dq_i[c] x_i[f]     dW_skip[c][f] = sum_i g_i[c] x_i[f]
//   dW_k[c][f] = sum_j dk_j[c] x_j[f]     dW_v[c][f]    = sum_j dv_j[c] x_j[f]
//   dw_e[c]    = sum_i scale q_i[c] U_i + g_i[c] A_i
//
// over every node of every env. The forward's structure: a workgroup holds
// max(1, 64 / E) envs, staged and checked by conv_stage_envs exactly as the
// forward stages them (a failed env is edgeless here too: its rows reach
// dW_skip only), with the k, v table or the recompute form. Per env group:
//
//   target pass  the forward's lane mapping over the output rows: q_i, skip_i
//                recomputed from the LDS row, D_i from g_i and out_i - skip_i,
//                a_ij = exp(s_ij - lse_i) with s_ij in the forward's operation
//                order; dq_i in registers; a_ij, ds_ij per (entry, head) ->
//                work, at the entry's own position in the edge arrays (read
//                back by this workgroup after a barrier: L2-resident)
//   source pass  the env graphs are symmetric with ascending columns, so row j
//                lists exactly the targets i that list j: node j walks its own
//                row and finds j inside row i, its position = the number of
//                row i's columns below j, counted by the slot's kLP lanes side
//                by side over row i's checked range [rs[i], rs[i+1]) (loads
//                that do not wait for one another, where a binary search's
//                do); reads a, ds there, recomputes q_i, reads g_i and sums
//                dk_j, dv_j in registers in ascending i. Every entry's reverse
//                entry is looked for; a missing one sets GSM_BATCH_ASYMMETRIC
//                and contributes nothing
//   weights      after each pass of kNPP rows the lanes' (dq, g) or (dk, dv)
//                go through an LDS stage; thread (array, channel c) adds
//                d[c] * x[f] of the staged rows in slot order to its eight
//                accumulators, which live in registers across the env groups
//                the workgroup walks (a capped grid, groups in order)
//
// A workgroup ends with one partial [3 or 4][HC][8] + [HC]; a second launch
// sums the partials of each value in index order. No float atomics anywhere:
// the summation order is fixed by the shape alone, so dw and dw_e are bitwise
// reproducible.

// grid cap = weight-gradient partials: the workgroups that are resident at once
// (three a CU at the table form's 168 VGPRs, two at the recompute form's, fewer
// when their LDS does not fit a CU's 160 KiB) on 256 CUs, so that no workgroup
// waits for another to end; constants, so the count, hence the summation order,
// is the same on every device
constexpr int kConvBwdMaxBlocks = 768;
constexpr int kConvBwdCus = 256, kConvBwdLdsPerCu = 160 * 1024;

struct ConvBwdParams {
    ConvParams f;                 // graph, weights, shape, status; f.out, f.lse, f.row_ptr_out unused
    const float *grad_out, *out, *lse;
    float *wa, *wds;              // [edge_limit][H]: a_ij, ds_ij at the entry's position
    float *part;                  // [gridDim.x][nblk*HC*8 + HC]
    int n_groups, want_dwe;
};

// the pass stage [2][kConvThreads * vec], then the weight-gradient accumulators [16][2 * HC]
__host__ __device__ inline int conv_bwd_stage_bytes(int vec, int HC) {
    return 2 * kConvThreads * vec * 4 + 16 * 2 * HC * 4;
}

// the rows staged by one pass -> this thread's eight accumulators (in LDS
// between the passes, stride apart, so that the walks have the registers), in
// slot order
template <int kLP, int kVec>
__device__ __forceinline__ void conv_bwd_accumulate(const float *__restrict__ col, const float *__restrict__ xs,
                                                    int base, int n_rows, int R, int E, float *__restrict__ racc,
                                                    int stride) {
    constexpr int kNPP = kConvThreads / kLP;
    const int n = min(kNPP, n_rows - base);
    int g = base / R, i = base - g * R;
    float acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = racc[f * stride];
    for (int s = 0; s < n; ++s) {
        const float d = col[s * kLP * kVec];
        const float *x = xs + (g * E + i) * 8;
        const float4 x0 = *(const float4 *)x, x1 = *(const float4 *)(x + 4);
        acc[0] += d * x0.x, acc[1] += d * x0.y, acc[2] += d * x0.z, acc[3] += d * x0.w;
        acc[4] += d * x1.x, acc[5] += d * x1.y, acc[6] += d * x1.z, acc[7] += d;
        if (++i == R) i = 0, ++g;
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) racc[f * stride] = acc[f];
}

template <int kLP, int kVec, bool kTable>
__global__ __launch_bounds__(kConvThreads, kTable ? 3 : 2) void gsm_env_conv_bwd_kernel(const ConvBwdParams bp) {
    using V = VecT<kVec>;
    using T = typename V::T;
    constexpr int kNPP = kConvThreads / kLP;                 // rows per pass of the block
    extern __shared__ float4 conv_smem[];
    char *sm = (char *)conv_smem;
    const ConvParams &p = bp.f;
    const int E = p.E, HC = p.HC, C = p.C, H = HC / C, R = p.n_rows_out;
    const ConvLds L = conv_lds(p.epb, E, HC, kTable);
    float *xs = (float *)(sm + L.xs);
    int64_t *est = (int64_t *)(sm + L.est);
    int *ebad = (int *)(sm + L.ebad), *rs = (int *)(sm + L.rs);
    float *ktab = (float *)(sm + L.tab), *vtab = ktab + p.epb * E * HC;
    float *stage = (float *)(sm + L.total);                  // [2][kConvThreads * kVec], then the accumulators
    const int tid = threadIdx.x;
    const int slot = tid / kLP, sub = tid % kLP, ch = sub * kVec;
    const bool chon = ch < HC;
    const int head = chon ? ch / C : 0;
    const int lanes_per_head = C / kVec;                     // power of two
    // weight gradients: thread (array ra, channel rc) of the first 2 * HC
    const bool red = tid < 2 * HC;
    const int ra = tid >= HC ? 1 : 0, rc = tid - ra * HC;
    const float *rcol = stage + ra * kConvThreads * kVec + (rc / kVec) * kVec + rc % kVec;
    // its accumulators [f][tid]: f < 8 the target pass (W_q | W_skip), then the source pass (W_k | W_v);
    // touched by this thread alone
    float *racc = stage + 2 * kConvThreads * kVec + tid;
    if (red)
        for (int f = 0; f < 16; ++f) racc[f * 2 * HC] = 0.0f;
    float wq[kVec][8], wk[kVec][8], wv[kVec][8];             // the skip block is fetched where a row needs it
    conv_load_w<kVec>(p.w, 0, HC, ch, chon, wq);
    if constexpr (!kTable) {
        conv_load_w<kVec>(p.w, 1, HC, ch, chon, wk);
        conv_load_w<kVec>(p.w, 2, HC, ch, chon, wv);
    }
    T we, dwe;
    for (int c = 0; c < kVec; ++c) {
        V::set(we, c, 0.0f);
        V::set(dwe, c, 0.0f);
    }
    if (chon && p.w_e) we = *(const T *)(p.w_e + ch);
    int bits = 0;

    for (int grp = blockIdx.x; grp < bp.n_groups; grp += gridDim.x) {
        const int b0 = grp * p.epb;
        const int ne = min(p.epb, p.B - b0), n_loc = ne * E;
        conv_stage_envs(p, L, sm, b0, ne, tid);
        if constexpr (kTable) {
            conv_load_w<kVec>(p.w, 1, HC, ch, chon, wk);
            conv_load_w<kVec>(p.w, 2, HC, ch, chon, wv);
            if (chon)
                for (int x = slot; x < n_loc; x += kNPP) {
                    const float4 x0 = *(const float4 *)(xs + x * 8), x1 = *(const float4 *)(xs + x * 8 + 4);
                    *(T *)(ktab + x * HC + ch) = conv_project<kVec>(wk, x0, x1);
                    *(T *)(vtab + x * HC + ch) = conv_project<kVec>(wv, x0, x1);
                }
            __syncthreads();
        }

        // target pass
        const int n_walk = ne * R;
        for (int base = 0; base < n_walk; base += kNPP) {    // block-uniform trip count
            const int idx = base + slot;
            const bool have = idx < n_walk, live = have && chon;
            const int id = have ? idx : 0;
            const int g = id / R, i = id - g * R, gE = g * E;
            const float4 x0 = *(const float4 *)(xs + (gE + i) * 8), x1 = *(const float4 *)(xs + (gE + i) * 8 + 4);
            const T qi = conv_project<kVec>(wq, x0, x1);
            const bool good = have && !ebad[g];
            const int r0 = good ? rs[g * (E + 1) + i] : 0;
            const int deg = good ? rs[g * (E + 1) + i + 1] - r0 : 0;
            const int64_t e0 = est[g] + r0;                  // the row's first entry in the edge arrays
            const int32_t *colp = p.ecol + e0;
            const float *attrp = p.edge_attr + e0;
            const uint32_t bE = (uint32_t)(b0 + g) * (uint32_t)E;
            const int64_t row = (int64_t)(b0 + g) * R + i;
            T gi, acc;
            for (int c = 0; c < kVec; ++c) {
                V::set(gi, c, 0.0f);
                V::set(acc, c, 0.0f);
            }
            float D = 0.0f, ls = 0.0f;
            if (live) {
                gi = *(const T *)(bp.grad_out + row * HC + ch);
                T om = *(const T *)(bp.out + row * HC + ch);
                if (p.skip) {
                    float ws[kVec][8];
                    conv_load_w<kVec>(p.w, 3, HC, ch, true, ws);
                    const T sk = conv_project<kVec>(ws, x0, x1);
                    for (int c = 0; c < kVec; ++c) V::set(om, c, V::get(om, c) - V::get(sk, c));
                }
#pragma unroll
                for (int c = 0; c < kVec; ++c) D += V::get(gi, c) * V::get(om, c);
                ls = bp.lse[row * H + head];
            }
#pragma unroll
            for (int o = 1; o < kLP; o <<= 1)
                if (o < lanes_per_head) D += __shfl_xor(D, o);
            int wdeg = deg;                                  // the wave runs its longest row
#pragma unroll
            for (int o = kLP; o < kWave; o <<= 1) wdeg = max(wdeg, __shfl_xor(wdeg, o));
            float U = 0.0f, A = 0.0f;
            int32_t jn = (live && deg > 0) ? colp[0] : 0;
            float wn = (live && deg > 0 && p.w_e) ? attrp[0] : 0.0f;
            for (int t = 0; t < wdeg; ++t) {
                const bool on = live && t < deg;
                const int jl = min(max((int)((uint32_t)jn - bE), 0), E - 1);   // checked by conv_stage_envs; clamped again
                const float w = wn;
                if (live && t + 1 < deg) {
                    jn = colp[t + 1];
                    if (p.w_e) wn = attrp[t + 1];
                }
                T kj, vj;
                for (int c = 0; c < kVec; ++c) {
                    V::set(kj, c, 0.0f);
                    V::set(vj, c, 0.0f);
                }
                if (on) {
                    if constexpr (kTable) {
                        kj = *(const T *)(ktab + (gE + jl) * HC + ch);
                        vj = *(const T *)(vtab + (gE + jl) * HC + ch);
                    } else {
                        const float4 y0 = *(const float4 *)(xs + (gE + jl) * 8),
                                     y1 = *(const float4 *)(xs + (gE + jl) * 8 + 4);
                        kj = conv_project<kVec>(wk, y0, y1);
                        vj = conv_project<kVec>(wv, y0, y1);
                    }
                }
                float sc = 0.0f, gm = 0.0f;
#pragma unroll
                for (int c = 0; c < kVec; ++c) {
                    sc += V::get(qi, c) * (V::get(kj, c) + w * V::get(we, c));
                    gm += V::get(gi, c) * (V::get(vj, c) + w * V::get(we, c));
                }
#pragma unroll
                for (int o = 1; o < kLP; o <<= 1)
                    if (o < lanes_per_head) {
                        sc += __shfl_xor(sc, o);
                        gm += __shfl_xor(gm, o);
                    }
                sc *= p.scale;
                const float a = on ? __expf(sc - ls) : 0.0f;
                const float ds = a * (gm - D);
#pragma unroll
                for (int c = 0; c < kVec; ++c)
                    V::set(acc, c, V::get(acc, c) + ds * (V::get(kj, c) + w * V::get(we, c)));
                U += w * ds;
                A += w * a;
                if (on && ch % C == 0) {
                    bp.wa[(e0 + t) * H + head] = a;
                    bp.wds[(e0 + t) * H + head] = ds;
                }
            }
#pragma unroll
            for (int c = 0; c < kVec; ++c) {
                stage[tid * kVec + c] = live ? V::get(acc, c) * p.scale : 0.0f;
                stage[(kConvThreads + tid) * kVec + c] = V::get(gi, c);
                if (live) V::set(dwe, c, V::get(dwe, c) + (p.scale * V::get(qi, c) * U + V::get(gi, c) * A));
            }
            __syncthreads();
            if (red && (ra == 0 || p.skip)) conv_bwd_accumulate<kLP, kVec>(rcol, xs, base, n_walk, R, E, racc, 2 * HC);
            __syncthreads();
        }
        // the barrier above also orders this workgroup's stores to work before the loads below

        // source pass
        for (int base = 0; base < n_loc; base += kNPP) {     // block-uniform trip count
            const int idx = base + slot;
            const bool have = idx < n_loc;
            const int id = have ? idx : 0;
            const int g = id / E, j = id - g * E, gE = g * E;
            const bool good = have && !ebad[g];              // every lane of the slot walks the row
            const int *rg = rs + g * (E + 1);
            const int r0 = good ? rg[j] : 0;
            const int deg = good ? rg[j + 1] - r0 : 0;
            const int32_t *ecol = p.ecol + est[g];           // the env's columns: positions [0, ecnt[g])
            const uint32_t bE = (uint32_t)(b0 + g) * (uint32_t)E;
            const int32_t self = (int32_t)(bE + (uint32_t)j);
            T ak, av;
            for (int c = 0; c < kVec; ++c) {
                V::set(ak, c, 0.0f);
                V::set(av, c, 0.0f);
            }
            int32_t in = deg > 0 ? ecol[r0] : 0;             // next entry's target fetched one iteration ahead
            for (int t = 0; t < deg; ++t) {
                const int il = min(max((int)((uint32_t)in - bE), 0), E - 1);   // checked by conv_stage_envs; clamped again
                if (t + 1 < deg) in = ecol[r0 + t + 1];
                // j inside row il: the slot's lanes count that row's columns below j and the
                // hits, every read inside the row's checked range [rg[il], rg[il + 1])
                const int lo = rg[il], hi = rg[il + 1];
                int cnt = 0;                                 // columns below j, hits << 16 (a row has < 2^16 entries)
                for (int x = lo + sub; x < hi; x += kLP) {
                    const int32_t cx = ecol[x];
                    cnt += (cx < self ? 1 : 0) + (cx == self ? 1 << 16 : 0);
                }
#pragma unroll
                for (int o = 1; o < kLP; o <<= 1) cnt += __shfl_xor(cnt, o);
                if (!(cnt >> 16)) {
                    bits |= GSM_BATCH_ASYMMETRIC;
                    continue;
                }
                if (il >= R || !chon) continue;              // not an output row: g_i = 0
                const int64_t e = (est[g] + lo + (cnt & 0xffff)) * H + head;
                const float a = bp.wa[e], ds = bp.wds[e];
                const float4 y0 = *(const float4 *)(xs + (gE + il) * 8), y1 = *(const float4 *)(xs + (gE + il) * 8 + 4);
                const T qi = conv_project<kVec>(wq, y0, y1);
                const T gi = *(const T *)(bp.grad_out + ((int64_t)(b0 + g) * R + il) * HC + ch);
#pragma unroll
                for (int c = 0; c < kVec; ++c) {
                    V::set(ak, c, V::get(ak, c) + ds * V::get(qi, c));
                    V::set(av, c, V::get(av, c) + a * V::get(gi, c));
                }
            }
#pragma unroll
            for (int c = 0; c < kVec; ++c) {
                stage[tid * kVec + c] = V::get(ak, c) * p.scale;
                stage[(kConvThreads + tid) * kVec + c] = V::get(av, c);
            }
            __syncthreads();
            if (red) conv_bwd_accumulate<kLP, kVec>(rcol, xs, base, n_loc, E, E, racc + 16 * HC, 2 * HC);
            __syncthreads();
        }
    }
    if (bits) atomicOr(p.status, bits);

    // this workgroup's partial: [nblk][HC][8], then dw_e [HC] summed in slot order
    const int nblk = p.skip ? 4 : 3;
    float *part = bp.part + (int64_t)blockIdx.x * (nblk * HC * 8 + HC);
    if (red) {
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            if (ra == 0 || p.skip) part[((ra ? 3 : 0) * HC + rc) * 8 + f] = racc[f * 2 * HC];
            part[((1 + ra) * HC + rc) * 8 + f] = racc[(8 + f) * 2 * HC];
        }
    }
#pragma unroll
    for (int c = 0; c < kVec; ++c) stage[tid * kVec + c] = V::get(dwe, c);
    __syncthreads();
    if (tid < HC) {
        float sum = 0.0f;
        if (bp.want_dwe)
            for (int s = 0; s < kNPP; ++s) sum += stage[(s * kLP + tid / kVec) * kVec + tid % kVec];
        part[nblk * HC * 8 + tid] = sum;
    }
}

int64_t env_conv_backward_work_floats(int64_t edge_limit, int heads, int HC, bool skip) {
    return 2 * edge_limit * heads + (int64_t)kConvBwdMaxBlocks * ((skip ? 4 : 3) * HC * 8 + HC);
}

hipError_t launch_env_conv_backward(const float *grad_out, const float *node_feat, const int64_t *edge_ptr,
                                    const int32_t *edge_index, int64_t edge_row_stride, const float *edge_attr,
                                    int64_t edge_limit, const float *w, const float *w_e, const float *out,
                                    const float *lse, int64_t B, int E, int HC, int C, float scale, bool skip,
                                    int n_rows_out, float *work, float *dw, float *dw_e, int32_t *status,
                                    hipStream_t s) {
    // the forward's choice of lanes, so that s_ij is formed in the forward's order
    const Lanes l = select_lanes(HC, C, aligned16({out, grad_out, w_e}));
    if (!l.ok) return hipErrorInvalidValue;
    const int H = HC / C, nblk = skip ? 4 : 3;
    ConvBwdParams bp;
    ConvParams &p = bp.f;
    p.node_feat = node_feat;
    p.edge_ptr = edge_ptr;
    p.erow = edge_index;
    p.ecol = edge_index ? edge_index + edge_row_stride : nullptr;
    p.edge_attr = edge_attr;
    p.edge_limit = edge_limit;
    p.w = w;
    p.w_e = w_e;
    p.B = (int)B;
    p.E = E;
    p.epb = E >= 64 ? 1 : 64 / E;
    p.HC = HC;
    p.C = C;
    p.skip = skip;
    p.n_rows_out = n_rows_out;
    p.scale = scale;
    p.out = nullptr;
    p.lse = nullptr;
    p.row_ptr_out = nullptr;
    p.status = status;
    bp.grad_out = grad_out;
    bp.out = out;
    bp.lse = lse;
    bp.wa = work;
    bp.wds = work + edge_limit * H;
    bp.part = work + 2 * edge_limit * H;
    bp.n_groups = (int)((B + p.epb - 1) / p.epb);
    bp.want_dwe = w_e && dw_e;
    // the table form when it fits with the stage, as launch_env_conv decides it
    const int stage = conv_bwd_stage_bytes(l.vec, HC);
    const bool table = conv_lds(p.epb, E, HC, true).total + stage <= kConvLdsMax;
    const size_t lds = (size_t)(conv_lds(p.epb, E, HC, table).total + stage);
    if (lds > (size_t)kConvLdsMax) return hipErrorInvalidValue;
    const int per_cu = min(table ? 3 : 2, max(1, kConvBwdLdsPerCu / (int)lds));
    const int cap = min(kConvBwdMaxBlocks, kConvBwdCus * per_cu);
    const unsigned blocks = (unsigned)(bp.n_groups < cap ? bp.n_groups : cap);
    (void)hipGetLastError();
    const hipError_t e = dispatch_lanes(l, [&](auto LP, auto VEC) {
        constexpr int kLP = decltype(LP)::value, kVec = decltype(VEC)::value;
        if (table) gsm_env_conv_bwd_kernel<kLP, kVec, true><<<blocks, kConvThreads, lds, s>>>(bp);
        else gsm_env_conv_bwd_kernel<kLP, kVec, false><<<blocks, kConvThreads, lds, s>>>(bp);
    });
    if (e != hipSuccess) return e;
    launch_partial_sum(bp.part, (int)blocks, {{nblk * HC * 8, dw}, {HC, dw_e}}, s);   // dw_e may be nullptr
    return hipGetLastError();
}

}  // namespace gsm
