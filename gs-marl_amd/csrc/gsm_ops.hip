// gsm_ops.hip — the stateless extern "C" entry points of libgsm.so (declared in
// include/gsm.h and include/gsm_optim.h): the kernels of the training chain on
// the caller's buffers and stream. Argument checks and one launcher call each;
// no handle, no allocation, no synchronisation.
#include <stdint.h>

#include "gsm.h"
#include "gsm_optim.h"
#include "gsm_host.h"
#include "gsm_internal.h"

extern "C" {

static int attn_forward(const float *q, const float *k, const float *v, const float *edge_w, const float *w_e,
                        const int64_t *row_ptr, const int32_t *col, const float *skip, int64_t n_nodes,
                        int32_t heads, int32_t channels, float scale, float *out, float *lse, bool want_lse,
                        void *stream, const char *what) {
    if (const int rc = nodes_range(n_nodes)) return rc;
    if (const int rc = heads_shape(heads, channels)) return rc;
    if (n_nodes == 0) return GSM_OK;
    if (!q || !k || !v || !row_ptr || !col || !out || (want_lse && !lse))
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    if (!!edge_w != !!w_e) return fail(nullptr, GSM_EINVAL, "edge_w and w_e go together");
    const hipError_t e = gsm::launch_attn_aggregate(q, k, v, edge_w, w_e, row_ptr, col, skip, n_nodes,
                                                    heads * channels, channels, scale, out, lse,
                                                    as_stream(stream));
    return launched(e, what);
}

int gsm_attn_aggregate(const float *q, const float *k, const float *v, const float *edge_w, const float *w_e,
                       const int64_t *row_ptr, const int32_t *col, const float *skip, int64_t n_nodes,
                       int32_t heads, int32_t channels, float scale, float *out, void *stream) {
    return attn_forward(q, k, v, edge_w, w_e, row_ptr, col, skip, n_nodes, heads, channels, scale, out, nullptr,
                        false, stream, "gsm_attn_aggregate launch");
}

int gsm_attn_aggregate_fwd(const float *q, const float *k, const float *v, const float *edge_w,
                           const float *w_e, const int64_t *row_ptr, const int32_t *col, const float *skip,
                           int64_t n_nodes, int32_t heads, int32_t channels, float scale, float *out, float *lse,
                           void *stream) {
    return attn_forward(q, k, v, edge_w, w_e, row_ptr, col, skip, n_nodes, heads, channels, scale, out, lse,
                        true, stream, "gsm_attn_aggregate_fwd launch");
}

int gsm_attn_backward_work_floats(int64_t n_nodes, int64_t n_edges, int32_t heads, int32_t channels,
                                  int64_t *n_floats) {
    if (const int rc = nodes_range(n_nodes)) return rc;
    if (const int rc = edges_range(n_edges)) return rc;
    if (const int rc = heads_shape(heads, channels)) return rc;
    if (!n_floats) return fail(nullptr, GSM_EINVAL, "n_floats is NULL");
    *n_floats = gsm::attn_backward_work_floats(n_edges, heads, heads * channels);
    return GSM_OK;
}

int gsm_attn_aggregate_bwd(const float *grad_out, const float *q, const float *k, const float *v,
                           const float *edge_w, const float *w_e, const int64_t *row_ptr, const int32_t *col,
                           const float *out, const float *skip, const float *lse, const int64_t *t_ptr,
                           const int32_t *t_edge, const int32_t *t_tgt, int64_t n_nodes, int64_t n_edges,
                           int32_t heads, int32_t channels, float scale, float *work, float *dq, float *dk,
                           float *dv, float *dedge_w, float *dw_e, void *stream) {
    if (const int rc = nodes_range(n_nodes)) return rc;
    if (const int rc = edges_range(n_edges)) return rc;
    if (const int rc = heads_shape(heads, channels)) return rc;
    if (n_nodes == 0 && n_edges > 0) return fail(nullptr, GSM_EINVAL, "edges without nodes");
    if (!!edge_w != !!w_e) return fail(nullptr, GSM_EINVAL, "edge_w and w_e go together");
    if (dedge_w && !edge_w) return fail(nullptr, GSM_EINVAL, "dedge_w needs edge_w");
    hipStream_t s = as_stream(stream);
    const size_t row = sizeof(float) * (size_t)(heads * channels);
    if (n_nodes == 0 || n_edges == 0) {
        // no edges: every gradient but dskip (= grad_out, the caller's) is 0
        if (n_nodes > 0 && (!dq || !dk || !dv)) return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
        const size_t all = row * (size_t)n_nodes;   // n_nodes == 0: dq, dk, dv are not looked at
        return launched(zero_all({{n_nodes ? dq : nullptr, all}, {n_nodes ? dk : nullptr, all},
                                  {n_nodes ? dv : nullptr, all}, {dw_e, row}}, s),
                        "gsm_attn_aggregate_bwd memset");
    }
    if (!grad_out || !q || !k || !v || !row_ptr || !col || !out || !lse || !t_ptr || !t_edge || !t_tgt || !work ||
        !dq || !dk || !dv)
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    const hipError_t e = gsm::launch_attn_backward(grad_out, q, k, v, edge_w, w_e, row_ptr, col, out, skip, lse, t_ptr, t_edge,
                                  t_tgt, n_nodes, n_edges, heads * channels, channels, scale, work, dq, dk, dv,
                                  dedge_w, dw_e, s);
    return launched(e, "gsm_attn_aggregate_bwd launch");
}

static int graph_batch_shape(int64_t n_slots, int64_t n_envs, int64_t edge_capacity, int64_t n_samples) {
    const int64_t lim = (int64_t)1 << 31;
    if (n_samples < 0 || n_samples >= lim) return fail(nullptr, GSM_EINVAL, "n_samples must be in [0, 2^31)");
    if (n_slots < 1 || n_slots >= lim || n_envs < 1 || n_envs >= lim)
        return fail(nullptr, GSM_EINVAL, "n_slots and n_envs must be in [1, 2^31)");
    if (edge_capacity < 0 || edge_capacity >= lim)
        return fail(nullptr, GSM_EINVAL, "edge_capacity must be in [0, 2^31)");
    return GSM_OK;
}

int gsm_graph_batch_ptr(const int64_t *edge_ptr, int64_t n_slots, int64_t n_envs, int64_t edge_capacity,
                        const int64_t *t_idx, const int64_t *b_idx, int64_t n_samples, int64_t *sample_ptr,
                        int32_t *status, void *stream) {
    if (const int rc = graph_batch_shape(n_slots, n_envs, edge_capacity, n_samples)) return rc;
    if (!sample_ptr || !status) return fail(nullptr, GSM_EINVAL, "sample_ptr or status is NULL");
    if (n_samples > 0 && (!edge_ptr || !t_idx || !b_idx))
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    const hipError_t e = gsm::launch_graph_batch_ptr(edge_ptr, n_slots, n_envs, edge_capacity, t_idx, b_idx,
                                                     n_samples, sample_ptr, status, as_stream(stream));
    return launched(e, "gsm_graph_batch_ptr launch");
}

int gsm_graph_batch_gather(const float *node_feat, const int32_t *edge_index, const float *edge_attr,
                           const int64_t *edge_ptr, int64_t n_slots, int64_t n_envs, int32_t n_entities,
                           int64_t edge_capacity, const int64_t *t_idx, const int64_t *b_idx,
                           const int64_t *sample_ptr, int64_t n_samples, int64_t n_edges, float *node_feat_out,
                           int64_t *row_ptr, int32_t *col, float *edge_attr_out, int32_t *t_edge,
                           int32_t *status, void *stream) {
    if (const int rc = graph_batch_shape(n_slots, n_envs, edge_capacity, n_samples)) return rc;
    const int64_t lim = (int64_t)1 << 31;
    if (n_entities < 1 || n_samples * n_entities >= lim || n_envs * n_entities >= lim)
        return fail(nullptr, GSM_EINVAL, "n_entities >= 1; n_samples*n_entities and n_envs*n_entities < 2^31");
    if (n_edges < 0 || n_edges >= lim) return fail(nullptr, GSM_EINVAL, "n_edges must be in [0, 2^31)");
    if (!row_ptr || !status) return fail(nullptr, GSM_EINVAL, "row_ptr or status is NULL");
    if (n_samples > 0 && (!node_feat || !edge_index || !edge_attr || !edge_ptr || !t_idx || !b_idx ||
                          !sample_ptr || !node_feat_out))
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    if (n_edges > 0 && (!col || !edge_attr_out)) return fail(nullptr, GSM_EINVAL, "col or edge_attr_out is NULL");
    if (n_samples == 0 && n_edges > 0) return fail(nullptr, GSM_EINVAL, "edges without samples");
    hipStream_t s = as_stream(stream);
    if (n_samples == 0) {
        const hipError_t e = hipMemsetAsync(row_ptr, 0, sizeof(int64_t), s);
        return launched(e, "gsm_graph_batch_gather memset");
    }
    const hipError_t e = gsm::launch_graph_batch_gather(node_feat, edge_index, edge_attr, edge_ptr, n_slots, n_envs,
                                                        n_entities, edge_capacity, t_idx, b_idx, sample_ptr,
                                                        n_samples, n_edges, node_feat_out, row_ptr, col,
                                                        edge_attr_out, t_edge, status, s);
    return launched(e, "gsm_graph_batch_gather launch");
}

// the shape limits the fused first layer's forward and backward share
static int env_conv_shape(int64_t n_envs, int32_t n_entities, int64_t edge_limit, int64_t edge_row_stride,
                          int32_t heads, int32_t channels, int32_t flags, int32_t n_rows_out) {
    const int64_t lim = (int64_t)1 << 31;
    if (const int rc = heads_shape(heads, channels)) return rc;
    if (n_entities < 1 || n_entities > GSM_CONV_MAX_ENTITIES)
        return fail(nullptr, GSM_EINVAL, "n_entities must be in [1, 288]");
    if (n_envs < 0 || n_envs >= lim || n_envs * n_entities >= lim)
        return fail(nullptr, GSM_EINVAL, "n_envs >= 0 and n_envs*n_entities < 2^31");
    if (n_rows_out < 1 || n_rows_out > n_entities)
        return fail(nullptr, GSM_EINVAL, "n_rows_out must be in [1, n_entities]");
    if (edge_limit < 0 || edge_limit >= lim) return fail(nullptr, GSM_EINVAL, "edge_limit must be in [0, 2^31)");
    if (edge_row_stride < edge_limit) return fail(nullptr, GSM_EINVAL, "edge_row_stride must be >= edge_limit");
    if (flags & ~GSM_CONV_SKIP) return fail(nullptr, GSM_EINVAL, "unknown flags");
    return GSM_OK;
}

static int env_conv_forward(const float *node_feat, const int64_t *edge_ptr, const int32_t *edge_index,
                            int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit, const float *w,
                            const float *w_e, int64_t n_envs, int32_t n_entities, int32_t heads, int32_t channels,
                            float scale, int32_t flags, int32_t n_rows_out, float *out, float *lse, bool want_lse,
                            int64_t *row_ptr_out, int32_t *status, void *stream, const char *what) {
    if (const int rc = env_conv_shape(n_envs, n_entities, edge_limit, edge_row_stride, heads, channels, flags,
                                      n_rows_out))
        return rc;
    if (!status) return fail(nullptr, GSM_EINVAL, "status is NULL");
    hipStream_t s = as_stream(stream);
    if (n_envs == 0) {
        if (row_ptr_out) {
            const hipError_t e = hipMemsetAsync(row_ptr_out, 0, sizeof(int64_t), s);
            if (e != hipSuccess) return hip_fail(nullptr, e, "gsm_env_conv memset");
        }
        return GSM_OK;
    }
    if (!node_feat || !edge_ptr || !w || !out || (want_lse && !lse))
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    if (edge_limit > 0 && (!edge_index || (w_e && !edge_attr)))
        return fail(nullptr, GSM_EINVAL, "edge_index or edge_attr is NULL");
    if ((uintptr_t)w % 16) return fail(nullptr, GSM_EINVAL, "w must be 16-byte aligned");
    const hipError_t e = gsm::launch_env_conv(node_feat, edge_ptr, edge_index, edge_row_stride, edge_attr, edge_limit,
                                              w, w_e, n_envs, n_entities, heads * channels, channels, scale,
                                              (flags & GSM_CONV_SKIP) != 0, n_rows_out, out, lse, row_ptr_out,
                                              status, s);
    return launched(e, what);
}

int gsm_env_conv(const float *node_feat, const int64_t *edge_ptr, const int32_t *edge_index,
                 int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit, const float *w,
                 const float *w_e, int64_t n_envs, int32_t n_entities, int32_t heads, int32_t channels, float scale,
                 int32_t flags, int32_t n_rows_out, float *out, int64_t *row_ptr_out, int32_t *status,
                 void *stream) {
    return env_conv_forward(node_feat, edge_ptr, edge_index, edge_row_stride, edge_attr, edge_limit, w, w_e, n_envs,
                            n_entities, heads, channels, scale, flags, n_rows_out, out, nullptr, false, row_ptr_out,
                            status, stream, "gsm_env_conv launch");
}

int gsm_env_conv_fwd(const float *node_feat, const int64_t *edge_ptr, const int32_t *edge_index,
                     int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit, const float *w,
                     const float *w_e, int64_t n_envs, int32_t n_entities, int32_t heads, int32_t channels,
                     float scale, int32_t flags, int32_t n_rows_out, float *out, float *lse, int64_t *row_ptr_out,
                     int32_t *status, void *stream) {
    return env_conv_forward(node_feat, edge_ptr, edge_index, edge_row_stride, edge_attr, edge_limit, w, w_e, n_envs,
                            n_entities, heads, channels, scale, flags, n_rows_out, out, lse, true, row_ptr_out,
                            status, stream, "gsm_env_conv_fwd launch");
}

int gsm_env_conv_backward_work_floats(int64_t n_envs, int32_t n_entities, int64_t edge_limit, int32_t heads,
                                      int32_t channels, int32_t flags, int64_t *n_floats) {
    if (const int rc = env_conv_shape(n_envs, n_entities, edge_limit, edge_limit, heads, channels, flags, 1)) return rc;
    if (!n_floats) return fail(nullptr, GSM_EINVAL, "n_floats is NULL");
    *n_floats = gsm::env_conv_backward_work_floats(edge_limit, heads, heads * channels, (flags & GSM_CONV_SKIP) != 0);
    return GSM_OK;
}

int gsm_env_conv_bwd(const float *grad_out, const float *node_feat, const int64_t *edge_ptr,
                     const int32_t *edge_index, int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit,
                     const float *w, const float *w_e, const float *out, const float *lse, int64_t n_envs,
                     int32_t n_entities, int32_t heads, int32_t channels, float scale, int32_t flags,
                     int32_t n_rows_out, float *work, float *dw, float *dw_e, int32_t *status, void *stream) {
    if (const int rc = env_conv_shape(n_envs, n_entities, edge_limit, edge_row_stride, heads, channels, flags,
                                      n_rows_out))
        return rc;
    if (!status || !dw) return fail(nullptr, GSM_EINVAL, "status or dw is NULL");
    if (dw_e && !w_e) return fail(nullptr, GSM_EINVAL, "dw_e needs w_e");
    hipStream_t s = as_stream(stream);
    const bool skip = (flags & GSM_CONV_SKIP) != 0;
    const size_t row = sizeof(float) * (size_t)(heads * channels);
    if (n_envs == 0) {
        return launched(zero_all({{dw, row * 8 * (skip ? 4 : 3)}, {dw_e, row}}, s), "gsm_env_conv_bwd memset");
    }
    if (!grad_out || !node_feat || !edge_ptr || !w || !out || !lse || !work)
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    if (edge_limit > 0 && (!edge_index || (w_e && !edge_attr)))
        return fail(nullptr, GSM_EINVAL, "edge_index or edge_attr is NULL");
    if ((uintptr_t)w % 16) return fail(nullptr, GSM_EINVAL, "w must be 16-byte aligned");
    const hipError_t e = gsm::launch_env_conv_backward(grad_out, node_feat, edge_ptr, edge_index, edge_row_stride,
                                                       edge_attr, edge_limit, w, w_e, out, lse, n_envs, n_entities,
                                                       heads * channels, channels, scale, skip, n_rows_out, work,
                                                       dw, dw_e, status, s);
    return launched(e, "gsm_env_conv_bwd launch");
}

// the shape limits of the actor head, before anything else is looked at
static int actor_shape(int64_t x_row_stride, int64_t n_envs, int32_t n_agents, int32_t in_features, int32_t hidden,
                       int32_t n_actions) {
    const int64_t lim = (int64_t)1 << 31;
    if (in_features < 4 || in_features > 128 || in_features % 4)
        return fail(nullptr, GSM_EINVAL, "in_features must be a multiple of 4 in [4, 128]");
    if (hidden != 0 && hidden != 16 && hidden != 32 && hidden != 64)
        return fail(nullptr, GSM_EINVAL, "hidden must be 0, 16, 32 or 64");
    if (n_actions < 2 || n_actions > 8) return fail(nullptr, GSM_EINVAL, "n_actions must be in [2, 8]");
    if (n_agents < 1 || n_envs < 0 || n_envs >= lim || n_envs * n_agents >= lim)
        return fail(nullptr, GSM_EINVAL, "n_agents >= 1, n_envs >= 0 and n_envs*n_agents < 2^31");
    if (x_row_stride < in_features || x_row_stride % 4)
        return fail(nullptr, GSM_EINVAL, "x_row_stride must be a multiple of 4 and >= in_features");
    return GSM_OK;
}

static int head_pointers(const float *x, const float *w1, const float *b1, const float *w2, const float *b2,
                          int32_t hidden) {
    if (!x || !w2 || !b2 || (hidden && (!w1 || !b1))) return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    if ((uintptr_t)x % 16) return fail(nullptr, GSM_EINVAL, "x must be 16-byte aligned");
    return GSM_OK;
}

static gsm::ActorParams actor_params(const float *x, int64_t x_row_stride, const float *w1, const float *b1,
                                     const float *w2, const float *b2, int64_t n_envs, int32_t n_agents,
                                     int32_t in_features, int32_t n_actions, int32_t *status) {
    gsm::ActorParams p = {};
    p.x = x;
    p.x_stride = x_row_stride;
    p.w1 = w1, p.b1 = b1, p.w2 = w2, p.b2 = b2;
    p.R = (int)(n_envs * n_agents);
    p.n_agents = n_agents;
    p.in = in_features;
    p.nA = n_actions;
    p.status = status;
    return p;
}

int gsm_actor_sample(const float *x, int64_t x_row_stride, const float *w1, const float *b1, const float *w2,
                     const float *b2, int64_t n_envs, int32_t n_agents, int32_t in_features, int32_t hidden,
                     int32_t n_actions, uint64_t seed, int64_t env_base, int64_t draw_host, const int64_t *draw_dev,
                     int32_t flags, int32_t *actions, float *logp, float *entropy, float *logits_out,
                     int32_t *status, void *stream) {
    if (const int rc = actor_shape(x_row_stride, n_envs, n_agents, in_features, hidden, n_actions)) return rc;
    if (flags & ~GSM_ACTOR_DETERMINISTIC) return fail(nullptr, GSM_EINVAL, "unknown flags");
    if (n_envs == 0) return GSM_OK;
    if (const int rc = head_pointers(x, w1, b1, w2, b2, hidden)) return rc;
    if (!actions || !logp) return fail(nullptr, GSM_EINVAL, "actions or logp is NULL");
    gsm::ActorParams p = actor_params(x, x_row_stride, w1, b1, w2, b2, n_envs, n_agents, in_features, n_actions,
                                      status);
    p.k0 = (uint32_t)seed, p.k1 = (uint32_t)(seed >> 32);
    p.env_base = env_base, p.draw_host = draw_host, p.draw_dev = draw_dev;
    p.deterministic = (flags & GSM_ACTOR_DETERMINISTIC) != 0;
    p.actions_out = actions, p.logp = logp, p.entropy = entropy, p.logits_out = logits_out;
    const hipError_t e = gsm::launch_actor_forward(p, hidden, false, as_stream(stream));
    return launched(e, "gsm_actor_sample launch");
}

int gsm_actor_eval(const float *x, int64_t x_row_stride, const float *w1, const float *b1, const float *w2,
                   const float *b2, int64_t n_envs, int32_t n_agents, int32_t in_features, int32_t hidden,
                   int32_t n_actions, const int32_t *actions, float *logp, float *entropy, int32_t *status,
                   void *stream) {
    if (const int rc = actor_shape(x_row_stride, n_envs, n_agents, in_features, hidden, n_actions)) return rc;
    if (n_envs == 0) return GSM_OK;
    if (const int rc = head_pointers(x, w1, b1, w2, b2, hidden)) return rc;
    if (!actions || !logp) return fail(nullptr, GSM_EINVAL, "actions or logp is NULL");
    gsm::ActorParams p = actor_params(x, x_row_stride, w1, b1, w2, b2, n_envs, n_agents, in_features, n_actions,
                                      status);
    p.actions_in = actions, p.logp = logp, p.entropy = entropy;
    const hipError_t e = gsm::launch_actor_forward(p, hidden, true, as_stream(stream));
    return launched(e, "gsm_actor_eval launch");
}

int gsm_actor_backward_work_floats(int32_t in_features, int32_t hidden, int32_t n_actions, int64_t *n_floats) {
    if (const int rc = actor_shape(in_features, 0, 1, in_features, hidden, n_actions)) return rc;
    if (!n_floats) return fail(nullptr, GSM_EINVAL, "n_floats is NULL");
    *n_floats = gsm::actor_backward_work_floats(in_features, hidden, n_actions);
    return GSM_OK;
}

int gsm_actor_eval_bwd(const float *g_logp, const float *g_ent, const float *x, int64_t x_row_stride,
                       const float *w1, const float *b1, const float *w2, const float *b2, int64_t n_envs,
                       int32_t n_agents, int32_t in_features, int32_t hidden, int32_t n_actions,
                       const int32_t *actions, float *work, float *dw1, float *db1, float *dw2, float *db2,
                       float *dx, int32_t *status, void *stream) {
    if (const int rc = actor_shape(x_row_stride, n_envs, n_agents, in_features, hidden, n_actions)) return rc;
    if (!dw2 || !db2 || (hidden && (!dw1 || !db1))) return fail(nullptr, GSM_EINVAL, "a gradient pointer is NULL");
    hipStream_t s = as_stream(stream);
    if (n_envs == 0) {
        const size_t f = sizeof(float);
        return launched(zero_all({{dw2, f * n_actions * (hidden ? hidden : in_features)},
                                  {db2, f * n_actions},
                                  {hidden ? dw1 : nullptr, f * hidden * in_features},
                                  {hidden ? db1 : nullptr, f * hidden}}, s),
                        "gsm_actor_eval_bwd memset");
    }
    if (const int rc = head_pointers(x, w1, b1, w2, b2, hidden)) return rc;
    if (!g_logp || !actions || !work) return fail(nullptr, GSM_EINVAL, "g_logp, actions or work is NULL");
    if ((uintptr_t)dx % 16) return fail(nullptr, GSM_EINVAL, "dx must be 16-byte aligned");
    gsm::ActorParams p = actor_params(x, x_row_stride, w1, b1, w2, b2, n_envs, n_agents, in_features, n_actions,
                                      status);
    p.actions_in = actions, p.g_logp = g_logp, p.g_ent = g_ent, p.dx = dx, p.part = work;
    const hipError_t e = gsm::launch_actor_backward(p, hidden, dw1, db1, dw2, db2, s);
    return launched(e, "gsm_actor_eval_bwd launch");
}

// the shape limits of the critic head, before anything else is looked at
static int critic_shape(int64_t x_row_stride, int64_t n_envs, int32_t n_agents, int32_t in_features, int32_t hidden,
                        int32_t n_out) {
    const int64_t lim = (int64_t)1 << 31;
    if (in_features < 4 || in_features > 64 || in_features % 4)
        return fail(nullptr, GSM_EINVAL, "in_features must be a multiple of 4 in [4, 64]");
    if (hidden != 16 && hidden != 32 && hidden != 64) return fail(nullptr, GSM_EINVAL, "hidden must be 16, 32 or 64");
    if (n_out < 1 || n_out > 2) return fail(nullptr, GSM_EINVAL, "n_out must be 1 or 2");
    if (n_agents < 1 || n_agents > 128 || n_envs < 0 || n_envs >= lim || n_envs * n_agents >= lim)
        return fail(nullptr, GSM_EINVAL, "n_agents in [1, 128], n_envs >= 0 and n_envs*n_agents < 2^31");
    if (x_row_stride < in_features || x_row_stride % 4)
        return fail(nullptr, GSM_EINVAL, "x_row_stride must be a multiple of 4 and >= in_features");
    return GSM_OK;
}

static gsm::CriticParams critic_params(const float *x, int64_t x_row_stride, const int32_t *n_valid, const float *w1,
                                       const float *b1, const float *w2, const float *b2, int64_t n_envs,
                                       int32_t n_agents, int32_t in_features, int32_t n_out, int32_t *status) {
    gsm::CriticParams p = {};
    p.x = x;
    p.x_stride = x_row_stride;
    p.n_valid = n_valid;
    p.w1 = w1, p.b1 = b1, p.w2 = w2, p.b2 = b2;
    p.n_envs = n_envs;
    p.R = n_envs * n_agents;
    p.n_agents = n_agents;
    p.in = in_features;
    p.nO = n_out;
    p.status = status;
    return p;
}

int gsm_critic_eval(const float *x, int64_t x_row_stride, const int32_t *n_valid, const float *w1, const float *b1,
                    const float *w2, const float *b2, const float *denorm, int64_t n_envs, int32_t n_agents,
                    int32_t in_features, int32_t hidden, int32_t n_out, float *values, int32_t *status,
                    void *stream) {
    if (const int rc = critic_shape(x_row_stride, n_envs, n_agents, in_features, hidden, n_out)) return rc;
    if (n_envs == 0) return GSM_OK;
    if (const int rc = head_pointers(x, w1, b1, w2, b2, hidden)) return rc;
    if (!values) return fail(nullptr, GSM_EINVAL, "values is NULL");
    gsm::CriticParams p = critic_params(x, x_row_stride, n_valid, w1, b1, w2, b2, n_envs, n_agents, in_features,
                                        n_out, status);
    p.denorm = denorm, p.values = values;
    const hipError_t e = gsm::launch_critic_forward(p, hidden, as_stream(stream));
    return launched(e, "gsm_critic_eval launch");
}

int gsm_critic_backward_work_floats(int32_t in_features, int32_t hidden, int32_t n_out, int64_t *n_floats) {
    if (const int rc = critic_shape(in_features, 0, 1, in_features, hidden, n_out)) return rc;
    if (!n_floats) return fail(nullptr, GSM_EINVAL, "n_floats is NULL");
    *n_floats = gsm::critic_backward_work_floats(in_features, hidden, n_out);
    return GSM_OK;
}

int gsm_critic_eval_bwd(const float *g, const float *x, int64_t x_row_stride, const int32_t *n_valid,
                        const float *w1, const float *b1, const float *w2, const float *b2, int64_t n_envs,
                        int32_t n_agents, int32_t in_features, int32_t hidden, int32_t n_out, float *work,
                        float *dw1, float *db1, float *dw2, float *db2, float *dx, int32_t *status, void *stream) {
    if (const int rc = critic_shape(x_row_stride, n_envs, n_agents, in_features, hidden, n_out)) return rc;
    if (!dw1 || !db1 || !dw2 || !db2) return fail(nullptr, GSM_EINVAL, "a gradient pointer is NULL");
    hipStream_t s = as_stream(stream);
    if (n_envs == 0) {
        const size_t f = sizeof(float);
        return launched(zero_all({{dw2, f * n_out * hidden}, {db2, f * n_out}, {dw1, f * hidden * 2 * in_features},
                                  {db1, f * hidden}}, s),
                        "gsm_critic_eval_bwd memset");
    }
    if (const int rc = head_pointers(x, w1, b1, w2, b2, hidden)) return rc;
    if (!g || !work) return fail(nullptr, GSM_EINVAL, "g or work is NULL");
    if ((uintptr_t)dx % 16) return fail(nullptr, GSM_EINVAL, "dx must be 16-byte aligned");
    gsm::CriticParams p = critic_params(x, x_row_stride, n_valid, w1, b1, w2, b2, n_envs, n_agents, in_features,
                                        n_out, status);
    p.g = g, p.dx = dx, p.part = work;
    const hipError_t e = gsm::launch_critic_backward(p, hidden, dw1, db1, dw2, db2, s);
    return launched(e, "gsm_critic_eval_bwd launch");
}

int gsm_ppo_loss_work_floats(int64_t n_rows, int64_t *n_floats) {
    if (n_rows < 0 || n_rows >= ((int64_t)1 << 31)) return fail(nullptr, GSM_EINVAL, "n_rows must be in [0, 2^31)");
    if (!n_floats) return fail(nullptr, GSM_EINVAL, "n_floats is NULL");
    *n_floats = gsm::ppo_loss_work_floats();
    return GSM_OK;
}

int gsm_ppo_loss(const float *logp, const float *ent, const float *values, const float *logp_old, const float *adv,
                 const float *v_old, const float *ret, const float *weight, const int32_t *n_valid, int64_t n_envs,
                 int32_t n_agents, int32_t n_out, const float *multiplier, float clip, float value_clip,
                 float ent_coef, float value_coef, float *work, float *loss, float *stats, float *g_logp,
                 float *g_ent, float *g_values, int32_t *status, void *stream) {
    const int64_t lim = (int64_t)1 << 31;
    // the shape limits, before anything else is looked at
    if (n_out < 1 || n_out > 2) return fail(nullptr, GSM_EINVAL, "n_out must be 1 or 2");
    if (n_agents < 1 || n_envs < 0 || n_envs >= lim || n_envs * n_agents >= lim)
        return fail(nullptr, GSM_EINVAL, "n_agents >= 1, n_envs >= 0 and n_envs*n_agents < 2^31");
    if (n_out == 2 && !multiplier) return fail(nullptr, GSM_EINVAL, "multiplier is NULL with n_out == 2");
    if (!work || !loss || !stats) return fail(nullptr, GSM_EINVAL, "work, loss or stats is NULL");
    const int n_g = (g_logp != nullptr) + (g_ent != nullptr) + (g_values != nullptr);
    if (n_g != 0 && n_g != 3) return fail(nullptr, GSM_EINVAL, "g_logp, g_ent and g_values: all or none");
    if (n_envs > 0 && (!logp || !ent || !values || !logp_old || !adv || !v_old || !ret))
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    gsm::LossParams p = {};
    p.logp = logp, p.ent = ent, p.values = values, p.logp_old = logp_old;
    p.adv = adv, p.v_old = v_old, p.ret = ret, p.weight = weight;
    p.n_valid = n_valid;
    p.lam = multiplier;
    p.R = n_envs * n_agents;
    p.n_agents = n_agents, p.nO = n_out;
    p.ratio_lo = (float)(1.0 - (double)clip), p.ratio_hi = (float)(1.0 + (double)clip);
    p.value_clip = value_clip, p.ent_coef = ent_coef, p.value_coef = value_coef;
    p.work = work, p.loss = loss, p.stats = stats;
    p.g_logp = g_logp, p.g_ent = g_ent, p.g_values = g_values;
    p.status = status;
    const hipError_t e = gsm::launch_ppo_loss(p, as_stream(stream));
    return launched(e, "gsm_ppo_loss launch");
}

int gsm_adam_work_floats(int64_t n_tensors, int64_t total_elements, int64_t *n_floats) {
    if (n_tensors < 0 || total_elements < 0) return fail(nullptr, GSM_EINVAL, "n_tensors and total_elements >= 0");
    if (!n_floats) return fail(nullptr, GSM_EINVAL, "n_floats is NULL");
    *n_floats = gsm::adam_work_floats(n_tensors, total_elements);
    return GSM_OK;
}

int gsm_adam_step(float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *n,
                  int64_t n_tensors, const float *lr, int32_t *step, double beta1, double beta2, double eps,
                  float max_norm, float *work, float *stats, int32_t *status, void *stream) {
    static_assert(GSM_OPT_NONFINITE == gsm::kOptNonfinite, "the status bit of gsm_optim.h");
    const int64_t lim = (int64_t)1 << 31;
    if (n_tensors < 0) return fail(nullptr, GSM_EINVAL, "n_tensors must be >= 0");
    if (n_tensors > 0 && (!p || !g || !m || !v || !n)) return fail(nullptr, GSM_EINVAL, "a tensor array is NULL");
    for (int64_t i = 0; i < n_tensors; ++i) {
        if (n[i] < 0 || n[i] >= lim) return fail(nullptr, GSM_EINVAL, "every n[i] must be in [0, 2^31)");
        if (n[i] > 0 && (!p[i] || !g[i] || !m[i] || !v[i]))
            return fail(nullptr, GSM_EINVAL, "a pointer of a tensor with elements is NULL");
    }
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
        return fail(nullptr, GSM_EINVAL, "beta1 and beta2 must be in [0, 1)");
    if (!(eps >= 0.0) || !(max_norm >= 0.0f)) return fail(nullptr, GSM_EINVAL, "eps and max_norm must be >= 0");
    if (!lr || !step || !work || !stats) return fail(nullptr, GSM_EINVAL, "lr, step, work or stats is NULL");
    if ((uintptr_t)work % 8) return fail(nullptr, GSM_EINVAL, "work must be 8-byte aligned");
    gsm::OptScalars sc = {};
    sc.beta1 = beta1, sc.beta2 = beta2, sc.eps = eps, sc.max_norm = max_norm;
    const hipError_t e = gsm::launch_adam_step(p, g, m, v, n, n_tensors, sc, lr, step, work, stats, status,
                                               as_stream(stream));
    return launched(e, "gsm_adam_step launch");
}

int gsm_gae(const float *reward, const float *value, const uint8_t *done, int64_t n_steps, int64_t n_envs,
            int32_t n_agents, float gamma, float gamma_lambda, float *ret, void *stream) {
    const int64_t lim = (int64_t)1 << 31;
    if (n_steps < 1 || n_steps >= lim) return fail(nullptr, GSM_EINVAL, "n_steps must be in [1, 2^31)");
    if (n_envs < 1 || n_agents < 1 || n_envs >= lim || n_envs * n_agents >= lim)
        return fail(nullptr, GSM_EINVAL, "n_envs, n_agents >= 1 and n_envs*n_agents < 2^31");
    if (!reward || !value || !done || !ret) return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    const hipError_t e = gsm::launch_gae(reward, value, done, n_steps, n_envs, n_agents, gamma, gamma_lambda, ret,
                                         as_stream(stream));
    return launched(e, "gsm_gae launch");
}

int gsm_render(const float *node_feat, int64_t n_envs, int32_t n_entities, const int64_t *edge_ptr,
               const int32_t *edge_index, int64_t edge_capacity, const int32_t *env_ids, int32_t n_frames,
               float half_width, float agent_size, float target_size, float obstacle_size, int32_t width,
               int32_t height, int32_t flags, uint8_t *rgba, void *stream) {
    if (n_frames < 0 || n_frames > 65535) return fail(nullptr, GSM_EINVAL, "n_frames must be in [0, 65535]");
    if (width < 1 || height < 1 || width > 8192 || height > 8192)
        return fail(nullptr, GSM_EINVAL, "width and height must be in [1, 8192]");
    if (n_entities < 1 || n_entities > 4096) return fail(nullptr, GSM_EINVAL, "n_entities must be in [1, 4096]");
    if (n_envs < 1) return fail(nullptr, GSM_EINVAL, "n_envs must be >= 1");
    if (!(agent_size >= 0.0f && target_size >= 0.0f && obstacle_size >= 0.0f))
        return fail(nullptr, GSM_EINVAL, "sizes must be >= 0");
    if (n_frames == 0) return GSM_OK;
    const bool edges = (flags & GSM_RENDER_EDGES) != 0;
    if (!node_feat || !env_ids || !rgba || (edges && (!edge_ptr || !edge_index || edge_capacity < 1)))
        return fail(nullptr, GSM_EINVAL, "a required pointer is NULL");
    if ((uintptr_t)rgba & 3) return fail(nullptr, GSM_EINVAL, "rgba must be 4-byte aligned");
    const hipError_t e = gsm::launch_render(node_feat, n_envs, n_entities, edge_ptr, edge_index, edge_capacity,
                                            env_ids, n_frames, half_width, agent_size, target_size,
                                            obstacle_size, width, height, edges ? 1 : 0, rgba,
                                            as_stream(stream));
    return launched(e, "gsm_render launch");
}

}  // extern "C"
