/*
 * gsm.h — C ABI of libgsm.so, the MI355X (gfx950) batched step path of
 * GS-MARL's MultiAgentGraphConstrainEnv.
 *
 * Drop-in boundary. The reference has no FFI: its boundary is the Python
 * env classes in gsmarl/envs/mpe_env/multiagent/environment.py
 * (/root/reference/GSMARL.egg-info/SOURCES.txt:15; contracts at
 * /root/reference/readme.md:29-41), constructed by make_env.py
 * (SOURCES.txt:12) and called from the vec-env workers (SOURCES.txt:11).
 * The reference sources are absent (readme.md:1), so each entry point below
 * cites the reference interface it replaces at the granularity available.
 * The binding a maintainer adds on the reference side (ctypes) is shown in
 * INTEGRATION.md; the in-tree binding is gs-marl_amd/gsmarl_amd/_lib.py.
 *
 * Rules of the ABI:
 *  - plain C types only; pointers to device memory are owned by the caller
 *    (PyTorch allocates them) and merely borrowed by the library;
 *  - nothing is allocated and nothing synchronises inside gsm_step /
 *    gsm_reset / gsm_observe, so they can be captured into a HIP graph;
 *  - every call returns GSM_OK (0) or a negative gsm_status; no C++
 *    exception crosses the boundary; gsm_last_error() has the message;
 *  - a handle is used from one host thread at a time (the GIL serialises);
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default).
 */
#ifndef GSM_H_
#define GSM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: lagged-emission graph chains (GSM_GRAPH_UNFUSED / _LAG_ONLY), gsm_render
 * 5: degenerate-state handling: gsm_config.strict_degenerate,
 *    gsm_buffers.degenerate */
/* 6: fused rollout graphs (GSM_GRAPH_ROLL, gsm_graph_roll_status, gsm_graph_info)
 * 7: gsm_get_state / gsm_set_state; rollout graphs emit every step's edges in
 *    their one launch (no separate emit launch)
 * 8: ragged rollouts (n_steps <= 4094), gsm_graph_roll_placement */
#define GSM_ABI_VERSION 8

typedef enum gsm_status {
    GSM_OK = 0,
    GSM_EINVAL = -1,   /* bad argument / config                        */
    GSM_EHIP = -2,     /* HIP runtime error (message has hipError_t)    */
    GSM_ESTATE = -3,   /* call out of order (e.g. step before bind)     */
} gsm_status;

typedef enum gsm_scenario {
    GSM_SCEN_NAVIGATION = 0,   /* scenarios/exp1.py|exp2.py (SOURCES.txt:21-22)          */
    GSM_SCEN_POLYGON = 1,      /* scenarios/simple_formation.py (SOURCES.txt:24; readme.md:89) */
    GSM_SCEN_LINE = 2,         /* scenarios/simple_line.py (SOURCES.txt:25; readme.md:90)      */
    GSM_SCEN_MIXED = 3,        /* env id mod 3 -> navigation/polygon/line, N per env drawn   */
} gsm_scenario;

/* Ragged batches (polygon, line, mixed): every env has its own agent count
 * N_env <= n_agents (= N_max <= GSM_RAGGED_MAX_AGENTS) and its own scenario,
 * stored padded: entity rows agents [0, N_max), targets [N_max, N_max+T_max),
 * obstacles [N_max+T_max, E). env_shape[b] = N_env | scenario << 8. */
#define GSM_RAGGED_MAX_AGENTS 32

typedef enum gsm_action_fmt {
    GSM_ACT_ONEHOT = 0,   /* float32 [B][N][5]; u = [a1-a2, a3-a4] (MPE discrete_action_space) */
    GSM_ACT_INDEX = 1,    /* int32   [B][N];    same mapping as the one-hot of the index        */
    GSM_ACT_CONT = 2,     /* float32 [B][N][2]; u = a (continuous)                              */
} gsm_action_fmt;

/* Launch modes of the step kernel (gsm_observe / gsm_reset reuse it). */
typedef enum gsm_mode {
    GSM_MODE_STEP = 0,
    GSM_MODE_RESET = 1,
    GSM_MODE_OBSERVE = 2,
} gsm_mode;

/* Environment configuration; mirrors gsmarl_amd.config.EnvConfig 1:1.
 * Replaces the env part of gsmarl/config.py (SOURCES.txt:7, readme.md:47)
 * and the constants of core.py / the scenario files. */
typedef struct gsm_config {
    int32_t abi_version;      /* = GSM_ABI_VERSION                           */
    int32_t scenario;         /* gsm_scenario                                */
    int32_t n_envs;           /* B: env instances held by this handle        */
    int32_t n_agents;         /* N (goals = N)                               */
    int32_t n_obstacles;      /* No                                          */
    int32_t episode_length;   /* readme.md:101 -> 100                        */
    int32_t auto_reset;       /* reset an env in-kernel when its episode ends */
    int32_t shared_reward;    /* every agent gets the sum of rewards         */
    int64_t env_base;         /* global id of env 0 (sharding; Philox key)   */
    uint64_t seed;
    float dt, damping, mass, contact_force, contact_margin, sensitivity;
    float max_speed;          /* <= 0: no clamp (MPE max_speed = None)       */
    float world_half;         /* L: layout box is [-L, L]^2                  */
    float agent_size, goal_size, obstacle_size;
    float sense_radius;       /* R: graph edge radius                        */
    float contact_cutoff;     /* skip pair force when d - dmin > cutoff*k     */
    /* ragged scenarios (ignored by navigation) */
    int32_t n_agents_min;     /* mixed: N_env drawn from [n_agents_min, n_agents] */
    float formation_radius;   /* polygon: N-gon radius (readme.md:89 -> 0.5)  */
    /* App. A S16. A coincident collider pair (d = 0, at least one agent) has
     * no direction: by default its contact force is guarded to zero; with
     * strict_degenerate != 0 it is NaN as in MPE's get_collision_force
     * (delta / dist with dist = 0), and, as MPE evaluates every pair, an
     * agent whose position is NaN makes the force of every agent of its env
     * NaN. Either way the env is flagged in gsm_buffers.degenerate. */
    int32_t strict_degenerate;
} gsm_config;

/* Sizes the caller must allocate (gsm_query_sizes). */
typedef struct gsm_sizes {
    int32_t n_entities;       /* E = 2N + No                                 */
    int32_t node_feat_dim;    /* 7                                           */
    int32_t obs_dim;          /* 6                                           */
    int32_t envs_per_block;   /* envs handled by one step-kernel workgroup   */
    int32_t n_blocks;         /* length of block_edge_sum                    */
    int32_t max_edges_per_env;
    int64_t edge_capacity;    /* length of edge_attr and of each edge_index row */
    int32_t n_colliders;      /* M: collider rows per env (agents + obstacles)  */
    int32_t n_targets;        /* T_max: goal/landmark rows per env            */
    int32_t mask_words;       /* W: uint64 words per mask row, ceil(M / 64)   */
} gsm_sizes;

/* Caller-owned device buffers (all contiguous, row-major). */
typedef struct gsm_buffers {
    /* state */
    float *pos;               /* [B][E][2]   agents, goals/landmarks, obstacles */
    float *vel;               /* [B][N][2]   agents only (landmarks immovable) */
    int32_t *step_count;      /* [B]         steps since reset                */
    int32_t *episode;         /* [B]         episode index (-1 before reset)  */
    float *ep_acc;            /* [B][2]      running (sum reward, sum cost)   */
    float *ep_last;           /* [B][2]      totals of the last finished episode */
    /* outputs of the last reset/step/observe */
    float *node_feat;         /* [B][E][7]   vx vy px py gx-px gy-py type     */
    float *reward;            /* [B][N]                                       */
    float *cost;              /* [B][N]      collision counts (exact ints)    */
    uint8_t *done;            /* [B]                                          */
    int32_t *edge_count;      /* [B]                                          */
    int32_t *block_edge_sum;  /* [n_blocks]  scratch                          */
    int64_t *edge_ptr;        /* [B+1]       CSR offsets into edge arrays     */
    int32_t *edge_index;      /* [2][edge_capacity] global node ids (b*E+e)   */
    float *edge_attr;         /* [edge_capacity]    distance                  */
    /* derived state, valid for the positions in `pos` after any reset/step/
     * observe; a caller that rewrites `pos`/`vel` must call gsm_observe      */
    uint64_t *row_mask;       /* [B][M][W] radius adjacency rows (bit = collider) */
    uint64_t *contact_mask;   /* [B][N][W] contact candidates of each agent        */
    /* ragged scenarios only (may be NULL for navigation) */
    int32_t *env_shape;       /* [B]    N_env | scenario << 8 (set at every layout) */
    int32_t *assign;          /* [B][N] polygon/line slot of each agent (LSA), -1 else */
    /* optional (NULL: not written): per env, after every reset/step/observe,
     * GSM_DEGENERATE_COINCIDENT if two colliders (at least one an agent) sit
     * at the same position — the next step meets d = 0 — and
     * GSM_DEGENERATE_NONFINITE if an agent position is not finite (strict
     * mode, or a caller-written state) */
    uint8_t *degenerate;      /* [B] */
    /* optional, polygon/line assignment warm start (NULL: every per-step
     * assignment is solved from scratch): the column duals and the matching
     * of each env's last assignment, kept by the library between launches.
     * A warm-started assignment is used only when certified to be the unique
     * optimum — then it IS scipy's result; otherwise the scipy recurrence runs
     * from scratch. Initialise lsa_col to -1 (lsa_v to 0).
     * The buffers need not belong to the state (set_state does not carry
     * them, and they survive resets): any contents are safe. lsa_col entries
     * outside [0, N_env) count as "no column"; a cache with a dual that is
     * non-finite or exceeds 4096 in magnitude is not used, and no assignment
     * is certified with such a dual (at larger duals float64 rounding of the
     * reduced costs reaches the certificate's 1e-9 margin). Such an env is
     * solved from scratch, which rewrites its cache. */
    double *lsa_v;            /* [B][N], |v| <= 4096 to be used */
    int32_t *lsa_col;         /* [B][N] */
    int32_t *lsa_stats;       /* [B][2] optional counters: certified warm starts, assignments solved */
} gsm_buffers;

#define GSM_DEGENERATE_COINCIDENT 1
#define GSM_DEGENERATE_NONFINITE 2

/* Output redirection (an on-device rollout buffer
 * filled without copies). Where one step / observe writes its outputs; NULL
 * members keep the bound buffers. edge_index is [2][edge_capacity] when
 * redirected; edges past edge_capacity are not written, while edge_ptr keeps
 * the true offsets (edge_ptr[B] > edge_capacity flags the overflow). A
 * redirected launch writes full node-feature rows (goal / obstacle rows are
 * otherwise rewritten only when a layout changes). */
typedef struct gsm_outputs {
    float *node_feat;         /* [B][E][7] */
    float *reward;            /* [B][N]    */
    float *cost;              /* [B][N]    */
    uint8_t *done;            /* [B]       */
    int32_t *edge_count;      /* [B]       */
    int64_t *edge_ptr;        /* [B+1]     */
    int32_t *edge_index;      /* [2][edge_capacity] */
    float *edge_attr;         /* [edge_capacity]    */
    int32_t *assign;          /* [B][N]  (ragged scenarios) */
    int64_t edge_capacity;
} gsm_outputs;

typedef struct gsm_handle gsm_handle;

int gsm_abi_version(void);

/* Validates cfg and fills sizes. Host-only, no HIP call. */
int gsm_query_sizes(const gsm_config *cfg, gsm_sizes *out);

/* Replaces make_env(scenario) -> MultiAgentGraphConstrainEnv(world, ...)
 * (make_env.py, SOURCES.txt:12; environment.py, SOURCES.txt:15). Host-only. */
int gsm_create(const gsm_config *cfg, gsm_handle **out);

/* Borrow caller-allocated device buffers (sizes from gsm_query_sizes). */
int gsm_bind(gsm_handle *h, const gsm_buffers *bufs);

/* Replaces env.reset() -> scenario.reset_world(world) (environment.py /
 * scenario.py, SOURCES.txt:15,19). reseed != 0: episode counters restart
 * and `seed` becomes the layout key. env_mask: device uint8 [B] or NULL
 * (= all envs). Outputs are recomputed for every env. */
int gsm_reset(gsm_handle *h, uint64_t seed, int reseed, const uint8_t *env_mask, void *stream);

/* Replaces env.step(action_n) (environment.py, SOURCES.txt:15): _set_action,
 * world.step() (core.py, SOURCES.txt:14), reward/cost/done callbacks and the
 * graph observation, for all B envs. actions: device pointer in action_fmt.
 * One kernel launch (the config's rollout kernel with one step) at 6-24
 * navigation agents, else a step kernel + an emit kernel; GSM_EAGER_ONE_LAUNCH=0
 * (read at gsm_bind) is the switch to the two launches everywhere. Same
 * outputs either way. */
int gsm_step(gsm_handle *h, const void *actions, int action_fmt, void *stream);

/* Recompute every output for the current state (after the caller rewrote
 * state buffers, e.g. set_state). */
int gsm_observe(gsm_handle *h, void *stream);

/* The simulator state (SURVEY.md §8(b) gsm_get_state / gsm_set_state):
 * device pointers of the caller; NULL members are skipped. Everything else
 * the library keeps (the row / contact masks, node features, edges) is
 * derived from it. */
typedef struct gsm_state {
    float *pos;               /* [B][E][2] */
    float *vel;               /* [B][N][2] */
    int32_t *step_count;      /* [B]       */
    int32_t *episode;         /* [B]       */
    float *ep_acc;            /* [B][2]    */
    float *ep_last;           /* [B][2]    */
    int32_t *env_shape;       /* [B]       ragged scenarios: N_env | scenario << 8 */
} gsm_state;

/* Checkpoint / injection of env state (what a reference caller does by
 * reading or writing the world's entity states directly, core.py
 * EntityState, SOURCES.txt:14). gsm_get_state copies the bound state into
 * `out`. gsm_set_state copies `in` into the bound state and then runs
 * gsm_observe, which re-derives every output and the derived per-position
 * state (row masks, contact candidates) the next step relies on — the one
 * call a non-Python caller needs after writing positions or velocities.
 * Stream-ordered device-to-device copies; no synchronisation. */
int gsm_get_state(gsm_handle *h, const gsm_state *out, void *stream);
int gsm_set_state(gsm_handle *h, const gsm_state *in, void *stream);

/* gsm_step / gsm_observe with their outputs redirected (gsm_outputs). */
int gsm_step_into(gsm_handle *h, const void *actions, int action_fmt, const gsm_outputs *out, void *stream);
int gsm_observe_into(gsm_handle *h, const gsm_outputs *out, void *stream);

/* Build HIP graph `slot` (0..GSM_GRAPH_SLOTS-1) of n_steps steps; the j-th
 * step reads its actions at actions + (j % n_actions) * action_stride_bytes.
 * flags: which kernels each step runs (GSM_GRAPH_STEP | GSM_GRAPH_EMIT; 0 =
 * both) and optional HIP event-record nodes: GSM_GRAPH_TIME_EACH brackets
 * every kernel, GSM_GRAPH_TIME_ENDS brackets the whole graph (per-kernel
 * means over back-to-back launches, no event nodes between kernels).
 * A graph running only GSM_GRAPH_EMIT re-emits the current step's edges.
 * Segmented (navigation, N + No <= 64) and ragged (polygon / line / mixed)
 * configs chain the two kernels with lagged emission: step j+1's kernel first emits step j's edges (they depend
 * only on its input positions and row masks), so a step is one launch and a
 * final emit launch ends the graph; every step's outputs are complete when
 * the graph has run, exactly as with the two-kernel chain (the library
 * allocates one n_blocks int32 buffer for this on first use).
 * GSM_GRAPH_UNFUSED forces the two-kernel chain (TIME_EACH implies it);
 * GSM_GRAPH_LAG_ONLY builds n_steps lagged step kernels and nothing else
 * (a timing tool: the last step's edges are left unemitted; segmented / ragged only).
 * Graphs are dropped by gsm_bind and by a reseed to a different seed. */
#define GSM_GRAPH_SLOTS 4
#define GSM_GRAPH_STEP 1
#define GSM_GRAPH_EMIT 2
#define GSM_GRAPH_TIME_EACH 4
#define GSM_GRAPH_TIME_ENDS 8
#define GSM_GRAPH_UNFUSED 16
#define GSM_GRAPH_LAG_ONLY 32
/* GSM_GRAPH_ROLL: all n_steps (<= 4094) steps and their edges run in ONE
 * launch (navigation configs with a compiled rollout shape — 3, 6, 12 or 24
 * agents with as many obstacles, one env per wave — the tile path, one env
 * per workgroup, and ragged batches, one env per wave; the whole batch in one
 * residency round). Each wave keeps its
 * env's state on chip across the steps; workgroups hand the CSR edge-count
 * prefix to each other through tagged granules (bounded waits), and a tail
 * iteration emits the last step's edges. Outputs after the graph are
 * identical to the lagged chain's (every step's edges are emitted; in the
 * bound buffers the earlier steps' go to a library scratch of the bound edge
 * capacity, allocated on first use, since a workgroup may trail its
 * successors by steps). Combines with GSM_GRAPH_TIME_ENDS only (the events
 * then bracket the launch: gsm_graph_kernel_ms gives its time per step);
 * GSM_EINVAL where the config has no rollout kernel, where the action rows
 * span 4 GiB or more (n_actions * action_stride_bytes >= 2^32: the rollout
 * kernels address them with 32-bit offsets), where n_steps > 4094, or where
 * the batch exceeds one residency round of the rollout kernel (occupancy x
 * CUs; on an MI355X 8192 envs of the one-env-per-wave and ragged rollouts —
 * 2048 workgroups, also the bound of the one-hop CSR prefix's 64 chunk sums of
 * 64 workgroups — 16384 of the packed small-env rollout, 1024 of the tile
 * rollout; shard larger batches across handles or GPUs, env_base). Without
 * GSM_GRAPH_ROLL such a capture takes the per-step chain instead. */
#define GSM_GRAPH_ROLL 64
int gsm_graph_capture(gsm_handle *h, int32_t slot, const void *actions, int64_t action_stride_bytes,
                      int32_t n_actions, int32_t n_steps, int action_fmt, int flags);
/* As gsm_graph_capture (both kernels, no timing events), with the j-th
 * step's outputs redirected to per_step[j] (n_steps entries). Where the config
 * has a rollout kernel (GSM_GRAPH_ROLL) and every redirected field of the
 * slots sits at a constant stride (a rollout buffer), the graph is one rollout
 * launch writing step j's outputs into slot j; else the per-step chain. */
int gsm_graph_capture_into(gsm_handle *h, int32_t slot, const void *actions, int64_t action_stride_bytes,
                           int32_t n_actions, int32_t n_steps, int action_fmt, const gsm_outputs *per_step);
/* Launch the graph in `slot` on `stream` (stream-ordered, asynchronous). A
 * rollout slot (GSM_GRAPH_ROLL, or a rollout buffer's single launch) holds a
 * kernel launch, not a hipGraph: the stored kernel is dispatched with a fresh
 * launch epoch for its hand-off tags and its half of the slot's chunk sums and
 * pacing counters (the environment knobs of the rollouts: INTEGRATION.md,
 * "Environment knobs"); so it cannot be recorded into a
 * stream capture (GSM_ESTATE on a capturing stream: capture the per-step chain
 * instead). The rollout slots of a handle share its state and scratch, so their
 * launches never overlap: a launch on a different stream than the handle's
 * previous rollout launch first waits, on the device, for an event the library
 * records behind every rollout launch (no host synchronisation; the previous
 * stream may have been destroyed since). */
int gsm_graph_launch(gsm_handle *h, int32_t slot, void *stream);
/* The graph in `slot`: its step count (0 if none) and whether it is one
 * fused rollout launch (GSM_GRAPH_ROLL, or gsm_graph_capture_into on a
 * rollout buffer) rather than a per-step chain. */
int gsm_graph_info(gsm_handle *h, int32_t slot, int32_t *steps, int32_t *fused);
/* After graph launches have completed: *gave_up = a non-zero reason code if
 * any bounded in-launch wait timed out (1: a rollout launch's CSR hand-off, or
 * the ragged lagged chain's staging wait) or an in-launch check failed (2: an
 * out-of-range CSR offset, 4: a doubly claimed env, 5: a placement slot
 * outside its table; 6, in a checked build (-DGSM_CHECKED): a hand-off granule
 * or slab address outside its allocation) since the last call (that launch's
 * outputs are then invalid), else 0. Clears the flag. Synchronises (reads a
 * device word). */
int gsm_graph_roll_status(gsm_handle *h, int32_t *gave_up);
/* Ragged mixed rollouts deal their envs to the SIMDs by estimated cost when
 * every wave of the launch is resident (else env = wave index; same outputs
 * either way). After launches have completed: how many dealt their envs and
 * how many fell back since the last call. Clears the counts; synchronises. */
int gsm_graph_roll_placement(gsm_handle *h, int64_t *dealt, int64_t *fallback);
/* After a timed launch of `slot` has completed: mean duration (ms) of the
 * step and emit kernels (TIME_EACH), and the whole graph (both flags). */
int gsm_graph_kernel_ms(gsm_handle *h, int32_t slot, float *step_mean_ms, float *emit_mean_ms,
                        float *total_ms);

/* Graph-attention message passing over a CSR graph (SURVEY.md §8(f) next #3:
 * the GNN encoder after the observation; replaces the edge-softmax /
 * aggregation of torch-geometric's TransformerConv, requirements.txt:119, as
 * used by the reference's GNN in gsmarl/algorithms, SOURCES.txt:8). For each
 * target i with sources j = col[row_ptr[i] .. row_ptr[i+1]), per head h:
 *   e_ij = edge_w[ij] * w_e[h*C + c]           (edge_w, w_e may be NULL: e = 0)
 *   a_ij = softmax_j(scale * <q_i[h], k_j[h] + e_ij>)
 *   out_i[h] = sum_j a_ij (v_j[h] + e_ij) + skip_i[h]      (skip may be NULL)
 * q, k, v, skip, out: device f32 [n_nodes][heads*channels]; row_ptr: int64
 * [n_nodes+1]; col: int32 source ids; channels a power of two and
 * heads*channels <= 64. Stateless; asynchronous on `stream`. */
int gsm_attn_aggregate(const float *q, const float *k, const float *v, const float *edge_w, const float *w_e,
                       const int64_t *row_ptr, const int32_t *col, const float *skip, int64_t n_nodes,
                       int32_t heads, int32_t channels, float scale, float *out, void *stream);
/* The same launch and the same `out`, and the row softmax statistics the
 * backward needs: lse[i][h] = max_j s_ij + log(sum_j exp(s_ij - max)), device
 * f32 [n_nodes][heads] (an empty row stores 0, which is never read). */
int gsm_attn_aggregate_fwd(const float *q, const float *k, const float *v, const float *edge_w,
                           const float *w_e, const int64_t *row_ptr, const int32_t *col, const float *skip,
                           int64_t n_nodes, int32_t heads, int32_t channels, float scale, float *out, float *lse,
                           void *stream);

/* Gradients of gsm_attn_aggregate. With m_ij = v_j + e_ij, s_ij the scaled
 * score and g_i = grad_out[i] (dskip = grad_out is left to the caller):
 *   D_i[h]   = <g_i[h], out_i[h] - skip_i[h]>
 *   ds_ij[h] = a_ij[h] * (<g_i[h], m_ij[h]> - D_i[h]),  a_ij = exp(s_ij - lse_i)
 *   dq_i[h]  = scale * sum_j ds_ij[h] (k_j[h] + e_ij[h])
 *   dk_j[h]  = scale * sum_{i: j in row i} ds_ij[h] q_i[h]
 *   dv_j[h]  =         sum_{i: j in row i} a_ij[h]  g_i[h]
 *   de_ij[c] = scale * ds_ij[h(c)] q_i[c] + a_ij[h(c)] g_i[c]
 *   dw_e[c]  = sum_ij edge_w[ij] de_ij[c],   dedge_w[ij] = sum_c de_ij[c] w_e[c]
 * out, lse: what gsm_attn_aggregate_fwd wrote for the same inputs. The sums
 * over the rows that contain j run over the transposed graph: t_ptr int64
 * [n_nodes+1] offsets per source, t_edge int32 [n_edges] the CSR entry ids
 * grouped by source (ascending within a source), t_tgt int32 [n_edges] each
 * listed entry's target row. work: device f32, gsm_attn_backward_work_floats
 * of them (a_ij and ds_ij per entry and head, and the dw_e block partials).
 * dq, dk, dv: f32 [n_nodes][heads*channels], every row written (a node that
 * is nobody's source gets dk = dv = 0); dedge_w f32 [n_edges] and dw_e f32
 * [heads*channels] may be NULL (not wanted). No atomics: the outputs are
 * bitwise reproducible. Shape limits as the forward; n_edges < 2^31; with
 * n_nodes == 0 or n_edges == 0 the gradients are zeros. Stateless;
 * asynchronous on `stream`. */
int gsm_attn_backward_work_floats(int64_t n_nodes, int64_t n_edges, int32_t heads, int32_t channels,
                                  int64_t *n_floats);
int gsm_attn_aggregate_bwd(const float *grad_out, const float *q, const float *k, const float *v,
                           const float *edge_w, const float *w_e, const int64_t *row_ptr, const int32_t *col,
                           const float *out, const float *skip, const float *lse, const int64_t *t_ptr,
                           const int32_t *t_edge, const int32_t *t_tgt, int64_t n_nodes, int64_t n_edges,
                           int32_t heads, int32_t channels, float scale, float *work, float *dq, float *dk,
                           float *dv, float *dedge_w, float *dw_e, void *stream);

/* Minibatch assembly from a rollout buffer (the
 * reader side): K samples (slot t_idx[k], env b_idx[k]) of stored env graphs
 * as one CSR batch for gsm_attn_aggregate*, with the transposed graph the
 * backward wants. The buffer: edge_ptr int64 [n_slots][n_envs+1] (per-slot CSR
 * offsets), edge_index int32 [n_slots][2][edge_capacity] (global ids
 * b*n_entities + e, rows in ascending source order), edge_attr f32
 * [n_slots][edge_capacity], node_feat f32 [n_slots][n_envs][n_entities][7].
 *
 * gsm_graph_batch_ptr (one launch, one workgroup): sample_ptr int64
 * [n_samples+1] = exclusive scan of the samples' entry counts. A sample whose
 * indices are out of range, whose slot range runs past edge_capacity (a
 * truncated slot) or whose offsets are not 0 <= start <= end counts 0 entries
 * and ORs a bit into status (device int32 [1], zeroed by the caller).
 *
 * gsm_graph_batch_gather (one launch, one wave per sample; n_edges =
 * sample_ptr[n_samples], read back by the caller to size the outputs):
 *   node_feat_out f32 [n_samples*n_entities][7]  the samples' rows, bit for bit
 *   row_ptr int64 [n_samples*n_entities+1]       per-node offsets (a node's is
 *                                                the lower bound of its id in
 *                                                the sample's source list)
 *   col int32 [n_edges]                          targets' column ids relabelled
 *                                                b*E + e -> k*E + e
 *   edge_attr_out f32 [n_edges]
 *   t_edge int32 [n_edges], or NULL              for entry p in row j with column
 *                                                i: the position of j inside row
 *                                                i (a binary search)
 * For the env's graphs (symmetric, columns ascending without duplicates inside
 * a row) the transposed CSR of gsm_attn_aggregate_bwd is t_ptr = row_ptr,
 * t_edge, t_tgt = col. An entry with an id outside its env's [b*E, (b+1)*E)
 * sets GSM_BATCH_OUT_OF_ENV and gets its column clamped into the sample; one
 * whose reverse entry is missing sets GSM_BATCH_ASYMMETRIC; both get t_edge[p]
 * = p. The offsets are checked again here (a sample whose sample_ptr range is
 * not its entry count inside [0, n_edges] writes no entries and sets
 * GSM_BATCH_BAD_OFFSETS; a bad sample's node rows are zeros), and every search
 * stays inside the sample's entries. n_samples*n_entities, n_envs*n_entities
 * and n_edges must be below 2^31. Both are stateless and asynchronous on
 * `stream`; arguments are checked on the host first (GSM_EINVAL). */
#define GSM_BATCH_BAD_INDEX 1    /* a slot or env index out of range            */
#define GSM_BATCH_TRUNCATED 2    /* a sample's slot overflowed edge_capacity    */
#define GSM_BATCH_BAD_OFFSETS 4  /* offsets not 0 <= start <= end / scan mismatch */
#define GSM_BATCH_OUT_OF_ENV 8   /* an entry's id outside its env               */
#define GSM_BATCH_ASYMMETRIC 16  /* an entry's reverse entry is missing         */
int gsm_graph_batch_ptr(const int64_t *edge_ptr, int64_t n_slots, int64_t n_envs, int64_t edge_capacity,
                        const int64_t *t_idx, const int64_t *b_idx, int64_t n_samples, int64_t *sample_ptr,
                        int32_t *status, void *stream);
int gsm_graph_batch_gather(const float *node_feat, const int32_t *edge_index, const float *edge_attr,
                           const int64_t *edge_ptr, int64_t n_slots, int64_t n_envs, int32_t n_entities,
                           int64_t edge_capacity, const int64_t *t_idx, const int64_t *b_idx,
                           const int64_t *sample_ptr, int64_t n_samples, int64_t n_edges, float *node_feat_out,
                           int64_t *row_ptr, int32_t *col, float *edge_attr_out, int32_t *t_edge,
                           int32_t *status, void *stream);

/* One TransformerConv layer (in_channels = 7, edge_dim = 1, concat) straight
 * from the env-form graph of a live env or of one rollout-buffer slot: the
 * projections q, k, v (and skip) and the attention of gsm_attn_aggregate in
 * one launch, an env kept on chip. node_feat f32 [n_envs][n_entities][7];
 * edge_ptr int64 [n_envs+1]; edge_index int32, row 0 (targets) at edge_index
 * and row 1 (sources) at edge_index + edge_row_stride, global ids
 * b*n_entities + e, an env's entries sorted by (row, col); edge_attr f32;
 * edge_limit: the valid entries of the edge arrays (the bound capacity, or a
 * slot's). w f32 [3 or 4][heads*channels][8], 16-byte aligned: the blocks q,
 * k, v and, with GSM_CONV_SKIP, skip; columns 0-6 of a row the weights of the
 * 7 features, column 7 the bias. w_e f32 [heads*channels] or NULL (no edge
 * term). For entry p of env b, i = row - bE, j = col - bE, per head h:
 *   q_i, k_j, v_j, skip_i: acc = bias; acc = acc + W[c][f] * x[f], f = 0..6,
 *                          one fp32 operation a step, in that order
 *   e_ij = edge_attr[p] * w_e[c];  a_ij = softmax_j(scale * <q_i[h], k_j[h] + e_ij>)
 *   out_i[h] = sum_j a_ij (v_j[h] + e_ij) + skip_i[h]
 * the row's entries in ascending order, no float atomics (bitwise
 * reproducible); an empty row gives skip_i, or exactly 0 without skip.
 * out f32 [n_envs][n_rows_out][heads*channels]: the first n_rows_out rows of
 * every env (n_entities: all, n_agents: the agents). row_ptr_out int64
 * [n_envs*n_entities+1] or NULL: the per-node offsets into the edge arrays
 * (row_ptr of gsm_attn_aggregate for a further layer). Every offset read is
 * checked before use, into status (device int32 [1], zeroed by the caller):
 * an env whose range is not 0 <= start <= end sets GSM_BATCH_BAD_OFFSETS, one
 * whose range runs past edge_limit GSM_BATCH_TRUNCATED, one with a row or col
 * outside [bE, (b+1)E) or a row below its predecessor's GSM_BATCH_OUT_OF_ENV;
 * such an env is treated as edgeless (its rows get skip_i or 0, its
 * row_ptr_out entries repeat its start clamped into [0, edge_limit]). Shape
 * limits: channels a power of two, heads*channels <= 64, n_entities <= 288,
 * n_envs*n_entities and edge_limit < 2^31, edge_row_stride >= edge_limit
 * (GSM_EINVAL). Stateless; asynchronous on `stream`. */
#define GSM_CONV_SKIP 1
#define GSM_CONV_MAX_ENTITIES 288
int gsm_env_conv(const float *node_feat, const int64_t *edge_ptr, const int32_t *edge_index,
                 int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit, const float *w,
                 const float *w_e, int64_t n_envs, int32_t n_entities, int32_t heads, int32_t channels, float scale,
                 int32_t flags, int32_t n_rows_out, float *out, int64_t *row_ptr_out, int32_t *status,
                 void *stream);
/* The same launch and the same `out`, bit for bit, and the row softmax
 * statistics the backward needs: lse f32 [n_envs][n_rows_out][heads], the
 * row's max_j s_ij + log(sum_j exp(s_ij - max)); an empty row, or a row of an
 * env treated as edgeless, stores 0, which is never read. */
int gsm_env_conv_fwd(const float *node_feat, const int64_t *edge_ptr, const int32_t *edge_index,
                     int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit, const float *w,
                     const float *w_e, int64_t n_envs, int32_t n_entities, int32_t heads, int32_t channels,
                     float scale, int32_t flags, int32_t n_rows_out, float *out, float *lse, int64_t *row_ptr_out,
                     int32_t *status, void *stream);

/* Gradients of gsm_env_conv with respect to its weights (node_feat and
 * edge_attr are env data and get none). grad_out f32
 * [n_envs][n_rows_out][heads*channels]; out, lse: what gsm_env_conv_fwd wrote
 * for the same inputs; the graph arguments, w, w_e, the shape, scale, flags
 * and n_rows_out as in the forward. With g_i = grad_out of row i (0 for the
 * rows i >= n_rows_out), x_i the node's seven features and a trailing 1, and
 * the formulas of gsm_attn_aggregate_bwd over an env's entries (m_ij = v_j +
 * e_ij, a_ij = exp(s_ij - lse_i), s_ij in the forward's operation order):
 *   D_i[h]   = <g_i[h], out_i[h] - skip_i[h]>
 *   ds_ij[h] = a_ij[h] * (<g_i[h], m_ij[h]> - D_i[h])
 *   dq_i[h]  = scale * sum_j ds_ij[h] (k_j[h] + e_ij[h])
 *   dk_j[h]  = scale * sum_{i: j in row i} ds_ij[h] q_i[h]
 *   dv_j[h]  =         sum_{i: j in row i} a_ij[h]  g_i[h]
 *   dW_q[c][f]    = sum_i dq_i[c] x_i[f]     dW_k[c][f] = sum_j dk_j[c] x_j[f]
 *   dW_skip[c][f] = sum_i g_i[c]  x_i[f]     dW_v[c][f] = sum_j dv_j[c] x_j[f]
 *   dw_e[c]       = sum_ij edge_attr[ij] (scale * ds_ij[h(c)] q_i[c] + a_ij[h(c)] g_i[c])
 * the sums over every node of every env (a padding row of a ragged batch has
 * zero features and reaches the bias column only). dw f32 [3 or 4][heads*
 * channels][8] in the layout of w (column 7 the bias gradient); dw_e f32
 * [heads*channels] or NULL (not wanted; it needs w_e). work: device f32,
 * gsm_env_conv_backward_work_floats of them (a_ij and ds_ij per entry position
 * and head, and one partial per workgroup).
 * The backward trusts no forward: every edge_ptr pair, every id and the row
 * order are checked again exactly as gsm_env_conv checks them, into status
 * (the same GSM_BATCH_* bits), and an env that fails is edgeless here as it
 * was there: its rows reach dW_skip only, so the result is the gradient of
 * what the forward computed. The sums over the rows that contain j use the
 * env graph's symmetry (columns ascending without duplicates inside a row, so
 * row j lists exactly the targets that list j): node j walks its own row and
 * finds itself inside row i by counting the columns below j over that row's
 * checked range, never outside it (no symmetry is needed by the forward).
 * Every entry's reverse entry is looked for; a missing one sets
 * GSM_BATCH_ASYMMETRIC and contributes nothing. No float atomics; the
 * summation order depends on the shape alone, so dw and dw_e are bitwise
 * reproducible. The forward's shape limits (GSM_EINVAL); with n_envs == 0 the
 * gradients are zeros. Stateless; asynchronous on `stream`. */
int gsm_env_conv_backward_work_floats(int64_t n_envs, int32_t n_entities, int64_t edge_limit, int32_t heads,
                                      int32_t channels, int32_t flags, int64_t *n_floats);
int gsm_env_conv_bwd(const float *grad_out, const float *node_feat, const int64_t *edge_ptr,
                     const int32_t *edge_index, int64_t edge_row_stride, const float *edge_attr, int64_t edge_limit,
                     const float *w, const float *w_e, const float *out, const float *lse, int64_t n_envs,
                     int32_t n_entities, int32_t heads, int32_t channels, float scale, int32_t flags,
                     int32_t n_rows_out, float *work, float *dw, float *dw_e, int32_t *status, void *stream);

/* The actor head: policy features -> MLP -> categorical distribution -> the
 * sampled action and its log-probability (the rollout) or log-probability and
 * entropy of stored actions with their gradients (the PPO / Lagrangian
 * update), one launch each. Rows r = b*n_agents + i, R = n_envs*n_agents.
 * x f32, row r at x + r*x_row_stride (floats; x_row_stride >= in_features and
 * a multiple of 4, the base 16-byte aligned: a view of gsm_env_conv's out
 * works). w1 f32 [hidden][in_features], b1 [hidden], w2 [n_actions][hidden],
 * b2 [n_actions] (the torch.nn.Linear layout):
 *   h = relu(W1 x + b1);  logits l = W2 h + b2
 * hidden == 0 is a linear head: w2 [n_actions][in_features], w1 = b1 = NULL.
 * Every dot product is one accumulation chain of explicit fmaf (one rounding
 * a step; the library is built with -ffp-contract=off, nothing else fuses)
 * that starts from the bias and takes the inputs in ascending index; relu(v)
 * = v < 0 ? 0 : v. The same chain in all three entry points.
 * The distribution, one correctly ordered fp32 operation a line:
 *   m = max_a l_a;  e_a = expf(l_a - m);  s = e_0 + e_1 + .. (ascending)
 *   logp_a = (l_a - m) - logf(s)
 *   entropy = logf(s) - (sum_a e_a * (l_a - m)) / s   (the sum ascending)
 * The draw: one Philox4x32-10 call per row, counter = (i, (uint32)draw,
 * (uint32)(env_base + b), kTagPolicy = 3), key = (seed lo32, seed hi32), u =
 * (x0 >> 8) * 2^-24; draw = draw_host + (draw_dev ? *draw_dev : 0), draw_dev a
 * device int64 [1] the kernel only reads (a counter a captured graph advances
 * on the device). A shard with env_base = b0 draws what rows b0.. of the full
 * batch draw. The sample: t = u * s; c = 0; for a ascending c = c + e_a; the
 * action is the first a with t < c, n_actions - 1 if none (u * s can round up
 * to s). With GSM_ACTOR_DETERMINISTIC the action is the lowest index that
 * attains m and nothing is drawn.
 * A row with a non-finite logit gets action 0, logp = entropy = NaN and ORs
 * GSM_ACTOR_NONFINITE into status (device int32 [1], zeroed by the caller;
 * NULL: not wanted); the other rows are not affected.
 *
 * gsm_actor_sample: actions int32 [R] (what gsm_step takes with
 * GSM_ACT_INDEX), logp f32 [R] of the chosen action, entropy f32 [R] or NULL,
 * logits_out f32 [R][n_actions] or NULL.
 * gsm_actor_eval: the same head on stored actions int32 [R]: logp f32 [R],
 * entropy f32 [R] or NULL. An action outside [0, n_actions) sets
 * GSM_ACTOR_BAD_ACTION and gets logp = NaN. For the same inputs the logp of
 * the actions gsm_actor_sample chose is bit-identical to the logp it returned
 * (either mode): the PPO ratio is exactly 1 before the first update.
 * gsm_actor_eval_bwd: g_logp f32 [R], g_ent f32 [R] or NULL (zeros). h, the
 * logits and p_a = e_a / s are recomputed on chip. With H the entropy:
 *   dlogit_a = g_logp * (1[a = action] - p_a) - g_ent * p_a * (logp_a + H)
 *   db2 = sum_r dlogit;  dW2 = sum_r dlogit (x) h
 *   dh = W2^T dlogit where h > 0, else 0
 *   db1 = sum_r dh;  dW1 = sum_r dh (x) x;  dx = W1^T dh
 * (hidden == 0: dW2 = sum_r dlogit (x) x, dx = W2^T dlogit; dw1 = db1 = NULL).
 * dw1, db1, dw2, db2 in the weights' layouts; dx f32 [R][in_features],
 * 16-byte aligned, or NULL (not wanted). An action outside [0, n_actions)
 * sets GSM_ACTOR_BAD_ACTION and has no indicator term; a non-finite row sets
 * GSM_ACTOR_NONFINITE and its NaN reaches the gradients as autograd's would.
 * work: device f32, gsm_actor_backward_work_floats of them (one partial per
 * workgroup of a capped grid). No float atomics; the summation order depends
 * on the shape alone, so the gradients are bitwise reproducible. With n_envs
 * == 0 the weight gradients are zeros and nothing else is launched.
 * Shape limits (GSM_EINVAL, checked first): in_features a multiple of 4 in
 * [4, 128]; hidden 0, 16, 32 or 64; n_actions in [2, 8]; n_envs*n_agents <
 * 2^31; x_row_stride as above. Stateless; asynchronous on `stream`. */
#define GSM_ACTOR_DETERMINISTIC 1 /* flags: argmax, no draw                    */
#define GSM_ACTOR_NONFINITE 1     /* status: a row had a non-finite logit      */
#define GSM_ACTOR_BAD_ACTION 2    /* status: a stored action out of range      */
int gsm_actor_sample(const float *x, int64_t x_row_stride, const float *w1, const float *b1, const float *w2,
                     const float *b2, int64_t n_envs, int32_t n_agents, int32_t in_features, int32_t hidden,
                     int32_t n_actions, uint64_t seed, int64_t env_base, int64_t draw_host, const int64_t *draw_dev,
                     int32_t flags, int32_t *actions, float *logp, float *entropy, float *logits_out,
                     int32_t *status, void *stream);
int gsm_actor_eval(const float *x, int64_t x_row_stride, const float *w1, const float *b1, const float *w2,
                   const float *b2, int64_t n_envs, int32_t n_agents, int32_t in_features, int32_t hidden,
                   int32_t n_actions, const int32_t *actions, float *logp, float *entropy, int32_t *status,
                   void *stream);
int gsm_actor_backward_work_floats(int32_t in_features, int32_t hidden, int32_t n_actions, int64_t *n_floats);
int gsm_actor_eval_bwd(const float *g_logp, const float *g_ent, const float *x, int64_t x_row_stride,
                       const float *w1, const float *b1, const float *w2, const float *b2, int64_t n_envs,
                       int32_t n_agents, int32_t in_features, int32_t hidden, int32_t n_actions,
                       const int32_t *actions, float *work, float *dw1, float *db1, float *dw2, float *db2,
                       float *dx, int32_t *status, void *stream);

/* The critic head: a centralised value readout, one or two values a row (the
 * reward critic and the Lagrangian cost critic) from the row's features and
 * the mean of its env's features, one launch; and its gradients. Rows r =
 * b*n_agents + i, R = n_envs*n_agents; n_envs is any number of groups (a whole
 * buffer of (T+1)*B stored steps is one call). x f32, row r at x +
 * r*x_row_stride under gsm_actor_sample's rules (a view of gsm_env_conv's out
 * works). n_valid int32 [n_envs] or NULL (every env has n_agents valid rows):
 * the env's own agent count in a ragged batch; rows i >= n_valid[b] are
 * padding, are never read (they may hold NaN), take no part in the pool and
 * get 0.0 in every head. w1 f32 [hidden][2*in_features], b1 [hidden], w2
 * [n_out][hidden], b2 [n_out]: the torch.nn.Linear layout over the
 * concatenated input [pool_b | x_r]. denorm: device f32 [n_out][2] = (mean,
 * std) per head, read when the kernel runs (a captured graph sees updated
 * statistics), or NULL. Every line one correctly rounded fp32 operation, every
 * dot product an explicit fmaf chain (the actor head's convention: the bias,
 * then the inputs in ascending index of [pool | x]):
 *   pool_b[j] = (x[b,0][j] + x[b,1][j] + ..  over valid i, ascending) / (float)n_b
 *               (n_b = 0: pool = 0)
 *   c_b[h] = chain from b1[h]: fmaf(w1[h][j], pool_b[j], acc), j ascending
 *   h_r[h] = relu(chain continued from c_b[h]: fmaf(w1[h][F+j], x_r[j], acc))
 *   v_r[o] = chain from b2[o]: fmaf(w2[o][h], h_r[h], acc), h ascending
 *   values[o][r] = denorm ? v_r[o] * std_o + mean_o (a multiply, then an add)
 *                         : v_r[o]
 * values f32 [n_out][R], head-major: a head is a contiguous [.., n_agents]
 * tensor. A row's result depends on its env's rows alone, bit for bit: not on
 * where the env falls in a tile, in the grid or in the batch, so a slice of
 * the batch gives the bits of its rows in the full batch, and a valid row of
 * a ragged env the bits of the same rows in a dense batch of n_b agents.
 * status (device int32 [1], OR-ed, zeroed by the caller; NULL: not wanted):
 * GSM_CRITIC_NONFINITE: a valid row produced a non-finite v (it is written;
 * other envs are not affected); GSM_CRITIC_BAD_COUNT: an n_valid[b] outside
 * [0, n_agents], clamped.
 *
 * gsm_critic_eval_bwd: g f32 [n_out][R], the gradient with respect to the raw
 * v (denormalisation is never differentiated: the value loss is formed on
 * normalised targets). h, pool and c are recomputed on chip. With dv_r =
 * g[:, r] (0 on padded rows) and F = in_features:
 *   db2 = sum_r dv;  dW2 = sum_r dv (x) h_r
 *   dh_r = W2^T dv_r where h_r > 0, else 0
 *   db1 = sum_r dh;  dW1[:, F:] = sum_r dh_r (x) x_r
 *   s_b = sum_{i valid} dh_{b,i} (ascending);  dW1[:, :F] = sum_b s_b (x) pool_b
 *   dpool_b = W1[:, :F]^T s_b;  dx_r = W1[:, F:]^T dh_r + dpool_b / n_b
 * (padded rows: dx = 0). dw1, db1, dw2, db2 in the weights' layouts; dx f32
 * [R][in_features], 16-byte aligned, or NULL (not wanted). work: device f32,
 * gsm_critic_backward_work_floats of them (one partial per workgroup of a
 * capped grid). No float atomics; the summation order depends on the shape
 * alone, so the gradients are bitwise reproducible. With n_envs == 0 the
 * weight gradients are zeros and nothing else is launched.
 * Shape limits (GSM_EINVAL, checked first): in_features a multiple of 4 in
 * [4, 64]; hidden 16, 32 or 64; n_out 1 or 2; n_agents in [1, 128];
 * n_envs*n_agents < 2^31; x_row_stride as for the actor head. Every shape
 * inside them launches. Stateless; asynchronous on `stream`. */
#define GSM_CRITIC_NONFINITE 1 /* status: a valid row had a non-finite value     */
#define GSM_CRITIC_BAD_COUNT 2 /* status: an n_valid[b] outside [0, n_agents]    */
int gsm_critic_eval(const float *x, int64_t x_row_stride, const int32_t *n_valid, const float *w1, const float *b1,
                    const float *w2, const float *b2, const float *denorm, int64_t n_envs, int32_t n_agents,
                    int32_t in_features, int32_t hidden, int32_t n_out, float *values, int32_t *status,
                    void *stream);
int gsm_critic_backward_work_floats(int32_t in_features, int32_t hidden, int32_t n_out, int64_t *n_floats);
int gsm_critic_eval_bwd(const float *g, const float *x, int64_t x_row_stride, const int32_t *n_valid,
                        const float *w1, const float *b1, const float *w2, const float *b2, int64_t n_envs,
                        int32_t n_agents, int32_t in_features, int32_t hidden, int32_t n_out, float *work,
                        float *dw1, float *db1, float *dw2, float *db2, float *dx, int32_t *status, void *stream);

/* The clipped PPO / Lagrangian loss the two heads end in: the loss, eight
 * statistics and the gradients with respect to logp, entropy and the values,
 * in one launch pair. Rows r = b*n_agents + i, R = n_envs*n_agents; logp, ent,
 * logp_old f32 [R]; values, adv, v_old, ret f32 [n_out][R], head-major as
 * gsm_critic_eval writes them (head 0 the reward critic, head 1 the cost
 * critic). weight f32 [R] or NULL (1); n_valid int32 [n_envs] or NULL, clamped
 * to [0, n_agents]. multiplier: device f32 [1], the Lagrange multiplier, read
 * when the kernel runs (a captured graph sees an updated multiplier); NULL
 * only with n_out == 1. With lam = multiplier[0]:
 *   w_r   = weight[r] * [i < n_valid[b]];  W = sum_r w_r
 *   A     = adv[0][r] - lam * adv[1][r]            (n_out == 1: adv[0][r])
 *   ratio = expf(logp - logp_old)                  (the actor head's expf)
 *   pol   = -min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A)
 *   vclip = v_old + clamp(v - v_old, -value_clip, value_clip)
 *   val_o = max((v_o - ret_o)^2, (vclip_o - ret_o)^2)
 *   t_r   = (pol - ent_coef * ent) + value_coef * (val_0 + val_1)
 *   loss  = (sum_r w_r * t_r) / W
 * every line one correctly rounded fp32 operation at a time; 1 -/+ clip are
 * formed in double and rounded once. A row with w_r == 0 is not used in any
 * input (it may hold NaN; a row past n_valid[b] may hold NaN in weight too)
 * and gets the gradient 0.0. The gradients, d(loss) / d(input), [R], [R] and
 * [n_out][R], each written as (w_r * d_r) * (1.0f / W):
 *   g_logp:   d = -(ratio * A)  if 1 - clip <= ratio <= 1 + clip or
 *                               ratio * A < clamp(ratio, ..) * A;  else 0
 *   g_ent:    d = -ent_coef
 *   g_values: d = (2 * (v - ret)) * value_coef  if |v - v_old| <= value_clip
 *                               or (v - ret)^2 > (vclip - ret)^2;  else 0
 * g_logp, g_ent and g_values all NULL: not wanted (the second launch is then
 * one workgroup). loss f32 [1]. stats f32 [8]: the weighted means (sum_r w_r
 * x_r) / W of [0] t (the loss), [1] pol, [2] ent, [3] val_0, [4] val_1 (0 for
 * an absent head), [5] logp_old - logp (the approximate KL), [6] [ratio
 * outside [1 - clip, 1 + clip]] (the clip fraction), and [7] W. With R == 0 or
 * W == 0 loss, stats and the gradients are zeros; nothing divides by zero.
 * work: device f32, gsm_ppo_loss_work_floats of them (one [8] partial per
 * workgroup of a capped grid). The first launch adds a thread's rows, the 64
 * lanes of a wave and the waves of a workgroup in a fixed order; the second
 * adds the partials in one fixed order, the same in every workgroup. No float
 * atomics: the summation order depends on the shape alone (not on alignment:
 * 16-byte loads are used when R % 4 == 0 and every pointer is 16-byte
 * aligned, scalar loads of the same rows in the same order otherwise), so two
 * calls on the same inputs give the same bits in every output.
 * status (device int32 [1], OR-ed, zeroed by the caller; NULL: not wanted):
 * GSM_LOSS_NONFINITE: a row with w_r != 0 gave a non-finite t (it is added, as
 * autograd would); GSM_LOSS_BAD_COUNT: an n_valid[b] outside [0, n_agents],
 * clamped; GSM_LOSS_BAD_WEIGHT: a weight negative or non-finite, taken as 0.
 * Shape limits (GSM_EINVAL, checked first, nothing is launched): n_out 1 or 2;
 * n_agents >= 1; n_envs*n_agents < 2^31; multiplier NULL with n_out == 2.
 * Stateless; asynchronous on `stream`; no host reads, so it can be captured. */
#define GSM_LOSS_NONFINITE 1  /* status: a weighted row had a non-finite term      */
#define GSM_LOSS_BAD_COUNT 2  /* status: an n_valid[b] outside [0, n_agents]       */
#define GSM_LOSS_BAD_WEIGHT 4 /* status: a weight negative or non-finite           */
int gsm_ppo_loss_work_floats(int64_t n_rows, int64_t *n_floats);
int gsm_ppo_loss(const float *logp, const float *ent, const float *values, const float *logp_old, const float *adv,
                 const float *v_old, const float *ret, const float *weight, const int32_t *n_valid, int64_t n_envs,
                 int32_t n_agents, int32_t n_out, const float *multiplier, float clip, float value_clip,
                 float ent_coef, float value_coef, float *work, float *loss, float *stats, float *g_logp,
                 float *g_ent, float *g_values, int32_t *status, void *stream);

/* GAE returns of a stored episode of T = n_steps actions in one launch, with
 * BN = [n_envs][n_agents]: reward f32 [T]BN (entry t: the reward of action t),
 * value f32 [T+1]BN, done uint8 [T+1][n_envs] (slot t+1: action t ended the
 * episode), ret f32 [T]BN. One thread per (env, agent) walks t = T-1 down to
 * 0, each line one correctly rounded fp32 operation at a time:
 *   m = 1 - done[t+1];  delta = (r[t] + (gamma * v[t+1]) * m) - v[t]
 *   gae = delta + (gamma_lambda * m) * gae;  ret[t] = gae + v[t]
 * gamma_lambda = the double product gamma * lambda rounded once to fp32 (the
 * caller forms it). Stateless; asynchronous on `stream`. */
int gsm_gae(const float *reward, const float *value, const uint8_t *done, int64_t n_steps, int64_t n_envs,
            int32_t n_agents, float gamma, float gamma_lambda, float *ret, void *stream);

/* Episode frames (replaces the pyglet viewer of
 * multiagent/rendering.py, SOURCES.txt:18, used by scripts/render_mpe.py,
 * SOURCES.txt:30, for the demo/ GIFs, readme.md:64). Draws env env_ids[f]
 * of a batch into frame f of rgba (uint8 [n_frames][height][width][4]) from
 * its node-feature rows (node_feat: f32 [n_envs][n_entities][7], position in
 * columns 2-3, type 0 agent / 1 goal-target / 2 obstacle / -1 padding in
 * column 6) and, with GSM_RENDER_EDGES, its packed CSR edges (edge_ptr int64
 * [n_envs+1], edge_index int32 [2][edge_capacity], global ids b*n_entities+e)
 * as black lines. Camera [-L, L]^2 with L = half_width, or sqrt(n_agents/3)
 * of the env when half_width <= 0; disc radii = the three sizes. Any rollout
 * slot can be rendered. Out-of-range env ids give white frames. Stateless;
 * asynchronous on `stream`. */
#define GSM_RENDER_EDGES 1
int gsm_render(const float *node_feat, int64_t n_envs, int32_t n_entities, const int64_t *edge_ptr,
               const int32_t *edge_index, int64_t edge_capacity, const int32_t *env_ids, int32_t n_frames,
               float half_width, float agent_size, float target_size, float obstacle_size, int32_t width,
               int32_t height, int32_t flags, uint8_t *rgba, void *stream);

/* Diagnostics: device buffer (uint64 [2 * n_blocks * 4][16]) that libraries
 * built with -DGSM_STAMPS fill with per-wave phase timestamps; ignored by the
 * product build. NULL disables. */
int gsm_debug_set_stamps(gsm_handle *h, void *stamps);

int gsm_destroy(gsm_handle *h);

/* Copies the last error message of h (or of the library when h == NULL). */
int gsm_last_error(const gsm_handle *h, char *buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* GSM_H_ */
