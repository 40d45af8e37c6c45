// gsm_abi.hip — extern "C" boundary of libgsm.so (declared in include/gsm.h):
// the env handle and everything that takes one. The stateless entry points of
// the training chain are in gsm_ops.hip.
//
// Host-only bookkeeping: validate the config, derive the fp32 constants the
// kernels use (same fp32 operations as oracle/batch_ref.py:Spec), borrow the
// caller's device buffers, launch, and optionally capture whole multi-step
// rollouts: a per-step chain into a HIP graph, a fused rollout as one stored
// kernel launch (planned by gsm_roll_plan.h). No allocation and no
// synchronisation happens in gsm_step / gsm_reset / gsm_observe.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <string>
#include <vector>

#include "gsm.h"
#include "gsm_host.h"
#include "gsm_internal.h"
#include "gsm_philox.h"
#include "gsm_roll_plan.h"

namespace {
// u64 words between the chunk sums of the segmented rollout's one-hop prefix
// (gsm_device.h roll_prefix): each on a 64-byte line of its own
constexpr int kCsumStride = 8;
// what gsm_roll_plan.h takes from gsm_internal.h
constexpr gsm::RollConsts kRollConsts{gsm::kWave,
                                      gsm::kWavesPerBlock,
                                      gsm::kPrefixChunk,
                                      kCsumStride,
                                      gsm::kRollMaxSteps,
                                      (size_t)gsm::kPaceKeys * gsm::kPaceStride,
                                      (size_t)gsm::kEpochReps * gsm::kEpochStride};
gsm::Knobs read_knobs() { return gsm::read_knobs(getenv, gsm::kRaggedRollMaxDepth); }
}  // namespace

struct gsm_handle {
    gsm_config cfg;
    gsm_sizes sz;
    gsm::DevParams dp;      // constants + bound buffers
    bool bound = false;
    std::string err;
    // graph capture
    hipStream_t cap_stream = nullptr;
    int32_t *bsum_alt = nullptr;   // second half of the per-workgroup edge-sum double buffer (lagged emission)
    int32_t *block_order = nullptr;   // ragged mixed: workgroup -> env block, heaviest first
    int32_t *order_host = nullptr;    // pinned staging of block_order's async upload
    int32_t *place_order = nullptr;   // ragged mixed: the rollout's placement order (inside block_order)
    hipEvent_t order_copied = nullptr;   // recorded after the last upload (staging free again)
    struct Slot {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        std::vector<hipEvent_t> events;   // timing event-record nodes
        int steps = 0;
        int kern = 0;
        bool each = false;
        // A rollout slot holds no graph: it is one stored kernel launch (fn,
        // grid, block, lds, args) — a plain dispatch costs the host less than a
        // graph launch, and every launch takes arguments of its own
        // (gsm_graph_launch).
        bool roll = false;
        const void *fn = nullptr;
        dim3 grid, block;
        unsigned lds = 0;
        gsm::DevParams args;
        uint64_t *gran = nullptr;     // its granules' used bytes, laid out by `lay`
        void *gran_base = nullptr;    // their allocation (gran_malloc: the used bytes end at its end)
        gsm::GranLayout lay{};
        // the one-hop rollouts' chunk sums and pace counters (paced: pacing
        // on) come in two halves: a launch uses half (launches & 1) and
        // zeroes the other for the slot's next launch
        bool paced = false;
        uint32_t launches = 0;
        uint32_t last_epoch = 0xffffffffu;   // the epoch of the slot's previous launch
        bool captured() const { return exec != nullptr || roll; }
    } slots[GSM_GRAPH_SLOTS];
    uint32_t *roll_status = nullptr;  // fused rollout: a bounded wait gave up (sticky until read)
    void *edge_scratch = nullptr;     // fused rollout in the bound buffers: edges of all but the last step
    void *slab = nullptr;             // ragged rollout: per-env edge slabs (depth + 1 steps)
    size_t slab_bytes = 0;
    // the stream of the last rollout-slot launch: rollout slots share the
    // handle's scratch (edge scratch, slabs) and state, so launches on
    // another stream first wait for it (gsm_graph_launch)
    hipStream_t roll_stream = nullptr;
    bool roll_launched = false;
    hipEvent_t roll_done = nullptr;   // recorded behind every rollout-slot launch
    // gsm_step as a one-step rollout launch (step + its edges in one kernel):
    // -1 not yet decided for this config, 0 no (two launches), 1 yes
    int eager_roll = -1;
    uint64_t *eager_gran = nullptr;   // its granules' used bytes (K = 1), laid out by eager_lay
    gsm::GranLayout eager_lay{};
    void *eager_base = nullptr;       // their allocation
};

// the thread's last error (gsm_last_error(NULL, ..)); fail is declared in
// gsm_host.h: gsm_ops.hip records its errors through it
static thread_local std::string g_err;

int fail(gsm_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    g_err = msg;
    return code;
}

namespace {

int align16(int x) { return (x + 15) & ~15; }

// Ragged mixed batches: the step kernel's workgroups take their env blocks
// heaviest first, so the long assignment chains (polygon/line envs with many
// agents) start in the first residency round instead of waiting behind light
// envs. Cost of an env ~ N_env^2 for polygon/line (assignment path
// iterations), N_env for navigation; a block costs its heaviest env. The
// order only schedules: every output is the same under any order (each
// workgroup writes its own env block's slots). Recomputed when the seed that
// draws the env shapes changes (never per step). The upload is stream-ordered
// on the caller's stream `s` (from pinned staging), so kernels enqueued on it
// before the reseed finish with the old order and every later one sees the new
// order; the staging buffer is reused only after the previous upload read it.
//
// The same upload carries the ragged rollout's placement order (after the nb
// block entries): the grid's W = 4 * ceil(B / 4) envs by descending cost per
// step, linear in N_env per family: polygon / line a + b N, navigation
// c + d N, from scans of the C4 launch time (`tools/gpu.sh envsweep TAG c4
// GSM_PLACE_MODEL a,b,c,d`). Round 3 (navigation sweep on the scalar path):
// 63 + 27 N and 55 + 18 N (20 + 7 N: 39.4 us per step, 55 + 18 N: 36.9,
// 70 + 24 N: 38.9). Round 4, with the navigation sweep and the assignment's
// passes off the scalar path the navigation envs cost a fraction of an
// assignment env and the assignment's cost is flatter in N
// (profiles/r4_stamps/stamps_c4.json): 200 + 20 N and 10 + 3 N, 27.2 us per
// step against 29.4 for the round-3 weights (profiles/r4_place); padding envs
// (b >= B) last. roll_place (gsm_ragged_kernels.hip) deals them to the
// SIMDs in strata.
constexpr int kXcds = 8;   // MI355X: 8 XCDs of 32 CUs
int update_block_order(gsm_handle *h, hipStream_t s) {
    const gsm::DevParams &p = h->dp;
    if (p.path != gsm::kPathRagged || p.scenario != gsm::kScnMixed) return GSM_OK;
    const int nb = h->sz.n_blocks, per = h->sz.envs_per_block;
    const int W = (p.B + gsm::kWavesPerBlock - 1) / gsm::kWavesPerBlock * gsm::kWavesPerBlock;
    std::vector<int64_t> key(nb), cost(W, 0);
    // cost units per env and step: polygon/line a + b N, navigation c + d N,
    // the C4 rollout's best of a scan (tools/gpu.sh envsweep,
    // GSM_PLACE_MODEL="a,b,c,d" overrides)
    const gsm::Knobs knobs = read_knobs();
    const int64_t ma = knobs.model[0], mb = knobs.model[1], mc = knobs.model[2], md = knobs.model[3];
    for (int b = 0; b < p.B; ++b) {
        const int64_t gid = p.env_base + b;
        const gsm::Philox4 x = gsm::philox4x32_10(0u, 0u, (uint32_t)gid, gsm::kTagShape, p.seed_lo, p.seed_hi);
        const int n = p.n_min + (int)(((uint64_t)x.x0 * (uint64_t)(p.N - p.n_min + 1)) >> 32);
        const bool lsa = (gid % 3) != gsm::kScnNav;
        cost[b] = lsa ? ma + mb * (int64_t)n : mc + md * (int64_t)n;
        const int64_t ce = lsa ? (int64_t)n * n : n;
        if (b / per < nb && ce > key[b / per]) key[b / per] = ce;
    }
    std::vector<int32_t> order(nb + W);
    for (int k = 0; k < nb; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.begin() + nb, [&](int32_t a, int32_t b) { return key[a] > key[b]; });
    for (int k = 0; k < W; ++k) order[nb + k] = k;
    // XCD-local dealing (round 5): roll_place gives SIMD i (XCD-major: the
    // SIMDs of XCD x are i in [x S/8, (x+1) S/8)) entry i of even strata and
    // S - 1 - i of odd ones. Each XCD takes a contiguous block of W/8 envs, its
    // own cost order cut into strata of S/8 and snaked over its SIMDs, so envs
    // next to each other in memory (their per-env outputs and CSR edges share
    // cache lines) are written from one XCD's L2 instead of up to eight, each
    // writing back its own partial copy of the line. GSM_PLACE_XCD=0: one cost
    // order over the whole grid (round 4).
    int n_cu = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        n_cu = 0;
    const int S = 4 * n_cu, SX = S / kXcds;
    if (knobs.place_xcd && S > 0 && S % kXcds == 0 && W % S == 0) {
        const int R = W / S, WX = W / kXcds;
        std::vector<int32_t> blk(WX);
        for (int x = 0; x < kXcds; ++x) {
            for (int k = 0; k < WX; ++k) blk[k] = x * WX + k;
            std::stable_sort(blk.begin(), blk.end(), [&](int32_t a, int32_t b) { return cost[a] > cost[b]; });
            for (int r = 0; r < R; ++r)
                for (int il = 0; il < SX; ++il) {
                    const int i = x * SX + il;                   // the SIMD
                    const int j = (r & 1) ? S - 1 - i : i;       // its table entry in stratum r
                    const int e = (r & 1) ? SX - 1 - il : il;    // snaked within the XCD
                    order[nb + (size_t)r * S + j] = blk[(size_t)r * SX + e];
                }
        }
    } else {
        std::stable_sort(order.begin() + nb, order.end(), [&](int32_t a, int32_t b) { return cost[a] > cost[b]; });
    }
    const size_t bytes = (size_t)(nb + W) * sizeof(int32_t);
    hipError_t e = hipSuccess;
    if (!h->block_order) {
        e = hipMalloc(&h->block_order, bytes);
        if (e != hipSuccess) {
            h->block_order = nullptr;
            return hip_fail(h, e, "hipMalloc (block order)");
        }
        e = hipHostMalloc((void **)&h->order_host, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            h->order_host = nullptr;
            return hip_fail(h, e, "hipHostMalloc (block order staging)");
        }
        e = hipEventCreateWithFlags(&h->order_copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            h->order_copied = nullptr;
            return hip_fail(h, e, "hipEventCreate (block order)");
        }
    } else {
        e = hipEventSynchronize(h->order_copied);   // the previous upload has read the staging
        if (e != hipSuccess) return hip_fail(h, e, "hipEventSynchronize (block order)");
    }
    memcpy(h->order_host, order.data(), bytes);
    e = hipMemcpyAsync(h->block_order, h->order_host, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(h, e, "hipMemcpyAsync (block order)");
    e = hipEventRecord(h->order_copied, s);
    if (e != hipSuccess) return hip_fail(h, e, "hipEventRecord (block order)");
    h->dp.block_order = h->block_order;
    h->place_order = h->block_order + nb;
    return GSM_OK;
}

int check_config(const gsm_config *c, std::string *why) {
    if (!c) { *why = "config is NULL"; return GSM_EINVAL; }
    if (c->abi_version != GSM_ABI_VERSION) {
        *why = "abi_version mismatch (library " + std::to_string(GSM_ABI_VERSION) + ", caller " +
               std::to_string(c->abi_version) + ")";
        return GSM_EINVAL;
    }
    if (c->scenario < GSM_SCEN_NAVIGATION || c->scenario > GSM_SCEN_MIXED) {
        *why = "unsupported scenario";
        return GSM_EINVAL;
    }
    if (c->n_envs < 1) { *why = "n_envs must be >= 1"; return GSM_EINVAL; }
    if (c->n_agents < 1 || c->n_agents > 1024) { *why = "n_agents must be in [1, 1024]"; return GSM_EINVAL; }
    if (c->n_obstacles < 0 || c->n_obstacles > 1024) { *why = "n_obstacles must be in [0, 1024]"; return GSM_EINVAL; }
    if (c->episode_length < 1) { *why = "episode_length must be >= 1"; return GSM_EINVAL; }
    const bool ragged = c->scenario != GSM_SCEN_NAVIGATION;
    if (!(c->dt > 0) || !(c->mass > 0) || !(c->contact_margin > 0)) {
        *why = "dt, mass and contact_margin must be > 0";
        return GSM_EINVAL;
    }
    if (ragged ? !(c->world_half >= 0) : !(c->world_half > 0)) {
        *why = "world_half must be > 0 (ragged scenarios: >= 0, 0 = sqrt(N_env/3) per env)";
        return GSM_EINVAL;
    }
    if (ragged) {
        if (c->n_agents > GSM_RAGGED_MAX_AGENTS) {
            *why = "polygon/line/mixed: n_agents must be <= GSM_RAGGED_MAX_AGENTS (32)";
            return GSM_EINVAL;
        }
        if (c->scenario == GSM_SCEN_MIXED ? c->n_obstacles != c->n_agents : c->n_obstacles != 0) {
            *why = "mixed needs n_obstacles == n_agents (navigation envs); polygon/line need n_obstacles == 0";
            return GSM_EINVAL;
        }
        if (c->scenario == GSM_SCEN_MIXED && (c->n_agents_min < 1 || c->n_agents_min > c->n_agents)) {
            *why = "mixed needs 1 <= n_agents_min <= n_agents";
            return GSM_EINVAL;
        }
        if (!(c->formation_radius >= 0) || !isfinite(c->formation_radius)) {
            *why = "formation_radius must be a finite value >= 0";
            return GSM_EINVAL;
        }
    }
    if (!(c->damping >= 0 && c->damping <= 1)) { *why = "damping must be in [0, 1]"; return GSM_EINVAL; }
    if (!(c->sense_radius >= 0) || !(c->contact_cutoff > 0)) {
        *why = "sense_radius must be >= 0 and contact_cutoff > 0";
        return GSM_EINVAL;
    }
    return GSM_OK;
}

// kernel family and envs per wave for a config
void choose_path(const gsm_config *c, int *path, int *G) {
    const int M = c->n_agents + c->n_obstacles;
    if (c->scenario != GSM_SCEN_NAVIGATION) {
        *path = gsm::kPathRagged;
        *G = 1;
    } else if (M <= gsm::kWave) {
        *path = gsm::kPathSeg;
        // as many envs per wave as fit (at most kMaxSegEnvsPerWave), but no
        // fewer waves than one workgroup per CU (256 x 4): a small batch of
        // small envs is latency-bound, and packing it into fewer waves leaves
        // CUs idle
        int g = gsm::kWave / M;
        g = g > gsm::kMaxSegEnvsPerWave ? gsm::kMaxSegEnvsPerWave : g;
        const int64_t fill = c->n_envs / 1024;
        *G = fill < g ? (fill < 1 ? 1 : (int)fill) : g;
    } else {
        *path = gsm::kPathTile;
        *G = 1;
    }
}

// target rows per env: navigation goals = N, polygon centre 1, line ends 2,
// mixed = N (its navigation envs)
int targets_of(const gsm_config *c) {
    switch (c->scenario) {
        case GSM_SCEN_POLYGON: return 1;
        case GSM_SCEN_LINE: return 2;
        default: return c->n_agents;
    }
}

void fill_sizes(const gsm_config *c, gsm_sizes *s) {
    const int N = c->n_agents, No = c->n_obstacles, M = N + No, T = targets_of(c);
    int path, G;
    choose_path(c, &path, &G);
    s->n_entities = N + T + No;
    s->node_feat_dim = 7;
    s->obs_dim = 6;
    s->envs_per_block = path == gsm::kPathTile ? 1 : gsm::kWavesPerBlock * G;
    s->n_blocks = (c->n_envs + s->envs_per_block - 1) / s->envs_per_block;
    // radius edges among colliders + the agent <-> target edges (2 per agent
    // per target it is tied to: own goal / centre: 1, line ends: 2)
    int max_edges = M * (M - 1) + 2 * N;
    if (c->scenario == GSM_SCEN_LINE) max_edges = N * (N - 1) + 4 * N;
    if (c->scenario == GSM_SCEN_MIXED && N * (N - 1) + 4 * N > max_edges) max_edges = N * (N - 1) + 4 * N;
    s->max_edges_per_env = max_edges;
    s->n_colliders = M;
    s->n_targets = T;
    s->mask_words = path == gsm::kPathTile ? (M + 63) / 64 : 1;
    s->edge_capacity = (int64_t)c->n_envs * s->max_edges_per_env;
}

// fp32 constants, formed exactly like oracle/batch_ref.py:Spec (fp32 mode).
void derive(const gsm_config *c, gsm::DevParams *p) {
    memset(p, 0, sizeof *p);
    const int N = c->n_agents, No = c->n_obstacles;
    p->B = c->n_envs;
    p->N = N;
    p->No = No;
    p->T = targets_of(c);
    p->E = N + p->T + No;
    p->M = N + No;
    p->scenario = c->scenario;
    p->n_min = c->scenario == GSM_SCEN_MIXED ? c->n_agents_min : N;
    choose_path(c, &p->path, &p->G);
    p->W = p->path == gsm::kPathTile ? (p->M + 63) / 64 : 1;
    p->EL = c->episode_length;
    p->auto_reset = c->auto_reset != 0;
    p->shared_reward = c->shared_reward != 0;
    p->seed_lo = (uint32_t)(c->seed & 0xFFFFFFFFull);
    p->seed_hi = (uint32_t)(c->seed >> 32);
    p->env_base = c->env_base;
    p->strict = c->strict_degenerate != 0;
    if (p->path == gsm::kPathRagged) {
        // assignment scratch (cost matrix, duals) + staged entity positions [E]
        p->wave_lds_step = align16(gsm::lsa_lds_bytes(N) + 8 * p->E);
        p->wave_lds_emit = align16(8 * p->E);
    } else if (p->path == gsm::kPathSeg) {
        // positions + staged node-feature rows of the wave's G envs
        p->wave_lds_step = align16(8 * p->G * p->E + 28 * p->G * p->E);
        // one env per wave: + the staged edge list (stage_rows)
        p->wave_lds_emit = align16(p->G == 1 ? 36 * p->E : 8 * p->G * p->E);
    } else {
        // tile: whole-workgroup LDS: positions, velocities, new positions, costs, reductions,
        // the two degenerate-state flags;
        // + the symmetric sweep's column pairs, agent-row words and obstacle-row
        // agent bits when they fit in 32 KB (gsm_tile_kernels.hip: obs_sweep_sym)
        p->wave_lds_step = align16(8 * p->E + 8 * N + 8 * N + 4 * N + 20 * (gsm::kTileBlock / gsm::kWave) + 8);
        const int sym = 16 * ((N + 1) / 2) + 16 * N * p->W + 8 * No * p->W + 16;
        p->tile_sym = sym <= 32768;
        if (p->tile_sym) p->wave_lds_step += sym;
        // emit: positions, reductions and the staged edge words (gsm::kTileEmitScr)
        p->wave_lds_emit = align16(8 * p->E + 4 * (gsm::kTileBlock / gsm::kWave) + 4 * gsm::kTileEmitScr);
    }
    const float L = c->world_half;
    p->L = L;
    p->twoL = L * 2.0f;
    p->fixed_L = p->path == gsm::kPathRagged ? (L > 0.0f ? L : 0.0f) : L;
    p->form_r = c->formation_radius;
    p->dt = c->dt;
    p->omd = 1.0f - c->damping;
    p->mass = c->mass;
    p->inv_mass = 1.0f / c->mass;
    p->cf = c->contact_force;
    p->k = c->contact_margin;
    p->inv_k = 1.0f / c->contact_margin;
    p->sens = c->sensitivity;
    p->max_speed = c->max_speed;
    const float R = c->sense_radius;
    p->R2 = R * R;
    const float sa = c->agent_size, so = c->obstacle_size;
    p->dmin_aa = sa + sa;
    p->dmin_ao = sa + so;
    p->dmin2_aa = p->dmin_aa * p->dmin_aa;
    p->dmin2_ao = p->dmin_ao * p->dmin_ao;
    // beyond d - dmin > cutoff*k the pair force is below cf*k*exp(-cutoff)
    // (4e-19 at the default cutoff 40): skipped (contact cutoff)
    const float caa = p->dmin_aa + c->contact_cutoff * c->contact_margin;
    const float cao = p->dmin_ao + c->contact_cutoff * c->contact_margin;
    p->cut2_aa = caa * caa;
    p->cut2_ao = cao * cao;
}

// Point a launch's outputs at `o` (NULL members keep the bound buffers).
int redirect(gsm_handle *h, gsm::DevParams *p, const gsm_outputs *o) {
    if (!o) return GSM_OK;
    if (o->edge_index && o->edge_capacity < 1)
        return fail(h, GSM_EINVAL, "redirected edge_index needs edge_capacity >= 1");
    if (o->edge_index && o->edge_capacity >= (int64_t)1 << 31)
        return fail(h, GSM_EINVAL, "edge_capacity must be < 2^31");
    if (!!o->edge_index != !!o->edge_attr)
        return fail(h, GSM_EINVAL, "edge_index and edge_attr are redirected together");
    if (o->node_feat) p->node_feat = o->node_feat;
    if (o->reward) p->reward = o->reward;
    if (o->cost) p->cost = o->cost;
    if (o->done) p->done = o->done;
    if (o->edge_count) p->edge_count = o->edge_count;
    if (o->edge_ptr) p->edge_ptr = o->edge_ptr;
    if (o->edge_index) {
        p->edge_index = o->edge_index;
        p->edge_attr = o->edge_attr;
        p->edge_capacity = o->edge_capacity;
    }
    if (o->assign) p->assign = o->assign;
    p->nf_full = 1;
    return GSM_OK;
}

uint32_t next_launch_epoch();
hipError_t clear_status(gsm_handle *h);
// a launch epoch other than `last` (the previous launch of the same granules:
// the process-wide counter wraps after 2^20 launches, and an idle slot's
// granules still carry its last launch's tags), recorded as the new last
uint32_t fresh_epoch(uint32_t &last) {
    uint32_t e = next_launch_epoch();
    if (e == last) e = next_launch_epoch();
    last = e;
    return e;
}

// The rollout granules (in-launch hand-off words, gsm_device.h) are allocated
// uncached: an agent-scope load of a granule line that this XCD's L2 still
// holds from an earlier read can be served stale until the line leaves the
// L2, and the hand-off then re-polls. Same box, one run each (profiles/
// r4_gran): C2 3.44 -> 3.16 us per step, H 8.46 -> 8.31, C3 and C4 within
// noise.
//
// The used bytes are placed at the END of a whole number of 4 KiB pages
// (*gran = *base + the slack): an access past the last granule leaves the
// allocation instead of reading its own slack unnoticed (gsm_device.h
// gran_chk; the checked build tests every address against the end).
hipError_t gran_malloc(void **base, uint64_t **gran, size_t bytes) {
    const size_t alloc = (bytes + 4095) & ~(size_t)4095;
    const hipError_t e = hipExtMallocWithFlags(base, alloc, hipDeviceMallocUncached);
    if (e != hipSuccess) {
        *base = nullptr;
        *gran = nullptr;
        return e;
    }
    *gran = (uint64_t *)((char *)*base + (alloc - bytes));
    return hipSuccess;
}

// the address of a GranLayout offset (gsm_roll_plan.h) in a granule
// allocation's used bytes: the only arithmetic on granule memory
template <typename T>
T *gran_at(uint64_t *gran, size_t off) {
    return reinterpret_cast<T *>(reinterpret_cast<char *>(gran) + off);
}

// the status word of the rollouts' bounded waits, allocated and cleared once
int ensure_status(gsm_handle *h) {
    if (h->roll_status) return GSM_OK;
    hipError_t e = hipMalloc(&h->roll_status, 16);
    if (e == hipSuccess) e = clear_status(h);
    if (e == hipSuccess) return GSM_OK;
    h->roll_status = nullptr;
    return hip_fail(h, e, "hipMalloc (rollout status)");
}

// the library's own stream: granule init and graph upload at capture
int ensure_cap_stream(gsm_handle *h) {
    if (h->cap_stream) return GSM_OK;
    const hipError_t e = hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking);
    return e == hipSuccess ? GSM_OK : hip_fail(h, e, "hipStreamCreate");
}

// what one residency round of a rollout kernel holds: workgroups per CU, CUs
hipError_t query_round(const gsm::RollForm &form, int *per_cu, int *n_cu) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, form.fn, form.threads, form.lds);
    return e;
}

// a rollout's outputs all in the launch's bound (or redirected) buffers
gsm::DevParams::RollOut bound_roll_out(const gsm::DevParams &p) {
    gsm::DevParams::RollOut ro{};
    ro.nf = p.node_feat;
    ro.rew = p.reward;
    ro.cost = p.cost;
    ro.done = p.done;
    ro.ecount = p.edge_count;
    ro.eptr = p.edge_ptr;
    ro.eidx = p.edge_index;
    ro.eattr = p.edge_attr;
    ro.cap = p.edge_capacity;
    ro.asg = p.assign;
    return ro;
}

// gsm_step as ONE launch: the config's fused rollout kernel with K = 1 (the
// step, then its edges at the CSR offset of the in-launch prefix) instead of
// the step kernel + the emit kernel — the same operations, so the same outputs
// (tests/test_gpu_roll.py), when the grid fits one residency round (decided
// once per handle). It runs for the one-env-per-wave segmented rollout
// (navigation with 6, 12 or 24 agents: 15.4 vs 16.5 us per step at H, 13.1 vs
// 15.5 at 12 x 8192; DESIGN.md §4, profiles/r5_ab/eager_forms) unless
// GSM_EAGER_ONE_LAUNCH=0 asks for the two launches. Every other config runs
// the two launches: for the packed small-env and tile rollouts they were the
// faster form (C2 8.7 vs 9.4, C3 27.9 vs 29.6 us), and the ragged path has no
// one-step form.
constexpr int kEagerIneligible = 1;
// Decided once per handle, at gsm_bind (the hand-off granules allocated and
// zeroed there, so that no step allocates or synchronises): h->eager_roll 1
// when the config has an eager rollout kernel whose grid fits one residency
// round and the two launches were not asked for, else 0.
int eager_setup(gsm_handle *h) {
    gsm::DevParams p = h->dp;
    p.action_fmt = GSM_ACT_INDEX;   // (every format's kernel has the same LDS and occupancy)
    h->eager_roll = 0;
    const gsm::RollForm form = gsm::roll_seg_eager_form(p);
    if (!form.fn) return GSM_OK;
    if (!read_knobs().eager_one_launch) return GSM_OK;
    // one step, per-workgroup hand-off: the workgroups' aggregates, two halves
    // of chunk sums, no pacing, then the device-side epoch replicas
    const gsm::RollShape shape = gsm::roll_shape(kRollConsts, 1, (p.B + form.envs - 1) / form.envs, false, true);
    int per_cu = 0, n_cu = 0;
    hipError_t e = query_round(form, &per_cu, &n_cu);
    if (e != hipSuccess) return hip_fail(h, e, "occupancy query (eager rollout)");
    if (gsm::roll_limits(kRollConsts, shape, 1, 0, per_cu, n_cu) != gsm::RollLimit::kNone) return GSM_OK;
    const gsm::GranLayout lay = gsm::gran_layout(kRollConsts, shape);
    if (h->eager_base) {   // (a retried setup)
        (void)hipFree(h->eager_base);
        h->eager_base = nullptr;
        h->eager_gran = nullptr;
    }
    e = gran_malloc(&h->eager_base, &h->eager_gran, lay.bytes);
    if (e != hipSuccess) return hip_fail(h, e, "hipMalloc (eager granules)");
    h->eager_lay = lay;
    e = gsm::launch_granule_init(h->eager_gran, lay.bytes, 0u, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) {   // the first epoch: a fresh one of the process-wide sequence, in every replica
        std::vector<uint32_t> ep(lay.epoch.bytes / sizeof(uint32_t), 0u);
        const uint32_t e0 = next_launch_epoch();
        for (int r = 0; r < gsm::kEpochReps; ++r) ep[(size_t)r * gsm::kEpochStride] = e0;
        e = hipMemcpy(gran_at<uint32_t>(h->eager_gran, lay.epoch.off), ep.data(), lay.epoch.bytes,
                      hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return hip_fail(h, e, "eager rollout setup");
    if (const int rc = ensure_status(h)) return rc;
    h->eager_roll = 1;
    return GSM_OK;
}

int launch_step_roll(gsm_handle *h, gsm::DevParams p, hipStream_t s) {
    if (h->eager_roll < 0) {   // (gsm_bind decides it; kept for a handle bound before)
        const int rc = eager_setup(h);
        if (rc) return rc;
    }
    if (h->eager_roll == 0) return kEagerIneligible;
    // The kernel takes its epoch and chunk-sum half from device memory and
    // advances them itself (gsm_roll_seg_kernel kEager), so the launch holds
    // no per-launch host state and may be recorded into a stream capture
    // (torch.cuda.graph around a policy + env.step).
    const gsm::RollForm form = gsm::roll_seg_eager_form(p);   // (the action format may differ per call)
    if (!form.fn) return kEagerIneligible;
    const int nb = (p.B + form.envs - 1) / form.envs;
    const gsm::GranLayout &lay = h->eager_lay;
    // the step's outputs: the bound (or redirected) buffers, its edges too
    p.ro = bound_roll_out(p);
    // (one step: no pacing; per-workgroup hand-off: no xW / xNG; the epoch
    // field unused)
    gsm::DevParams::Roll r{};
    r.actions = (const char *)p.actions;
    r.n_actions = 1;
    r.K = 1;
    r.gran = gran_at<uint64_t>(h->eager_gran, lay.granules.off);
    r.status = h->roll_status;
    // (the halves in a fixed order: the kernel picks by the epoch's parity)
    r.csum = gran_at<uint64_t>(h->eager_gran, lay.csum[0].off);
    r.csum_next = gran_at<uint64_t>(h->eager_gran, lay.csum[1].off);
    r.csum_stride = kCsumStride;
    r.gran_end = gran_at<uint64_t>(h->eager_gran, lay.bytes);
    r.dev_epoch = gran_at<uint32_t>(h->eager_gran, lay.epoch.off);
    p.roll = r;
    void *args[] = {&p};
    const hipError_t e = hipLaunchKernel(form.fn, dim3(nb), dim3(form.threads), args, (unsigned)form.lds, s);
    if (e != hipSuccess) return hip_fail(h, e, "hipLaunchKernel (one-step rollout)");
    return GSM_OK;
}

int launch(gsm_handle *h, int mode, const void *actions, int fmt, const uint8_t *mask, int reseed,
           hipStream_t s, const gsm_outputs *out = nullptr) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (!h->bound) return fail(h, GSM_ESTATE, "gsm_bind has not been called");
    if (mode == GSM_MODE_STEP) {
        if (!actions) return fail(h, GSM_EINVAL, "actions is NULL");
        if (fmt < GSM_ACT_ONEHOT || fmt > GSM_ACT_CONT) return fail(h, GSM_EINVAL, "bad action_fmt");
    }
    gsm::DevParams p = h->dp;
    const int rc = redirect(h, &p, out);
    if (rc) return rc;
    p.mode = mode;
    p.actions = actions;
    p.action_fmt = fmt;
    p.env_mask = mask;
    p.reseed = reseed;
    if (mode == GSM_MODE_STEP) {
        const int r = launch_step_roll(h, p, s);
        if (r != kEagerIneligible) return r;
    }
    const hipError_t e = gsm::launch_step(p, s);
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
    return GSM_OK;
}

void drop_slot(gsm_handle::Slot &s) {
    if (s.exec) (void)hipGraphExecDestroy(s.exec);
    if (s.graph) (void)hipGraphDestroy(s.graph);
    for (hipEvent_t ev : s.events) (void)hipEventDestroy(ev);
    if (s.gran_base) (void)hipFree(s.gran_base);
    s.gran_base = nullptr;
    s.gran = nullptr;
    s.lay = gsm::GranLayout{};
    s.paced = false;
    s.launches = 0;
    s.roll = false;
    s.fn = nullptr;
    s.exec = nullptr;
    s.graph = nullptr;
    s.events.clear();
    s.steps = 0;
    s.kern = 0;
    s.each = false;
}

void drop_graph(gsm_handle *h) {
    for (auto &s : h->slots) drop_slot(s);
}

bool bad_slot(int32_t slot) { return slot < 0 || slot >= GSM_GRAPH_SLOTS; }

// The epoch of every rollout launch in the process (DevParams::Roll::epoch):
// one counter, started at a random point so that a granule left in device
// memory by an earlier process does not carry the first epochs of this one.
// A granule of launch L can match only launch L + 2^20 (gsm_device.h
// roll_epoch_tag), whatever graph or allocation either belongs to.
uint32_t next_launch_epoch() {
    static std::atomic<uint32_t> next{[] {
        uint64_t x = (uint64_t)time(nullptr) * 0x9E3779B97F4A7C15ull ^ (uint64_t)getpid() * 0xBF58476D1CE4E5B9ull;
        x ^= x >> 31;
        return (uint32_t)x;
    }()};
    return next.fetch_add(1u) & 0xfffffu;
}

// the status word is read by agent-scope loads in the kernels: cleared by the
// same kind of stores (gsm_kernels.hip launch_granule_init), synchronously
hipError_t clear_status(gsm_handle *h) {
    hipError_t e = gsm::launch_granule_init(h->roll_status, 16, 0u, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

}  // namespace

// A per-step output field of the slots: every slot redirected at a constant
// stride (base, stride), or none (the bound buffer, stride 0).
template <typename T>
static bool slot_field(const gsm_outputs *o, int n, T *gsm_outputs::*f, T **base, int64_t *stride) {
    T *const b0 = o[0].*f;
    if (!b0) {
        for (int j = 1; j < n; ++j)
            if (o[j].*f) return false;
        return true;
    }
    const int64_t st = n > 1 ? (int64_t)(o[1].*f - b0) : 0;
    for (int j = 0; j < n; ++j)
        if (o[j].*f != b0 + j * st) return false;
    *base = b0;
    *stride = st;
    return true;
}

extern "C" {

int gsm_abi_version(void) { return GSM_ABI_VERSION; }

int gsm_query_sizes(const gsm_config *cfg, gsm_sizes *out) {
    std::string why;
    const int rc = check_config(cfg, &why);
    if (rc) return fail(nullptr, rc, why);
    if (!out) return fail(nullptr, GSM_EINVAL, "sizes is NULL");
    fill_sizes(cfg, out);
    if (out->edge_capacity >= (int64_t)1 << 31 ||
        (int64_t)cfg->n_envs * out->n_entities >= (int64_t)1 << 31)
        return fail(nullptr, GSM_EINVAL, "n_envs too large for int32 edge ids/offsets; shard the envs");
    return GSM_OK;
}

int gsm_create(const gsm_config *cfg, gsm_handle **out) {
    if (!out) return fail(nullptr, GSM_EINVAL, "out is NULL");
    *out = nullptr;
    gsm_sizes sz;
    const int rc = gsm_query_sizes(cfg, &sz);
    if (rc) return rc;
    gsm_handle *h = new (std::nothrow) gsm_handle();
    if (!h) return fail(nullptr, GSM_EINVAL, "out of host memory");
    h->cfg = *cfg;
    h->sz = sz;
    derive(cfg, &h->dp);
    h->dp.edge_capacity = sz.edge_capacity;
    *out = h;
    return GSM_OK;
}

int gsm_bind(gsm_handle *h, const gsm_buffers *b) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (!b) return fail(h, GSM_EINVAL, "buffers is NULL");
    const void *req[] = {b->pos, b->vel, b->step_count, b->episode, b->ep_acc, b->ep_last,
                         b->node_feat, b->reward, b->cost, b->done, b->edge_count,
                         b->block_edge_sum, b->edge_ptr, b->edge_index, b->edge_attr,
                         b->row_mask, b->contact_mask};
    for (const void *q : req)
        if (!q) return fail(h, GSM_EINVAL, "a required buffer pointer is NULL");
    const bool ragged = h->dp.path == gsm::kPathRagged;
    if (ragged && (!b->env_shape || !b->assign))
        return fail(h, GSM_EINVAL, "polygon/line/mixed need the env_shape and assign buffers");
    if (ragged) {
        const hipError_t e = gsm::upload_ragged_tables();
        if (e != hipSuccess) return hip_fail(h, e, "ragged constant tables");
        const int rc = update_block_order(h, nullptr);
        if (rc) return rc;
        const hipError_t es = hipStreamSynchronize(nullptr);   // bind is not stream-ordered
        if (es != hipSuccess) return hip_fail(h, es, "hipStreamSynchronize (block order)");
    }
    if (((uintptr_t)b->pos | (uintptr_t)b->vel | (uintptr_t)b->ep_acc | (uintptr_t)b->ep_last) & 7)
        return fail(h, GSM_EINVAL, "pos/vel/ep_acc/ep_last must be 8-byte aligned");
    gsm::DevParams &p = h->dp;
    p.pos = (float2 *)b->pos;
    p.vel = (float2 *)b->vel;
    p.step_count = b->step_count;
    p.episode = b->episode;
    p.ep_acc = (float2 *)b->ep_acc;
    p.ep_last = (float2 *)b->ep_last;
    p.node_feat = b->node_feat;
    p.reward = b->reward;
    p.cost = b->cost;
    p.done = b->done;
    p.edge_count = b->edge_count;
    p.block_edge_sum = b->block_edge_sum;
    p.edge_ptr = b->edge_ptr;
    p.edge_index = b->edge_index;
    p.edge_attr = b->edge_attr;
    p.row_mask = b->row_mask;
    p.contact_mask = b->contact_mask;
    p.env_shape = b->env_shape;
    p.assign = b->assign;
    p.degenerate = b->degenerate;
    p.lsa_v = (b->lsa_v && b->lsa_col) ? b->lsa_v : nullptr;
    p.lsa_col = p.lsa_v ? b->lsa_col : nullptr;
    p.lsa_stats = b->lsa_stats;
    h->bound = true;
    drop_graph(h);   // a captured graph holds the old pointers
    // (a failure here, e.g. no device yet, leaves the decision to the first
    // step, which reports it)
    if (h->eager_roll < 0 && eager_setup(h) != GSM_OK) h->eager_roll = -1;
    return GSM_OK;
}

int gsm_reset(gsm_handle *h, uint64_t seed, int reseed, const uint8_t *env_mask, void *stream) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (reseed && seed != h->cfg.seed) {
        h->cfg.seed = seed;
        h->dp.seed_lo = (uint32_t)(seed & 0xFFFFFFFFull);
        h->dp.seed_hi = (uint32_t)(seed >> 32);
        drop_graph(h);   // captured auto-resets would use the old key
        if (h->bound) {
            const int rc = update_block_order(h, as_stream(stream));   // mixed: the env shapes follow the seed
            if (rc) return rc;
        }
    }
    return launch(h, GSM_MODE_RESET, nullptr, 0, env_mask, reseed ? 1 : 0, as_stream(stream));
}

int gsm_step(gsm_handle *h, const void *actions, int action_fmt, void *stream) {
    return launch(h, GSM_MODE_STEP, actions, action_fmt, nullptr, 0, as_stream(stream));
}

int gsm_observe(gsm_handle *h, void *stream) {
    return launch(h, GSM_MODE_OBSERVE, nullptr, 0, nullptr, 0, as_stream(stream));
}

// state copies (gsm_state): direction 0 = bound -> caller, 1 = caller -> bound
static int copy_state(gsm_handle *h, const gsm_state *st, int dir, hipStream_t s) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (!h->bound) return fail(h, GSM_ESTATE, "gsm_bind has not been called");
    if (!st) return fail(h, GSM_EINVAL, "state is NULL");
    const gsm::DevParams &p = h->dp;
    const size_t B = (size_t)p.B;
    struct F { void *caller, *bound; size_t bytes; } f[] = {
        {st->pos, p.pos, B * p.E * 8}, {st->vel, p.vel, B * p.N * 8},
        {st->step_count, p.step_count, B * 4}, {st->episode, p.episode, B * 4},
        {st->ep_acc, p.ep_acc, B * 8}, {st->ep_last, p.ep_last, B * 8},
        {st->env_shape, p.env_shape, B * 4},
    };
    for (const F &x : f) {
        if (!x.caller || !x.bound) continue;   // skipped (env_shape: navigation binds none)
        const hipError_t e = dir ? hipMemcpyAsync(x.bound, x.caller, x.bytes, hipMemcpyDeviceToDevice, s)
                                 : hipMemcpyAsync(x.caller, x.bound, x.bytes, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hip_fail(h, e, "hipMemcpyAsync (state)");
    }
    return GSM_OK;
}

int gsm_get_state(gsm_handle *h, const gsm_state *out, void *stream) {
    return copy_state(h, out, 0, as_stream(stream));
}

int gsm_set_state(gsm_handle *h, const gsm_state *in, void *stream) {
    const int rc = copy_state(h, in, 1, as_stream(stream));
    if (rc) return rc;
    return launch(h, GSM_MODE_OBSERVE, nullptr, 0, nullptr, 0, as_stream(stream));
}

int gsm_step_into(gsm_handle *h, const void *actions, int action_fmt, const gsm_outputs *out, void *stream) {
    if (!out) return fail(h, GSM_EINVAL, "outputs is NULL");
    return launch(h, GSM_MODE_STEP, actions, action_fmt, nullptr, 0, as_stream(stream), out);
}

int gsm_observe_into(gsm_handle *h, const gsm_outputs *out, void *stream) {
    if (!out) return fail(h, GSM_EINVAL, "outputs is NULL");
    return launch(h, GSM_MODE_OBSERVE, nullptr, 0, nullptr, 0, as_stream(stream), out);
}

static int capture_impl(gsm_handle *h, int32_t slot, const void *actions, int64_t stride, int32_t n_actions,
                        int32_t n_steps, int action_fmt, int flags, const gsm_outputs *per_step);
static int capture_roll(gsm_handle *h, int32_t slot, const void *actions, int64_t stride, int32_t n_actions,
                        int32_t n_steps, int action_fmt, int flags, const gsm_outputs *per_step = nullptr,
                        bool fallback = false);
constexpr int kRollIneligible = 1;   // capture_roll(fallback = true): use the per-step chain instead

int gsm_graph_capture(gsm_handle *h, int32_t slot, const void *actions, int64_t stride,
                      int32_t n_actions, int32_t n_steps, int action_fmt, int flags) {
    return capture_impl(h, slot, actions, stride, n_actions, n_steps, action_fmt, flags, nullptr);
}

int gsm_graph_capture_into(gsm_handle *h, int32_t slot, const void *actions, int64_t stride,
                           int32_t n_actions, int32_t n_steps, int action_fmt, const gsm_outputs *per_step) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (!h->bound) return fail(h, GSM_ESTATE, "gsm_bind has not been called");
    if (bad_slot(slot)) return fail(h, GSM_EINVAL, "bad graph slot");
    if (!per_step) return fail(h, GSM_EINVAL, "per_step outputs is NULL");
    // one rollout launch when the config has a rollout kernel and the slots
    // sit at constant strides (a rollout buffer), else the per-step chain
    const int rc = capture_roll(h, slot, actions, stride, n_actions, n_steps, action_fmt, 0, per_step, true);
    if (rc != kRollIneligible) return rc;
    return capture_impl(h, slot, actions, stride, n_actions, n_steps, action_fmt, 0, per_step);
}

// Step k's outputs at base + k * stride, from a rollout buffer's slots:
// *regular where every redirected field sits at a constant stride. p ends up
// describing the last slot (redirect validates each one).
static int roll_out_slots(gsm_handle *h, const gsm_outputs *per_step, int n_steps, bool ragged, gsm::DevParams *p,
                          gsm::DevParams::RollOut *ro, bool *regular) {
    int64_t cost_s = 0;
    bool ok = slot_field(per_step, n_steps, &gsm_outputs::node_feat, &ro->nf, &ro->nf_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::reward, &ro->rew, &ro->rc_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::cost, &ro->cost, &cost_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::done, &ro->done, &ro->done_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::edge_count, &ro->ecount, &ro->ec_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::edge_ptr, &ro->eptr, &ro->ep_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::edge_index, &ro->eidx, &ro->ei_s) &&
              slot_field(per_step, n_steps, &gsm_outputs::edge_attr, &ro->eattr, &ro->ea_s) &&
              cost_s == ro->rc_s && (ragged ? slot_field(per_step, n_steps, &gsm_outputs::assign, &ro->asg, &ro->as_s)
                                            : !per_step[0].assign);
    for (int j = 0; ok && j < n_steps; ++j) {
        const int rc = redirect(h, p, &per_step[j]);
        if (rc) return rc;
        ok = !per_step[0].edge_index || per_step[j].edge_capacity == per_step[0].edge_capacity;
    }
    if (ok && per_step[0].edge_index) ro->cap = per_step[0].edge_capacity;
    *regular = ok;
    return GSM_OK;
}

// What a rollout capture decides before it acquires anything.
struct RollPlan {
    const char *refused = nullptr;   // why this is not one rollout launch (then nothing else is set)
    gsm::Knobs knobs;
    gsm::RollForm form{};
    gsm::DevParams p;                // the launch's arguments but for p.roll (the outputs: the last slot's)
    gsm::RollShape shape{};
    gsm::GranLayout lay{};
    int n_cu = 0;
    int depth = 0;                   // ragged: edges packed this many steps late
    size_t slab_bytes = 0;           // ragged: the env slabs it needs
};

static int plan_roll(gsm_handle *h, int64_t stride, int32_t n_actions, int32_t n_steps, int action_fmt,
                     const gsm_outputs *per_step, RollPlan *plan) {
    plan->knobs = read_knobs();
    gsm::DevParams &p = plan->p;
    p = h->dp;
    p.mode = GSM_MODE_STEP;
    p.action_fmt = action_fmt;
    p.env_mask = nullptr;
    p.reseed = 0;
    const bool tile = p.path == gsm::kPathTile, ragged = p.path == gsm::kPathRagged;
    const bool slots = per_step != nullptr;
    // what the launch runs: the kernel, its workgroup, envs per workgroup and
    // LDS. The segmented path chooses among several kernels by the launch's
    // arguments (gsm_seg_kernels.hip pick_roll_seg); of those it depends on,
    // only nf_full changes below (redirect, rollout buffers only), and a
    // rollout buffer's choice does not depend on it
    plan->form = tile ? gsm::RollForm{gsm::roll_tile_kernel_fn(p, slots), gsm::block_threads(p), 1,
                                      gsm::roll_tile_kernel_lds(p), false}
                      : ragged ? gsm::RollForm{gsm::roll_ragged_kernel_fn(p, slots), gsm::block_threads(p),
                                               gsm::kWavesPerBlock, gsm::roll_ragged_kernel_lds(p), true}
                               : gsm::roll_seg_form(p, slots, plan->knobs.pace_on);
    const gsm::RollForm &form = plan->form;
    if (!form.fn) {
        plan->refused = "GSM_GRAPH_ROLL: no fused rollout kernel for this config (segmented path with a compiled "
                        "shape, tile path with the symmetric sweep, or a ragged batch)";
        return GSM_OK;
    }
    // step k's outputs at base + k * stride (a rollout buffer's slots) or all
    // in the bound buffers
    p.ro = bound_roll_out(p);
    if (per_step) {
        bool regular = false;
        const int rc = roll_out_slots(h, per_step, n_steps, ragged, &p, &p.ro, &regular);
        if (rc) return rc;
        if (!regular) {
            plan->refused = "GSM_GRAPH_ROLL: per-step outputs must sit at constant strides";
            return GSM_OK;
        }
    }
    // segmented / ragged rollout: one env per wave whatever the config's G (4
    // per workgroup), two per wave (8, gsm_roll_pair_kernel), or four small
    // envs per wave (16 per workgroup); per-wave granules (Xfer) for the
    // ragged and packed small envs, the other segmented shapes and the tile
    // path look back per workgroup
    plan->shape = gsm::roll_shape(kRollConsts, n_steps, (p.B + form.envs - 1) / form.envs, form.per_wave);
    if (ragged) plan->shape.place_words = gsm::PlaceArea::words(plan->shape.xW);
    int per_cu = 0;
    const hipError_t e = query_round(form, &per_cu, &plan->n_cu);
    if (e != hipSuccess) return hip_fail(h, e, "occupancy query");
    const gsm::RollLimit limit =
        gsm::roll_limits(kRollConsts, plan->shape, (uint64_t)n_actions, (uint64_t)stride, per_cu, plan->n_cu);
    if (limit != gsm::RollLimit::kNone) {
        plan->refused = gsm::roll_limit_text(limit);
        return GSM_OK;
    }
    plan->lay = gsm::gran_layout(kRollConsts, plan->shape);
    if (ragged) {
        // the env slabs of depth + 1 steps (each env's edges at a fixed stride:
        // max_edges_per_env + 1 words, then as many distances)
        plan->depth = plan->knobs.depth;
        plan->slab_bytes = (size_t)(plan->depth + 1) * p.B * 8 * ((size_t)h->sz.max_edges_per_env + 1);
    }
    return GSM_OK;
}

// A deeper ring than before: the slabs are replaced by `fresh`, and every
// earlier ragged rollout slot is re-pointed at them (a slab holds only the
// edges in flight within one launch, so nothing in the old one outlives its
// launches: drained first).
static int replace_slabs(gsm_handle *h, void *fresh, size_t bytes) {
    if (h->slab) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            return hip_fail(h, e, "hipDeviceSynchronize (slabs)");
        }
        (void)hipFree(h->slab);
    }
    for (auto &o : h->slots)
        if (o.roll && o.args.path == gsm::kPathRagged) {
            o.args.roll.slab = (int32_t *)fresh;
            o.args.roll.slab_end = (int32_t *)((char *)fresh + bytes);
        }
    h->slab = fresh;
    h->slab_bytes = bytes;
    return GSM_OK;
}

// Fused rollout (GSM_GRAPH_ROLL): ONE gsm_roll_seg_kernel /
// gsm_roll_tile_kernel / gsm_roll_ragged_kernel launch for all n_steps steps
// and all their edges (a tail after the loop emits the last ones; that launch
// also advances the granule epoch). Every output equals the per-step chain's.
// The slot stores the launch (kernel, grid, arguments), not a graph:
// gsm_graph_launch completes the arguments and dispatches it.
static int capture_roll(gsm_handle *h, int32_t slot, const void *actions, int64_t stride, int32_t n_actions,
                        int32_t n_steps, int action_fmt, int flags, const gsm_outputs *per_step, bool fallback) {
    // 1. the arguments. Every caller checks the first three; repeated so that
    // no path reaches the slot or the bound buffers without them
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (!h->bound) return fail(h, GSM_ESTATE, "gsm_bind has not been called");
    if (bad_slot(slot)) return fail(h, GSM_EINVAL, "bad graph slot");
    if (flags & ~(GSM_GRAPH_ROLL | GSM_GRAPH_TIME_ENDS))
        return fail(h, GSM_EINVAL, "GSM_GRAPH_ROLL combines with GSM_GRAPH_TIME_ENDS only");
    if (!actions || n_actions < 1 || stride < 0) return fail(h, GSM_EINVAL, "bad capture arguments");
    if (n_steps < 1) return fail(h, GSM_EINVAL, "n_steps must be >= 1");
    if (action_fmt < GSM_ACT_ONEHOT || action_fmt > GSM_ACT_CONT) return fail(h, GSM_EINVAL, "bad action_fmt");

    // 2. the plan: kernel, outputs, limits, granule layout. Where this cannot
    // be one rollout launch, a caller that can fall back takes the per-step
    // chain (which needs none of what follows), any other gets the reason
    RollPlan plan;
    if (const int rc = plan_roll(h, stride, n_actions, n_steps, action_fmt, per_step, &plan)) return rc;
    if (plan.refused) return fallback ? kRollIneligible : fail(h, GSM_EINVAL, plan.refused);
    auto no_memory = [&](hipError_t err, const char *what) {
        return fallback ? kRollIneligible : hip_fail(h, err, what);
    };
    const gsm::RollShape &shape = plan.shape;
    const gsm::GranLayout &lay = plan.lay;
    const bool ragged = plan.p.path == gsm::kPathRagged;

    // 3. what the handle's rollout slots share
    hipError_t e = hipSuccess;
    if (h->slab_bytes < plan.slab_bytes) {
        void *fresh = nullptr;
        e = hipMalloc(&fresh, plan.slab_bytes);
        if (e != hipSuccess) return no_memory(e, "hipMalloc (rollout edge slabs)");
        if (const int rc = replace_slabs(h, fresh, plan.slab_bytes)) return rc;
    }
    if (const int rc = ensure_status(h)) return rc;
    if (const int rc = ensure_cap_stream(h)) return rc;
    // in the bound buffers, the edges of every step but the last go to a
    // scratch of the bound capacity (DevParams::RollOut); allocated once
    if (!per_step && !h->edge_scratch) {
        e = hipMalloc(&h->edge_scratch, 12 * (size_t)h->sz.edge_capacity);
        if (e != hipSuccess) {
            h->edge_scratch = nullptr;
            return no_memory(e, "hipMalloc (rollout edge scratch)");
        }
    }

    // 4. the slot: its granules, its timing events, the stored launch
    gsm_handle::Slot &sl = h->slots[slot];
    drop_slot(sl);
    e = gran_malloc(&sl.gran_base, &sl.gran, lay.bytes);
    if (e != hipSuccess) return no_memory(e, "hipMalloc (rollout granules)");
    // Zeroed once (tag 0 never matches). Every launch then takes its own
    // epoch (next_launch_epoch, set in gsm_graph_launch): a memset or
    // store-zeroed allocation was seen to still show an agent-scope load
    // granules left at that address by a freed slot's last launch, and with
    // per-capture epochs those could carry this slot's tags. The untagged
    // chunk sums and counters are zeroed by the launch before the one that
    // uses them.
    e = gsm::launch_granule_init(sl.gran, lay.bytes, 0u, h->cap_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->cap_stream);
    if (e != hipSuccess) { drop_slot(sl); return hip_fail(h, e, "rollout granule init"); }
    sl.lay = lay;
    sl.paced = plan.knobs.pace_on && lay.pace[0].bytes != 0;
    // timing (TIME_ENDS): the events bracket the rollout launch alone, so
    // gsm_graph_kernel_ms reports its time per step
    sl.events.resize((flags & GSM_GRAPH_TIME_ENDS) ? 2 : 0, nullptr);
    for (auto &ev : sl.events) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) { drop_slot(sl); return hip_fail(h, e, "hipEventCreate"); }
    }
    // all steps and their edges in one launch; the last step's sums go to the
    // bound edge-sum buffer (later eager emits read it)
    gsm::DevParams &p = plan.p;
    p.actions = actions;
    if (!per_step) {
        p.ro.eidx_mid = (int32_t *)h->edge_scratch;
        p.ro.eattr_mid = (float *)(p.ro.eidx_mid + 2 * h->sz.edge_capacity);
    }
    gsm::DevParams::Roll r{};
    r.actions = (const char *)actions;
    r.stride = stride;
    r.n_actions = n_actions;
    r.K = n_steps;
    r.xW = shape.xW;
    r.xNG = shape.xNG;
    r.depth = plan.depth;
    r.slab_e = h->sz.max_edges_per_env;
    // ragged mixed: envs dealt to the SIMDs by cost when the grid fills every
    // SIMD with the same number of waves (GSM_ROLL_PLACE=0: env = wave index)
    r.place_S = 4 * plan.n_cu;
    if (ragged && h->place_order && plan.knobs.place && shape.xW % r.place_S == 0) r.place_R = shape.xW / r.place_S;
    r.place = r.place_R ? h->place_order : nullptr;
    r.place_force = plan.knobs.place_force;
    r.gran = gran_at<uint64_t>(sl.gran, lay.granules.off);
    r.gran_end = gran_at<uint64_t>(sl.gran, lay.bytes);
    r.status = h->roll_status;
    r.slab = (int32_t *)h->slab;
    r.slab_end = h->slab ? (int32_t *)((char *)h->slab + h->slab_bytes) : nullptr;
    r.pace_q = plan.knobs.pace_q;
    r.csum_stride = kCsumStride;   // (epoch, csum, pace: set per launch, gsm_graph_launch)
    p.roll = r;
    sl.fn = plan.form.fn;
    sl.grid = dim3(shape.nb);
    sl.block = dim3(plan.form.threads);
    sl.lds = (unsigned)plan.form.lds;
    sl.args = p;
    sl.each = false;
    sl.kern = GSM_GRAPH_STEP;
    sl.steps = n_steps;
    sl.roll = true;
    return GSM_OK;
}

int gsm_graph_info(gsm_handle *h, int32_t slot, int32_t *steps, int32_t *fused) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (bad_slot(slot)) return fail(h, GSM_EINVAL, "bad graph slot");
    const gsm_handle::Slot &sl = h->slots[slot];
    if (steps) *steps = sl.captured() ? sl.steps : 0;
    if (fused) *fused = sl.roll ? 1 : 0;
    return GSM_OK;
}

int gsm_graph_roll_status(gsm_handle *h, int32_t *gave_up) {
    if (!h || !gave_up) return fail(h, GSM_EINVAL, "NULL argument");
    *gave_up = 0;
    if (!h->roll_status) return GSM_OK;
    uint32_t v = 0;
    hipError_t e = hipMemcpy(&v, h->roll_status, sizeof v, hipMemcpyDeviceToHost);
    if (e == hipSuccess && v) {   // word 0 only (words 1-2: the placement counts)
        e = gsm::launch_granule_init(h->roll_status, sizeof(uint32_t), 0u, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) return hip_fail(h, e, "rollout status read");
    *gave_up = (int32_t)v;   // the reason code (gsm.h), 0 if none
    return GSM_OK;
}

int gsm_graph_roll_placement(gsm_handle *h, int64_t *dealt, int64_t *fallback) {
    if (!h || !dealt || !fallback) return fail(h, GSM_EINVAL, "NULL argument");
    *dealt = *fallback = 0;
    if (!h->roll_status) return GSM_OK;
    uint32_t v[2] = {0, 0};
    hipError_t e = hipMemcpy(v, h->roll_status + 1, sizeof v, hipMemcpyDeviceToHost);
    if (e == hipSuccess && (v[0] || v[1])) {
        e = gsm::launch_granule_init(h->roll_status + 1, sizeof v, 0u, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) return hip_fail(h, e, "rollout placement read");
    *fallback = v[0];
    *dealt = v[1];
    return GSM_OK;
}

static int capture_impl(gsm_handle *h, int32_t slot, const void *actions, int64_t stride, int32_t n_actions,
                        int32_t n_steps, int action_fmt, int flags, const gsm_outputs *per_step) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (!h->bound) return fail(h, GSM_ESTATE, "gsm_bind has not been called");
    if (bad_slot(slot)) return fail(h, GSM_EINVAL, "bad graph slot");
    if (flags & GSM_GRAPH_ROLL) return capture_roll(h, slot, actions, stride, n_actions, n_steps, action_fmt, flags);
    int kern = flags & (GSM_GRAPH_STEP | GSM_GRAPH_EMIT);
    if (!kern) kern = GSM_GRAPH_STEP | GSM_GRAPH_EMIT;
    const bool each = (flags & GSM_GRAPH_TIME_EACH) != 0, ends = (flags & GSM_GRAPH_TIME_ENDS) != 0;
    const bool lag_only = (flags & GSM_GRAPH_LAG_ONLY) != 0;
    const bool can_lag = gsm::lag_step_kernel_fn(h->dp) != nullptr;
    if (lag_only && (!can_lag || each || (flags & (GSM_GRAPH_STEP | GSM_GRAPH_EMIT | GSM_GRAPH_UNFUSED))))
        return fail(h, GSM_EINVAL, "GSM_GRAPH_LAG_ONLY: segmented / ragged configs only, no other kernel/timing-each flags");
    if (lag_only) kern = GSM_GRAPH_STEP;
    // lagged emission: step_0, lag_step_1 .. lag_step_{T-1}, emit_{T-1}
    const bool lag = lag_only || (can_lag && !each && kern == (GSM_GRAPH_STEP | GSM_GRAPH_EMIT) &&
                                  !(flags & GSM_GRAPH_UNFUSED));
    if ((kern & GSM_GRAPH_STEP) && (!actions || n_actions < 1 || stride < 0))
        return fail(h, GSM_EINVAL, "bad capture arguments");
    if (n_steps < 1) return fail(h, GSM_EINVAL, "n_steps must be >= 1");
    if (action_fmt < GSM_ACT_ONEHOT || action_fmt > GSM_ACT_CONT) return fail(h, GSM_EINVAL, "bad action_fmt");
    gsm_handle::Slot &sl = h->slots[slot];
    drop_slot(sl);
    hipError_t e;
    if (lag && !h->bsum_alt) {
        e = hipMalloc(&h->bsum_alt, (size_t)h->sz.n_blocks * sizeof(int32_t) + 16);
        if (e != hipSuccess) { h->bsum_alt = nullptr; return hip_fail(h, e, "hipMalloc (edge-sum buffer)"); }
    }
    if (const int rc = ensure_cap_stream(h)) return rc;
    // The graph is built node by node (a linear chain) rather than by stream
    // capture: event-record nodes for timing are then explicit (the capture
    // path of the HIP runtime bundled with PyTorch rejects
    // hipEventRecordWithFlags(..., hipEventRecordExternal)).
    //   TIME_EACH:  [E0] step_0 [E1] emit_0 [E2] step_1 ...   (events: 2 per step + 1)
    //   TIME_ENDS:  [E0] step_0 emit_0 step_1 ... [E1]
    const size_t n_ev = each ? 2 * (size_t)n_steps + 1 : (ends ? 2 : 0);
    sl.events.resize(n_ev, nullptr);
    for (auto &ev : sl.events) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) { drop_slot(sl); return hip_fail(h, e, "hipEventCreate"); }
    }
    sl.each = each;
    sl.kern = kern;
    e = hipGraphCreate(&sl.graph, 0);
    if (e != hipSuccess) { drop_slot(sl); return hip_fail(h, e, "hipGraphCreate"); }
    if (lag) {   // the ragged lagged step's bounded wait reports through the status word
        const int rc = ensure_status(h);
        if (rc) { drop_slot(sl); return rc; }
    }
    gsm::DevParams p = h->dp;
    p.mode = GSM_MODE_STEP;
    p.action_fmt = action_fmt;
    p.env_mask = nullptr;
    p.reseed = 0;
    if (lag) p.roll.status = h->roll_status;
    hipGraphNode_t prev = nullptr;
    const char *what = "";
    int at = 0;
    auto add_event = [&](hipEvent_t ev) -> hipError_t {
        hipGraphNode_t n;
        const hipError_t r = hipGraphAddEventRecordNode(&n, sl.graph, prev ? &prev : nullptr, prev ? 1 : 0, ev);
        if (r == hipSuccess) prev = n;
        return r;
    };
    auto add_kernel = [&](const void *fn, size_t lds) -> hipError_t {
        hipKernelNodeParams kp = {};
        void *args[] = {&p};
        kp.func = const_cast<void *>(fn);
        kp.gridDim = dim3(fn == gsm::emit_kernel_fn(p) ? gsm::grid_blocks(p) : gsm::step_grid_blocks(p));
        kp.blockDim = dim3(gsm::block_threads(p));
        kp.sharedMemBytes = (unsigned)lds;
        kp.kernelParams = args;
        kp.extra = nullptr;
        hipGraphNode_t n;
        const hipError_t r = hipGraphAddKernelNode(&n, sl.graph, prev ? &prev : nullptr, prev ? 1 : 0, &kp);
        if (r == hipSuccess) prev = n;
        return r;
    };
    what = "event node";
    e = n_ev ? add_event(sl.events[0]) : hipSuccess;
    const gsm::DevParams p_bound = p;
    // edge-sum halves: the bound buffer holds the sums of the current state
    // before and after every graph (eager emits read it); a lagged chain
    // alternates so that its last step writes the bound half.
    int32_t *half[2] = {p_bound.block_edge_sum, h->bsum_alt};
    gsm::DevParams last = p_bound;   // outputs of the previous step
    for (int t = 0; t < n_steps && e == hipSuccess; ++t) {
        at = t;
        if (per_step) {
            p = p_bound;
            const int rc = redirect(h, &p, &per_step[t]);
            if (rc) {
                drop_slot(sl);
                return rc;
            }
        }
        const bool lag_node = lag && (lag_only || t > 0);
        if (lag) {
            // lag-only: node t reads half t%2; chain: node t writes half (T-1-t)%2
            const int w = lag_only ? (t + 1) % 2 : (n_steps - 1 - t) % 2;
            p.block_edge_sum = half[w];
            p.lag = gsm::DevParams::Lag{half[1 - w], last.edge_count, last.edge_ptr, last.edge_index,
                                        last.edge_attr, last.edge_capacity};
        }
        if (kern & GSM_GRAPH_STEP) {
            p.actions = (const char *)actions + (int64_t)(t % n_actions) * stride;
            what = lag_node ? "lagged step kernel node" : "step kernel node";
            e = add_kernel(lag_node ? gsm::lag_step_kernel_fn(p) : gsm::step_kernel_fn(p), gsm::step_kernel_lds(p));
            if (e == hipSuccess && each) { what = "event node"; e = add_event(sl.events[2 * t + 1]); }
        }
        // the two-kernel chain emits every step; a lagged chain only the last
        if (e == hipSuccess && (kern & GSM_GRAPH_EMIT) && (!lag || t == n_steps - 1)) {
            what = "emit kernel node";
            e = add_kernel(gsm::emit_kernel_fn(p), gsm::emit_kernel_lds(p));
        }
        if (e == hipSuccess && each) { what = "event node"; e = add_event(sl.events[2 * t + 2]); }
        last = p;
    }
    if (e == hipSuccess && ends && !each) { what = "event node"; e = add_event(sl.events[1]); }
    if (e != hipSuccess) {
        drop_slot(sl);
        char where[96];
        snprintf(where, sizeof where, "graph build (step %d, %s)", at, what);
        return hip_fail(h, e, where);
    }
    e = hipGraphInstantiate(&sl.exec, sl.graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { drop_slot(sl); return hip_fail(h, e, "hipGraphInstantiate"); }
    e = hipGraphUpload(sl.exec, h->cap_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->cap_stream);
    if (e != hipSuccess) { drop_slot(sl); return hip_fail(h, e, "hipGraphUpload"); }
    sl.steps = n_steps;
    return GSM_OK;
}

int gsm_graph_launch(gsm_handle *h, int32_t slot, void *stream) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (bad_slot(slot)) return fail(h, GSM_EINVAL, "bad graph slot");
    gsm_handle::Slot &sl = h->slots[slot];
    if (!sl.captured()) return fail(h, GSM_ESTATE, "no graph captured in this slot");
    if (sl.roll) {   // a rollout slot: its stored kernel launch
        // (GSM_GRAPH_TIME_ENDS: events recorded on the stream around it — as
        // graph event nodes they added ≈7% to the launch they bracketed)
        hipStream_t st = as_stream(stream);
        // Every launch takes its own epoch and its half of the slot's double
        // buffers, set in the arguments here: a launch captured into the
        // caller's graph would replay one of each every time (stale granules
        // matching its tags, unzeroed chunk sums)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hipError_t e = hipStreamIsCapturing(st, &cs);
        if (e != hipSuccess) return hip_fail(h, e, "hipStreamIsCapturing");
        if (cs != hipStreamCaptureStatusNone)
            return fail(h, GSM_ESTATE, "a rollout graph cannot be launched into a stream capture (every launch "
                                       "takes its own hand-off epoch); capture the per-step chain instead");
        if (!h->roll_done) {
            e = hipEventCreateWithFlags(&h->roll_done, hipEventDisableTiming);
            if (e != hipSuccess) { h->roll_done = nullptr; return hip_fail(h, e, "hipEventCreate (rollout)"); }
        }
        // rollout launches of one handle never overlap: they share its
        // scratch and state, so a launch on another stream than the previous
        // one waits for it, asynchronously (an event recorded behind every
        // launch: nothing here depends on the previous stream still existing)
        if (h->roll_launched && h->roll_stream != st) {
            e = hipStreamWaitEvent(st, h->roll_done, 0);
            if (e != hipSuccess) return hip_fail(h, e, "hipStreamWaitEvent (previous rollout launch)");
        }
        sl.args.roll.epoch = fresh_epoch(sl.last_epoch);   // copied with the arguments at the launch
        const int par = (int)(sl.launches & 1u);
        if (sl.lay.csum[0].bytes) {
            sl.args.roll.csum = gran_at<uint64_t>(sl.gran, sl.lay.csum[par].off);
            sl.args.roll.csum_next = gran_at<uint64_t>(sl.gran, sl.lay.csum[1 - par].off);
        }
        if (sl.paced) {
            sl.args.roll.pace = gran_at<uint32_t>(sl.gran, sl.lay.pace[par].off);
            sl.args.roll.pace_next = gran_at<uint32_t>(sl.gran, sl.lay.pace[1 - par].off);
        }
        void *args[] = {&sl.args};
        e = sl.events.empty() ? hipSuccess : hipEventRecord(sl.events.front(), st);
        if (e == hipSuccess) e = hipLaunchKernel(sl.fn, sl.grid, sl.block, args, sl.lds, st);
        if (e != hipSuccess) return hip_fail(h, e, "hipLaunchKernel (rollout)");
        sl.launches++;
        h->roll_stream = st;
        h->roll_launched = true;
        e = sl.events.empty() ? hipSuccess : hipEventRecord(sl.events.back(), st);
        if (e == hipSuccess) e = hipEventRecord(h->roll_done, st);
        if (e != hipSuccess) return hip_fail(h, e, "hipEventRecord (rollout)");
        return GSM_OK;
    }
    const hipError_t e = hipGraphLaunch(sl.exec, as_stream(stream));
    if (e != hipSuccess) return hip_fail(h, e, "hipGraphLaunch");
    return GSM_OK;
}

int gsm_graph_kernel_ms(gsm_handle *h, int32_t slot, float *step_ms, float *emit_ms, float *total_ms) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    if (bad_slot(slot)) return fail(h, GSM_EINVAL, "bad graph slot");
    const gsm_handle::Slot &sl = h->slots[slot];
    if (!sl.captured() || sl.events.empty()) return fail(h, GSM_ESTATE, "no timed graph in this slot");
    float total = 0;
    hipError_t e = hipEventElapsedTime(&total, sl.events.front(), sl.events.back());
    if (e != hipSuccess) return hip_fail(h, e, "hipEventElapsedTime");
    double a = 0, b = 0;
    if (sl.each) {
        for (int t = 0; t < sl.steps; ++t) {
            float x = 0, y = 0;
            if (sl.kern & GSM_GRAPH_STEP) e = hipEventElapsedTime(&x, sl.events[2 * t], sl.events[2 * t + 1]);
            if (e == hipSuccess && (sl.kern & GSM_GRAPH_EMIT))
                e = hipEventElapsedTime(&y, sl.events[2 * t + ((sl.kern & GSM_GRAPH_STEP) ? 1 : 0)],
                                        sl.events[2 * t + 2]);
            if (e != hipSuccess) return hip_fail(h, e, "hipEventElapsedTime");
            a += x;
            b += y;
        }
        a /= sl.steps;
        b /= sl.steps;
    } else {
        // back-to-back launches of one kind: the mean per launch
        if (sl.kern == GSM_GRAPH_STEP) a = total / sl.steps;
        else if (sl.kern == GSM_GRAPH_EMIT) b = total / sl.steps;
    }
    if (step_ms) *step_ms = (float)a;
    if (emit_ms) *emit_ms = (float)b;
    if (total_ms) *total_ms = total;
    return GSM_OK;
}

int gsm_debug_set_stamps(gsm_handle *h, void *stamps) {
    if (!h) return fail(nullptr, GSM_EINVAL, "handle is NULL");
    h->dp.stamps = (uint64_t *)stamps;
    drop_graph(h);
    return GSM_OK;
}

int gsm_destroy(gsm_handle *h) {
    if (!h) return GSM_OK;
    drop_graph(h);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->bsum_alt) (void)hipFree(h->bsum_alt);
    if (h->roll_status) (void)hipFree(h->roll_status);
    if (h->edge_scratch) (void)hipFree(h->edge_scratch);
    if (h->slab) (void)hipFree(h->slab);
    if (h->eager_base) (void)hipFree(h->eager_base);
    if (h->order_copied) (void)hipEventSynchronize(h->order_copied);
    if (h->block_order) (void)hipFree(h->block_order);
    if (h->order_host) (void)hipHostFree(h->order_host);
    if (h->order_copied) (void)hipEventDestroy(h->order_copied);
    if (h->roll_done) (void)hipEventDestroy(h->roll_done);
    delete h;
    return GSM_OK;
}

int gsm_last_error(const gsm_handle *h, char *buf, size_t len) {
    const std::string &m = h ? h->err : g_err;
    if (buf && len) {
        const size_t n = m.size() < len - 1 ? m.size() : len - 1;
        memcpy(buf, m.data(), n);
        buf[n] = 0;
    }
    return (int)m.size();
}

}  // extern "C"
