// gsm_roll_plan.h — what the host decides about a rollout launch before it
// touches the GPU: the layout of the hand-off granule allocation, the shape
// limits of the rollout kernels, and the environment knobs. Plain C++17 with
// no HIP and no libc, so a host compiler alone builds and tests it
// (tests/test_roll_plan.py); gsm_abi.hip passes in the constants of
// gsm_internal.h (RollConsts) and the process's getenv.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gsm {

// the constants of gsm_internal.h that the plan depends on
struct RollConsts {
    int wave;             // kWave
    int waves_per_block;  // kWavesPerBlock
    int prefix_chunk;     // kPrefixChunk: workgroups per chunk sum
    int csum_stride;      // u64 words between chunk sums (each on a 64-byte line of its own)
    int max_steps;        // kRollMaxSteps
    size_t pace_words;    // u32 words of one half of the pace counters (kPaceKeys * kPaceStride)
    size_t epoch_words;   // u32 words of the eager step's epoch replicas (kEpochReps * kEpochStride)
};

// The grid of a rollout launch as its hand-off sees it. Per-wave hand-off
// (ragged and packed small envs): counts [K][xW] and group sums [K][xNG].
// Otherwise (one env per wave or per workgroup, the tile path) the one-hop
// prefix: aggregates [K][nb] and nc chunk sums per step.
struct RollShape {
    int K, nb;
    bool per_wave;
    int xW, xNG;          // waves of the grid, groups of `wave` of them
    size_t nc;            // chunk sums per step
    size_t place_words;   // ragged: the u64 words of its PlaceArea, else 0
    bool eager;           // the one-launch eager step: K = 1, no pacing, device-side epoch replicas
};

inline RollShape roll_shape(const RollConsts &c, int K, int nb, bool per_wave, bool eager = false) {
    RollShape s{};
    s.K = K;
    s.nb = nb;
    s.per_wave = per_wave;
    s.xW = nb * c.waves_per_block;
    s.xNG = (s.xW + c.wave - 1) / c.wave;
    s.nc = ((size_t)nb + c.prefix_chunk - 1) / c.prefix_chunk;
    s.eager = eager;
    return s;
}

// The granule allocation, as byte offsets from the start of its used bytes
// (gran_malloc places them at the end of whole pages): a 16-byte header
// (unused), the 8-byte granules, two halves of chunk sums (a launch uses one
// and zeroes the other for the next), two halves of pace counters, the ragged
// rollout's placement words, the eager step's epoch replicas. A region that a
// launch form does not have is empty. Granules are zeroed once (they are
// tagged with the launch epoch, so replays never clear them).
struct GranLayout {
    struct Region {
        size_t off, bytes;
    };
    Region header, granules, csum[2], pace[2], place, epoch;
    size_t bytes;
    size_t csum_half;   // u64 words of one half of the chunk sums
};

inline GranLayout gran_layout(const RollConsts &c, const RollShape &s) {
    GranLayout g{};
    const bool one_hop = !s.per_wave;
    g.csum_half = one_hop ? (size_t)s.K * s.nc * c.csum_stride : 0;
    const size_t pace_half = one_hop && !s.eager ? c.pace_words * sizeof(uint32_t) : 0;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const GranLayout::Region r{at, bytes};
        at += bytes;
        return r;
    };
    g.header = take(16);
    g.granules = take((size_t)s.K * (s.per_wave ? (size_t)(s.xW + s.xNG) : (size_t)s.nb) * sizeof(uint64_t));
    for (auto &h : g.csum) h = take(g.csum_half * sizeof(uint64_t));
    for (auto &h : g.pace) h = take(pace_half);
    g.place = take(s.place_words * sizeof(uint64_t));
    g.epoch = take(s.eager ? c.epoch_words * sizeof(uint32_t) : 0);
    g.bytes = at;
    return g;
}

// Why a launch cannot run as one rollout kernel, in the order they are tested.
enum class RollLimit { kNone, kActionSpan, kResidency, kSteps, kWaveGroups, kChunkSums };

inline const char *roll_limit_text(RollLimit r) {
    switch (r) {
        case RollLimit::kActionSpan: return "GSM_GRAPH_ROLL: the action rows must span < 4 GiB";
        case RollLimit::kResidency:
            return "GSM_GRAPH_ROLL: the batch exceeds one residency round of the rollout kernel";
        case RollLimit::kSteps: return "GSM_GRAPH_ROLL: n_steps must be <= 4094";
        case RollLimit::kWaveGroups: return "GSM_GRAPH_ROLL: more than 8192 envs in one rollout launch";
        case RollLimit::kChunkSums: return "GSM_GRAPH_ROLL: more than 4096 workgroups in one rollout launch";
        default: return "";
    }
}

// every workgroup resident at once (a workgroup only waits on lower-numbered
// ones, so this is for speed, not for progress)
inline bool fits_one_round(int64_t per_cu, int64_t n_cu, int64_t nb) { return per_cu * n_cu >= nb; }

inline RollLimit roll_limits(const RollConsts &c, const RollShape &s, uint64_t n_actions, uint64_t stride,
                             int64_t per_cu, int64_t n_cu) {
    // the rollout kernels address the action rows with 32-bit byte offsets
    if (n_actions * stride >= ((uint64_t)1 << 32)) return RollLimit::kActionSpan;
    if (!fits_one_round(per_cu, n_cu, s.nb)) return RollLimit::kResidency;
    // granule tags carry the step in 12 bits
    if (s.K > c.max_steps) return RollLimit::kSteps;
    // per-wave granules in groups of `wave` waves, at most 2 * wave groups
    // (one residency round holds <= 8192 waves)
    if (s.per_wave && s.xNG > 2 * c.wave) return RollLimit::kWaveGroups;
    // roll_prefix: one chunk sum per lane
    if (!s.per_wave && s.nc > (size_t)c.wave) return RollLimit::kChunkSums;
    return RollLimit::kNone;
}

// The environment knobs of the rollout host path (A/B and test switches; the
// defaults are the measured best). Read afresh at every capture, at
// eager_setup and at update_block_order — never cached, so a process may
// change them between captures.
struct Knobs {
    // GSM_ROLL_PACE=off|q: pacing off, or the rank offset in quarter steps
    // (default 0; outputs are the same either way)
    bool pace_on = true;
    int pace_q = 0;
    // GSM_ROLL_DEPTH: the ragged rollout packs each step's edges this many
    // steps late (default 4, clamped to 2..max_depth)
    int depth = 4;
    // GSM_ROLL_PLACE=0: env = wave index; =2, a test knob: every wave
    // registers, then the launch decides identity
    bool place = true, place_force = false;
    // GSM_PLACE_XCD=0: one cost order over the whole grid
    bool place_xcd = true;
    // GSM_PLACE_MODEL=a,b,c,d: cost units per env and step, polygon/line
    // a + b N, navigation c + d N
    int64_t model[4] = {200, 20, 10, 3};
    // GSM_EAGER_ONE_LAUNCH=0: gsm_step as the step kernel + the emit kernel
    bool eager_one_launch = true;
};

// a decimal integer as sscanf's %lld takes it (blanks, a sign, digits);
// false, *s unmoved, where there is none
inline bool scan_int(const char **s, int64_t *v) {
    const char *p = *s;
    while (*p == ' ' || (*p >= '\t' && *p <= '\r')) ++p;
    const bool neg = *p == '-';
    if (*p == '-' || *p == '+') ++p;
    if (*p < '0' || *p > '9') return false;
    int64_t x = 0;
    for (; *p >= '0' && *p <= '9'; ++p)
        if (x < ((int64_t)1 << 56)) x = x * 10 + (*p - '0');
    *v = neg ? -x : x;
    *s = p;
    return true;
}

// atoi: 0 where the text does not begin with a number
inline int knob_int(const char *s) {
    int64_t v = 0;
    if (!scan_int(&s, &v)) return 0;
    return v > INT32_MAX ? INT32_MAX : v < INT32_MIN ? INT32_MIN : (int)v;
}

using GetEnv = char *(*)(const char *);

inline Knobs read_knobs(GetEnv get, int max_depth) {
    Knobs k;
    if (const char *ev = get("GSM_ROLL_PACE")) {
        if (ev[0] == 'o' && ev[1] == 'f' && ev[2] == 'f' && !ev[3])
            k.pace_on = false;
        else
            k.pace_q = knob_int(ev) > 0 ? knob_int(ev) : 0;
    }
    if (const char *ev = get("GSM_ROLL_DEPTH")) k.depth = knob_int(ev);
    k.depth = k.depth < 2 ? 2 : k.depth > max_depth ? max_depth : k.depth;
    if (const char *ev = get("GSM_ROLL_PLACE")) {
        k.place = knob_int(ev) != 0;
        k.place_force = knob_int(ev) == 2;
    }
    if (const char *ev = get("GSM_PLACE_XCD")) k.place_xcd = knob_int(ev) != 0;
    if (const char *ev = get("GSM_PLACE_MODEL")) {
        int64_t x[4];
        bool ok = true;   // all four, a comma right behind each of the first three
        for (int i = 0; ok && i < 4; ++i) ok = scan_int(&ev, &x[i]) && (i == 3 || *ev++ == ',');
        for (int i = 0; ok && i < 4; ++i) k.model[i] = x[i];
    }
    if (const char *ev = get("GSM_EAGER_ONE_LAUNCH")) k.eager_one_launch = !(*ev && knob_int(ev) == 0);
    return k;
}

}  // namespace gsm
