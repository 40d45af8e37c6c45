"""The rollout host plan (csrc/gsm_roll_plan.h) on the CPU: the granule
allocation's layout against byte totals worked out by hand from the
expressions it replaced, the shape limits at and below each bound, and the
environment knobs' parsing. A stand-alone C++ program (its own main, only that
header) is built with the address and undefined-behaviour sanitizers and run
directly."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gs-marl_amd" / "csrc"

PROGRAM = r"""
#include "gsm_roll_plan.h"

#include <stdio.h>
#include <string.h>

using namespace gsm;

// gsm_internal.h: kWave, kWavesPerBlock, kPrefixChunk; gsm_abi.hip kCsumStride;
// kRollMaxSteps; kPaceKeys * kPaceStride; kEpochReps * kEpochStride
static const RollConsts C{64, 4, 64, 8, 4094, 2048 * 16, 64 * 16};
static int failed = 0;
#define CHECK(x) \
    do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); failed = 1; } } while (0)

// regions in order, each beginning where the previous one ends, the last
// ending at `bytes`, none negative (as size_t: none past the end), and the
// total as the parent's expression gives it
static void layout(const char *name, const RollShape &s, size_t want) {
    const GranLayout g = gran_layout(C, s);
    const GranLayout::Region r[] = {g.header, g.granules, g.csum[0], g.csum[1], g.pace[0], g.pace[1], g.place, g.epoch};
    size_t at = 0;
    for (const auto &x : r) {
        CHECK(x.off == at);
        CHECK(x.bytes <= g.bytes && x.off <= g.bytes);
        at = x.off + x.bytes;
    }
    CHECK(at == g.bytes);
    CHECK(g.header.bytes == 16 && g.granules.off == 16);
    CHECK(g.csum[0].bytes == g.csum[1].bytes && g.csum[0].bytes == g.csum_half * 8);
    CHECK(g.pace[0].bytes == g.pace[1].bytes);
    CHECK((g.csum[0].bytes != 0) == !s.per_wave);
    CHECK((g.pace[0].bytes != 0) == (!s.per_wave && !s.eager));
    CHECK((g.epoch.bytes != 0) == s.eager);
    CHECK(g.place.bytes == s.place_words * 8);
    printf("%-28s bytes %zu (want %zu)\n", name, g.bytes, want);
    CHECK(g.bytes == want);
}

static const int64_t kFits = 1 << 20;   // a residency round that holds any grid below

static void limits() {
    const RollShape ok = roll_shape(C, 100, 1024, false);
    // the action rows: n_actions * stride < 2^32
    CHECK(roll_limits(C, ok, 1, 0xffffffffull, kFits, 1) == RollLimit::kNone);
    CHECK(roll_limits(C, ok, 2, 0x80000000ull, kFits, 1) == RollLimit::kActionSpan);
    // one residency round: per_cu * n_cu >= nb
    CHECK(roll_limits(C, roll_shape(C, 100, 2048, false), 1, 16, 8, 256) == RollLimit::kNone);
    CHECK(roll_limits(C, roll_shape(C, 100, 2049, false), 1, 16, 8, 256) == RollLimit::kResidency);
    CHECK(fits_one_round(8, 256, 2048) && !fits_one_round(8, 256, 2049));
    // steps: the 12-bit step field of the granule tags
    CHECK(roll_limits(C, roll_shape(C, 4094, 1, false), 1, 16, kFits, 1) == RollLimit::kNone);
    CHECK(roll_limits(C, roll_shape(C, 4095, 1, false), 1, 16, kFits, 1) == RollLimit::kSteps);
    // per-wave hand-off: at most 128 groups of 64 waves (only where it is used)
    CHECK(roll_shape(C, 1, 2048, true).xNG == 128 && roll_shape(C, 1, 2049, true).xNG == 129);
    CHECK(roll_limits(C, roll_shape(C, 1, 2048, true), 1, 16, kFits, 1) == RollLimit::kNone);
    CHECK(roll_limits(C, roll_shape(C, 1, 2049, true), 1, 16, kFits, 1) == RollLimit::kWaveGroups);
    CHECK(roll_limits(C, roll_shape(C, 1, 2049, false), 1, 16, kFits, 1) == RollLimit::kNone);
    // one-hop prefix: at most 64 chunk sums of 64 workgroups (only where it is used)
    CHECK(roll_shape(C, 1, 4096, false).nc == 64 && roll_shape(C, 1, 4097, false).nc == 65);
    CHECK(roll_limits(C, roll_shape(C, 1, 4096, false), 1, 16, kFits, 1) == RollLimit::kNone);
    CHECK(roll_limits(C, roll_shape(C, 1, 4097, false), 1, 16, kFits, 1) == RollLimit::kChunkSums);
    // the first limit missed is the one reported
    CHECK(roll_limits(C, roll_shape(C, 4095, 4097, false), 2, 0x80000000ull, 1, 1) == RollLimit::kActionSpan);
    CHECK(roll_limits(C, roll_shape(C, 4095, 4097, false), 1, 16, 1, 1) == RollLimit::kResidency);
    CHECK(roll_limits(C, roll_shape(C, 4095, 4097, false), 1, 16, kFits, 1) == RollLimit::kSteps);
    // the texts that callers and tests match
    CHECK(strstr(roll_limit_text(RollLimit::kActionSpan), "4 GiB"));
    CHECK(strstr(roll_limit_text(RollLimit::kResidency), "residency round"));
    CHECK(strstr(roll_limit_text(RollLimit::kSteps), "<= 4094"));
    CHECK(strstr(roll_limit_text(RollLimit::kWaveGroups), "8192 envs"));
    CHECK(strstr(roll_limit_text(RollLimit::kChunkSums), "4096 workgroups"));
}

static const char *const *g_env = nullptr;   // name, value, ..., nullptr
static char *fake_getenv(const char *name) {
    for (const char *const *e = g_env; e && *e; e += 2)
        if (!strcmp(e[0], name)) return const_cast<char *>(e[1]);
    return nullptr;
}
static Knobs knobs(const char *const *env) {
    g_env = env;
    return read_knobs(fake_getenv, 8);
}

static void knob_parsing() {
    const Knobs d = knobs(nullptr);
    CHECK(d.pace_on && d.pace_q == 0 && d.depth == 4 && d.place && !d.place_force && d.place_xcd &&
          d.eager_one_launch);
    CHECK(d.model[0] == 200 && d.model[1] == 20 && d.model[2] == 10 && d.model[3] == 3);
    { const char *e[] = {"GSM_ROLL_PACE", "off", nullptr}; const Knobs k = knobs(e); CHECK(!k.pace_on && k.pace_q == 0); }
    { const char *e[] = {"GSM_ROLL_PACE", "2", nullptr}; const Knobs k = knobs(e); CHECK(k.pace_on && k.pace_q == 2); }
    { const char *e[] = {"GSM_ROLL_PACE", "-3", nullptr}; const Knobs k = knobs(e); CHECK(k.pace_on && k.pace_q == 0); }
    { const char *e[] = {"GSM_ROLL_PACE", "offx", nullptr}; const Knobs k = knobs(e); CHECK(k.pace_on && k.pace_q == 0); }
    { const char *e[] = {"GSM_ROLL_DEPTH", "1", nullptr}; CHECK(knobs(e).depth == 2); }
    { const char *e[] = {"GSM_ROLL_DEPTH", "6", nullptr}; CHECK(knobs(e).depth == 6); }
    { const char *e[] = {"GSM_ROLL_DEPTH", "99", nullptr}; CHECK(knobs(e).depth == 8); }
    { const char *e[] = {"GSM_ROLL_DEPTH", "", nullptr}; CHECK(knobs(e).depth == 2); }
    { const char *e[] = {"GSM_ROLL_DEPTH", "99999999999999999999999", nullptr}; CHECK(knobs(e).depth == 8); }
    { const char *e[] = {"GSM_ROLL_PLACE", "0", nullptr}; const Knobs k = knobs(e); CHECK(!k.place && !k.place_force); }
    { const char *e[] = {"GSM_ROLL_PLACE", "2", nullptr}; const Knobs k = knobs(e); CHECK(k.place && k.place_force); }
    { const char *e[] = {"GSM_ROLL_PLACE", "1", nullptr}; const Knobs k = knobs(e); CHECK(k.place && !k.place_force); }
    { const char *e[] = {"GSM_PLACE_XCD", "0", nullptr}; CHECK(!knobs(e).place_xcd); }
    { const char *e[] = {"GSM_PLACE_XCD", "1", nullptr}; CHECK(knobs(e).place_xcd); }
    { const char *e[] = {"GSM_PLACE_MODEL", "63,27,55,18", nullptr}; const Knobs k = knobs(e);
      CHECK(k.model[0] == 63 && k.model[1] == 27 && k.model[2] == 55 && k.model[3] == 18); }
    { const char *e[] = {"GSM_PLACE_MODEL", " 7, -2,+5, 1x", nullptr}; const Knobs k = knobs(e);
      CHECK(k.model[0] == 7 && k.model[1] == -2 && k.model[2] == 5 && k.model[3] == 1); }
    { const char *e[] = {"GSM_PLACE_MODEL", "63,27,55", nullptr}; const Knobs k = knobs(e);
      CHECK(k.model[0] == 200 && k.model[3] == 3); }
    { const char *e[] = {"GSM_PLACE_MODEL", "63 ,27,55,18", nullptr}; CHECK(knobs(e).model[0] == 200); }
    { const char *e[] = {"GSM_EAGER_ONE_LAUNCH", "0", nullptr}; CHECK(!knobs(e).eager_one_launch); }
    { const char *e[] = {"GSM_EAGER_ONE_LAUNCH", "", nullptr}; CHECK(knobs(e).eager_one_launch); }
    { const char *e[] = {"GSM_EAGER_ONE_LAUNCH", "1", nullptr}; CHECK(knobs(e).eager_one_launch); }
    { const char *e[] = {"GSM_ROLL_PACE", "off", "GSM_ROLL_DEPTH", "3", "GSM_PLACE_XCD", "0", nullptr};
      const Knobs k = knobs(e); CHECK(!k.pace_on && k.depth == 3 && !k.place_xcd && k.place); }
}

int main() {
    // 24 agents x 8192 envs, two envs per wave (8 per workgroup), K = 100: nb = 1024, nc = 16:
    // 16 + (100*1024 + 2*100*16*8)*8 + 2*2048*16*4
    layout("24x8192 pair K=100", roll_shape(C, 100, 8192 / 8, false), 1286160);
    // the same batch as the eager step (4 per workgroup, K = 1): nb = 2048, nc = 32:
    // 16 + (2048 + 2*32*8)*8 + 64*16*4
    layout("24x8192 eager K=1", roll_shape(C, 1, 8192 / 4, false, true), 24592);
    // 3 x 4096 packed (16 per workgroup, per-wave): nb = 256, xW = 1024, xNG = 16: 16 + 100*(1024+16)*8
    layout("3x4096 packed K=100", roll_shape(C, 100, 4096 / 16, true), 832016);
    // 96 x 1024 tile (one env per workgroup), K = 20: 16 + (20*1024 + 2*20*16*8)*8 + 2*2048*16*4
    layout("96x1024 tile K=20", roll_shape(C, 20, 1024, false), 466960);
    // ragged, 32 agents x 1024 envs (4 per workgroup, per-wave) with its PlaceArea of
    // 2*8192 + 8 + 3*8*64 + 1024/2 = 18440 words: 16 + 100*(1024+16)*8 + 18440*8
    RollShape ragged = roll_shape(C, 100, 1024 / 4, true);
    ragged.place_words = 18440;
    layout("ragged 32x1024 K=100", ragged, 979536);
    // the longest launch on one workgroup: 16 + (4094 + 2*4094*1*8)*8 + 2*2048*16*4
    layout("K=4094 nb=1", roll_shape(C, 4094, 1, false), 818944);
    // one workgroup past the chunk sums (nc = 65, refused by roll_limits): 16 + (4097 + 2*65*8)*8 + 2*2048*16*4
    layout("K=1 nb=4097", roll_shape(C, 1, 4097, false), 303256);
    limits();
    knob_parsing();
    printf(failed ? "FAILED\n" : "OK\n");
    return failed;
}
"""


def test_roll_plan_layout_limits_knobs(tmp_path):
    src = tmp_path / "roll_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "roll_plan_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", str(CSRC), str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr


def test_roll_plan_header_is_plain_cxx():
    """Only <stddef.h> / <stdint.h>: no HIP, no libc calls, so the program above is the whole of it."""
    text = (CSRC / "gsm_roll_plan.h").read_text()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>"]
