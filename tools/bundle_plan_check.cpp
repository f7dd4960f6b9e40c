// bundle_plan_check.cpp -- stand-alone check of plan_bundle (libjitsi_amd/csrc/
// bundle_plan.h), the one rule that says which kernels a bundle runs, for a
// sanitizer build (no GPU, no Python, no HIP).  Two parts:
//   literal cases   the launch list of a bundle at each size and hook where the
//                   route changes, written out by hand as names (not computed
//                   by a second copy of the rule), with the path, small_ctr and
//                   gcm_route word; the sort fields by table size;
//   a sweep         every n in 1..300, each threshold +-1 and every power of two
//                   up to 2^18, every combination of the five key-set flags and
//                   of the nine debug flags, both ways, both abort settings:
//                   the invariants every plan keeps, and each step's stage.
//
//   make -C tools bundle_plan_check      (built with -fsanitize=address,undefined)
//   tools/bundle_plan_check
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../libjitsi_amd/csrc/bundle_plan.h"

using namespace srtp;

static int failures = 0;
static long cases = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

static const char *const kLaunchName[] = {"small", "parse", "sort_tile", "sort", "unprotect", "ctr_small", "skein",
                                          "gcm", "walk", "unprotect_fix", "ext", "protect", "ctr_wide", "mac_wide"};
static const char *const kGcmName[] = {"seal", "verify", "decipher", "open", "fix"};

static int steps_of(const BundlePlan &p) { return p.n_steps < kPlanMaxSteps ? p.n_steps : kPlanMaxSteps; }

static std::string render(const BundlePlan &p) {
    std::string s;
    for (int i = 0; i < steps_of(p); i++) {
        const PlanStep &st = p.steps[i];
        if (i) s += " ";
        if (st.launch > kLaunchMacWide) return s + "?";
        s += kLaunchName[st.launch];
        if (st.launch == kLaunchWalk) s += st.pass == kWalkFirst ? "0" : st.pass == kWalkSecond ? "1" : "?";
        if (st.launch == kLaunchGcm)
            s += std::string("(") + (st.pass <= kGcmFix ? kGcmName[st.pass] : "?") + (p.gcm_wave ? ",wave)" : ",lane)");
    }
    return s;
}

// Each step under the stage the engine times it: small by direction; parse,
// the sorts and the walks their own; around the walk VERIFY before it
// (unprotect only) and DECRYPT or PROTECT after it.
static void check_stages(const BundlePlan &p, bool reverse) {
    bool walked = false;
    for (int i = 0; i < steps_of(p); i++) {
        const PlanStep &st = p.steps[i];
        int want;
        switch (st.launch) {
        case kLaunchSmall: want = reverse ? kStageVerify : kStageProtect; break;
        case kLaunchParse: want = kStageParse; break;
        case kLaunchSortTile:
        case kLaunchSort: want = kStageSort; break;
        case kLaunchWalk: want = kStageWalk; walked = true; break;
        default: want = !walked ? kStageVerify : reverse ? kStageDecrypt : kStageProtect; CHECK(walked || reverse); break;
        }
        CHECK(st.stage == want);
    }
}

enum { DBG_STALL = 0x1, DBG_FORCE_WIDE = 0x2, DBG_NO_WIDE = 0x4, DBG_NO_SMALL = 0x8, DBG_NO_GCM_WAVE = 0x10,
       DBG_FORCE_GCM_WAVE = 0x20, DBG_FORCE_SMALL = 0x40, DBG_NO_GCM_SPEC = 0x80, DBG_FORCE_GCM_SPEC = 0x100 };

static EngineShape shape(bool gcm, bool skein, bool ext, bool all_wide, bool all_small, uint32_t dbg = 0,
                         int ctx_bits = 14) {
    EngineShape s;
    s.has_gcm = gcm; s.has_skein = skein; s.has_ext = ext;
    s.all_wide = all_wide; s.all_small = all_small;
    s.ctx_bits = ctx_bits;
    s.dbg = dbg;
    s.sort_tile = 2048u;
    return s;
}
// key sets all AES-CM + HMAC-SHA1 / only AES-GCM ones / GCM, Skein and ext ones
static EngineShape plain(uint32_t dbg = 0) { return shape(false, false, false, true, true, dbg); }
static EngineShape gcm(uint32_t dbg = 0) { return shape(true, false, false, false, true, dbg); }
static EngineShape mixed(uint32_t dbg = 0) { return shape(true, true, true, false, false, dbg); }

static void lit(int line, const EngineShape &e, uint32_t n, bool reverse, bool abort, int path, int small_ctr,
                const char *launches, int gcm_route = -1) {
    cases++;
    const BundlePlan p = plan_bundle(e, n, reverse, abort);
    const std::string got = render(p);
    const bool ok = p.path == path && p.small_ctr == small_ctr && got == launches && p.n_steps <= kPlanMaxSteps &&
                    (gcm_route < 0 || p.gcm_route == gcm_route) && bundle_path(e, n) == path;
    if (!ok) {
        if (failures < 20)
            printf("FAIL line %d: n %u reverse %d: path %d small_ctr %d gcm_route %d [%s], expected path %d small_ctr %d "
                   "gcm_route %d [%s]\n", line, n, (int)reverse, p.path, p.small_ctr, p.gcm_route, got.c_str(), path,
                   small_ctr, gcm_route, launches);
        failures++;
    }
    check_stages(p, reverse);
}
#define LIT(...) lit(__LINE__, __VA_ARGS__)

static void literal_cases() {
    const bool P = false, U = true; // protect, unprotect
    for (uint32_t n : {1u, 255u})
        for (bool r : {P, U}) LIT(plain(), n, r, false, kPathSmall, 2, "small");
    LIT(plain(), 256, P, false, kPathFused, 1, "parse sort_tile walk0 walk1 ctr_small protect");
    LIT(plain(), 256, U, false, kPathFused, 1, "parse sort_tile unprotect ctr_small walk0 walk1 unprotect_fix");
    LIT(plain(DBG_NO_SMALL), 100, P, false, kPathFused, 1, "parse sort_tile walk0 ctr_small protect");
    LIT(plain(DBG_NO_SMALL), 100, P, true, kPathFused, 1, "parse sort_tile walk0 walk1 ctr_small protect");
    LIT(plain(DBG_STALL), 100, P, false, kPathFused, 1, "parse sort_tile walk0 walk1 ctr_small protect");
    LIT(plain(DBG_FORCE_WIDE), 100, P, false, kPathSplit, 2, "parse sort_tile walk0 ctr_wide mac_wide");
    LIT(plain(), 2047, P, false, kPathFused, 1, "parse sort_tile walk0 walk1 ctr_small protect");
    LIT(plain(), 2048, P, false, kPathSplit, 2, "parse sort_tile walk0 walk1 ctr_wide mac_wide");
    LIT(plain(), 2048, U, false, kPathSplit, 2, "parse sort_tile mac_wide walk0 walk1 ctr_wide");
    for (uint32_t n : {2049u, 65536u}) {
        LIT(plain(), n, P, false, kPathSplit, 2, "parse sort walk0 walk1 ctr_wide mac_wide");
        LIT(plain(), n, U, false, kPathSplit, 2, "parse sort mac_wide walk0 walk1 ctr_wide");
    }
    LIT(plain(DBG_NO_WIDE), 4096, P, false, kPathFused, 1, "parse sort walk0 walk1 ctr_small protect");
    LIT(plain(), 65537, P, false, kPathFused, 0, "parse sort walk0 walk1 protect");
    LIT(plain(), 65537, U, false, kPathFused, 0, "parse sort unprotect walk0 walk1 unprotect_fix");

    for (bool r : {P, U}) LIT(gcm(), 8, r, false, kPathSmall, 2, "small");
    for (bool r : {P, U}) LIT(gcm(DBG_FORCE_SMALL), 255, r, false, kPathSmall, 2, "small");
    for (bool r : {P, U}) LIT(gcm(DBG_FORCE_GCM_SPEC), 3, r, false, kPathSmall, 2, "small");
    LIT(gcm(), 9, P, false, kPathFused, 1, "parse sort_tile walk0 ctr_small protect gcm(seal,wave)", 0);
    LIT(gcm(), 9, U, false, kPathFused, 1,
        "parse sort_tile unprotect ctr_small gcm(verify,wave) walk0 unprotect_fix gcm(decipher,wave)", 0);
    LIT(gcm(), 4095, U, false, kPathFused, 1,
        "parse sort unprotect ctr_small gcm(verify,wave) walk0 walk1 unprotect_fix gcm(decipher,wave)", 0);
    for (uint32_t n : {4096u, 8192u})
        LIT(gcm(), n, U, false, kPathFused, 1,
            "parse sort unprotect ctr_small gcm(open,wave) walk0 walk1 unprotect_fix gcm(fix,wave)", kGcmRouteSpec);
    for (uint32_t d : {(uint32_t)DBG_NO_GCM_SPEC, (uint32_t)(DBG_NO_GCM_SPEC | DBG_FORCE_GCM_SPEC)})
        LIT(gcm(d), 4096, U, false, kPathFused, 1,
            "parse sort unprotect ctr_small gcm(verify,wave) walk0 walk1 unprotect_fix gcm(decipher,wave)", 0);
    LIT(gcm(), 8193, U, false, kPathFused, 0,
        "parse sort unprotect gcm(verify,lane) walk0 walk1 unprotect_fix gcm(decipher,lane)", 0);
    for (uint32_t d : {(uint32_t)DBG_NO_GCM_WAVE, (uint32_t)(DBG_NO_GCM_WAVE | DBG_FORCE_GCM_WAVE)}) {
        LIT(gcm(d), 8, U, false, kPathFused, 1,
            "parse sort_tile unprotect ctr_small gcm(verify,lane) walk0 unprotect_fix gcm(decipher,lane)", kGcmRouteLane);
        LIT(gcm(d | DBG_FORCE_GCM_SPEC), 8, U, false, kPathFused, 1,
            "parse sort_tile unprotect ctr_small gcm(open,lane) walk0 unprotect_fix gcm(fix,lane)",
            kGcmRouteLane | kGcmRouteSpec);
    }
    LIT(mixed(), 100, U, false, kPathFused, 1,
        "parse sort_tile unprotect ctr_small skein gcm(verify,wave) walk0 unprotect_fix ext gcm(decipher,wave)");
    LIT(mixed(), 100, P, false, kPathFused, 1, "parse sort_tile walk0 ctr_small protect ext skein gcm(seal,wave)");

    // the sort, by the context table's size
    struct { int ctx_bits, kind, key_bits, passes, bits, hi_bits; } const sorts[] = {
        {7, kSort8Bit, 8, 1, 8, 0},    {15, kSort8Bit, 16, 2, 8, 0}, {16, kSortHybrid, 17, 2, 8, 9},
        {18, kSortHybrid, 19, 2, 8, 11}, {19, kSortWide, 20, 2, 10, 0}, {21, kSortWide, 22, 2, 11, 0},
        {22, kSort8Bit, 23, 3, 8, 0},
    };
    for (const auto &s : sorts)
        for (uint32_t n : {1u, 300u, 4096u}) {
            cases++;
            const BundlePlan p = plan_bundle(shape(false, false, false, true, true, 0, s.ctx_bits), n, false, false);
            CHECK(p.sort_kind == s.kind && p.sort_key_bits == s.key_bits && p.sort_passes == s.passes &&
                  p.sort_bits == s.bits && p.sort_hi_bits == s.hi_bits);
        }
}

static void invariants(const EngineShape &e, uint32_t n, bool reverse, bool abort) {
    cases++;
    const BundlePlan p = plan_bundle(e, n, reverse, abort);
    CHECK(p.n_steps >= 1 && p.n_steps <= kPlanMaxSteps);
    int count[kLaunchMacWide + 1] = {0}, walk[2] = {0, 0}, pass[kGcmFix + 1] = {0};
    for (int i = 0; i < steps_of(p); i++) {
        const PlanStep &st = p.steps[i];
        if (st.launch > kLaunchMacWide) { CHECK(st.launch <= kLaunchMacWide); return; }
        count[st.launch]++;
        if (st.launch == kLaunchWalk) { CHECK(st.pass <= kWalkSecond); walk[st.pass & 1]++; }
        if (st.launch == kLaunchGcm) { CHECK(st.pass <= kGcmFix); pass[st.pass <= kGcmFix ? st.pass : 0]++; }
    }
    const bool small = p.path == kPathSmall, split = p.path == kPathSplit, fused = p.path == kPathFused;
    CHECK(small || split || fused);
    CHECK(bundle_path(e, n) == p.path);
    // exactly one of small or parse, and small stands alone
    CHECK(count[kLaunchSmall] + count[kLaunchParse] == 1);
    CHECK(small == (count[kLaunchSmall] == 1));
    CHECK(!small || p.n_steps == 1);
    if (!small) {
        CHECK(p.steps[0].launch == kLaunchParse);
        CHECK(count[kLaunchSortTile] + count[kLaunchSort] == 1 && p.steps[1].stage == kStageSort);
        CHECK((count[kLaunchSortTile] == 1) == (n <= e.sort_tile));
        CHECK(walk[0] == 1);
        CHECK(walk[1] == (abort || n >= kLongMin || (e.dbg & DBG_STALL) ? 1 : 0));
    }
    // split kernels and fused crypto kernels are never in one plan
    const int n_split = count[kLaunchCtrWide] + count[kLaunchMacWide];
    const int n_fused = count[kLaunchUnprotect] + count[kLaunchUnprotectFix] + count[kLaunchProtect] +
                        count[kLaunchCtrSmall] + count[kLaunchSkein] + count[kLaunchExt] + count[kLaunchGcm];
    CHECK(!(n_split && n_fused));
    CHECK(split == (n_split == 2) && (split || n_split == 0));
    CHECK(fused == (n_fused > 0));
    CHECK(!split || e.all_wide);
    CHECK(!small || (e.all_small && n <= 255u));
    // A GCM step iff the engine has GCM key sets and the path is not small.  The
    // sweep also holds flag sets no engine can have (a GCM, Skein or ext key set
    // is not the split path's, and the split path's key sets are k_small's);
    // there a split bundle has no GCM step either.
    const bool possible = !(e.all_wide && (e.has_gcm || e.has_skein || e.has_ext || !e.all_small)) &&
                          !(e.all_small && (e.has_skein || e.has_ext));
    CHECK((count[kLaunchGcm] > 0) == (e.has_gcm && fused));
    if (possible) CHECK((count[kLaunchGcm] > 0) == (e.has_gcm && !small));
    CHECK(count[kLaunchGcm] == (e.has_gcm && fused ? (reverse ? 2 : 1) : 0));
    // open and fix together and only with the Spec bit; verify and decipher together
    CHECK(pass[kGcmOpen] == pass[kGcmFix] && pass[kGcmVerify] == pass[kGcmDecipher]);
    CHECK(!pass[kGcmOpen] || (p.gcm_route & kGcmRouteSpec));
    CHECK(!pass[kGcmOpen] || !pass[kGcmVerify]);
    CHECK(!(p.gcm_route & kGcmRouteSpec) == !p.gcm_one_pass);
    CHECK(!p.gcm_one_pass || !pass[kGcmVerify]);
    CHECK(!p.gcm_one_pass || e.has_gcm);
    // the hooks' precedences
    if (e.dbg & DBG_NO_GCM_SPEC) CHECK(!p.gcm_one_pass);
    else if (e.has_gcm && (e.dbg & DBG_FORCE_GCM_SPEC)) CHECK(p.gcm_one_pass);
    if (e.dbg & DBG_NO_GCM_WAVE) CHECK(!p.gcm_wave && (p.gcm_route & kGcmRouteMask) == kGcmRouteLane);
    else if (e.dbg & DBG_FORCE_GCM_WAVE) CHECK(p.gcm_wave && (p.gcm_route & kGcmRouteMask) == kGcmRouteWave);
    else CHECK((p.gcm_route & kGcmRouteMask) == 0);
    if (e.dbg & (DBG_NO_SMALL | DBG_NO_WIDE | DBG_FORCE_WIDE | DBG_STALL | DBG_NO_GCM_WAVE | DBG_FORCE_GCM_WAVE)) CHECK(!small);
    if (e.dbg & DBG_NO_WIDE) CHECK(!split);
    // unprotect-only and protect-only launchers
    const int n_rev = count[kLaunchUnprotect] + count[kLaunchUnprotectFix] + pass[kGcmVerify] + pass[kGcmDecipher] +
                      pass[kGcmOpen] + pass[kGcmFix];
    const int n_fwd = count[kLaunchProtect] + pass[kGcmSeal];
    CHECK(reverse ? n_fwd == 0 : n_rev == 0);
    if (fused) CHECK(reverse ? count[kLaunchUnprotect] == 1 && count[kLaunchUnprotectFix] == 1 : count[kLaunchProtect] == 1);
    CHECK((p.small_ctr == 2) == (small || split));
    CHECK(p.small_ctr == 2 || p.small_ctr == (n <= 8192u ? 1 : 0));
    CHECK(fused ? (count[kLaunchCtrSmall] == (p.small_ctr ? 1 : 0)) : count[kLaunchCtrSmall] == 0);
    check_stages(p, reverse);
}

int main() {
    literal_cases();
    const long literal = cases;
    std::vector<uint32_t> ns;
    for (uint32_t n = 1; n <= 300; n++) ns.push_back(n);
    for (uint32_t t : {kSmallGcmMax, kSmallMaxN, kLongMin, 2048u, kWideMin, kGcmOpenWaveMin, kSmallCtrMax, kGcmWaveMax,
                       kGcmOpenWaveMax, kWideMax, kGcmOpenLaneMin})
        for (uint32_t n : {t - 1u, t, t + 1u}) ns.push_back(n);
    for (int lg = 0; lg <= 18; lg++) ns.push_back(1u << lg);
    for (uint32_t flags = 0; flags < 32; flags++)
        for (uint32_t dbg = 0; dbg <= kPlanDbgAll; dbg++) {
            const EngineShape e = shape(flags & 1, flags & 2, flags & 4, flags & 8, flags & 16, dbg);
            for (uint32_t n : ns)
                for (int ra = 0; ra < 4; ra++) invariants(e, n, ra & 1, ra & 2);
        }
    printf("bundle_plan_check: %ld literal cases, %ld swept\n", literal, cases - literal);
    printf("bundle_plan_check: %ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
