// bundle_plan.h -- which kernels one bundle runs, in which order and under
// which stage's timer: the one place where a bundle's route is decided.  The
// engine fills BundleArgs, asks plan_bundle() once and launches the steps it
// gets (engine.cpp transform_locked); the launchers (srtp_kernels.hip) take
// what the plan decided.  The size thresholds of every route live here with
// the measurements they came from.  Plain C++17 that a host compiler takes as
// it stands (no HIP include, no engine type, no heap), so the rule is checked
// without a GPU: tools/bundle_plan_check.cpp under AddressSanitizer + UBSan.
//
// The routes:
//   small   every phase in one launch (k_small): up to kSmallMaxN packets of an
//           engine whose key sets are all k_small's (AES-CM / NULL cipher +
//           HMAC-SHA1, or AES-GCM); once the engine holds a GCM key set, up to
//           kSmallGcmMax.  Every hook that asks for a kernel of the chain keeps
//           a bundle off it; SRTP_DEBUG_FORCE_SMALL only lifts the GCM engines'
//           limit, and the GCM one-pass hooks do not touch it.
//   split   k_ctr_wide + k_mac_wide around the walk: kWideMin..kWideMax packets
//           of an engine whose key sets are all AES-CM / NULL cipher +
//           HMAC-SHA1 (SRTP_DEBUG_FORCE_WIDE: every size; _NO_WIDE: never).
//   fused   k_protect / k_unprotect + k_unprotect_fix, with k_ctr_small for the
//           AES-CM keystream up to kSmallCtrMax packets, then k_ext, k_skein and
//           the k_gcm passes where the engine has such key sets.
#pragma once
#include <stdint.h>

namespace srtp {

// ---- thresholds
// Context chains of at least this many records in a bundle are walked by the
// wave-parallel (speculative) walk, shorter ones lane-serially.
#ifndef SRTP_LONG_MIN
#define SRTP_LONG_MIN 256
#endif
constexpr uint32_t kLongMin = SRTP_LONG_MIN;
// a small bundle's AES-CM keystream by k_ctr_small (a lane per counter-block
// pair; the fused kernels only MAC): up to 8192 packets (128 waves: under
// one wave per SIMD; profiles/r04/kernel_experiments.md 9)
constexpr uint32_t kSmallCtrMax = 8192u; // k_ctr_small takes bundles up to this size
// The split path (k_ctr_wide + k_mac_wide) for bundles of kWideMin..kWideMax
// packets: there the fused kernels' lane per packet leaves most CUs idle or
// latency-bound; from 2^17 packets on the fused kernels are faster
// (profiles/r06/kernel_experiments.md, bundle-size sweep)
#ifndef SRTP_WIDE_MIN
#define SRTP_WIDE_MIN 2048u
#endif
constexpr uint32_t kWideMin = SRTP_WIDE_MIN, kWideMax = 65536u;
// The sort's keys (slot or table size = not walked) have ctx_bits + 1 bits:
// 8-bit digits up to 16 bits, two 9-11-bit digits up to 22 (the wide sort),
// else 8-bit again.  17-19 bits: an 8-bit pass and one wide pass (hybrid);
// 20-22: two wide passes (profiles/r04/kernel_experiments.md 8)
constexpr int kSortWideMaxBits = 11;
// Engines with AES-GCM key sets (k_gcm).  A bundle of up to kGcmWaveMax packets
// takes k_gcm_wave, a wave per packet (the per-packet paths' bundles), a larger
// one k_gcm, a lane per packet; SRTP_DEBUG_NO_GCM_WAVE / _FORCE_GCM_WAVE
// override the size rule (NO wins).  8192: the largest size of the measured
// sweep (1 .. 8192 1200-byte packets, profiles/gcm_wave/sweep.json) at which the
// wave route's median lies below the lane route's by more than the lane route's
// spread, protect and unprotect; it did at every size of the sweep, by 3.7-4.3x
// up to 64 packets and by 6-18 % at 8192.
constexpr uint32_t kGcmWaveMax = 8192u;
// BundleArgs::gcm_route: bits 0-1 the hook's route (0: by bundle size), and
// kGcmRouteSpec: unprotect in one pass
constexpr int32_t kGcmRouteLane = 1, kGcmRouteWave = 2, kGcmRouteMask = 3, kGcmRouteSpec = 4;
// Unprotect in one pass over the packet bytes (kGcmRouteSpec): kGcmOpen in
// kGcmVerify's place checks the tag under the ROC guess and deciphers in the
// same trip where gcm_spec_ok (gcm_job.h) allows; kGcmFix in kGcmDecipher's
// place repairs the packets whose verdict the walk overturned (gcm_fix_action)
// and is otherwise a launch whose workgroups leave at once.  Results are those
// of the two passes to the bit.  It is the default at the sizes of the measured
// sweep (profiles/gcm_open/sweep.json) at which its median lies below the
// two-pass route's by more than that route's own p90 - p10, for GCM-128 and
// GCM-256, on a clean bundle and on one with 2.5 % replays and forgeries:
//   wave route  4096 and 8192 packets, by 9-11 % clean and 2-5 % with the mix.
//               Below that a bundle is bound by its launches' latency, and one
//               packet to repair costs the fix pass what the whole decipher
//               pass costs: 5-8 % slower at 256 and 1024 with the mix (5-7 %
//               faster clean there and at 1, 16 and 64).
//   lane route  nowhere: 2-7 % faster on a clean bundle of 2^18, but 20-36 %
//               slower with the mix (a wave's 64 lanes wait for the one that
//               repairs), and 5-73 % slower at 2^14 and 2^16 (one lane's serial
//               AES + GHASH chain, where two shorter passes overlap better).
//               Its code is reached by SRTP_DEBUG_FORCE_GCM_SPEC alone.
// SRTP_DEBUG_NO_GCM_SPEC keeps every bundle on the two passes, _FORCE_GCM_SPEC
// puts every bundle of the multi-kernel path on the one-pass route (NO wins).
constexpr uint32_t kGcmOpenLaneMin = 0x7FFFFFFFu; // no bundle is that large (kRecIdxMask): never
constexpr uint32_t kGcmOpenWaveMin = 4096u;
constexpr uint32_t kGcmOpenWaveMax = kGcmWaveMax;
// A bundle of up to kSmallMaxN packets (engines whose key sets are all AES-CM
// or NULL cipher with HMAC-SHA1): parse, sort, (tag check,)
// walk, keystream and (MAC, trailer) in one workgroup and one launch (k_small).
constexpr uint32_t kSmallMaxN = 255u;
// An engine that holds AES-GCM key sets launches k_small's GCM instance, for
// bundles of up to kSmallGcmMax packets: workgroup 0's eight waves verify the
// bundle's GCM tags before the walk, a wave per packet, and from two packets
// per wave on the chain's k_gcm_wave (every packet's wave at once) is faster.
// The largest size of profiles/gcm_small/sweep.json at which the one-launch
// route's median lies below the chain's by more than the chain's spread, both
// ways, for GCM and for AES-CM + HMAC bundles.  SRTP_DEBUG_FORCE_SMALL: up to
// kSmallMaxN.
constexpr uint32_t kSmallGcmMax = 8u;

// ---- what this header restates of include/srtp_mi355x.h (it stands alone;
// engine.cpp pins each against the public header)
constexpr uint32_t kPlanDbgForceChainStall = 0x1u, kPlanDbgForceWide = 0x2u, kPlanDbgNoWide = 0x4u,
                   kPlanDbgNoSmall = 0x8u, kPlanDbgNoGcmWave = 0x10u, kPlanDbgForceGcmWave = 0x20u,
                   kPlanDbgForceSmall = 0x40u, kPlanDbgNoGcmSpec = 0x80u, kPlanDbgForceGcmSpec = 0x100u;
constexpr uint32_t kPlanDbgAll = 0x1FFu;
enum PlanStage : uint8_t { // SRTP_STAGE_*
    kStageParse = 0, kStageSort = 1, kStageVerify = 2, kStageWalk = 3, kStageProtect = 4, kStageDecrypt = 5
};

// ---- the plan
// The passes of launch_gcm.  Seal (protect, after k_protect): tag and SRTCP's
// E|index word written.  Verify (unprotect, beside k_skein): the tag check under
// k_unprotect's ROC guess.  Decipher (unprotect, after k_unprotect_fix): the
// accepted packets deciphered.  Open / Fix: the one-pass route's pair (above).
enum GcmPass : int { kGcmSeal = 0, kGcmVerify = 1, kGcmDecipher = 2, kGcmOpen = 3, kGcmFix = 4 };
// The passes of launch_walk.  Second: abort-on-throw's limit pass when a packet
// may throw, else the wave-parallel walk of context chains longer than the
// first pass's window (returns at once when there are none).
enum WalkPass : int { kWalkFirst = 0, kWalkSecond = 1 };
enum PlanPath : uint8_t { kPathSmall, kPathSplit, kPathFused };
enum PlanSort : uint8_t { kSort8Bit, kSortHybrid, kSortWide };
enum PlanLaunch : uint8_t { // launch_* of srtp_kernels.h
    kLaunchSmall, kLaunchParse, kLaunchSortTile, kLaunchSort, kLaunchUnprotect, kLaunchCtrSmall, kLaunchSkein,
    kLaunchGcm, kLaunchWalk, kLaunchUnprotectFix, kLaunchExt, kLaunchProtect, kLaunchCtrWide, kLaunchMacWide
};

struct PlanStep {
    uint8_t launch; // PlanLaunch
    uint8_t pass;   // kLaunchGcm: its GcmPass; kLaunchWalk: its WalkPass; else 0
    uint8_t stage;  // PlanStage: the timer the launch runs under
};
// the longest list: an unprotect bundle of 256 packets or more of an engine with
// GCM, Skein and ext key sets has 11 steps
constexpr int kPlanMaxSteps = 12;

// What a route depends on, and nothing else.
struct EngineShape {
    bool has_gcm, has_skein, has_ext; // the engine holds AES-GCM / Skein-MAC / k_ext key sets
    bool all_wide;                    // every key set is the split path's (AES-CM / NULL cipher + HMAC-SHA1)
    bool all_small;                   // every key set is k_small's (the split path's, or AES-GCM)
    int32_t ctx_bits;                 // log2 of the context table's slots
    uint32_t dbg;                     // srtp_engine_set_debug
    uint32_t sort_tile;               // sort_tile_records()
};

struct BundlePlan {
    uint8_t path;        // PlanPath
    uint8_t sort_kind;   // PlanSort
    bool gcm_wave;       // the k_gcm passes a wave per packet (k_gcm_wave), else a lane per packet
    bool gcm_one_pass;   // unprotect's k_gcm passes are Open and Fix
    int32_t small_ctr;   // BundleArgs::small_ctr
    int32_t gcm_route;   // BundleArgs::gcm_route
    int32_t sort_key_bits, sort_hi_bits, sort_passes, sort_bits; // BundleArgs::sort_*
    int32_t n_steps;
    PlanStep steps[kPlanMaxSteps];
};

// The path of a bundle of n packets (no other input decides it).
inline PlanPath bundle_path(const EngineShape &e, uint32_t n) {
    const uint32_t small_max = e.has_gcm && !(e.dbg & kPlanDbgForceSmall) ? kSmallGcmMax : kSmallMaxN;
    // a hook that needs the multi-kernel chain (the split path's, the walk's, the GCM route's) keeps it
    const uint32_t chain_hooks = kPlanDbgForceChainStall | kPlanDbgNoWide | kPlanDbgForceWide | kPlanDbgNoSmall |
                                 kPlanDbgNoGcmWave | kPlanDbgForceGcmWave;
    if (e.all_small && n <= small_max && !(e.dbg & chain_hooks)) return kPathSmall;
    const bool wide_ok = e.all_wide && !(e.dbg & kPlanDbgNoWide);
    if (wide_ok && ((n >= kWideMin && n <= kWideMax) || (e.dbg & kPlanDbgForceWide))) return kPathSplit;
    return kPathFused;
}

inline BundlePlan plan_bundle(const EngineShape &e, uint32_t n, bool reverse, bool abort_on_error) {
    BundlePlan p{};
    p.path = bundle_path(e, n);
    p.small_ctr = p.path != kPathFused ? 2 : n <= kSmallCtrMax ? 1 : 0;

    const int32_t hook = (e.dbg & kPlanDbgNoGcmWave) ? kGcmRouteLane : (e.dbg & kPlanDbgForceGcmWave) ? kGcmRouteWave : 0;
    p.gcm_wave = hook ? hook == kGcmRouteWave : n <= kGcmWaveMax;
    // the one-pass open: where the sweep made it the default on the route this
    // bundle takes, or as the hooks say
    p.gcm_one_pass = !e.has_gcm || (e.dbg & kPlanDbgNoGcmSpec) ? false
                     : (e.dbg & kPlanDbgForceGcmSpec)          ? true
                     : p.gcm_wave ? n >= kGcmOpenWaveMin && n <= kGcmOpenWaveMax
                                  : n >= kGcmOpenLaneMin;
    p.gcm_route = hook | (p.gcm_one_pass ? kGcmRouteSpec : 0);

    const int key_bits = e.ctx_bits + 1;
    const bool big = key_bits > 16 && key_bits <= 2 * kSortWideMaxBits;
    p.sort_kind = !big ? kSort8Bit : key_bits <= 8 + kSortWideMaxBits ? kSortHybrid : kSortWide;
    p.sort_key_bits = key_bits;
    p.sort_hi_bits = p.sort_kind == kSortHybrid ? key_bits - 8 : 0;
    p.sort_passes = big ? 2 : (key_bits + 7) / 8;
    p.sort_bits = p.sort_kind == kSortWide ? (key_bits + 1) / 2 : 8;

    auto add = [&p](PlanLaunch l, PlanStage st, int pass = 0) {
        if (p.n_steps < kPlanMaxSteps) p.steps[p.n_steps] = PlanStep{(uint8_t)l, (uint8_t)pass, (uint8_t)st};
        p.n_steps++; // past kPlanMaxSteps: not stored, and the count says so
    };
    if (p.path == kPathSmall) {
        add(kLaunchSmall, reverse ? kStageVerify : kStageProtect);
        return p;
    }
    const bool split = p.path == kPathSplit;
    add(kLaunchParse, kStageParse);
    // a one-tile bundle is sorted by one workgroup in one launch
    add(n <= e.sort_tile ? kLaunchSortTile : kLaunchSort, kStageSort);
    if (reverse && split) {
        add(kLaunchMacWide, kStageVerify); // tag check under the ROC guess, no decryption yet
    } else if (reverse) {
        add(kLaunchUnprotect, kStageVerify);
        if (p.small_ctr) add(kLaunchCtrSmall, kStageVerify); // the speculative decryption
        if (e.has_skein) add(kLaunchSkein, kStageVerify);
        // tag check under the ROC guess (Open: and the decipher, in the same trip)
        if (e.has_gcm) add(kLaunchGcm, kStageVerify, p.gcm_one_pass ? kGcmOpen : kGcmVerify);
    }
    add(kLaunchWalk, kStageWalk, kWalkFirst);
    // The second pass's long chains a bundle of fewer than kLongMin packets
    // cannot hold: a small bundle without abort-on-throw saves the launch.
    if (abort_on_error || n >= kLongMin || (e.dbg & kPlanDbgForceChainStall)) add(kLaunchWalk, kStageWalk, kWalkSecond);
    if (reverse && split) {
        add(kLaunchCtrWide, kStageDecrypt); // final statuses, decryption under the walk's ROC
    } else if (split) {
        add(kLaunchCtrWide, kStageProtect); // the keystream, then the MAC and trailer
        add(kLaunchMacWide, kStageProtect);
    } else if (reverse) {
        add(kLaunchUnprotectFix, kStageDecrypt);
        if (e.has_ext) add(kLaunchExt, kStageDecrypt);
        // the accepted packets deciphered (Fix: only the verdicts the walk overturned repaired)
        if (e.has_gcm) add(kLaunchGcm, kStageDecrypt, p.gcm_one_pass ? kGcmFix : kGcmDecipher);
    } else {
        if (p.small_ctr) add(kLaunchCtrSmall, kStageProtect); // the keystream, then k_protect MACs
        add(kLaunchProtect, kStageProtect);
        if (e.has_ext) add(kLaunchExt, kStageProtect);
        if (e.has_skein) add(kLaunchSkein, kStageProtect);
        if (e.has_gcm) add(kLaunchGcm, kStageProtect, kGcmSeal); // sealed: tag, SRTCP's E|index word
    }
    return p;
}

} // namespace srtp
