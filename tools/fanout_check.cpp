// fanout_check.cpp -- stand-alone check of fanout_job (libjitsi_amd/csrc/
// fanout_job.h), the one function k_fanout takes every byte count from, for a
// sanitizer build (no GPU, no Python): sweeps it over every source length
// 0..80 and the lengths around 1024, 2048, 4096 and 65535, source and
// destination capacities around each of those, indices inside and outside
// [0, m), the status values and the SKIP flag (and lengths and capacities
// that are negative as ints or past 65535); asserts the rules the header
// states; then replays each copy, 16 bytes at a time as the kernel moves them,
// between heap buffers of exactly src_cap and dst_cap rounded up to 16 bytes,
// so that AddressSanitizer sees any byte outside either region.
//
//   make -C tools fanout_check      (built with -fsanitize=address,undefined)
//   tools/fanout_check
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../libjitsi_amd/csrc/fanout_job.h"

using srtp::FanoutJob;

static int failures = 0;
static long cases = 0, replayed = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            if (failures < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                              \
        }                                                            \
    } while (0)

static uint8_t pattern[65536];
static int up16(int v) { return (v + 15) & ~15; }
static int imin(int a, int b) { return a < b ? a : b; }

static void one(int idx, int m, int L, int sc, int st, int dc, uint32_t fl) {
    cases++;
    const FanoutJob j = srtp::fanout_job(idx, m, L, sc, st, dc, fl);
    const bool by_source = idx < 0 || idx >= m || st != 0;
    const bool skip = by_source || (fl & srtp::kFanFlagSkip);
    CHECK(j.by_source == (by_source ? 1 : 0));
    if (skip) {
        CHECK(j.copy_bytes == 0 && j.len_out == 0 && j.flags_out == (fl | srtp::kFanFlagSkip));
        return;
    }
    CHECK(j.flags_out == fl && j.len_out == L);
    CHECK(j.copy_bytes >= 0 && j.copy_bytes % 16 == 0);
    if (L < 0 || sc < 0 || dc < 0) {
        CHECK(j.copy_bytes == 0);
        return;
    }
    if (L <= 65535 && sc <= 65535 && dc <= 65535) CHECK(j.copy_bytes == up16(imin(L, imin(sc, dc))));
    CHECK(j.copy_bytes <= 65536);
    if (sc > 65535 || dc > 65535) return; // no such region exists: nothing to replay
    CHECK(j.copy_bytes <= up16(sc) && j.copy_bytes <= up16(dc));
    // the copy, as k_fanout makes it, between regions of exactly the size they own
    std::vector<uint8_t> src((size_t)up16(sc)), dst((size_t)up16(dc));
    uint8_t *sp = src.data(), *dp = dst.data(); // null for an empty region: never touched then
    if (!src.empty()) memcpy(sp, pattern, src.size());
    if (!dst.empty()) memset(dp, 0xEE, dst.size());
    for (int o = 0; o < j.copy_bytes; o += 16) memcpy(dp + o, sp + o, 16);
    const int got = imin(L, imin(sc, dc));
    CHECK(got == 0 || memcmp(dp, pattern, (size_t)got) == 0);
    for (int i = j.copy_bytes; i < (int)dst.size(); i++) // nothing behind the copy
        if (dp[i] != 0xEE) {
            CHECK(dp[i] == 0xEE);
            break;
        }
    replayed++;
}

int main() {
    for (size_t i = 0; i < sizeof pattern; i++) pattern[i] = (uint8_t)(i * 7 + 3);
    std::vector<int> lens, caps;
    for (int L = 0; L <= 80; L++) lens.push_back(L);
    for (int c : {1024, 2048, 4096, 65535})
        for (int d = -17; d <= 17; d++)
            if (c + d <= 65535 + 2) lens.push_back(c + d);
    for (int c : {0, 16, 64, 1024, 2048, 4096, 65535})
        for (int d : {-17, -16, -1, 0, 1, 16})
            if (c + d >= 0 && c + d <= 65535) caps.push_back(c + d);
    const int statuses[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, -1};
    const uint32_t flagv[] = {0u, 0x2u, 0x6u, srtp::kFanFlagSkip, srtp::kFanFlagSkip | 0x4u};
    for (int L : lens)
        for (int sc : caps)
            for (int dc : caps)
                for (uint32_t fl : {0u, srtp::kFanFlagSkip}) one(1, 3, L, sc, 0, dc, fl);
    // indices and statuses, over a smaller set of shapes
    const int idxs[] = {-2147483647 - 1, -1, 0, 1, 2, 3, 4, 2147483647};
    for (int idx : idxs)
        for (int m : {0, 1, 3, 2147483647})
            for (int st : statuses)
                for (uint32_t fl : flagv)
                    for (int L : {0, 8, 12, 17, 1200, 65535})
                        for (int c : {0, 16, 1216, 65535}) one(idx, m, L, c, st, c, fl);
    // values no caller may pass, which a device array can still hold
    for (int L : {-2147483647 - 1, -1, 65536, 70000, 2147483647})
        for (int sc : {-2147483647 - 1, -1, 0, 100, 65535, 65536, 2147483647})
            for (int dc : {-2147483647 - 1, -1, 0, 100, 65535, 65536, 2147483647}) {
                one(0, 1, L, sc, 0, dc, 0u);
                one(0, 1, 100, sc, 0, dc, 0u);
            }
    printf("fanout_check: %ld cases, %ld copies replayed, %d failures\n", cases, replayed, failures);
    return failures ? 1 : 0;
}
