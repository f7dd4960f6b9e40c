#!/usr/bin/env python3
"""GCM unprotect through the engine in one pass over the packet bytes (k_gcm<open>
/ <fix>) against the two-pass route (tag check, walk, decipher), on one MI355X.

GCM-128 and GCM-256 unprotect of 1200-byte SRTP packets over 10k streams, on
the lane route (SRTP_DEBUG_NO_GCM_WAVE) and the wave route (_FORCE_GCM_WAVE),
each bundle clean and with a 2.5 % fault mix (every 40th packet in turn a copy
of an earlier packet of the bundle or a forgery).  The two routes are
interleaved on one engine through set_debug: per case 5 warm-up and `--steps`
(default 20) timed calls of each, HIP events around srtp_transform_device,
every call on a fresh transformer over a fresh copy of the sealed input.
Reported: median, p10 and p90 per route, and whether the one-pass route's
median lies below the two-pass route's by more than the latter's p90 - p10
(the rule the default limits are set by).  At the largest lane size also GCM
SRTCP and the AES_CM_128_HMAC_SHA1_80 yardstick on the same bundle.

    python tools/gcm_open_bench.py [--out sweep.json] [--lane 14,16,18] [--wave 1,16,64,256,1024,4096,8192]
                                   [--steps 20] [--once LG]

--once LG: one unprotect of 2^LG clean packets per route and key size, no
events (the workload for a kernel trace).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libjitsi_amd import (SRTCPTransformer, SRTPContextFactory, SRTPEngine, SRTPTransformer,  # noqa: E402
                          profile_policies, synth)
from libjitsi_amd import _native as N  # noqa: E402

PKT, NSSRC, WARM = 1200, 10000, 5


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--lane", default="14,16,18")
    ap.add_argument("--wave", default="1,16,64,256,1024,4096,8192")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--once", type=int)
    args = ap.parse_args()
    import torch
    d = torch.device("cuda", 0)
    steps = max(args.steps, 1)
    rows = []
    lane = [1 << int(x) for x in args.lane.split(",") if x]
    wave = [int(x) for x in args.wave.split(",") if x]
    if args.once is not None:
        lane, wave = [1 << args.once], []
    cases = [("lane", n) for n in lane] + [("wave", n) for n in wave]
    top = max(lane) if lane else 0

    for kernels, n in cases:
        route = N.DEBUG_NO_GCM_WAVE if kernels == "lane" else N.DEBUG_FORCE_GCM_WAVE

        def bundle(kind):
            if kind == "rtcp":
                b = synth.rtcp_bundle(n, NSSRC, (PKT - 4, PKT - 4), seed=synth.SEED_BASE + n)
                assert (b.cap >= b.length + 20).all()
            else:
                b = synth.rtp_bundle(n, min(NSSRC, n), PKT, seed=synth.SEED_BASE + n)
            t = lambda a: torch.from_numpy(a.view(np.int32)).to(d)
            return b, torch.from_numpy(b.seg).to(d), t(b.off), t(b.cap), t(b.length)

        def measure(eng, name, pols, key, salt, kind, faults, flag_sets):
            """flag_sets: {route name: debug flags}, interleaved call by call."""
            b, seg0, off, cap, ln0 = bundle(kind)
            T = SRTCPTransformer if kind == "rtcp" else SRTPTransformer
            st = torch.empty(n, dtype=torch.int32, device=d)
            seg, ln = seg0.clone(), ln0.clone()
            snd = T(SRTPContextFactory(True, key, salt, *pols, engine=eng))
            eng.set_debug(0)
            eng.transform_device(False, snd.tid, seg, off, ln, cap, st)
            torch.cuda.synchronize()
            assert int((st != 0).sum()) == 0
            snd.close()
            sealed, sln = seg.clone(), ln.clone()
            want_bad = 0
            if faults:  # every 40th packet: a copy of an earlier one (a replay), or one flipped bit (a forgery)
                o, L = b.off.astype(np.int64), int(sln[0])
                assert bool((sln == L).all())
                for k, i in enumerate(range(40, n, 40)):
                    at, src = int(o[i]), int(o[i - 17])
                    if k % 2 == 0:
                        sealed[at:at + L] = sealed[src:src + L].clone()
                    else:
                        sealed[at + 700:at + 701] ^= 0x04
                    want_bad += 1

            def call(flags, timed):
                t = T(SRTPContextFactory(False, key, salt, *pols, engine=eng))
                eng.set_debug(flags)
                seg.copy_(sealed)
                ln.copy_(sln)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if timed:
                    a.record()
                eng.transform_device(True, t.tid, seg, off, ln, cap, st)
                if timed:
                    e.record()
                torch.cuda.synchronize()
                assert int((st != 0).sum()) == want_bad, (name, int((st != 0).sum()), want_bad)
                t.close()
                return a.elapsed_time(e) if timed else 0.0

            if args.once is not None:
                for fl in flag_sets.values():
                    call(fl, False)
                return
            for _ in range(WARM):
                for fl in flag_sets.values():
                    call(fl, False)
            ms = {k: [] for k in flag_sets}
            for _ in range(steps):
                for k, fl in flag_sets.items():
                    ms[k].append(call(fl, True))
            eng.set_debug(0)
            r = {"route": kernels, "packets": n, "case": name, "faults": bool(faults)}
            for k, v in ms.items():
                r[k] = {"median_ms": round(pct(v, 50), 4), "p10_ms": round(pct(v, 10), 4), "p90_ms": round(pct(v, 90), 4),
                        "mpps": round(n / pct(v, 50) / 1e3, 2)}
            if "fused" in r and "two_pass" in r:
                spread = r["two_pass"]["p90_ms"] - r["two_pass"]["p10_ms"]
                r["two_pass_spread_ms"] = round(spread, 4)
                r["fused_over_two_pass"] = round(r["fused"]["median_ms"] / r["two_pass"]["median_ms"], 3)
                r["fused_wins"] = bool(r["two_pass"]["median_ms"] - r["fused"]["median_ms"] > spread)
            rows.append(r)
            print(json.dumps(r), flush=True)

        rng = np.random.default_rng(n)
        eng = SRTPEngine(device=0, max_contexts=1 << 16, max_factories=1024, max_transformers=1024, max_batch=n)
        eng.enable_aead()
        ab = {"fused": route | N.DEBUG_FORCE_GCM_SPEC, "two_pass": route | N.DEBUG_NO_GCM_SPEC}
        for klen in (16, 32):
            pols = profile_policies("AEAD_AES_%d_GCM" % (8 * klen))
            key = bytes(rng.integers(0, 256, klen, dtype=np.uint8))
            salt = bytes(rng.integers(0, 256, 12, dtype=np.uint8))
            for faults in ((False,) if args.once is not None else (False, True)):
                if faults and n < 80:
                    continue  # no 40th packet with an earlier one to copy and a second to forge
                measure(eng, "gcm%d_srtp_unprotect" % (8 * klen), pols, key, salt, "rtp", faults, ab)
        if kernels == "lane" and n == top and args.once is None:
            pols = profile_policies("AEAD_AES_128_GCM")
            key, salt = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 12, dtype=np.uint8))
            measure(eng, "gcm128_srtcp_unprotect", pols, key, salt, "rtcp", False, ab)
        eng.close()
        if kernels == "lane" and n == top and args.once is None:
            # the yardstick on an engine of its own (one with a GCM key set takes no split path)
            eng = SRTPEngine(device=0, max_contexts=1 << 16, max_factories=1024, max_transformers=1024, max_batch=n)
            (k, s), = synth.keys(1, 1)
            measure(eng, "aes_cm_128_hmac_sha1_80_unprotect", profile_policies("AES_CM_128_HMAC_SHA1_80"), k, s, "rtp",
                    False, {"yardstick": 0})
            eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "warmup": WARM, "steps": steps, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
