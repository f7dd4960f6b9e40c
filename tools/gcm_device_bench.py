#!/usr/bin/env python3
"""Rate of the stateless GPU AES-GCM batch (srtp_aes_gcm_device, k_gcm_aead) on
one MI355X, beside the engine's AES_CM_128_HMAC_SHA1_80 path on the same
packets as the yardstick.

Bundles of 2^14 and 2^18 1200-byte SRTP packets over 10k streams: the GCM batch
takes the 12-byte RTP header as AAD and the 1188 payload bytes as data (the
RFC 7714 SRTP shape; its IVs here are random, the batch has no contexts), seal
and open, 128- and 256-bit keys.  The yardstick is the engine's protect and
unprotect of the same bundle (parse, sort, walk and the fused AES-CM + HMAC
kernels: it does more than the bare AEAD, which is all the batch is).

Where the time of a seal goes -- GHASH against AES-CTR -- is measured with the
same 1200 bytes as AAD only (aad_len = 1200, len = 0: 75 GHASH blocks and the
one AES pair of the tag mask): the difference to the full seal is the AES-CTR
pass and its stores.

HIP events around `reps` back-to-back calls, after a warm-up call; the median
of `rounds` such measurements.

    python tools/gcm_device_bench.py [--out file.json] [--sizes 14,18] [--once]

--once: one call per case and no events (the workload for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/gcm_device_bench.py --once).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libjitsi_amd import (SRTPContextFactory, SRTPEngine, SRTPTransformer, profile_policies,  # noqa: E402
                          srtp, synth)

PKT, HDR, NSSRC = 1200, 12, 10000


def event_ms(torch, fn, reps, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="14,18")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    d = torch.device("cuda", 0)
    rows = []
    for lg in (int(x) for x in args.sizes.split(",")):
        n = 1 << lg
        reps, rounds = (1, 1) if args.once else ((20, 5) if lg <= 14 else (3, 5))
        b = synth.rtp_bundle(n, NSSRC, PKT, seed=synth.SEED_BASE + lg)
        assert (b.length == PKT).all()
        eng = SRTPEngine(device=0, max_contexts=1 << 16, max_factories=64, max_transformers=64, max_batch=n)
        seg0 = torch.from_numpy(b.seg).to(d)
        off = torch.from_numpy(b.off.view(np.int32)).to(d)
        rng = np.random.default_rng(lg)
        iv = torch.from_numpy(rng.integers(0, 256, 12 * n, dtype=np.uint8)).to(d)
        tag = torch.empty(16 * n, dtype=torch.uint8, device=d)
        res = torch.empty(n, dtype=torch.int32, device=d)
        full = lambda v: torch.full((n,), v, dtype=torch.int32, device=d)  # noqa: E731
        shapes = {"srtp": (full(HDR), full(PKT - HDR)), "aad_only": (full(PKT), full(0))}
        for klen in (16, 32):
            key = bytes(rng.integers(0, 256, klen, dtype=np.uint8))
            for shape, (al, dl) in shapes.items():
                seg = seg0.clone()
                ms = event_ms(torch, lambda: srtp.aes_gcm_device(eng, key, seg, off, al, dl, iv, tag), reps, rounds)
                rows.append({"packets": n, "case": f"gcm{klen * 8}_seal_{shape}", "ms": round(ms, 4),
                             "pps": round(n / ms * 1e3, 1)})
                if shape != "srtp":
                    continue
                # open what one seal made: the data is deciphered in place, so
                # every timed call gets a fresh copy of the sealed segment
                sealed = seg0.clone()
                srtp.aes_gcm_device(eng, key, sealed, off, al, dl, iv, tag)
                work = sealed.clone()

                def open_():
                    work.copy_(sealed)
                    srtp.aes_gcm_device(eng, key, work, off, al, dl, iv, tag, result=res, open=True)
                ms_c = event_ms(torch, lambda: work.copy_(sealed), reps, rounds)
                ms_o = event_ms(torch, open_, reps, rounds)
                assert int(res.sum()) == 0 and torch.equal(work, seg0)
                rows.append({"packets": n, "case": f"gcm{klen * 8}_open_srtp", "ms": round(ms_o - ms_c, 4),
                             "pps": round(n / (ms_o - ms_c) * 1e3, 1),
                             "note": "segment copy of %.4f ms subtracted" % ms_c})
        # the yardstick: the engine's AES_CM_128_HMAC_SHA1_80 on the same bundle
        pols = profile_policies("AES_CM_128_HMAC_SHA1_80")
        (k, s), = synth.keys(1, 1)
        cap = torch.from_numpy(b.cap.view(np.int32)).to(d)
        st = torch.empty(n, dtype=torch.int32, device=d)
        ln0 = torch.from_numpy(b.length.view(np.int32)).to(d)
        seg, ln = seg0.clone(), ln0.clone()

        def engine_ms(reverse, src_seg, src_len):
            # every timed call needs unseen sequence numbers (the replay
            # window, both ways), so it is one call on a fresh transformer;
            # the first call warms the kernels and is not counted
            ts = []
            for r in range(1 if args.once else rounds + 1):
                t = SRTPTransformer(SRTPContextFactory(not reverse, k, s, *pols, engine=eng))
                seg.copy_(src_seg)
                ln.copy_(src_len)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.transform_device(reverse, t.tid, seg, off, ln, cap, st)
                e.record()
                torch.cuda.synchronize()
                assert int((st != 0).sum()) == 0
                if r or args.once:
                    ts.append(a.elapsed_time(e))
                t.close()
            return statistics.median(ts)
        ms_p = engine_ms(False, seg0, ln0)
        pseg, pln = seg.clone(), ln.clone()
        ms_u = engine_ms(True, pseg, pln)
        for case, ms in (("protect", ms_p), ("unprotect", ms_u)):
            rows.append({"packets": n, "case": "aes_cm_128_hmac_sha1_80_" + case, "ms": round(ms, 4),
                         "pps": round(n / ms * 1e3, 1)})
        eng.close()
    by = {(r["packets"], r["case"]): r for r in rows}
    for r in rows:
        if r["case"].startswith("gcm") and r["case"].endswith("_srtp"):
            y = by[(r["packets"], "aes_cm_128_hmac_sha1_80_" + ("protect" if "_seal_" in r["case"] else "unprotect"))]
            r["of_yardstick"] = round(r["pps"] / y["pps"], 3)
        if r["case"].endswith("_seal_srtp"):
            g = by[(r["packets"], r["case"].replace("_srtp", "_aad_only"))]
            r["ghash_share"] = round(g["ms"] / r["ms"], 3)
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
