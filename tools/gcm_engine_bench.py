#!/usr/bin/env python3
"""Rate of the RFC 7714 AES-GCM profiles through the engine's packet path
(srtp_transform_device behind srtp_engine_enable_aead) on one MI355X, beside
the stateless batch (srtp_aes_gcm_device) at the same size and the engine's
AES_CM_128_HMAC_SHA1_80 path on the same bundle.

Bundles of 2^18 and 2^14 1200-byte SRTP packets over 10k streams.  Per case a
warm-up call, then `--steps` (default 20) timed calls, each between two HIP
events; every call runs on a fresh transformer (a bundle's sequence numbers
must be unseen, both ways) over a fresh copy of its input.  The median is
reported, with the engine's own per-stage times (srtp_engine_set_timing:
parse, sort, verify, walk, protect, decrypt) from five further calls.

    python tools/gcm_engine_bench.py [--out file.json] [--sizes 18,14] [--steps 20] [--once]

--once: one call per case and no events (the workload for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/gcm_engine_bench.py --once).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="18,14")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    d = torch.device("cuda", 0)
    steps = 1 if args.once else max(args.steps, 1)
    rows = []
    for lg in (int(x) for x in args.sizes.split(",")):
        n = 1 << lg
        b = synth.rtp_bundle(n, NSSRC, PKT, seed=synth.SEED_BASE + lg)
        assert (b.length == PKT).all() and (b.cap >= PKT + 16).all()
        seg0 = torch.from_numpy(b.seg).to(d)
        off = torch.from_numpy(b.off.view(np.int32)).to(d)
        cap = torch.from_numpy(b.cap.view(np.int32)).to(d)
        ln0 = torch.from_numpy(b.length.view(np.int32)).to(d)
        st = torch.empty(n, dtype=torch.int32, device=d)
        seg, ln = seg0.clone(), ln0.clone()

        def engine_case(eng, pols, key, salt, reverse, src_seg, src_len):
            """(median ms, stage ms) of one direction of one profile."""
            def call(timed):
                t = SRTPTransformer(SRTPContextFactory(not reverse, key, salt, *pols, engine=eng))
                seg.copy_(src_seg)
                ln.copy_(src_len)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if timed:
                    a.record()
                eng.transform_device(reverse, t.tid, seg, off, ln, cap, st)
                if timed:
                    e.record()
                torch.cuda.synchronize()
                assert int((st != 0).sum()) == 0
                t.close()
                return a.elapsed_time(e) if timed else 0.0
            if args.once:
                call(False)
                return 0.0, {}
            call(False)  # warm-up
            ms = statistics.median(call(True) for _ in range(steps))
            eng.set_timing(True)
            eng.read_timing()
            for _ in range(5):
                call(False)
            stage = {k: round(v[0] / v[1], 4) for k, v in eng.read_timing().items() if v[1]}
            eng.set_timing(False)
            return ms, stage

        def add(case, ms, stage=None, **kw):
            r = {"packets": n, "case": case, "ms": round(ms, 4), "pps": round(n / ms * 1e3, 1) if ms else None}
            if stage:
                r["stage_ms"] = stage
            r.update(kw)
            rows.append(r)

        rng = np.random.default_rng(lg)
        # the engine's GCM path
        eng = SRTPEngine(device=0, max_contexts=1 << 16, max_factories=512, max_transformers=512, max_batch=n)
        eng.enable_aead()
        for klen in (16, 32):
            pols = profile_policies("AEAD_AES_%d_GCM" % (8 * klen))
            key, salt = bytes(rng.integers(0, 256, klen, dtype=np.uint8)), bytes(rng.integers(0, 256, 12, dtype=np.uint8))
            ms_p, st_p = engine_case(eng, pols, key, salt, False, seg0, ln0)
            pseg, pln = seg.clone(), ln.clone()
            ms_u, st_u = engine_case(eng, pols, key, salt, True, pseg, pln)
            o0 = int(b.off[0])  # the round trip gave the plaintext back
            assert torch.equal(ln, ln0) and torch.equal(seg[o0:o0 + PKT], seg0[o0:o0 + PKT])
            add("engine_gcm%d_protect" % (8 * klen), ms_p, st_p)
            add("engine_gcm%d_unprotect" % (8 * klen), ms_u, st_u)
            del pseg
        # the stateless batch at the same size (header as AAD, payload as data)
        iv = torch.from_numpy(rng.integers(0, 256, 12 * n, dtype=np.uint8)).to(d)
        tag = torch.empty(16 * n, dtype=torch.uint8, device=d)
        res = torch.empty(n, dtype=torch.int32, device=d)
        al = torch.full((n,), HDR, dtype=torch.int32, device=d)
        dl = torch.full((n,), PKT - HDR, dtype=torch.int32, device=d)
        for klen in (16, 32):
            key = bytes(rng.integers(0, 256, klen, dtype=np.uint8))
            sealed = seg0.clone()
            srtp.aes_gcm_device(eng, key, sealed, off, al, dl, iv, tag)
            for open_ in (False, True):
                def call(timed):
                    seg.copy_(sealed if open_ else seg0)
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    srtp.aes_gcm_device(eng, key, seg, off, al, dl, iv, tag, result=res if open_ else None, open=open_)
                    e.record()
                    torch.cuda.synchronize()
                    return a.elapsed_time(e)
                call(False)
                ms = statistics.median(call(True) for _ in range(steps))
                add("batch_gcm%d_%s" % (8 * klen, "open" if open_ else "seal"), ms)
        eng.close()
        # the yardstick on an engine of its own (one with a GCM key set takes no split path)
        eng = SRTPEngine(device=0, max_contexts=1 << 16, max_factories=512, max_transformers=512, max_batch=n)
        pols = profile_policies("AES_CM_128_HMAC_SHA1_80")
        (k, s), = synth.keys(1, 1)
        ms_p, st_p = engine_case(eng, pols, k, s, False, seg0, ln0)
        pseg, pln = seg.clone(), ln.clone()
        ms_u, st_u = engine_case(eng, pols, k, s, True, pseg, pln)
        add("engine_aes_cm_128_hmac_sha1_80_protect", ms_p, st_p)
        add("engine_aes_cm_128_hmac_sha1_80_unprotect", ms_u, st_u)
        eng.close()
        del pseg, seg, seg0
    # each engine GCM time against the batch time + that run's parse + sort + walk
    by = {(r["packets"], r["case"]): r for r in rows}
    for r in rows:
        if r["case"].startswith("engine_gcm") and r.get("stage_ms"):
            bits, way = r["case"][10:13], r["case"].split("_")[-1]
            batch = by[(r["packets"], "batch_gcm%s_%s" % (bits, "seal" if way == "protect" else "open"))]
            s = r["stage_ms"]
            floor = batch["ms"] + s.get("parse", 0) + s.get("sort", 0) + s.get("walk", 0)
            r["batch_plus_parse_sort_walk_ms"] = round(floor, 4)
            r["over_that_sum"] = round(r["ms"] / floor, 3)
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": steps, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
