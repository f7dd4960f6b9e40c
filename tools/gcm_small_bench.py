#!/usr/bin/env python3
"""Small AES-GCM bundles on one MI355X: where a wave per packet (k_gcm_wave)
beats a lane per packet (k_gcm), where one launch (k_small's GCM instance)
beats the multi-kernel chain, and what a lone per-packet call costs.

sweep   protect and unprotect of n 1200-byte GCM-128 SRTP packets (n distinct
        streams) through srtp_transform_device, each call between two HIP
        events, for n in --sizes.  Both routes run on the same engine,
        interleaved call by call (SRTP_DEBUG_NO_GCM_WAVE / _FORCE_GCM_WAVE);
        --warmup calls per route first, then --steps timed ones.  Per route the
        median, p10 and p90; `spread` is p90 - p10.  The wave route `wins` at n
        when its median is below the lane route's by more than the lane
        route's spread, in both directions: kGcmWaveMax (bundle_plan.h) is
        the largest such n.
small   the same sweep with the one-launch route (SRTP_DEBUG_FORCE_SMALL: at
        every size up to k_small's 255) against the chain (SRTP_DEBUG_NO_SMALL)
        on an engine that holds a GCM factory, for GCM-128 SRTP bundles and
        for AES_CM_128_HMAC_SHA1_80 bundles (--profile gcm,aescm).  The
        one-launch route `wins` at n when its median is below the chain's by
        more than the chain's spread, in both directions: kSmallGcmMax
        (bundle_plan.h) is the largest n up to which it wins for both
        profiles.
lone    the per-packet drop-in: p50 / p90 wall time of --calls synchronous
        srtp_aggregator_transform calls from one thread, for a 1200-byte GCM
        SRTP packet, a 200-byte GCM SRTCP packet and the 1200-byte
        AES_CM_128_HMAC_SHA1_80 yardstick, per route.  On a tree without the
        20-byte trailer room the SRTCP call answers ERR_CAPACITY; it is then
        measured as a one-packet srtp_transform_host bundle and marked so.
once    one small GCM bundle each way and nothing else (the workload for
        rocprofv3 --kernel-trace --stats -- python tools/gcm_small_bench.py once).

    python tools/gcm_small_bench.py sweep|small|lone|once [--out file.json] [--route default|lane|wave|nosmall]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libjitsi_amd import (SRTCPTransformer, SRTPAggregator, SRTPContextFactory, SRTPEngine,  # noqa: E402
                          SRTPTransformer, profile_policies, synth)
from libjitsi_amd import _native as N  # noqa: E402

PKT = 1200
ROUTES = {"default": 0, "lane": getattr(N, "DEBUG_NO_GCM_WAVE", None), "wave": getattr(N, "DEBUG_FORCE_GCM_WAVE", None),
          "small": getattr(N, "DEBUG_FORCE_SMALL", None), "chain": getattr(N, "DEBUG_NO_SMALL", None),
          "nosmall": getattr(N, "DEBUG_NO_SMALL", None)}


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def summary(v):
    return {"median": round(statistics.median(v), 4), "p10": round(pct(v, 0.1), 4), "p90": round(pct(v, 0.9), 4),
            "spread": round(pct(v, 0.9) - pct(v, 0.1), 4)}


def gcm_engine(n):
    eng = SRTPEngine(device=0, max_contexts=1 << 15, max_factories=1024, max_transformers=1024, max_batch=max(n, 64))
    eng.enable_aead()
    return eng


def sweep(args, old="lane", new="wave", profile="gcm"):
    """`new` against `old` (two of ROUTES), interleaved call by call on one engine."""
    import torch
    d = torch.device("cuda", 0)
    rows = []
    gpols = profile_policies("AEAD_AES_128_GCM")
    rng = np.random.default_rng(1)
    key, salt = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 12, dtype=np.uint8))
    pols = gpols
    if profile == "aescm":  # AES-CM + HMAC-SHA1 bundles of an engine that holds a GCM factory
        pols = profile_policies("AES_CM_128_HMAC_SHA1_80")
        (key, salt), = synth.keys(1, 1)
    for n in (int(x) for x in args.sizes.split(",")):
        eng = gcm_engine(n)
        held = SRTPContextFactory(True, bytes(16), bytes(12), *gpols, engine=eng)  # noqa: F841 -- the engine's GCM key sets
        b = synth.rtp_bundle(n, n, PKT, seed=synth.SEED_BASE + n)
        seg0 = torch.from_numpy(b.seg).to(d)
        off = torch.from_numpy(b.off.view(np.int32)).to(d)
        cap = torch.from_numpy(b.cap.view(np.int32)).to(d)
        ln0 = torch.from_numpy(b.length.view(np.int32)).to(d)
        st = torch.empty(n, dtype=torch.int32, device=d)
        seg, ln = seg0.clone(), ln0.clone()
        sealed = [None, None]

        def call(route, reverse):
            eng.set_debug(ROUTES[route])
            t = SRTPTransformer(SRTPContextFactory(not reverse, key, salt, *pols, engine=eng))
            seg.copy_(sealed[0] if reverse else seg0)
            ln.copy_(sealed[1] if reverse else ln0)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.transform_device(reverse, t.tid, seg, off, ln, cap, st)
            e.record()
            torch.cuda.synchronize()
            assert int((st != 0).sum()) == 0
            t.close()
            return a.elapsed_time(e) * 1e3  # us

        ms = {(r, rev): [] for r in (old, new) for rev in (False, True)}
        for rev in (False, True):
            for i in range(args.warmup + args.steps):
                for r in (old, new):
                    v = call(r, rev)
                    if i >= args.warmup:
                        ms[(r, rev)].append(v)
            if not rev:
                sealed = [seg.clone(), ln.clone()]
        row = {"packets": n, "unit": "us"}
        if (old, new) != ("lane", "wave"):
            row["profile"] = profile
        wins = True
        for rev in (False, True):
            way = "unprotect" if rev else "protect"
            so, sn = summary(ms[(old, rev)]), summary(ms[(new, rev)])
            row[way] = {old: so, new: sn}
            wins = wins and sn["median"] < so["median"] - so["spread"]
        row[new + "_wins"] = wins
        rows.append(row)
        print(json.dumps(row), flush=True)
        eng.close()
    return rows


def small(args):
    rows = []
    for profile in args.profile.split(","):
        rows += sweep(args, "chain", "small", profile)
    return rows


def lone(args):
    rows = []
    rng = np.random.default_rng(2)
    routes = [r for r in args.route.split(",") if ROUTES.get(r) is not None]
    for route in routes:
        eng = gcm_engine(64)
        if ROUTES[route]:
            eng.set_debug(ROUTES[route])
        agg = SRTPAggregator(eng, None, max_packets=4096, max_bytes=8 << 20, deadline_us=500, depth=4)
        room = getattr(agg, "trailer_room", 16)
        cases = []
        gp = profile_policies("AEAD_AES_128_GCM")
        gk = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 12, dtype=np.uint8))
        (ak, asalt), = synth.keys(1, 1)
        ap = profile_policies("AES_CM_128_HMAC_SHA1_80")
        hdr = lambda ssrc, seq: bytes([0x80, 96]) + (seq & 0xFFFF).to_bytes(2, "big") + bytes(4) + ssrc.to_bytes(4, "big")  # noqa: E731
        body = bytes(rng.integers(0, 256, PKT, dtype=np.uint8))
        cases.append(("gcm128_srtp_1200", SRTPTransformer, gp, gk, lambda i: hdr(0x51, i) + body[:PKT - 12]))
        cases.append(("gcm128_srtcp_200", SRTCPTransformer, gp, gk,
                      lambda i: bytes([0x80, 200, 0, 49]) + (0x52).to_bytes(4, "big") + body[:192]))
        cases.append(("aes_cm_128_hmac_sha1_80_srtp_1200", SRTPTransformer, ap, (ak, asalt),
                      lambda i: hdr(0x53, i) + body[:PKT - 12]))
        for name, cls, pols, (k, s), mk in cases:
            snd = cls(SRTPContextFactory(True, k, s, *pols, engine=eng))
            rcv = cls(SRTPContextFactory(False, k, s, *pols, engine=eng))
            via = "srtp_aggregator_transform"
            st, _ = agg.transform(False, snd, mk(0))
            if st == N.STATUS_ERR_CAPACITY:  # a tree whose per-packet paths leave 16 bytes: the bundle path, n = 1
                via = "srtp_transform_host, n = 1"

            def one(reverse, t, data):
                if via == "srtp_aggregator_transform":
                    return agg.transform(reverse, t, data)
                cap = (len(data) + 20 + 15) & ~15
                seg = np.zeros(cap, np.uint8)
                seg[:len(data)] = np.frombuffer(data, np.uint8)
                ln = np.array([len(data)], np.uint32)
                st = eng.transform_host(reverse, t.tid, seg, np.zeros(1, np.uint32), ln, np.array([cap], np.uint32))
                return int(st[0]), seg[:int(ln[0])].tobytes()

            tp, tu = [], []
            for i in range(1, args.warm_calls + args.calls + 1):
                data = mk(i)
                t0 = time.perf_counter_ns()
                st, out = one(False, snd, data)
                t1 = time.perf_counter_ns()
                st2, back = one(True, rcv, out)
                t2 = time.perf_counter_ns()
                assert st == 0 and st2 == 0 and back == data, (name, i, st, st2)
                if i > args.warm_calls:
                    tp.append((t1 - t0) / 1e3)
                    tu.append((t2 - t1) / 1e3)
            row = {"case": name, "route": route, "via": via, "room": room, "calls": args.calls, "unit": "us",
                   "protect": summary(tp), "unprotect": summary(tu)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        agg.close()
        eng.close()
    return rows


def once(args):
    eng = gcm_engine(64)
    if ROUTES.get(args.route.split(",")[0]):
        eng.set_debug(ROUTES[args.route.split(",")[0]])
    pols = profile_policies("AEAD_AES_128_GCM")
    key, salt = bytes(range(16)), bytes(range(12))
    b = synth.rtp_bundle(16, 16, PKT, seed=synth.SEED_BASE)
    seg, ln = b.seg.copy(), b.length.copy()
    for reverse in (False, True):
        t = SRTPTransformer(SRTPContextFactory(not reverse, key, salt, *pols, engine=eng))
        st = eng.transform_host(reverse, t.tid, seg, b.off, ln, b.cap)
        assert (st == 0).all()
    eng.close()
    return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sweep", "small", "lone", "once"])
    ap.add_argument("--out")
    ap.add_argument("--sizes", help="default: 1,4,16,64,256,1024,4096,8192 (sweep); 1,4,8,16,64,255 (small)")
    ap.add_argument("--profile", default="gcm,aescm")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warm-calls", type=int, default=200)
    ap.add_argument("--route", default="default,lane,wave")
    args = ap.parse_args()
    if not args.sizes:
        args.sizes = "1,4,8,16,64,255" if args.mode == "small" else "1,4,16,64,256,1024,4096,8192"
    import torch
    rows = {"sweep": sweep, "small": small, "lone": lone, "once": once}[args.mode](args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "mode": args.mode, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
