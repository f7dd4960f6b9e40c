#!/usr/bin/env python3
"""Fan-out on the device against the routes the engine offered before it.

  --host    2^16 destinations of 1200-byte sources, N in {1, 2, 4, 8, 16} peers,
            AES_CM_128_HMAC_SHA1_80 and AEAD_AES_128_GCM: SRTPEngine.fanout_host
            against host expansion into a pinned segment (timed: the application
            pays it) plus transform_host.  Both routes interleaved on one engine,
            5 warm-up and 20 timed calls each, wall-clock medians with p10 / p90
            and the host-to-device bytes of a call; per N, whether the medians
            differ by more than the wider of the two spreads.
  --device  n = 2^18, N = 8: fanout_device against transform_device on a
            pre-expanded bundle, HIP events; and a plain device copy of the bytes
            k_fanout writes, in the same process.
  --once    three fanout_device calls of the --device shape and nothing else
            (for a kernel trace of k_fanout in a run of its own); with
            --rewrite, three fanout_device_rw calls instead (k_fanout_rw).
  --rewrite per-destination rewriting (srtp_fanout_*_rw), every entry with all
            four fields set.  Device route, n = 2^18, N = 8: fanout_device_rw
            against fanout_device, alternating call by call, HIP events.  Host
            route, 2^16 destinations at N in {1, 4, 16}: fanout_host_rw against
            what such a bridge does without it -- host expansion with the four
            setters applied (numpy, one thread, timed) plus transform_host.
  --stamp   abs-send-time stamping (srtp_fanout_*_ast): 1200-byte sources with
            X set and three one-byte-header elements, the abs-send-time one (ID
            3) the second, no CSRC; every entry's record on, with a value of
            its own per call.  Device route, n = 2^18, N = 8: fanout_device_ast
            with stamp records only, and with rewrite records as well, against
            fanout_device_rw and fanout_device over the same sources, the four
            alternating call by call, HIP events.  Host route, 2^16
            destinations at N in {1, 4, 16}: fanout_host_ast against host
            expansion with the three bytes written into every copy (numpy,
            timed) plus transform_host.  With --once: three fanout_device_ast
            calls (stamp records only) and nothing else (a trace of
            k_fanout_ast); --stamp-records off | miss takes the walk, or the
            stamp, out of that trace.
  --payload payload patches (srtp_fanout_*_pay): the --stamp sources (a header
            of 28 bytes); every entry's record has both patches on, an FEC SN
            base at bytes 42..43 (patch 0) and the RTX OSN at bytes 28..29
            (patch 1), with bytes of its own per call.  Device route, n = 2^18,
            N = 8: fanout_device_pay with patch records only, and with rewrite
            and stamp records as well, against fanout_device_ast (stamp only),
            fanout_device_rw and fanout_device over the same sources, the five
            alternating call by call, HIP events.  With --once: three
            fanout_device_pay calls (patch records only) and nothing else (a
            trace of k_fanout_pay).
  --plain   fanout_device of the --device shape and nothing else, 5 warm-up and
            20 timed calls (one side of a comparison between two builds of the
            library, a process each).

Every call gets sources with new sequence numbers (not timed, for either
route), so that no destination is a replay.  One JSON document on stdout, or
in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libjitsi_amd import (HostBuffer, SRTPContextFactory, SRTPEngine, SRTPTransformer,  # noqa: E402
                          profile_policies)

LEN, SRC_STRIDE, ROOM = 1200, 1200, 20
DST_CAP = LEN + ROOM
DST_STRIDE = (DST_CAP + 15) & ~15
WARM, TIMED = 5, 20


def peers(eng, profile, count):
    rng = np.random.default_rng(11)
    gcm = profile.startswith("AEAD")
    out = []
    for _ in range(count):
        mk = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        ms = rng.integers(0, 256, 12 if gcm else 14, dtype=np.uint8).tobytes()
        out.append(SRTPTransformer(SRTPContextFactory(True, mk, ms, *profile_policies(profile), engine=eng)))
    return out


class Sources:
    """m RTP packets of LEN bytes over up to 4096 SSRCs; advance() gives every one a new sequence number."""

    def __init__(self, m, seg):
        self.m, self.ssrcs = m, min(m, 4096)
        self.seg = seg
        self.rows = seg[:m * SRC_STRIDE].reshape(m, SRC_STRIDE)
        self.rows[:] = np.random.default_rng(5).integers(0, 256, (m, SRC_STRIDE), dtype=np.uint8)
        self.rows[:, 0], self.rows[:, 1] = 0x80, 96
        ssrc = (0x10000 + np.arange(m) % self.ssrcs).astype(">u4")
        self.rows[:, 8:12] = ssrc.view(np.uint8).reshape(m, 4)
        self.per_call = (m + self.ssrcs - 1) // self.ssrcs
        self.base = 1
        self.off = (np.arange(m) * SRC_STRIDE).astype(np.uint32)
        self.len = np.full(m, LEN, np.uint32)
        self.cap = np.full(m, SRC_STRIDE, np.uint32)
        self.advance()

    def with_extension(self):
        """X set and a one-byte-header extension of three words: ID 1 (1 byte), the
        abs-send-time element ID 3 (bytes 18..21, stamped at STAMP_AT), ID 5 (2 bytes)."""
        self.rows[:, 0] = 0x90
        self.rows[:, 12:28] = np.frombuffer(bytes([0xBE, 0xDE, 0, 3, 0x10, 0x77, 0x32, 0xA0, 0xA1, 0xA2, 0x51, 0x88, 0x99,
                                                   0, 0, 0]), np.uint8)
        return self

    def advance(self):
        self.seq = (self.base + np.arange(self.m) // self.ssrcs) & 0xFFFF  # this call's, host order
        seq = self.seq.astype(">u2")
        self.rows[:, 2:4] = seq.view(np.uint8).reshape(self.m, 2)
        self.base += self.per_call


def pct(xs):
    xs = np.sort(np.array(xs))
    return {"median_ms": float(np.median(xs)), "p10_ms": float(np.percentile(xs, 10)),
            "p90_ms": float(np.percentile(xs, 90))}


def verdict(a, b):
    """a: fan-out, b: the other route."""
    spread = max(a["p90_ms"] - a["p10_ms"], b["p90_ms"] - b["p10_ms"])
    d = b["median_ms"] - a["median_ms"]
    return "fan-out faster" if d > spread else "fan-out slower" if -d > spread else "no difference beyond the spread"


def host_case(eng, profile, n, fan):
    m = n // fan
    ts = peers(eng, profile, fan)
    hs, hd = HostBuffer(m * SRC_STRIDE), HostBuffer(n * DST_STRIDE)
    src = Sources(m, hs.array)
    src_idx = np.repeat(np.arange(m, dtype=np.int32), fan)  # source-major, doWrite's order
    tids = np.tile(np.array([t.tid for t in ts], np.int32), m)
    off = (np.arange(n, dtype=np.int64) * DST_STRIDE).astype(np.uint32)
    cap = np.full(n, DST_CAP, np.uint32)
    dst_rows = hd.array.reshape(n, DST_STRIDE)
    t_fan, t_old, t_expand = [], [], []
    for it in range(WARM + TIMED):
        src.advance()
        t0 = time.perf_counter()
        ln, st = eng.fanout_host(tids, src.seg, src.off, src.len, src.cap, src_idx, hd.array, off, cap)
        t1 = time.perf_counter()
        assert not st.any() and (ln == LEN + (16 if profile.startswith("AEAD") else 10)).all()
        src.advance()
        t2 = time.perf_counter()
        dst_rows[:, :LEN] = src.rows[src_idx]  # the N host-made copies
        ln = np.full(n, LEN, np.uint32)
        t3 = time.perf_counter()
        st = eng.transform_host(False, tids, hd.array, off, ln, cap)
        t4 = time.perf_counter()
        assert not st.any()
        if it >= WARM:
            t_fan.append((t1 - t0) * 1e3)
            t_old.append((t4 - t2) * 1e3)
            t_expand.append((t3 - t2) * 1e3)
    for t in ts:
        t.close()
    hs.close()
    hd.close()
    a, b = pct(t_fan), pct(t_old)
    small = 4 * n  # a uint32 / int32 array of n entries
    return {"profile": profile, "N": fan, "n": n, "m": m, "fanout_host": a, "expand_plus_transform_host": b,
            "host_expansion_alone": pct(t_expand),
            "h2d_bytes_fanout": m * SRC_STRIDE + 3 * 4 * m + 4 * small,  # sources, their 3 arrays; idx, off, cap, tids
            "h2d_bytes_expand": n * DST_STRIDE + 4 * small,              # the copies; off, len, cap, tids
            "verdict": verdict(a, b)}


def device_case(eng, n, fan, once):
    import torch
    m = n // fan
    ts = peers(eng, "AES_CM_128_HMAC_SHA1_80", fan)
    src = Sources(m, np.zeros(m * SRC_STRIDE, np.uint8))
    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    src_idx = np.repeat(np.arange(m, dtype=np.int32), fan)
    tids = d(np.tile(np.array([t.tid for t in ts], np.int32), m))
    off = d((np.arange(n, dtype=np.int64) * DST_STRIDE).astype(np.uint32))
    cap, s_off, s_len, s_cap, idx = d(np.full(n, DST_CAP, np.uint32)), d(src.off), d(src.len), d(src.cap), d(src_idx)
    seg = torch.zeros(n * DST_STRIDE, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    idx64 = idx.long()
    stream = torch.cuda.Stream()
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def fresh():
        src.advance()
        return d(src.seg)

    def fan_call(s_seg):
        eng.fanout_device(tids, s_seg, s_off, s_len, s_cap, idx, seg, off, ln, cap, st, stream=stream)

    if once:
        for _ in range(3):
            s_seg = fresh()
            torch.cuda.synchronize()
            fan_call(s_seg)
            eng.sync(stream.cuda_stream)
        assert not st.any().item()
        return {"once": 3, "n": n, "m": m}
    t_fan, t_old, t_copy = [], [], []
    plain_src = torch.zeros(n * LEN, dtype=torch.uint8, device="cuda")
    plain_dst = torch.zeros(n * LEN, dtype=torch.uint8, device="cuda")
    for it in range(WARM + TIMED):
        s_seg = fresh()
        torch.cuda.synchronize()
        a, b = ev(), ev()
        with torch.cuda.stream(stream):
            a.record()
            fan_call(s_seg)
            b.record()
        b.synchronize()
        eng.sync(stream.cuda_stream)
        assert not st.any().item()
        # the pre-expanded bundle: the copies made beforehand, outside the timing
        s_seg = fresh()
        seg.view(n, DST_STRIDE)[:, :LEN] = s_seg.view(m, SRC_STRIDE)[idx64]
        ln.fill_(LEN)
        torch.cuda.synchronize()
        c, e = ev(), ev()
        with torch.cuda.stream(stream):
            c.record()
            eng.transform_device(False, tids, seg, off, ln, cap, st, stream=stream)
            e.record()
        e.synchronize()
        eng.sync(stream.cuda_stream)
        assert not st.any().item()
        f, g = ev(), ev()
        with torch.cuda.stream(stream):
            f.record()
            plain_dst.copy_(plain_src)
            g.record()
        g.synchronize()
        if it >= WARM:
            t_fan.append(a.elapsed_time(b))
            t_old.append(c.elapsed_time(e))
            t_copy.append(f.elapsed_time(g))
    pa, pb, pc = pct(t_fan), pct(t_old), pct(t_copy)
    moved = n * LEN + m * LEN  # bytes k_fanout writes + distinct bytes it reads
    return {"n": n, "N": fan, "m": m, "fanout_device": pa, "transform_device_pre_expanded": pb,
            "plain_device_copy_of_n_x_1200_bytes": pc,
            "plain_copy_GBps_read_plus_written": 2 * n * LEN / (pc["median_ms"] * 1e6),
            "k_fanout_bytes_moved": moved,
            "k_fanout_ms_by_difference_of_medians": pa["median_ms"] - pb["median_ms"],
            "packets_per_s_fanout": n / (pa["median_ms"] * 1e-3),
            "packets_per_s_pre_expanded": n / (pb["median_ms"] * 1e-3)}


REWRITE_DTYPE = np.dtype([("mask", "<u4"), ("ssrc", "<u4"), ("timestamp", "<u4"), ("seq", "<u2"), ("pt", "u1"),
                          ("reserved", "u1")])  # srtp_fanout_rewrite


class Targets:
    """One record per destination entry with all four fields set: peer k sends
    source SSRC s on as 0x01000000 * (k + 1) + s, the source's sequence number
    + 7, a timestamp of its own and payload type 100.  update() follows the
    sources' new sequence numbers (not timed, for either route: the state
    machine that chooses the values runs on the host either way)."""

    def __init__(self, src, src_idx, fan):
        n = len(src_idx)
        self.src, self.src_idx = src, src_idx
        self.rw = np.zeros(n, REWRITE_DTYPE)
        self.rw["mask"] = 0xF
        peer = np.tile(np.arange(fan, dtype=np.uint32), n // fan)
        self.rw["ssrc"] = 0x01000000 * (peer + 1) + 0x10000 + src_idx % src.ssrcs
        self.rw["pt"] = 100
        self.update()

    def update(self):
        seq = (self.src.seq[self.src_idx] + 7) & 0xFFFF
        self.rw["seq"] = seq
        self.rw["timestamp"] = 0x5A000000 + 960 * seq

    def apply(self, rows):
        """RawPacket's four setters on the host-made copies (rows: n x stride bytes)."""
        rows[:, 1] = (rows[:, 1] & 0x80) | (self.rw["pt"] & 0x7F)
        rows[:, 2:4] = self.rw["seq"].astype(">u2").view(np.uint8).reshape(-1, 2)
        rows[:, 4:8] = self.rw["timestamp"].astype(">u4").view(np.uint8).reshape(-1, 4)
        rows[:, 8:12] = self.rw["ssrc"].astype(">u4").view(np.uint8).reshape(-1, 4)


def rewrite_host_case(eng, n, fan):
    profile = "AES_CM_128_HMAC_SHA1_80"
    m = n // fan
    ts = peers(eng, profile, fan)
    hs, hd = HostBuffer(m * SRC_STRIDE), HostBuffer(n * DST_STRIDE)
    src = Sources(m, hs.array)
    src_idx = np.repeat(np.arange(m, dtype=np.int32), fan)
    tids = np.tile(np.array([t.tid for t in ts], np.int32), m)
    off = (np.arange(n, dtype=np.int64) * DST_STRIDE).astype(np.uint32)
    cap = np.full(n, DST_CAP, np.uint32)
    dst_rows = hd.array.reshape(n, DST_STRIDE)
    tg = Targets(src, src_idx, fan)
    t_fan, t_old, t_expand = [], [], []
    for it in range(WARM + TIMED):
        src.advance()
        tg.update()
        t0 = time.perf_counter()
        ln, st = eng.fanout_host_rw(tids, src.seg, src.off, src.len, src.cap, src_idx, hd.array, off, cap,
                                    rewrite=tg.rw)
        t1 = time.perf_counter()
        assert not st.any() and (ln == LEN + 10).all()
        assert (dst_rows[:, 8:12] == tg.rw["ssrc"].astype(">u4").view(np.uint8).reshape(-1, 4)).all()
        src.advance()
        tg.update()
        t2 = time.perf_counter()
        dst_rows[:, :LEN] = src.rows[src_idx]  # the N host-made copies
        tg.apply(dst_rows)                     # and the send chain's setters on each
        ln = np.full(n, LEN, np.uint32)
        t3 = time.perf_counter()
        st = eng.transform_host(False, tids, hd.array, off, ln, cap)
        t4 = time.perf_counter()
        assert not st.any()
        if it >= WARM:
            t_fan.append((t1 - t0) * 1e3)
            t_old.append((t4 - t2) * 1e3)
            t_expand.append((t3 - t2) * 1e3)
    for t in ts:
        t.close()
    hs.close()
    hd.close()
    a, b = pct(t_fan), pct(t_old)
    return {"profile": profile, "N": fan, "n": n, "m": m, "fanout_host_rw": a,
            "expand_rewrite_plus_transform_host": b, "host_expansion_and_setters_alone": pct(t_expand),
            "h2d_bytes_fanout_rw": m * SRC_STRIDE + 3 * 4 * m + 4 * 4 * n + 16 * n,  # ... and the records
            "h2d_bytes_expand": n * DST_STRIDE + 4 * 4 * n, "verdict": verdict(a, b)}


def device_setup(eng, n, fan):
    import torch
    m = n // fan
    ts = peers(eng, "AES_CM_128_HMAC_SHA1_80", fan)
    src = Sources(m, np.zeros(m * SRC_STRIDE, np.uint8))
    d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    src_idx = np.repeat(np.arange(m, dtype=np.int32), fan)
    w = {"m": m, "src": src, "src_idx": src_idx, "d": d,
         "tids": d(np.tile(np.array([t.tid for t in ts], np.int32), m)),
         "off": d((np.arange(n, dtype=np.int64) * DST_STRIDE).astype(np.uint32)),
         "cap": d(np.full(n, DST_CAP, np.uint32)), "s_off": d(src.off), "s_len": d(src.len), "s_cap": d(src.cap),
         "idx": d(src_idx), "seg": torch.zeros(n * DST_STRIDE, dtype=torch.uint8, device="cuda"),
         "ln": torch.zeros(n, dtype=torch.int32, device="cuda"), "st": torch.zeros(n, dtype=torch.int32, device="cuda"),
         "stream": torch.cuda.Stream()}
    return w


def timed_fanout(eng, w, rewrite, stamp=None, pay=None):
    """One fan-out of fresh sources on the stream, between two HIP events: ms."""
    import torch
    w["src"].advance()
    s_seg = w["d"](w["src"].seg)
    rw = None
    if rewrite is not None:
        rewrite.update()
        rw = torch.from_numpy(rewrite.rw.view(np.uint8)).cuda()
    ast = None
    if stamp is not None:
        stamp.update()
        ast = torch.from_numpy(stamp.ast.view(np.uint8)).cuda()
    py = None
    if pay is not None:
        pay.update()
        py = torch.from_numpy(pay.pay.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(w["stream"]):
        a.record()
        if py is not None:
            eng.fanout_device_pay(w["tids"], s_seg, w["s_off"], w["s_len"], w["s_cap"], w["idx"], w["seg"], w["off"],
                                  w["ln"], w["cap"], w["st"], rw, ast, py, stream=w["stream"])
        elif ast is not None:
            eng.fanout_device_ast(w["tids"], s_seg, w["s_off"], w["s_len"], w["s_cap"], w["idx"], w["seg"], w["off"],
                                  w["ln"], w["cap"], w["st"], rw, ast, stream=w["stream"])
        elif rw is None:
            eng.fanout_device(w["tids"], s_seg, w["s_off"], w["s_len"], w["s_cap"], w["idx"], w["seg"], w["off"],
                              w["ln"], w["cap"], w["st"], stream=w["stream"])
        else:
            eng.fanout_device_rw(w["tids"], s_seg, w["s_off"], w["s_len"], w["s_cap"], w["idx"], w["seg"], w["off"],
                                 w["ln"], w["cap"], w["st"], rw, stream=w["stream"])
        b.record()
    b.synchronize()
    eng.sync(w["stream"].cuda_stream)
    assert not w["st"].any().item()
    return a.elapsed_time(b)


def rewrite_device_case(eng, n, fan):
    w = device_setup(eng, n, fan)
    tg = Targets(w["src"], w["src_idx"], fan)
    t_rw, t_plain = [], []
    for it in range(WARM + TIMED):
        x = timed_fanout(eng, w, tg)
        hdr = w["seg"].view(n, DST_STRIDE)[:: max(1, n // 64), 8:12].cpu().numpy()
        assert (hdr == tg.rw["ssrc"][:: max(1, n // 64)].astype(">u4").view(np.uint8).reshape(-1, 4)).all()
        y = timed_fanout(eng, w, None)
        if it >= WARM:
            t_rw.append(x)
            t_plain.append(y)
    a, b = pct(t_rw), pct(t_plain)
    spread = max(a["p90_ms"] - a["p10_ms"], b["p90_ms"] - b["p10_ms"])
    return {"n": n, "N": fan, "m": w["m"], "fanout_device_rw_all_four_fields": a, "fanout_device": b,
            "difference_of_medians_ms": a["median_ms"] - b["median_ms"], "wider_p90_minus_p10_ms": spread,
            "differ_by_more_than_the_spread": abs(a["median_ms"] - b["median_ms"]) > spread,
            "record_bytes_read": 16 * n, "bytes_written": n * LEN}


STAMP_AT = 19
AST_DTYPE = np.dtype([("value", "<u4"), ("id", "u1"), ("on", "u1"), ("reserved", "<u2")])  # srtp_fanout_abs_send_time


class Stamps:
    """One record per destination entry, on, ID 3; update() gives every entry a new 24-bit value."""

    def __init__(self, n, records="on"):
        self.n, self.tick = n, 0
        self.ast = np.zeros(n, AST_DTYPE)
        # off: no entry walks; miss: every entry walks past all three elements and stamps nothing
        self.ast["id"], self.ast["on"] = (9 if records == "miss" else 3), (0 if records == "off" else 1)
        self.update()

    def update(self):
        self.tick += 1
        self.ast["value"] = (np.arange(self.n, dtype=np.uint64) * 2654435761 + 977 * self.tick) & 0xFFFFFF

    def bytes3(self):
        v = self.ast["value"]
        return np.stack([(v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF], 1).astype(np.uint8)


def stamp_device_case(eng, n, fan):
    w = device_setup(eng, n, fan)
    w["src"].with_extension()
    tg, sp = Targets(w["src"], w["src_idx"], fan), Stamps(n)
    t = {"fanout_device_ast_stamp_only": [], "fanout_device_ast_stamp_and_rewrite": [],
         "fanout_device_rw_all_four_fields": [], "fanout_device": []}
    pick = slice(None, None, max(1, n // 64))
    for it in range(WARM + TIMED):
        for name, (rw, st) in zip(t, ((None, sp), (tg, sp), (tg, None), (None, None))):
            x = timed_fanout(eng, w, rw, st)
            if st is not None:
                got = w["seg"].view(n, DST_STRIDE)[pick, STAMP_AT:STAMP_AT + 3].cpu().numpy()
                assert (got == sp.bytes3()[pick]).all()
            if it >= WARM:
                t[name].append(x)
    res = {k: pct(v) for k, v in t.items()}
    a, r, p = (res[k] for k in ("fanout_device_ast_stamp_only", "fanout_device_rw_all_four_fields", "fanout_device"))
    spread = max(x["p90_ms"] - x["p10_ms"] for x in res.values())
    res.update({"n": n, "N": fan, "m": w["m"], "ast_minus_rw_ms": a["median_ms"] - r["median_ms"],
                "ast_minus_plain_ms": a["median_ms"] - p["median_ms"], "rw_minus_plain_ms": r["median_ms"] - p["median_ms"],
                "widest_p90_minus_p10_ms": spread, "record_bytes_read": 8 * n, "bytes_written": n * LEN})
    return res


def stamp_host_case(eng, n, fan):
    profile = "AES_CM_128_HMAC_SHA1_80"
    m = n // fan
    ts = peers(eng, profile, fan)
    hs, hd = HostBuffer(m * SRC_STRIDE), HostBuffer(n * DST_STRIDE)
    src = Sources(m, hs.array).with_extension()
    src_idx = np.repeat(np.arange(m, dtype=np.int32), fan)
    tids = np.tile(np.array([t.tid for t in ts], np.int32), m)
    off = (np.arange(n, dtype=np.int64) * DST_STRIDE).astype(np.uint32)
    cap = np.full(n, DST_CAP, np.uint32)
    dst_rows = hd.array.reshape(n, DST_STRIDE)
    sp = Stamps(n)
    t_fan, t_old, t_expand = [], [], []
    for it in range(WARM + TIMED):
        src.advance()
        sp.update()
        t0 = time.perf_counter()
        ln, st = eng.fanout_host_ast(tids, src.seg, src.off, src.len, src.cap, src_idx, hd.array, off, cap,
                                     stamp=sp.ast)
        t1 = time.perf_counter()
        assert not st.any() and (ln == LEN + 10).all()
        assert (dst_rows[:, STAMP_AT:STAMP_AT + 3] == sp.bytes3()).all()
        src.advance()
        sp.update()
        t2 = time.perf_counter()
        dst_rows[:, :LEN] = src.rows[src_idx]                # the N host-made copies
        dst_rows[:, STAMP_AT:STAMP_AT + 3] = sp.bytes3()     # and the send chain's stamp on each (no walk: a known offset)
        ln = np.full(n, LEN, np.uint32)
        t3 = time.perf_counter()
        st = eng.transform_host(False, tids, hd.array, off, ln, cap)
        t4 = time.perf_counter()
        assert not st.any()
        if it >= WARM:
            t_fan.append((t1 - t0) * 1e3)
            t_old.append((t4 - t2) * 1e3)
            t_expand.append((t3 - t2) * 1e3)
    for t in ts:
        t.close()
    hs.close()
    hd.close()
    a, b = pct(t_fan), pct(t_old)
    return {"profile": profile, "N": fan, "n": n, "m": m, "fanout_host_ast": a,
            "expand_stamp_plus_transform_host": b, "host_expansion_and_stamp_alone": pct(t_expand),
            "h2d_bytes_fanout_ast": m * SRC_STRIDE + 3 * 4 * m + 4 * 4 * n + 8 * n,  # ... and the records
            "h2d_bytes_expand": n * DST_STRIDE + 4 * 4 * n, "verdict": verdict(a, b)}


PAY_DTYPE = np.dtype([("at0", "<u2"), ("b0", "u1", (2,)), ("at1", "<u2"), ("b1", "u1", (2,))])  # srtp_fanout_payload
FEC_AT, OSN_AT = 42, 28


class Payloads:
    """One record per destination entry with both patches on; update() gives every entry new bytes."""

    def __init__(self, n):
        self.n, self.tick = n, 0
        self.pay = np.zeros(n, PAY_DTYPE)
        self.pay["at0"], self.pay["at1"] = FEC_AT, OSN_AT
        self.update()

    def update(self):
        self.tick += 1
        v = (np.arange(self.n, dtype=np.uint64) * 2246822519 + 131 * self.tick) & 0xFFFFFFFF
        self.pay["b0"] = np.stack([v & 0xFF, v & 0xFF], 1)  # rewriteFEC stores the low byte twice
        self.pay["b1"] = np.stack([(v >> 24) & 0xFF, (v >> 16) & 0xFF], 1)


def payload_device_case(eng, n, fan):
    w = device_setup(eng, n, fan)
    w["src"].with_extension()
    tg, sp, py = Targets(w["src"], w["src_idx"], fan), Stamps(n), Payloads(n)
    t = {"fanout_device_pay_patches_only": [], "fanout_device_pay_all_three_records": [],
         "fanout_device_ast_stamp_only": [], "fanout_device_rw_all_four_fields": [], "fanout_device": []}
    pick = slice(None, None, max(1, n // 64))
    for it in range(WARM + TIMED):
        for name, (rw, st, pp) in zip(t, ((None, None, py), (tg, sp, py), (None, sp, None), (tg, None, None),
                                          (None, None, None))):
            x = timed_fanout(eng, w, rw, st, pp)
            if st is not None:  # the stamp is in the clear; the patched bytes are payload and leave enciphered
                got = w["seg"].view(n, DST_STRIDE)[pick, STAMP_AT:STAMP_AT + 3].cpu().numpy()
                assert (got == sp.bytes3()[pick]).all()
            if it >= WARM:
                t[name].append(x)
    res = {k: pct(v) for k, v in t.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    spread = max(x["p90_ms"] - x["p10_ms"] for x in res.values())
    res.update({"n": n, "N": fan, "m": w["m"],
                "pay_minus_plain_ms": med["fanout_device_pay_patches_only"] - med["fanout_device"],
                "rw_minus_plain_ms": med["fanout_device_rw_all_four_fields"] - med["fanout_device"],
                "ast_minus_plain_ms": med["fanout_device_ast_stamp_only"] - med["fanout_device"],
                "pay_all_three_minus_plain_ms": med["fanout_device_pay_all_three_records"] - med["fanout_device"],
                "widest_p90_minus_p10_ms": spread, "record_bytes_read": 8 * n, "bytes_written": n * LEN})
    return res


def plain_device_case(eng, n, fan):
    w = device_setup(eng, n, fan)
    t = [timed_fanout(eng, w, None) for _ in range(WARM + TIMED)][WARM:]
    return {"n": n, "N": fan, "m": w["m"], "fanout_device": pct(t)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--rewrite", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--stamp", action="store_true")
    ap.add_argument("--payload", action="store_true")
    ap.add_argument("--stamp-records", choices=("on", "off", "miss"), default="on",
                    help="with --once --stamp: every record on (default), off, or on under the ID of no element")
    ap.add_argument("--log2n-host", type=int, default=16)
    ap.add_argument("--log2n-device", type=int, default=18)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.device or args.once or args.rewrite or args.plain or args.stamp or args.payload:
        import torch  # asked before the engine library initialises HIP: torch caches its first answer
        assert torch.cuda.is_available()
    eng = SRTPEngine(device=0, max_contexts=1 << 19, max_factories=256, max_transformers=256,
                     max_batch=1 << max(args.log2n_host, args.log2n_device))
    eng.enable_aead()
    res = {}
    if args.host:
        res["host"] = [host_case(eng, prof, 1 << args.log2n_host, fan)
                       for prof in ("AES_CM_128_HMAC_SHA1_80", "AEAD_AES_128_GCM") for fan in (1, 2, 4, 8, 16)]
    if args.once and args.payload:  # three fanout_device_pay calls and nothing else (a trace of k_fanout_pay)
        w = device_setup(eng, 1 << args.log2n_device, 8)
        w["src"].with_extension()
        py = Payloads(1 << args.log2n_device)
        res["device"] = {"once_pay_ms": [timed_fanout(eng, w, None, None, py) for _ in range(3)]}
    elif args.payload:
        res["payload_device"] = payload_device_case(eng, 1 << args.log2n_device, 8)
    elif args.once and args.stamp:  # three fanout_device_ast calls and nothing else (a trace of k_fanout_ast)
        w = device_setup(eng, 1 << args.log2n_device, 8)
        w["src"].with_extension()
        sp = Stamps(1 << args.log2n_device, args.stamp_records)
        res["device"] = {"once_ast_ms": [timed_fanout(eng, w, None, sp) for _ in range(3)]}
    elif args.stamp:
        res["stamp_device"] = stamp_device_case(eng, 1 << args.log2n_device, 8)
        res["stamp_host"] = [stamp_host_case(eng, 1 << args.log2n_host, fan) for fan in (1, 4, 16)]
    elif args.once and args.rewrite:  # three fanout_device_rw calls and nothing else (a trace of k_fanout_rw)
        w = device_setup(eng, 1 << args.log2n_device, 8)
        tg = Targets(w["src"], w["src_idx"], 8)
        res["device"] = {"once_rw_ms": [timed_fanout(eng, w, tg) for _ in range(3)]}
    elif args.device or args.once:
        res["device"] = device_case(eng, 1 << args.log2n_device, 8, args.once)
    elif args.rewrite:
        res["rewrite_device"] = rewrite_device_case(eng, 1 << args.log2n_device, 8)
        res["rewrite_host"] = [rewrite_host_case(eng, 1 << args.log2n_host, fan) for fan in (1, 4, 16)]
    if args.plain:
        res["plain_device"] = plain_device_case(eng, 1 << args.log2n_device, 8)
    res["fanout_stats"] = eng.fanout_stats()
    eng.close()
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
