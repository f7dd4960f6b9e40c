#!/usr/bin/env python3
"""What making the ulpfec packets on the device costs a fan-out
(srtp_fanout_device_fec / _host_fec, k_fanout_fec), and what it saves.

tools/fanout_bench.py's conventions: HIP events around the whole call (the
expansion, the FEC pass and the protect chain) on a stream, 5 warm-up and 20
timed calls, medians with p10-p90, the alternatives alternating call by call on
one engine on one box.  The workload: n media entries of 1200-byte sources, N =
16 peers, every entry with a rewrite record (all four fields), and one FEC entry
per peer after every 4 sources (rate 4): n / 4 FEC entries of 1214 bytes.

Device route (n = 2^18):
  A   fanout_device_red over the n media entries (the call as it was)
  B   fanout_device_fec over the n media entries and n / 4 FEC entries
  C   what a caller does today: the n / 4 FEC packets made on the host, outside
      the timing, and fanned out by fanout_device_red as n / 4 extra sources
      toward one peer each
Host route (--host, n = 2^16): B against C with C's host XOR (numpy, over the
rewritten copies of every peer) inside the timing, and C's upload of the FEC
packets with it: the comparison the feature exists for.

B - A, the FEC pass and the protection of its packets, is also set against a
device-to-device copy of the member bytes the pass reads, in the same process.
--once fec: three B calls and nothing else (for a kernel trace).

  python tools/fanout_fec_bench.py --out profiles/fanout_fec/bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fanout_bench import (DST_CAP, DST_STRIDE, LEN, SRC_STRIDE, TIMED, WARM, HostBuffer, SRTPEngine, Sources,  # noqa: E402
                          Targets, device_setup, peers, pct)

FEC_DTYPE = np.dtype([("first", "<u4"), ("ssrc", "<u4"), ("count", "u1"), ("pt", "u1"), ("red_pt", "u1"),
                      ("mode", "u1")])  # srtp_fanout_fec
RATE, FEC_PT = 4, 116
FEC_LEN = LEN + 14
FEC_CAP = FEC_LEN + 20
FEC_STRIDE = (FEC_CAP + 15) & ~15


class Layout:
    """n media entries, source-major, then one FEC entry per (group of RATE sources, peer)."""

    def __init__(self, n, fan):
        self.n, self.fan, self.m = n, fan, n // fan
        self.groups = self.m // RATE
        self.g = self.groups * fan
        grp, peer = np.divmod(np.arange(self.g, dtype=np.int64), fan)
        self.grp, self.peer = grp, peer
        # entry (RATE * grp + r) * fan + peer, r = 0 .. RATE - 1
        self.members = (((RATE * grp)[:, None] + np.arange(RATE)[None, :]) * fan + peer[:, None]).astype(np.int32)
        self.fec = np.zeros(n + self.g, FEC_DTYPE)
        self.fec["first"][n:] = np.arange(self.g) * RATE
        self.fec["ssrc"][n:] = 0x40000000 + grp * 64 + peer
        self.fec["count"][n:], self.fec["pt"][n:], self.fec["mode"][n:] = RATE, FEC_PT, 1
        self.off = np.concatenate((np.arange(n, dtype=np.int64) * DST_STRIDE,
                                   n * DST_STRIDE + np.arange(self.g, dtype=np.int64) * FEC_STRIDE)).astype(np.uint32)
        self.cap = np.concatenate((np.full(n, DST_CAP, np.uint32), np.full(self.g, FEC_CAP, np.uint32)))
        self.seg_bytes = n * DST_STRIDE + self.g * FEC_STRIDE

    def host_fec(self, src, tg):
        """FECSender.FECPacket over every group's rewritten copies, vectorised: g rows of FEC_LEN bytes."""
        rows = np.zeros((self.g, FEC_LEN), np.uint8)
        mem = self.members  # g x RATE entry indices
        head = np.zeros((self.g, RATE, 12), np.uint8)
        head[:, :, 0] = 0x80
        head[:, :, 1] = tg.rw["pt"][mem] & 0x7F
        head[:, :, 2:4] = tg.rw["seq"][mem].astype(">u2").view(np.uint8).reshape(self.g, RATE, 2)
        head[:, :, 4:8] = tg.rw["timestamp"][mem].astype(">u4").view(np.uint8).reshape(self.g, RATE, 4)
        x = head[:, 0]
        for r in range(1, RATE):
            x = x ^ head[:, r]
        rows[:, 12:20] = x[:, :8]
        rows[:, 14:16] = head[:, 0, 2:4]
        rows[:, 0], rows[:, 1] = 0x80, FEC_PT
        seq = (tg.rw["seq"][mem[:, -1]].astype(np.uint32) + 1) & 0xFFFF
        rows[:, 2:4] = seq.astype(">u2").view(np.uint8).reshape(-1, 2)
        rows[:, 4:8] = head[:, -1, 4:8]
        rows[:, 8:12] = self.fec["ssrc"][self.n:].astype(">u4").view(np.uint8).reshape(-1, 4)
        rows[:, 20:22] = 0  # RATE equal lengths XOR to zero
        rows[:, 22:24] = np.array([(LEN - 12) >> 8, (LEN - 12) & 0xFF], np.uint8)
        rows[:, 24:26] = np.array([0xF0, 0x00], np.uint8)
        pay = src.rows[:, 12:LEN].reshape(self.groups, RATE, LEN - 12)
        xp = pay[:, 0] ^ pay[:, 1] ^ pay[:, 2] ^ pay[:, 3]
        rows[:, 26:] = xp[self.grp]  # the payload does not depend on the peer: the rewrite touches the header
        return rows


def device(eng, n, fan, once):
    import torch
    w = device_setup(eng, n, fan)
    lay = Layout(n, fan)
    tg = Targets(w["src"], w["src_idx"], fan)
    d = w["d"]
    g, m = lay.g, lay.m
    tids_all = torch.cat((w["tids"], w["tids"][:fan].repeat(lay.groups)))
    off, cap = d(lay.off), d(lay.cap)
    seg = torch.zeros(lay.seg_bytes, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n + g, dtype=torch.int32, device="cuda")
    st = torch.zeros(n + g, dtype=torch.int32, device="cuda")
    fo = torch.zeros(n + g, dtype=torch.int8, device="cuda")
    idx_b = d(np.concatenate((w["src_idx"], np.full(g, -1, np.int32))))
    idx_c = d(np.concatenate((w["src_idx"], m + np.arange(g, dtype=np.int32))))
    fec, members = torch.from_numpy(lay.fec.view(np.uint8)).cuda(), d(lay.members.reshape(-1))
    s_off_c = d(np.concatenate((w["src"].off, m * SRC_STRIDE + np.arange(g, dtype=np.int64) * FEC_STRIDE)).astype(np.uint32))
    s_len_c = d(np.concatenate((w["src"].len, np.full(g, FEC_LEN, np.uint32))))
    s_cap_c = d(np.concatenate((w["src"].cap, np.full(g, FEC_STRIDE, np.uint32))))
    rw_all = np.zeros(n + g, tg.rw.dtype)
    stream = w["stream"]

    def call(kind):
        w["src"].advance()
        tg.update()
        rw_all[:n] = tg.rw
        rw = torch.from_numpy(rw_all.view(np.uint8)).cuda()
        if kind == "C":
            rows = np.zeros((g, FEC_STRIDE), np.uint8)
            rows[:, :FEC_LEN] = lay.host_fec(w["src"], tg)
            s_seg = d(np.concatenate((w["src"].seg[:m * SRC_STRIDE], rows.reshape(-1))))
        else:
            s_seg = d(w["src"].seg)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            if kind == "A":
                eng.fanout_device_red(w["tids"], s_seg, w["s_off"], w["s_len"], w["s_cap"], w["idx"], seg, off, ln, cap, st,
                                      rw, None, None, None, None, n=n, stream=stream)
            elif kind == "B":
                eng.fanout_device_fec(tids_all, s_seg, w["s_off"], w["s_len"], w["s_cap"], idx_b, seg, off, ln, cap, st, rw,
                                      None, None, None, None, fec, members, fo, stream=stream)
            else:
                eng.fanout_device_red(tids_all, s_seg, s_off_c, s_len_c, s_cap_c, idx_c, seg, off, ln, cap, st, rw, None,
                                      None, None, None, stream=stream)
            b.record()
        b.synchronize()
        eng.sync(stream.cuda_stream)
        k = n if kind == "A" else n + g
        assert not st[:k].any().item()
        if kind == "B":
            assert (fo[n:] == 1).all().item() and (ln[n:] == FEC_LEN + 10).all().item()
        return a.elapsed_time(b)

    if once:
        for _ in range(3):
            call("B")
        print(json.dumps({"once": once, "n": n, "fec_stats": eng.fanout_fec_stats()}))
        return None
    t = {"A": [], "B": [], "C": []}
    for it in range(WARM + TIMED):
        for kind in t:
            x = call(kind)
            if it >= WARM:
                t[kind].append(x)
    res = {"A_fanout_device_red_media_only": pct(t["A"]), "B_fanout_device_fec": pct(t["B"]),
           "C_fanout_device_red_host_made_fec_as_sources": pct(t["C"])}
    A, B, C = (res[k]["median_ms"] for k in res)
    # the bytes k_fanout_fec reads, as one device-to-device copy in the same process
    src_buf = torch.zeros(int(lay.g) * RATE * LEN, dtype=torch.uint8, device="cuda")
    dst_buf = torch.zeros(int(lay.g) * RATE * LEN, dtype=torch.uint8, device="cuda")
    tc = []
    for it in range(WARM + TIMED):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst_buf.copy_(src_buf)
        b.record()
        b.synchronize()
        if it >= WARM:
            tc.append(a.elapsed_time(b))
    copy = pct(tc)
    return {"n": n, "N": fan, "m": m, "rate": RATE, "fec_entries": int(g), "bytes_per_source": LEN, "fec_bytes": FEC_LEN,
            "warm": WARM, "timed": TIMED, **res, "B_minus_A_ms": B - A, "C_minus_A_ms": C - A, "B_over_A": B / A,
            "B_over_C": B / C, "A_p90_minus_p10_ms": res["A_fanout_device_red_media_only"]["p90_ms"]
            - res["A_fanout_device_red_media_only"]["p10_ms"], "member_bytes_read_per_call": int(lay.g) * RATE * LEN,
            "packet_bytes_written_per_call": int(lay.g) * FEC_LEN, "device_copy_of_the_member_bytes": copy,
            "B_minus_A_over_copy": (B - A) / copy["median_ms"], "fec_stats": eng.fanout_fec_stats()}


def host(eng, n, fan):
    """Host route: B, fanout_host_fec, against C, the host XOR (timed) and fanout_host_red with the FEC packets
    as extra sources."""
    lay = Layout(n, fan)
    m, g = lay.m, lay.g
    ts = peers(eng, "AES_CM_128_HMAC_SHA1_80", fan)
    hs = HostBuffer(m * SRC_STRIDE + g * FEC_STRIDE)
    hd = HostBuffer(lay.seg_bytes)
    src = Sources(m, hs.array)
    src_idx = np.repeat(np.arange(m, dtype=np.int32), fan)
    tg = Targets(src, src_idx, fan)
    tids = np.concatenate((np.tile(np.array([t.tid for t in ts], np.int32), m),
                           np.tile(np.array([t.tid for t in ts], np.int32), lay.groups)))
    idx_b = np.concatenate((src_idx, np.full(g, -1, np.int32)))
    idx_c = np.concatenate((src_idx, m + np.arange(g, dtype=np.int32)))
    s_off_c = np.concatenate((src.off, m * SRC_STRIDE + np.arange(g, dtype=np.int64) * FEC_STRIDE)).astype(np.uint32)
    s_len_c = np.concatenate((src.len, np.full(g, FEC_LEN, np.uint32)))
    s_cap_c = np.concatenate((src.cap, np.full(g, FEC_STRIDE, np.uint32)))
    rw_all = np.zeros(n + g, tg.rw.dtype)
    fec_rows = hs.array[m * SRC_STRIDE:].reshape(g, FEC_STRIDE)
    media_seg = hs.array[:m * SRC_STRIDE]
    t_b, t_c, t_xor = [], [], []
    for it in range(WARM + TIMED):
        src.advance()
        tg.update()
        rw_all[:n] = tg.rw
        t0 = time.perf_counter()
        ln, st, _, fo = eng.fanout_host_fec(tids, media_seg, src.off, src.len, src.cap, idx_b, hd.array, lay.off, lay.cap,
                                            rewrite=rw_all, fec=lay.fec, members=lay.members.reshape(-1))
        t1 = time.perf_counter()
        assert not st.any() and (fo[n:] == 1).all() and (ln[n:] == FEC_LEN + 10).all()
        src.advance()
        tg.update()
        rw_all[:n] = tg.rw
        t2 = time.perf_counter()
        fec_rows[:, :FEC_LEN] = lay.host_fec(src, tg)
        t3 = time.perf_counter()
        ln, st, _ = eng.fanout_host_red(tids, hs.array, s_off_c, s_len_c, s_cap_c, idx_c, hd.array, lay.off, lay.cap,
                                        rewrite=rw_all)
        t4 = time.perf_counter()
        assert not st.any()
        if it >= WARM:
            t_b.append((t1 - t0) * 1e3)
            t_c.append((t4 - t2) * 1e3)
            t_xor.append((t3 - t2) * 1e3)
    for t in ts:
        t.close()
    hs.close()
    hd.close()
    b, c = pct(t_b), pct(t_c)
    return {"n": n, "N": fan, "m": m, "rate": RATE, "fec_entries": int(g), "B_fanout_host_fec": b,
            "C_host_xor_plus_fanout_host_red": c, "C_host_xor_alone": pct(t_xor), "B_over_C": b["median_ms"] / c["median_ms"],
            "h2d_bytes_B": m * SRC_STRIDE + 12 * (n + g) + 4 * RATE * g, "h2d_bytes_C": m * SRC_STRIDE + g * FEC_STRIDE}


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--host-log2n", type=int, default=16)
    ap.add_argument("--fan", type=int, default=16)
    ap.add_argument("--once", choices=("fec",))
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available()  # asked before the engine library initialises HIP: torch caches its first answer
    n = 1 << args.log2n
    eng = SRTPEngine(device=0, max_contexts=1 << 20, max_factories=256, max_transformers=256, max_batch=n + n // RATE)
    if args.once:
        device(eng, n, args.fan, args.once)
        return
    out = {"device": device(eng, n, args.fan, None)}
    eng2 = SRTPEngine(device=0, max_contexts=1 << 20, max_factories=256, max_transformers=256,
                      max_batch=(1 << args.host_log2n) * 5 // 4)
    out["host"] = host(eng2, 1 << args.host_log2n, args.fan)
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
