#!/usr/bin/env python3
"""What recovering lost packets from ulpfec on the device costs
(srtp_fec_recover_device, k_fec_recover), and what it replaces.

The workload: n = 2^18 received entries over 4096 video SSRCs, 64 entries each:
twelve groups of four 1200-byte media packets and their FEC packet (1214
bytes), and four more media packets.  One record for every FEC packet (49152),
each with its SSRC's 64 entries as candidates (the records of an SSRC share
them).  5 % of the groups have lost one packet: its entry carries a status that
is not OK, as a packet that failed authentication does.  The tables are
plaintext, as an unprotect leaves them.

5 warm-up and 20 timed calls, medians with p10 - p90, the alternatives
alternating call by call on one engine, HIP events on one stream:
  recover   fec_recover_device over the whole table
  copy      a device-to-device copy of as many bytes as the kernel reads of the
            needed members and FEC packets and writes, in the same process
  host      what the feature replaces, for the same lost groups: the needed
            members and FEC packets gathered and copied to the host, the XOR in
            numpy, the recovered packets uploaded; wall clock, each step timed

Not measured here: transform_device(reverse) + fec_recover_device against
transform_device(reverse) alone (the pipeline needs a protected stream that
advances every call), and the kernel in a serial kernel trace of its own.
--once: three recover calls and nothing else (for such a trace).

  python tools/fec_recover_bench.py --out profiles/fec_recover/bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libjitsi_amd import SRTPEngine  # noqa: E402
from libjitsi_amd import _native as N  # noqa: E402

WARM, TIMED = 5, 20
LEN, FEC_LEN, STRIDE, PER = 1200, 1214, 1216, 64
GROUPS = 12


def pct(v):
    v = np.sort(np.asarray(v, float))
    return dict(median=round(float(np.median(v)), 4), p10=round(float(v[int(0.1 * (len(v) - 1))]), 4),
                p90=round(float(v[int(round(0.9 * (len(v) - 1)))]), 4))


def workload(n, seed=5109):
    rng = np.random.default_rng(seed)
    ssrcs = n // PER
    rows = rng.integers(0, 256, (ssrcs, PER, STRIDE), dtype=np.uint8)
    pos = np.arange(PER)
    is_fec = (pos % 5 == 4) & (pos < 5 * GROUPS)
    seq = (rng.integers(0, 60000, ssrcs)[:, None] + pos[None, :]).astype(np.uint16)  # no wrap: the quirk is not the workload
    rows[:, :, 0] = 0x80
    rows[:, :, 1] = np.where(is_fec, 116, 96)[None, :]
    rows[:, :, 2], rows[:, :, 3] = seq >> 8, seq & 0xFF
    ssrc = (0x50000000 + np.arange(ssrcs, dtype=np.uint32)).astype(">u4").view(np.uint8).reshape(ssrcs, 4)
    rows[:, :, 8:12] = ssrc[:, None, :]
    ln = np.where(is_fec, FEC_LEN, LEN).astype(np.uint32)
    for g in range(GROUPS):  # the FEC packet of group g: RFC 5109 over entries 5 g .. 5 g + 3
        m = rows[:, 5 * g:5 * g + 4]
        f = rows[:, 5 * g + 4]
        x = m[:, 0] ^ m[:, 1] ^ m[:, 2] ^ m[:, 3]
        f[:, 12:20] = x[:, 0:8]
        f[:, 12] &= 0xBF  # the short mask
        f[:, 14:16] = m[:, 0, 2:4]
        f[:, 20:22] = 0  # four equal lengths
        f[:, 22], f[:, 23] = (LEN - 12) >> 8, (LEN - 12) & 0xFF
        f[:, 24], f[:, 25] = 0xF0, 0
        f[:, 26:FEC_LEN] = x[:, 12:LEN]
    status = np.zeros((ssrcs, PER), np.int32)
    lost_group = rng.random((ssrcs, GROUPS)) < 0.05
    which = rng.integers(0, 4, (ssrcs, GROUPS))
    s_idx, g_idx = np.nonzero(lost_group)
    status[s_idx, 5 * g_idx + which[s_idx, g_idx]] = N.STATUS_DROP_AUTH
    rec = np.zeros(ssrcs * GROUPS, N.FEC_RECOVER_DTYPE)
    rec["fec"] = (np.arange(ssrcs)[:, None] * PER + 5 * np.arange(GROUPS)[None, :] + 4).reshape(-1)
    rec["first"] = np.repeat(np.arange(ssrcs) * PER, GROUPS)
    rec["ssrc"] = np.repeat(0x50000000 + np.arange(ssrcs, dtype=np.uint32), GROUPS)
    rec["count"], rec["on"] = PER, 1
    return dict(seg=rows.reshape(-1), off=(np.arange(n, dtype=np.uint64) * STRIDE).astype(np.uint32),
                len=np.tile(ln, ssrcs), cap=np.full(n, STRIDE, np.uint32), status=status.reshape(-1), rec=rec,
                cand=np.arange(n, dtype=np.int32), lost=lost_group.reshape(-1),
                lost_entry=(s_idx * PER + 5 * g_idx + which[s_idx, g_idx]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--out")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    w = workload(a.n)
    eng = SRTPEngine(device=0, max_contexts=4096, max_factories=16, max_transformers=16)
    d = lambda x: torch.from_numpy(x.view(np.uint8) if x.dtype.names else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()
    n_rec = len(w["rec"])
    seg, off, ln, cap, st = d(w["seg"]), d(w["off"]), d(w["len"]), d(w["cap"]), d(w["status"])
    rec, cand = d(w["rec"]), d(w["cand"])
    out_seg = torch.zeros(n_rec * STRIDE, dtype=torch.uint8, device="cuda")
    out_off = d((np.arange(n_rec, dtype=np.uint64) * STRIDE).astype(np.uint32))
    out_cap = d(np.full(n_rec, STRIDE, np.uint32))
    out_len = torch.zeros(n_rec, dtype=torch.int32, device="cuda")
    out_st = torch.zeros(n_rec, dtype=torch.int32, device="cuda")
    code = torch.zeros(n_rec, dtype=torch.int8, device="cuda")
    s = torch.cuda.Stream()
    recover = lambda: eng.fec_recover_device(seg, off, ln, cap, st, rec, cand, out_seg, out_off, out_cap, out_len,
                                             out_st, code, stream=s)
    recover()
    s.synchronize()
    # every result is checked once: the lost groups recover their packet, the others are complete
    c = code.cpu().numpy()
    assert (c[w["lost"]] == N.FECRX_RECOVERED).all() and (c[~w["lost"]] == N.FECRX_COMPLETE).all()
    got = out_seg.cpu().numpy().reshape(n_rec, STRIDE)[w["lost"]][:, :LEN]
    want = w["seg"].reshape(-1, STRIDE)[w["lost_entry"]][:, :LEN]
    assert np.array_equal(got, want) and (out_len.cpu().numpy()[w["lost"]] == LEN).all()
    lost = int(w["lost"].sum())
    if a.once:
        for _ in range(3):
            recover()
        s.synchronize()
        return
    moved = lost * (3 * LEN + FEC_LEN + LEN)  # read of the needed members and the FEC packet, written once
    src_c = torch.zeros(moved, dtype=torch.uint8, device="cuda")
    dst_c = torch.empty_like(src_c)
    # the host's way, for the same groups: the needed members and the FEC packets gathered first (on the device)
    lost_rec = np.nonzero(w["lost"])[0]
    fec_e = w["rec"]["fec"][lost_rec].astype(np.int64)
    members = fec_e[:, None] - 4 + np.arange(4)[None, :]
    members = members[members != w["lost_entry"][:, None]].reshape(lost, 3)
    gather = torch.from_numpy(np.concatenate((members, fec_e[:, None]), 1).reshape(-1)).cuda()
    table = seg.view(-1, STRIDE)
    host_pinned = torch.empty((lost * 4, STRIDE), dtype=torch.uint8).pin_memory()
    up_pinned = torch.empty((lost, STRIDE), dtype=torch.uint8).pin_memory()
    up_dev = torch.empty((lost, STRIDE), dtype=torch.uint8, device="cuda")
    t_rec, t_copy, t_down, t_xor, t_up = [], [], [], [], []
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for it in range(WARM + TIMED):
        e0, e1, e2 = ev(), ev(), ev()
        with torch.cuda.stream(s):
            e0.record(s)
            recover()
            e1.record(s)
            dst_c.copy_(src_c)
            e2.record(s)
        s.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            host_pinned.copy_(table.index_select(0, gather), non_blocking=True)
        s.synchronize()
        t1 = time.perf_counter()
        h = host_pinned.numpy().reshape(lost, 4, STRIDE)
        r = up_pinned.numpy()
        x = h[:, 0] ^ h[:, 1] ^ h[:, 2]
        r[:, 0:8] = x[:, 0:8] ^ h[:, 3, 12:20]
        r[:, 0] = (r[:, 0] & 0x3F) | 0x80
        r[:, 8:12] = h[:, 0, 8:12]
        r[:, 12:LEN] = x[:, 12:LEN] ^ h[:, 3, 26:FEC_LEN]
        t2 = time.perf_counter()
        with torch.cuda.stream(s):
            up_dev.copy_(up_pinned, non_blocking=True)
        s.synchronize()
        t3 = time.perf_counter()
        if it >= WARM:
            t_rec.append(e0.elapsed_time(e1))
            t_copy.append(e1.elapsed_time(e2))
            t_down.append(1e3 * (t1 - t0))
            t_xor.append(1e3 * (t2 - t1))
            t_up.append(1e3 * (t3 - t2))
    res = dict(n=a.n, records=n_rec, lost_groups=lost, candidates_per_record=PER, bytes_moved_by_the_copy=moved,
               recover_ms=pct(t_rec), copy_ms=pct(t_copy), ratio_copy_over_recover=round(float(np.median(t_copy) / np.median(t_rec)), 3),
               host_gather_and_download_ms=pct(t_down), host_xor_ms=pct(t_xor), host_upload_ms=pct(t_up),
               host_total_ms=pct(np.array(t_down) + np.array(t_xor) + np.array(t_up)),
               stats=eng.fec_recover_stats(), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
