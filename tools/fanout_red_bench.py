#!/usr/bin/env python3
"""What the RED step costs a device fan-out (srtp_fanout_device_red, k_fanout_red).

tools/fanout_bench.py's conventions: HIP events around the whole call (the
expansion and the protect chain) on a stream, 5 warm-up and 20 timed calls,
medians with p10-p90, the alternatives alternating call by call on one engine on
one box.  The workload: 2^18 destinations of 1200-byte sources, N = 16, sources
with a two-word BEDE extension (h = 24) whose first element is abs-send-time and
whose byte 24 is a single-block RED header; every destination has a rewrite
record (all four fields) and a stamp record.

  A   fanout_device_pay, rewrite + stamp records (k_fanout_ast: the yardstick,
      a kernel this change does not touch)
  A2  the same with an all-zero pay array (k_fanout_pay, likewise untouched)
  B   fanout_device_red, the same records, red records all off
  C   ... all strip
  D   ... all wrap

Reported: the medians, B/A, C/A, D/A (and against A2), and A's own spread.

  python tools/fanout_red_bench.py --out profiles/fanout_red/bench.json
  python tools/fanout_red_bench.py --once strip     three calls and nothing else (for a kernel trace)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fanout_bench import (DST_STRIDE, LEN, TIMED, WARM, PAY_DTYPE, SRTPEngine, Stamps, Targets, device_setup,  # noqa: E402
                          pct)

RED_DTYPE = np.dtype([("mode", "u1"), ("red_pt", "u1"), ("reserved", "u1", (2,))])  # srtp_fanout_red
H, RED_PT, BLOCK_PT = 24, 96, 100
EXT = bytes([0xBE, 0xDE, 0, 2, 0x32, 0xA0, 0xA1, 0xA2, 0x10, 0x77, 0, 0])  # abs-send-time (ID 3) first: stamped at 17


def call(eng, w, tg, sp, pay, red, ro):
    """One fan-out of fresh sources on the stream, between two HIP events: ms."""
    import torch
    w["src"].advance()
    s_seg = w["d"](w["src"].seg)
    tg.update()
    sp.update()
    rw = torch.from_numpy(tg.rw.view(np.uint8)).cuda()
    ast = torch.from_numpy(sp.ast.view(np.uint8)).cuda()
    py = None if pay is None else torch.from_numpy(pay.view(np.uint8)).cuda()
    rd = None if red is None else torch.from_numpy(red.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    args = (w["tids"], s_seg, w["s_off"], w["s_len"], w["s_cap"], w["idx"], w["seg"], w["off"], w["ln"], w["cap"], w["st"])
    with torch.cuda.stream(w["stream"]):
        a.record()
        if rd is None:
            eng.fanout_device_pay(*args, rw, ast, py, stream=w["stream"])
        else:
            eng.fanout_device_red(*args, rw, ast, py, rd, ro, stream=w["stream"])
        b.record()
    b.synchronize()
    eng.sync(w["stream"].cuda_stream)
    assert not w["st"].any().item()
    return a.elapsed_time(b)


def check(w, sp, n, mode, ro):
    """A sample of the copies: the stamp (in the clear), the lengths and the result codes."""
    pick = slice(None, None, max(1, n // 64))
    got = w["seg"].view(n, DST_STRIDE)[pick, 17:20].cpu().numpy()
    assert (got == sp.bytes3()[pick]).all()
    d = {0: 0, 1: -1, 2: 1}[mode]
    assert (w["ln"][pick].cpu().numpy() == LEN + d + 10).all()
    if mode:
        assert (ro[pick].cpu().numpy() == mode).all()


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--fan", type=int, default=16)
    ap.add_argument("--once", choices=("pay", "off", "strip", "wrap"))
    ap.add_argument("--out")
    args = ap.parse_args()
    n = 1 << args.log2n
    assert torch.cuda.is_available()  # asked before the engine library initialises HIP: torch caches its first answer
    eng = SRTPEngine(device=0, max_contexts=1 << 19, max_factories=256, max_transformers=256, max_batch=n)
    w = device_setup(eng, n, args.fan)
    w["src"].rows[:, 0] = 0x90
    w["src"].rows[:, 12:24] = np.frombuffer(EXT, np.uint8)
    w["src"].rows[:, H] = BLOCK_PT
    tg, sp = Targets(w["src"], w["src_idx"], args.fan), Stamps(n)
    ro = torch.zeros(n, dtype=torch.int8, device="cuda")
    reds = {}
    for name, mode in (("off", 0), ("strip", 1), ("wrap", 2)):
        reds[name] = np.zeros(n, RED_DTYPE)
        reds[name]["mode"], reds[name]["red_pt"] = mode, RED_PT
    runs = {"A_fanout_device_pay_rewrite_stamp": (None, None, 0),
            "A2_fanout_device_pay_all_zero_pay": (np.zeros(n, PAY_DTYPE), None, 0),
            "B_fanout_device_red_all_off": (None, reds["off"], 0),
            "C_fanout_device_red_all_strip": (None, reds["strip"], 1),
            "D_fanout_device_red_all_wrap": (None, reds["wrap"], 2)}
    if args.once:
        key = {"pay": "A2", "off": "B_", "strip": "C_", "wrap": "D_"}[args.once]
        pay, red, mode = next(v for k, v in runs.items() if k.startswith(key))
        for _ in range(3):
            call(eng, w, tg, sp, pay, red, ro)
            check(w, sp, n, mode, ro)
        print(json.dumps({"once": args.once, "n": n, "red_stats": eng.fanout_red_stats()}))
        return
    t = {k: [] for k in runs}
    for it in range(WARM + TIMED):
        for name, (pay, red, mode) in runs.items():
            x = call(eng, w, tg, sp, pay, red, ro)
            check(w, sp, n, mode, ro)
            if it >= WARM:
                t[name].append(x)
    res = {k: pct(v) for k, v in t.items()}
    A, A2 = res["A_fanout_device_pay_rewrite_stamp"], res["A2_fanout_device_pay_all_zero_pay"]
    out = {"n": n, "N": args.fan, "m": w["m"], "bytes_per_source": LEN, "h": H, "warm": WARM, "timed": TIMED, **res,
           "A_p90_minus_p10_ms": A["p90_ms"] - A["p10_ms"], "A_spread_over_median": (A["p90_ms"] - A["p10_ms"]) / A["median_ms"]}
    for k in ("B", "C", "D"):
        name = next(x for x in res if x.startswith(k + "_"))
        out[k + "_over_A"] = res[name]["median_ms"] / A["median_ms"]
        out[k + "_over_A2"] = res[name]["median_ms"] / A2["median_ms"]
    out["red_stats"] = eng.fanout_red_stats()
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
