#!/usr/bin/env python3
"""Receive with the audio level read on the device against the call it wraps.

n = 2^18 audio-shaped RTP packets over 4096 SSRCs: 172 bytes, no CSRC, X set, a
one-byte-header (BEDE) extension of two words whose second element is the
ssrc-audio-level (ID 1); every eighth packet carries level 127 (a muted
source).  Every call receives a bundle protected on the device just before
(not timed) under new sequence numbers, so that no packet is a replay.

  --ab      transform_device_lvl (ext_id 1) against transform_device(reverse)
            given a flags array made outside the timing, each on a receiver of
            its own, alternating call by call on one engine: 5 warm-up and 20
            timed calls each, HIP events, medians with p10 / p90.
  --once    three transform_device_lvl calls and nothing else timed (for a
            kernel trace in a run of its own: k_audio_level beside k_parse).
  --plain   transform_device(reverse) alone, 5 warm-up and 20 timed calls (one
            side of a comparison between two builds of the library, a process
            each; uses nothing the parent's library lacks).

One JSON document on stdout, or in --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libjitsi_amd import SRTPContextFactory, SRTPEngine, SRTPTransformer, profile_policies  # noqa: E402

LEN, TAG, STRIDE = 172, 10, 192
SSRCS = 4096
WARM, TIMED = 5, 20
PROFILE = "AES_CM_128_HMAC_SHA1_80"
SILENCE = 0x4


class Audio:
    """The plaintext bundle on the host; advance() gives every packet a new sequence number."""

    def __init__(self, n):
        self.n = n
        rng = np.random.default_rng(17)
        self.rows = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
        self.rows[:, 0], self.rows[:, 1] = 0x90, 111
        self.rows[:, 8:12] = (0x20000 + np.arange(n) % SSRCS).astype(">u4").view(np.uint8).reshape(n, 4)
        self.level = np.where(np.arange(n) % 8 == 0, 127, np.arange(n) % 127).astype(np.uint8)
        # BEDE, two words: ID 3 with three bytes (abs-send-time), ID 1 with one byte (the level), two padding bytes
        self.rows[:, 12:20] = np.frombuffer(bytes([0xBE, 0xDE, 0, 2, 0x32, 0xA0, 0xA1, 0xA2]), np.uint8)
        self.rows[:, 20], self.rows[:, 21], self.rows[:, 22:24] = 0x10, self.level, 0
        self.per_call = (n + SSRCS - 1) // SSRCS
        self.base = 1
        self.off = (np.arange(n, dtype=np.int64) * STRIDE).astype(np.uint32)
        self.cap = np.full(n, STRIDE, np.uint32)
        self.flags = np.where(self.level == 127, SILENCE, 0).astype(np.uint32)  # what a host parse would hand over

    def advance(self):
        seq = ((self.base + np.arange(self.n) // SSRCS) & 0xFFFF).astype(">u2")
        self.rows[:, 2:4] = seq.view(np.uint8).reshape(self.n, 2)
        self.base += self.per_call


def pct(xs):
    xs = np.sort(np.array(xs))
    return {"median_ms": float(np.median(xs)), "p10_ms": float(np.percentile(xs, 10)),
            "p90_ms": float(np.percentile(xs, 90))}


class Bench:
    def __init__(self, eng, n, receivers):
        import torch
        self.torch, self.eng, self.n = torch, eng, n
        rng = np.random.default_rng(23)
        mk, ms = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
        pol = profile_policies(PROFILE)
        self.snd = SRTPTransformer(SRTPContextFactory(True, mk, ms, *pol, engine=eng))
        self.rcv = [SRTPTransformer(SRTPContextFactory(False, mk, ms, *pol, engine=eng)) for _ in range(receivers)]
        self.audio = Audio(n)
        d = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        self.d = d
        self.off, self.cap, self.flags = d(self.audio.off), d(self.audio.cap), d(self.audio.flags)
        self.ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.st = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.level = torch.zeros(n, dtype=torch.int8, device="cuda")
        self.stream = torch.cuda.Stream()

    def protected(self):
        """A new bundle as the network delivers it (not timed)."""
        self.audio.advance()
        seg = self.d(self.audio.rows.reshape(-1))
        self.ln.fill_(LEN)
        self.eng.transform_device(False, self.snd.tid, seg, self.off, self.ln, self.cap, self.st, stream=self.stream)
        self.eng.sync(self.stream.cuda_stream)
        assert not self.st.any().item() and (self.ln == LEN + TAG).all().item()
        return seg

    def timed(self, seg, rcv, lvl):
        torch = self.torch
        seg = seg.clone()
        self.ln.fill_(LEN + TAG)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            a.record()
            if lvl:
                self.eng.transform_device_lvl(rcv.tid, seg, self.off, self.ln, self.cap, self.st, self.level,
                                              ext_id=1, stream=self.stream)
            else:
                self.eng.transform_device(True, rcv.tid, seg, self.off, self.ln, self.cap, self.st, self.flags,
                                          stream=self.stream)
            b.record()
        b.synchronize()
        self.eng.sync(self.stream.cuda_stream)
        assert not self.st.any().item() and (self.ln == LEN).all().item()
        if lvl:
            assert (self.level.cpu().numpy().view(np.uint8) == self.audio.level).all()
        # a muted packet's payload is left as it came; every other packet is the sender's plaintext
        rows = seg.view(self.n, STRIDE)[:: max(1, self.n // 256), :LEN].cpu().numpy()
        want = self.audio.rows[:: max(1, self.n // 256), :LEN]
        muted = self.audio.level[:: max(1, self.n // 256)] == 127
        assert (rows[~muted] == want[~muted]).all() and (rows[muted, :24] == want[muted, :24]).all()
        assert (rows[muted, 24:] != want[muted, 24:]).any()
        return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch  # asked before the engine library initialises HIP: torch caches its first answer
    assert torch.cuda.is_available()
    n = 1 << args.log2n
    eng = SRTPEngine(device=0, max_contexts=1 << 16, max_factories=16, max_transformers=16, max_batch=n)
    res = {"n": n, "packet_bytes": LEN, "muted_fraction": 1 / 8}
    if args.ab:
        b = Bench(eng, n, 2)
        t_lvl, t_plain = [], []
        for it in range(WARM + TIMED):
            seg = b.protected()
            x = b.timed(seg, b.rcv[0], True)
            y = b.timed(seg, b.rcv[1], False)
            if it >= WARM:
                t_lvl.append(x)
                t_plain.append(y)
        pa, pb = pct(t_lvl), pct(t_plain)
        spread = max(pa["p90_ms"] - pa["p10_ms"], pb["p90_ms"] - pb["p10_ms"])
        res.update({"transform_device_lvl": pa, "transform_device_with_host_made_flags": pb,
                    "difference_of_medians_ms": pa["median_ms"] - pb["median_ms"], "wider_p90_minus_p10_ms": spread,
                    "differ_by_more_than_the_spread": abs(pa["median_ms"] - pb["median_ms"]) > spread,
                    "audio_level_stats": eng.audio_level_stats()})
    elif args.once:
        b = Bench(eng, n, 1)
        res["once_lvl_ms"] = [b.timed(b.protected(), b.rcv[0], True) for _ in range(3)]
    elif args.plain:
        b = Bench(eng, n, 1)
        res["transform_device_reverse"] = pct([b.timed(b.protected(), b.rcv[0], False)
                                               for _ in range(WARM + TIMED)][WARM:])
    eng.close()
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
