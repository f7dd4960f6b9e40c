"""Fan-out with per-destination rewriting as seen without a GPU: the entry
points and the 16-byte record agree between the header, _native.py and the
built library; a NULL engine is refused before any device is touched;
srtp_fanout_rewrite_job (fanout_job.h, the text k_fanout_rw compiles) agrees,
over the sweep of tools/fanout_rewrite_check.cpp, with a few lines of Python
that restate the rule byte by byte; that tool builds and runs clean under
AddressSanitizer + UBSan; fan_out_rw of nothing is nothing."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_fanout_device_rw", "srtp_fanout_host_rw", "srtp_fanout_rewrite_job")
SKIP = N.PKT_FLAG_SKIP
FIELDS = ["mask", "ssrc", "timestamp", "seq", "pt", "reserved"]


def test_entry_points_and_record_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\} srtp_fanout_rewrite;", text).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint32_t mask, ssrc, timestamp; uint16_t seq; uint8_t pt, reserved;"
    assert [n for n, _ in N.FanoutRewrite._fields_] == FIELDS
    assert C.sizeof(N.FanoutRewrite) == 16
    assert [getattr(N.FanoutRewrite, n).offset for n in FIELDS] == [0, 4, 8, 12, 14, 15]
    dt = N.FANOUT_REWRITE_DTYPE
    assert dt.itemsize == 16 and list(dt.names) == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0, 4, 8, 12, 14, 15]
    for name, value in (("SSRC", 1), ("SEQ", 2), ("TIMESTAMP", 4), ("PT", 8)):
        assert re.search(r"#define SRTP_REWRITE_%s 0x%xu\b" % (name, value), header)
        assert getattr(N, "REWRITE_" + name) == value
    # rewrite follows flags in both entries
    for name in ENTRY[:2]:
        proto = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        args = [a.strip().split("*")[-1].split()[-1] for a in proto.split(",")]
        assert args[args.index("flags") + 1] == "rewrite" and args[args.index("rewrite") + 1] == "status"
    assert int(re.search(r"#define SRTP_MI355X_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION
    # the fan-out stats did not grow
    assert C.sizeof(N.FanoutStats) == 40


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    rw = (N.FanoutRewrite * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_fanout_device_rw(None, p(buf), p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), p(w), p(w), p(w),
                                   None, p(rw), p(i), n, None) == -1
    assert L.srtp_fanout_host_rw(None, p(buf), 64, p(w), p(w), p(w), None, 1, p(i), None, 0, p(buf), 64, p(w), p(w),
                                 p(w), None, p(rw), p(i), n) == -1
    assert L.srtp_fanout_rewrite_job(0, 1, 12, 16, 0, 16, 0, rw, w, None) == -1
    assert L.srtp_fanout_rewrite_job(0, 1, 12, 16, 0, 16, 0, None, w, C.byref(N.FanoutRewritePlan())) == -1


def test_python_mirrors():
    from libjitsi_amd import SRTPEngine, fan_out_rw
    import libjitsi_amd.srtp as S
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.fanout_device_rw) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                                "seg", "off", "length", "cap", "status", "rewrite", "src_status",
                                                "flags", "m", "n", "stream"]
    assert sig(SRTPEngine.fanout_host_rw) == ["self", "tid", "src_seg", "src_off", "src_len", "src_cap", "src_idx",
                                              "seg", "off", "cap", "src_status", "flags", "rewrite"]
    assert sig(fan_out_rw) == ["pkts", "transformers", "rewriters", "exclusion"]
    assert "ExtendedSequenceNumberInterval.java:163-229" in S.fan_out_rw.__doc__
    assert "MediaStreamImpl.java:986-1035" in S.fan_out_rw.__doc__
    assert fan_out_rw([], [], []) == []
    assert fan_out_rw([None], [], []) == []
    with pytest.raises(ValueError):
        fan_out_rw([], [], [None])


def setters(b, mask, ssrc, ts, seq, pt):
    """RawPacket.setPayloadType / setSequenceNumber / setTimestamp / setSSRC on header bytes b."""
    b = bytearray(b)
    if mask & 8:
        b[1] = (b[1] & 0x80) | (pt & 0x7F)
    if mask & 2:
        b[2:4] = seq.to_bytes(2, "big")
    if mask & 4:
        b[4:8] = ts.to_bytes(4, "big")
    if mask & 1:
        b[8:12] = ssrc.to_bytes(4, "big")
    return bytes(b)


def rule(idx, m, L, sc, st, dc, fl, mask):
    """fanout_rewrite_applies restated."""
    if idx < 0 or idx >= m or st != 0 or fl & SKIP or not mask & 0xF:
        return False
    return min(L, sc, dc) >= 12


VALUES = ((0x11223344, 0x55667788, 0x99AA, 0xBB, 0xCC), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF, 0xFF, 0xFF), (0, 0, 0, 0, 0))


def sweep():
    lens = list(range(33)) + [1200 + d for d in range(-17, 18)]
    caps = sorted({c + d for c in (0, 16, 32, 1200, 1216) for d in (-17, -16, -5, -4, -1, 0, 1, 16) if c + d >= 0}
                  | set(range(8, 14)))
    for L in lens:
        for sc in caps:
            for dc in (sc - 5, sc - 1, sc, sc + 1, 11, 12, 1216):
                if dc >= 0:
                    for mask in range(16):
                        yield 0, 1, L, sc, 0, dc, 0, mask, VALUES[(L + mask) % 3]
    for L in (0, 11, 12, 16, 1200, -1, 65536, 2 ** 31 - 1):
        for c in (0, 11, 12, 16, 1216, -1, 2 ** 31 - 1):
            for mask in (0, 0xF, 0x10, 0x1F, 0xFFFFFFF0, 0xFFFFFFFF, 0x80000001):
                for fl in (0, 2, SKIP, SKIP | 4):
                    for idx, m, st in ((0, 1, 0), (0, 1, 2), (1, 1, 0), (-1, 3, 0)):
                        yield idx, m, L, c, st, c, fl, mask, VALUES[0]


def test_rewrite_job_agrees_with_the_rule():
    job = N.lib().srtp_fanout_rewrite_job
    out, rec = N.FanoutRewritePlan(), N.FanoutRewrite()
    words = (C.c_uint32 * 3)()
    hdr = bytes([0x80, 0xE0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
    cases = applied = 0
    for idx, m, L, sc, st, dc, fl, mask, (ssrc, ts, seq, pt, res) in sweep():
        h = hdr if (L + mask) & 1 else bytes([0x90, 0x60]) + hdr[2:]
        words[:] = [int.from_bytes(h[k:k + 4], "little") for k in (0, 4, 8)]
        rec.mask, rec.ssrc, rec.timestamp, rec.seq, rec.pt, rec.reserved = mask, ssrc, ts, seq, pt, res
        assert job(idx, m, L, sc, st, dc, fl, C.byref(rec), words, C.byref(out)) == 0
        want = rule(idx, m, L, sc, st, dc, fl, mask)
        case = (idx, m, L, sc, st, dc, fl, mask)
        assert out.applies == int(want), case
        got = b"".join(int(w).to_bytes(4, "little") for w in out.words)
        assert got == (setters(h, mask, ssrc, ts, seq, pt) if want else h), case
        cases += 1
        applied += want
    assert cases > 100000 and applied > 10000


def test_fanout_rewrite_check_builds_and_runs_clean(tmp_path):
    """tools/fanout_rewrite_check (the Makefile's recipe, built out of tree):
    the copy replayed 16 bytes at a time with the first piece patched, between
    exact-size heap buffers, against the four setters; a program of its own
    under AddressSanitizer + UBSan."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^fanout_rewrite_check: fanout_rewrite_check\.cpp .*fanout_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fanout_rewrite_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fanout_rewrite_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"fanout_rewrite_check: \d+ cases, \d+ copies replayed, [1-9]\d* patched, 0 failures", r.stdout)


def test_record_dtype_round_trips():
    """A numpy record and the ctypes struct are the same 16 bytes."""
    a = np.zeros(1, N.FANOUT_REWRITE_DTYPE)
    a["mask"], a["ssrc"], a["timestamp"], a["seq"], a["pt"] = 0xF, 0x11223344, 0x55667788, 0x99AA, 0x3B
    r = N.FanoutRewrite.from_buffer_copy(a.tobytes())
    assert (r.mask, r.ssrc, r.timestamp, r.seq, r.pt, r.reserved) == (0xF, 0x11223344, 0x55667788, 0x99AA, 0x3B, 0)
