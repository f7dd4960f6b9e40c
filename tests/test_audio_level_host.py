"""The ssrc-audio-level stage as seen without a GPU: the entry points and the
stats struct agree between the header, _native.py and the built library; a NULL
engine is refused before any device is touched; audio_level_ref -- the Java
methods restated -- gives the answers worked out by hand from RawPacket.java;
srtp_audio_level_job (audio_level_job.h, the text k_audio_level compiles) agrees
with it over the shapes tests/test_audio_level.py runs on the device, cut at
every length, under every ID, and over seeded random headers;
tools/audio_level_check builds and runs clean under AddressSanitizer + UBSan."""
import ctypes as C
import inspect
import os
import random
import re
import shutil
import subprocess

import pytest

import audio_level_ref as R
from libjitsi_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("srtp_transform_device_lvl", "srtp_transform_host_lvl", "srtp_engine_audio_level_stats",
         "srtp_audio_level_job")
SKIP, SILENCE, DISCARD = N.PKT_FLAG_SKIP, N.PKT_FLAG_SILENCE, N.PKT_FLAG_DISCARD


def test_entry_points_and_struct_agree():
    with open(N.HEADER_PATH) as fh:
        header = fh.read()
    lib = C.CDLL(N.LIB_PATH)
    for name in ENTRY:
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"int {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\} srtp_audio_level_stats;", text).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint64_t calls, entries_read, levels_found, silent;"
    assert [n for n, _ in N.AudioLevelStats._fields_] == ["calls", "entries_read", "levels_found", "silent"]
    assert C.sizeof(N.AudioLevelStats) == 32
    for name in ENTRY[:2]:  # ext_ids, ext_id, level follow flags; status follows level
        proto = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        args = [a.strip().split("*")[-1].split()[-1] for a in proto.split(",")]
        i = args.index("flags")
        assert args[i + 1:i + 5] == ["ext_ids", "ext_id", "level", "status"]
        assert "reverse" not in args
    assert "audio_level_job.h" in N.KERNEL_SOURCES
    assert (N.AUDIO_LEVEL_NONE, N.AUDIO_LEVEL_MUTED) == (R.NONE, R.MUTED) == (-128, 127)
    # srtp_stats and the fan-out stats stay as they are
    assert C.sizeof(N.FanoutStats) == 40 and C.sizeof(N.Stats) == 8 * (2 + N.NUM_STATUS + 12)
    assert int(re.search(r"#define SRTP_MI355X_ABI_VERSION (\d+)", header).group(1)) == N.ABI_VERSION


@pytest.mark.parametrize("n", [0, 1])
def test_null_engine_is_einval(n):
    """Before any device call: this runs where there is no device."""
    L = N.lib()
    buf = (C.c_uint8 * 64)()
    w = (C.c_uint32 * 4)()
    i = (C.c_int32 * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert L.srtp_transform_device_lvl(None, None, 0, p(buf), p(w), p(w), p(w), None, None, 1, p(buf), p(i), n,
                                       None) == -1
    assert L.srtp_transform_host_lvl(None, None, 0, p(buf), 64, p(w), p(w), p(w), None, None, 1, p(buf), p(i),
                                     n) == -1
    assert L.srtp_engine_audio_level_stats(None, C.byref(N.AudioLevelStats())) == -1
    lv, fo = C.c_int8(5), C.c_uint32(6)
    assert L.srtp_audio_level_job(p(buf), 20, 20, 0, 1, None, C.byref(fo)) == -1
    assert L.srtp_audio_level_job(p(buf), 20, 20, 0, 1, C.byref(lv), None) == -1
    assert L.srtp_audio_level_job(None, 20, 20, 0, 1, C.byref(lv), C.byref(fo)) == -1  # read, but no bytes
    assert (lv.value, fo.value) == (5, 6)
    assert L.srtp_audio_level_job(None, 20, 20, 0, 0, C.byref(lv), C.byref(fo)) == 0  # ID 0: no byte is read
    assert (lv.value, fo.value) == (-128, 0)


def test_python_mirrors():
    from libjitsi_amd import SRTPEngine, reverse_transform_levels
    import libjitsi_amd.srtp as S
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SRTPEngine.transform_device_lvl) == ["self", "tid", "seg", "off", "length", "cap", "status", "level",
                                                    "flags", "ext_ids", "ext_id", "n", "stream"]
    assert sig(SRTPEngine.transform_host_lvl) == ["self", "tid", "seg", "off", "length", "cap", "flags", "ext_ids",
                                                  "ext_id"]
    assert sig(reverse_transform_levels) == ["pkts", "transformer", "ext_id"]
    assert callable(SRTPEngine.audio_level_stats)
    for f in (SRTPEngine.transform_device_lvl, SRTPEngine.transform_host_lvl, reverse_transform_levels):
        assert "SsrcTransformEngine.java:226-274" in f.__doc__
    assert "before authentication" in " ".join(reverse_transform_levels.__doc__.split())
    assert reverse_transform_levels([], None, 1) == []
    assert S.audio_level_job(bytes([0x90]) + bytes(11) + b"\xBE\xDE\x00\x01\x10\x7F\x00\x00", 20, 20, 0, 1) == (127, 4)


def test_reference_restates_the_java_by_hand():
    """Vectors worked out by hand from RawPacket.java:305-318, 331-394, 419-443, 504-556, 640-648."""
    def pkt(tail, b0=0x90):
        return bytearray(bytes([b0]) + bytes(11) + bytes(tail))
    rt = lambda p, i, fl=0, cap=None: R.reverse_transform(p, len(p), len(p) if cap is None else cap, fl, i)
    bede = [0xBE, 0xDE, 0x00, 0x01]
    assert rt(pkt(bede + [0x10, 0xFF, 0, 0]), 1) == (127, SILENCE)           # 0x7F & 0xFF: muted, the V bit dropped
    assert rt(pkt(bede + [0x10, 0x8A, 0, 0]), 1) == (10, 0)
    assert rt(pkt(bede + [0x10, 0x7F, 0, 0]), 1, DISCARD) == (127, DISCARD | SILENCE)
    assert rt(pkt(bede + [0x90, 0xFF, 0, 0]), 9) == (R.NONE, 0)              # 0x90 >> 4 as a byte is -7
    assert rt(pkt(bede + [0x90, 0xFF, 0, 0]), 0xF9) == (R.NONE, 0)           # and a byte ID of -7 is off
    assert rt(pkt([0xBE, 0xDE, 0, 0, 0x10, 0xFF, 0, 0]), 1) == (R.NONE, 0)   # length word 0
    assert rt(pkt(bede + [0x10, 0xFF, 0, 0], b0=0x50), 1) == (R.NONE, 0)     # version 1
    assert rt(pkt(bede + [0x10, 0xFF, 0, 0], b0=0x80), 1) == (R.NONE, 0)     # no X
    assert rt(pkt(bede + [0x10, 0xFF, 0, 0]), 0) == (R.NONE, 0) and rt(pkt(bede + [0x10, 0xFF, 0, 0]), 128) == (R.NONE, 0)
    assert rt(pkt(bede + [0x10, 0xFF, 0, 0]), 1, SKIP) == (R.NONE, SKIP)
    assert rt(pkt(bede + [0x10, 0xFF, 0, 0]), 1, 0, cap=19) == (R.NONE, 0)   # isInvalid
    assert rt(pkt([0xBE, 0xDE, 0x80, 0x01, 0x10, 0xFF, 0, 0]), 1) == (R.NONE, 0)  # a negative length: no walk
    assert rt(pkt([0xBE, 0xDE, 0x00, 0x02, 0x00, 0x10, 0x10, 0x05, 0, 0, 0, 0]), 1) == (5, 0)   # padding swallows a byte
    assert rt(pkt([0xBE, 0xDE, 0x00, 0x02, 0x22, 1, 2, 3, 0x10, 0x7F, 0, 0]), 1) == (127, SILENCE)  # second element
    assert rt(pkt([0xBE, 0xDF, 0x00, 0x01, 0x10, 0xFF, 0, 0]), 1) == (R.NONE, 0)  # neither form
    two = [0x10, 0x00, 0x00, 0x01]
    assert rt(pkt(two + [0x64, 0x01, 0x7F, 0]), 100) == (127, SILENCE)       # the two-byte form, ID 100
    assert rt(pkt(two + [0x64, 0x00, 0x33, 0]), 100) == (0x33, 0)            # length 0: levelsCount 0 is not < 0
    assert rt(pkt(two + [0x64, 0x80, 0x7F, 0]), 100) == (R.NONE, 0)          # the match's length byte negative
    assert rt(pkt([0x10, 0x00, 0x00, 0x02, 0x05, 0xFE, 1, 2, 0x64, 0x01, 0x7F, 0]), 100) == (R.NONE, 0)  # backwards
    assert rt(pkt([0x10, 0x10, 0x00, 0x01, 0x64, 0x01, 0x7F, 0]), 100) == (R.NONE, 0)   # 0x10 >> 4 is not 0
    assert rt(pkt([0x10, 0x0F, 0x00, 0x01, 0x64, 0x01, 0x7F, 0]), 100) == (127, SILENCE)
    assert rt(pkt(bede + [0, 0, 0, 0x10]), 1) == (R.NONE, 0)                 # the data byte lies at len
    assert rt(pkt([0xBE, 0xDE, 0x00, 0x02, 0, 0, 0, 0x10]), 1) == (R.NONE, 0)
    assert rt(pkt([0xBE, 0xDE, 0x00]), 1) == (R.NONE, 0)                     # the length word past the packet


# ------------------------------------------------------------------ the sweep
IDS = (0, 1, 2, 7, 8, 9, 15, 100, 127, 128, 255)


def sweep():
    """(region bytes, len, cap, flags, ext_id)"""
    for eid, lvl in ((1, 0x7F), (7, 0x8A), (100, 0xFF)):
        for name, build, _ in R.header_shapes(eid, lvl):
            p = build(0x1234, 7, bytes(range(20)))
            n = len(p)
            region = p + bytes([0x5A]) * 16
            for i in IDS + (eid, eid & 15):
                yield region, n, n + 8, 0, i
            for ln in range(0, min(n + 12, 110)):
                yield region, ln, ln + (ln & 1), 0, eid
                yield region, ln, n + 16, 0, eid & 15 or 1
            for fl in (SKIP, DISCARD, SILENCE, SKIP | SILENCE, 0x40000001):
                yield region, n, n, fl, eid
            for ln, cap in ((n, n - 1), (-1, n), (n, -1), (n, 0)):
                yield region, ln, cap, 0, eid


def randoms(count, seed=20240611):
    rng = random.Random(seed)
    for k in range(count):
        n = rng.randrange(0, 120)
        p = bytearray(rng.randrange(256) for _ in range(n + 8))
        cc = rng.randrange(4)
        if k % 8:
            p[0] = 0x90 | cc
        x = 12 + 4 * (p[0] & 15)
        if len(p) > x + 3 and k % 4:
            p[x:x + 2] = b"\xBE\xDE" if k % 3 else bytes([0x10, rng.randrange(16)])
            p[x + 2], p[x + 3] = 0, rng.randrange(12)
        eid = rng.randrange(16) if k % 5 else rng.randrange(256)
        yield bytes(p), n, n + 8 if k % 3 else rng.randrange(130), 0 if k % 11 else rng.choice((SKIP, DISCARD, SILENCE)), eid


def test_job_agrees_with_the_reference():
    job = N.lib().srtp_audio_level_job
    lv, fo = C.c_int8(), C.c_uint32()
    cases = found = silent = 0
    for source in (sweep(), randoms(6000)):
        for region, ln, cap, fl, eid in source:
            have = min(max(ln, 0), 65535)
            assert len(region) >= have or ln > cap
            assert job(region[:have], ln, cap, fl, eid, C.byref(lv), C.byref(fo)) == 0
            want = R.reverse_transform(region, ln, cap, fl, eid)
            assert (lv.value, fo.value) == want, (region.hex(), ln, cap, fl, eid, lv.value, fo.value, want)
            cases += 1
            found += want[0] >= 0
            silent += want[0] == 127
    assert cases > 15000 and found > 1000 and silent > 300, (cases, found, silent)


def test_audio_level_check_builds_and_runs_clean(tmp_path):
    """tools/audio_level_check (the Makefile's recipe, built out of tree): the
    rule over exact-size heap buffers against the Java restated with int8_t
    bytes; a program of its own under AddressSanitizer + UBSan."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^audio_level_check: audio_level_check\.cpp .*audio_level_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "audio_level_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "audio_level_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"audio_level_check: \d+ cases, [1-9]\d* found, [1-9]\d* silent, 0 failures", r.stdout)
