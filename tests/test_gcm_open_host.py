"""The one-pass GCM open as seen without a GPU: the debug flag, srtp_gcm_stats
and the new entries agree between the header, _native.py and the built
library; srtp_stats is still what test_gcm_small_abi.py pins; the two rules the
kernels compile from gcm_job.h -- srtp_gcm_spec_ok, srtp_gcm_fix_action --
agree, over the whole sweep of tools/gcm_job_check.cpp, with a few lines of
Python that restate them, and those lines with what gcm_ref.process_one
deciphers; tools/gcm_open_check builds and runs clean under AddressSanitizer +
UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import gcm_ref as G
import test_gcm_engine_host as H
import test_gcm_small_abi as ABI
from libjitsi_amd import _native as N

ROOT = H.ROOT
NEW = {"srtp_engine_gcm_stats": "int", "srtp_dispatch_gcm_stats": "int", "srtp_gcm_open_lane_min": "int32_t",
       "srtp_gcm_open_wave_min": "int32_t",
       "srtp_gcm_open_wave_max": "int32_t", "srtp_gcm_spec_ok": "int32_t", "srtp_gcm_fix_action": "int32_t"}
OK, REPLAY, AUTH, MALFORMED, NOT_PROCESSED = 0, 1, 2, 6, 8


def _header():
    with open(N.HEADER_PATH) as fh:
        return fh.read()


def test_flag_struct_and_exports_agree():
    header = _header()
    assert re.search(r"#define SRTP_DEBUG_NO_GCM_SPEC 0x80u\b", header)
    assert N.DEBUG_NO_GCM_SPEC == 0x80
    assert re.search(r"#define SRTP_DEBUG_FORCE_GCM_SPEC 0x100u\b", header) and N.DEBUG_FORCE_GCM_SPEC == 0x100
    others = [N.DEBUG_FORCE_CHAIN_STALL, N.DEBUG_FORCE_WIDE, N.DEBUG_NO_WIDE, N.DEBUG_NO_SMALL, N.DEBUG_NO_GCM_WAVE,
              N.DEBUG_FORCE_GCM_WAVE, N.DEBUG_FORCE_SMALL]
    assert all(not ((N.DEBUG_NO_GCM_SPEC | N.DEBUG_FORCE_GCM_SPEC) & f) for f in others)
    lib = C.CDLL(N.LIB_PATH)
    for name, ret in NEW.items():
        assert name in N.EXPORTED
        assert hasattr(lib, name)
        assert f"{ret} {name}(" in header
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\} srtp_gcm_stats;", text).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "uint64_t opened, restored, late;"
    assert [n for n, _ in N.GcmStats._fields_] == ["opened", "restored", "late"]
    assert C.sizeof(N.GcmStats) == 24 and N.GcmStats().as_dict() == {"opened": 0, "restored": 0, "late": 0}
    for v, name in ((N.GCM_FIX_NONE, "NONE"), (N.GCM_FIX_RESTORE, "RESTORE"), (N.GCM_FIX_DECIPHER, "DECIPHER")):
        assert re.search(rf"#define SRTP_GCM_FIX_{name} {v}\b", header)
    # a NULL engine / dispatcher is refused before any device is touched
    assert N.lib().srtp_engine_gcm_stats(None, C.byref(N.GcmStats())) == -1
    assert N.lib().srtp_dispatch_gcm_stats(None, C.byref(N.GcmStats())) == -1
    assert N.lib().srtp_gcm_spec_ok(2, 40, 60, 12, 0, 1, 0x80) == -1
    # the limits: a lane-route limit lies past the wave route's range, the wave route's inside it
    wmax = int(N.lib().srtp_gcm_wave_max())
    assert int(N.lib().srtp_gcm_open_lane_min()) > wmax
    assert 0 <= int(N.lib().srtp_gcm_open_wave_min()) <= int(N.lib().srtp_gcm_open_wave_max()) <= wmax


def test_srtp_stats_is_unchanged():
    """srtp_stats exactly as test_gcm_small_abi.py pins it: the three new
    counters live in a struct of their own."""
    ABI.test_stats_ends_with_small_aead_bundles()
    ABI.test_stats_is_eight_bytes_larger()
    ABI.test_header_agrees()
    assert not {"opened", "restored", "late"} & {n for n, _ in N.Stats._fields_}


# ---- the two rules, restated
def py_fixed(b0):
    return 12 + 4 * (b0 & 15) + (4 if b0 & 0x10 else 0)


def py_wanted(kind, j, status, e):
    """The packet is to leave deciphered."""
    return status == OK and bool(j.decipher) and (kind == 0 or e == 1)


def py_spec_ok(kind, j, h, b0, e):
    if j.status != -1 or not j.decipher or j.data_len <= 0:
        return 0
    if kind == 1:
        return int(e == 1)
    return int(h != N.GCM_HDR_THROW and h >= py_fixed(b0))


def py_fix_action(spec_done, status, wanted, rtp, g0, cw):
    if spec_done and wanted:
        return N.GCM_FIX_RESTORE | N.GCM_FIX_DECIPHER if rtp and g0 != cw else N.GCM_FIX_NONE
    if spec_done:
        return N.GCM_FIX_RESTORE
    return N.GCM_FIX_DECIPHER if wanted else N.GCM_FIX_NONE


def _cases():
    for L in range(0, 81):
        for cap in (L, L + 15, L + 16, L + 19, L + 20, L + 36):
            for kind in (0, 1):
                for shape in (H.SHAPES if kind == 0 else ("plain",)):
                    for flags in ((0, 2) if kind == 0 else (0,)):
                        for e in ((0, 1) if kind == 1 else (1,)):
                            yield kind, shape, L, cap, flags, e


def _geometry(kind, shape, L, cap, e, seed):
    buf = H._packet(kind, shape, L, cap, seed)
    if len(buf) < cap:
        return None
    if kind == 1 and L >= 20:
        buf[L - 4:L] = ((0x80000000 if e else 0) | 5).to_bytes(4, "big")
    h = H._header_len(buf, cap) if kind == 0 and L >= 12 else 12
    return buf, h


def test_spec_ok_over_the_sweep():
    """srtp_gcm_spec_ok against the restated rule on every unprotect shape of
    the sweep; among them no speculation for DISCARD, for E = 0, for a header
    length below the fixed header, for a packet without data."""
    lib, n, yes, seen = N.lib(), 0, 0, set()
    for kind, shape, L, cap, flags, e in _cases():
        g = _geometry(kind, shape, L, cap, e, L)
        if g is None:
            continue
        buf, h = g
        j = H.job(kind, True, L, cap, h, flags, e)
        b0 = buf[0] if cap else 0
        got = lib.srtp_gcm_spec_ok(kind, L, cap, h, flags, e, b0)
        assert got == py_spec_ok(kind, j, h, b0, e), (kind, shape, L, cap, h, flags, e)
        n += 1
        yes += got
        if j.status == -1 and not got:
            seen.add("discard" if not j.decipher else "e0" if kind == 1 and not e else "empty" if j.data_len == 0
                     else "short_header")
            if j.decipher and j.data_len > 0 and not (kind == 1 and not e):
                assert kind == 0 and 0 <= h < py_fixed(b0)
    assert n > 5000 and yes > 500
    assert seen == {"discard", "e0", "empty", "short_header"}


def test_fix_action_over_every_verdict():
    lib = N.lib()
    for spec_done in (0, 1):
        for status in (OK, REPLAY, AUTH, MALFORMED, NOT_PROCESSED, 3, 4, 5, 7, 9, 10):
            for wanted in (0, 1):
                for rtp in (0, 1):
                    for g0, cw in ((7, 7), (7, 8), (0, 0xFFFFFFFF), (0x80000005, 0x80000005)):
                        got = lib.srtp_gcm_fix_action(spec_done, status, wanted, rtp, g0, cw)
                        want = py_fix_action(spec_done, status, bool(wanted) and status == OK, rtp, g0, cw)
                        assert got == want, (spec_done, status, wanted, rtp, g0, cw)
    # the ones the issue names
    for st in (REPLAY, AUTH, MALFORMED, NOT_PROCESSED):
        assert lib.srtp_gcm_fix_action(1, st, 0, 1, 3, 3) == N.GCM_FIX_RESTORE
        assert lib.srtp_gcm_fix_action(0, st, 0, 1, 3, 3) == N.GCM_FIX_NONE
    assert lib.srtp_gcm_fix_action(0, OK, 1, 1, 3, 4) == N.GCM_FIX_DECIPHER
    assert lib.srtp_gcm_fix_action(1, OK, 1, 1, 3, 3) == N.GCM_FIX_NONE
    assert lib.srtp_gcm_fix_action(1, OK, 1, 0, 3, 4) == N.GCM_FIX_NONE  # SRTCP: g0 and cw play no part
    assert lib.srtp_gcm_fix_action(1, OK, 1, 1, 3, 4) == N.GCM_FIX_RESTORE | N.GCM_FIX_DECIPHER


def test_rules_are_held_to_the_reference():
    """For packets the reference accepts -- every header shape, DISCARD, E = 0
    and 1, a few lengths -- gcm_ref.process_one changes bytes exactly where the
    restated rule says the packet leaves deciphered: after the open pass alone
    (speculated, fix action NONE) or after the fix pass's DECIPHER."""
    mk, ms = G.payload(16, 1), G.payload(12, 2)
    fac = G.Factory(True, mk, ms, G.policy(16), G.policy(16))
    lib, n, ways = N.lib(), 0, set()
    for kind, shape, L, cap, flags, e in _cases():
        if L not in (28, 29, 33, 40, 45, 48, 52, 61, 64, 77, 80) or cap not in (L + 20, L + 36):
            continue
        g = _geometry(kind, shape, L, cap, e, L)
        if g is None:
            continue
        buf, h = g
        j = H.job(kind, True, L, cap, h, flags, e)
        if j.status != -1:
            continue
        # make the bytes as they lie a sealed packet: the tag over them, under
        # the IV the receiver will form from them
        enc, salt = G.derive(mk, ms, kind == 1)
        rks = G.expand_key(enc)
        if kind == 0:
            iv = G.rtp_iv(salt, bytes(buf[8:12]), 0, (buf[2] << 8) | buf[3])
            aad = bytes(buf[:j.aad_len])
        else:
            iv = G.rtcp_iv(salt, bytes(buf[4:8]), 5)
            aad = bytes(buf[:j.aad_len]) + bytes(buf[j.word_at:j.word_at + 4])
        ct = bytes(buf[j.data_at:j.data_at + j.data_len])
        buf[j.tag_at:j.tag_at + 16] = G._tag(rks, iv, aad, ct)
        if kind == 0 and H._header_len(buf, cap) != h:
            continue  # the tag fell on the extension length of a short packet: another packet now
        before = bytes(buf)
        t = G.Transformer(kind, fac, fac)
        st, nl = G.process_one(t, True, buf, L, cap, flags)
        assert (st, nl) == (OK, j.new_len), (kind, shape, L, flags, e, st)
        changed = bytes(buf) != before
        if changed:
            assert all(j.data_at <= i < j.data_at + j.data_len for i in range(cap) if buf[i] != before[i])
        wanted = py_wanted(kind, j, st, e)
        assert changed == (wanted and j.data_len > 0)
        spec = lib.srtp_gcm_spec_ok(kind, L, cap, h, flags, e, before[0])
        act = lib.srtp_gcm_fix_action(spec, st, int(wanted), int(kind == 0), 0, 0)
        deciphered = bool(spec) != bool(act & N.GCM_FIX_RESTORE) or bool(act & N.GCM_FIX_DECIPHER)
        assert (deciphered and j.data_len > 0) == changed
        ways.add((bool(spec), act))
        n += 1
    assert n > 100
    assert ways == {(True, N.GCM_FIX_NONE), (False, N.GCM_FIX_DECIPHER), (False, N.GCM_FIX_NONE)}


def test_gcm_open_check_builds_and_runs_clean(tmp_path):
    """tools/gcm_open_check (the Makefile's recipe, built out of tree): the open
    pass, every verdict and the fix pass on exact-size buffers, a program of its
    own under AddressSanitizer + UBSan."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^gcm_open_check: gcm_open_check\.cpp .*gcm_job\.h", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gcm_open_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "gcm_open_check.cpp"),
           os.path.join(ROOT, "libjitsi_amd", "csrc", "host_crypto.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gcm_open_check: ok" in r.stdout
