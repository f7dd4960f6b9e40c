"""Host-side mirror of libjitsi's SRTP transformer API over the MI355X engine.

Same class and method names, argument meaning and error behaviour as the
reference (paths relative to src/org/jitsi/impl/neomedia/):

* ``SRTPPolicy``            transform/srtp/SRTPPolicy.java:24-120
* ``SRTPContextFactory``    transform/srtp/SRTPContextFactory.java:24-108
* ``RawPacket``             RawPacket.java (buffer/offset/length/flags + accessors)
* ``PacketTransformer``     transform/PacketTransformer.java:28-53
* ``SRTPTransformer``       transform/srtp/SRTPTransformer.java:53-219
* ``SRTCPTransformer``      transform/srtp/SRTCPTransformer.java:30-207

``transform(pkts)`` / ``reverseTransform(pkts)`` follow
SinglePacketTransformer.java:121-216: packets are processed in array order,
``None`` elements are skipped, each element is replaced by the transformed
packet or ``None`` (drop), and a packet on which the reference would throw
raises ``SRTPTransformException`` after the earlier packets were transformed
(the remaining elements of the array are left untouched).

All per-packet work runs on the GPU (libsrtp_mi355x.so); this module only
packs RawPackets into one bundle and unpacks the results.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import threading
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N


class SRTPTransformException(RuntimeError):
    """What SinglePacketTransformer rethrows (RuntimeException)."""


class SRTPPolicy:
    NULL_ENCRYPTION = 0
    AESCM_ENCRYPTION = 1
    AESF8_ENCRYPTION = 2
    TWOFISH_ENCRYPTION = 3
    TWOFISHF8_ENCRYPTION = 4
    AESGCM_ENCRYPTION = 5  # RFC 7714 AEAD_AES_128_GCM / AEAD_AES_256_GCM (later libjitsi's constant)
    NULL_AUTHENTICATION = 0
    HMACSHA1_AUTHENTICATION = 1
    SKEIN_AUTHENTICATION = 2

    def __init__(self, encType: int, encKeyLength: int, authType: int, authKeyLength: int,
                 authTagLength: int, saltKeyLength: int):
        self.encType = encType
        self.encKeyLength = encKeyLength
        self.authType = authType
        self.authKeyLength = authKeyLength
        self.authTagLength = authTagLength
        self.saltKeyLength = saltKeyLength

    def getEncType(self): return self.encType
    def getEncKeyLength(self): return self.encKeyLength
    def getAuthType(self): return self.authType
    def getAuthKeyLength(self): return self.authKeyLength
    def getAuthTagLength(self): return self.authTagLength
    def getSaltKeyLength(self): return self.saltKeyLength

    def _c(self) -> N.Policy:
        return N.Policy(self.encType, self.encKeyLength, self.authType, self.authKeyLength,
                        self.authTagLength, self.saltKeyLength)

    def __repr__(self):
        return (f"SRTPPolicy(enc={self.encType}/{self.encKeyLength}, auth={self.authType}/"
                f"{self.authKeyLength}, tag={self.authTagLength}, salt={self.saltKeyLength})")


class SRTPPipeline:
    """Pinned-host bundle pipeline over one engine (srtp_pipeline_*, C ABI).

    ``depth`` slots of pinned host memory; a caller packs a bundle straight
    into a slot's arrays (``slot(i)``: numpy views ``seg``, ``off``, ``len``,
    ``cap``, ``flags``, ``tids``, ``status``), ``submit``s it (H2D on a copy
    stream, the engine's kernels, D2H on a second copy stream) and ``wait``s
    for the results in the same arrays.  Bundles run in submission order;
    while slot i's kernels run, slot j's copies proceed.  This is the bundle
    former the reference lacks (its I/O layer hands 1-element RawPacket[]
    arrays to PacketTransformer.transform, RTPConnectorOutputStream.java:268-300)."""

    def __init__(self, engine: "SRTPEngine", max_packets: int, max_seg_bytes: int, depth: int = 3):
        self.engine = engine
        h = C.c_void_p()
        N.check(N.lib().srtp_pipeline_create(engine.h, max_packets, max_seg_bytes, depth,
                                             C.byref(h)), engine.h, "srtp_pipeline_create")
        self.h = h
        self.depth = depth
        self._slots = []
        for i in range(depth):
            sl = N.PipelineSlot()
            N.check(N.lib().srtp_pipeline_slot_get(self.h, i, C.byref(sl)), engine.h, "slot_get")
            m = sl.max_packets

            def view(ptr, ct, count):
                return np.ctypeslib.as_array((ct * count).from_address(ptr))
            self._slots.append(dict(
                seg=view(sl.seg, C.c_uint8, sl.seg_cap), off=view(sl.off, C.c_uint32, m),
                len=view(sl.len, C.c_uint32, m), cap=view(sl.cap, C.c_uint32, m),
                flags=view(sl.flags, C.c_uint32, m), tids=view(sl.tids, C.c_int32, m),
                status=view(sl.status, C.c_int32, m)))

    def slot(self, i: int) -> dict:
        return self._slots[i]

    def submit(self, i: int, reverse: bool, n: int, seg_bytes: int, tid=None,
               use_flags: bool = False) -> None:
        """Enqueue slot i's first n packets; ``tid`` = one transformer id, or
        None to use the slot's per-packet ``tids``."""
        N.check(N.lib().srtp_pipeline_submit(self.h, i, int(reverse), int(tid is None),
                                             -1 if tid is None else int(tid), int(use_flags),
                                             n, seg_bytes), self.engine.h, "srtp_pipeline_submit")

    def wait(self, i: int) -> None:
        N.check(N.lib().srtp_pipeline_wait(self.h, i), self.engine.h, "srtp_pipeline_wait")

    def close(self) -> None:
        if self.h:
            self._slots = []
            N.lib().srtp_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def profile_policies(profile: str):
    """(srtpPolicy, srtcpPolicy) of a DTLS-SRTP protection profile, as the table
    in transform/dtls/DtlsPacketTransformer.java:574-612 builds them (note the
    10-byte SRTCP tag of the _32 profiles), of the SDES F8 crypto suite
    (transform/sdes/SDesTransformEngine.java:129-176: AES-F8, 10-byte tags), or
    of the AES-256-CM suites (RFC 6188; SDesControlImpl.java:71-72 lists them,
    ZRTP's AES3 yields the same policy, ZRTPTransformEngine.java:873-900)."""
    P = SRTPPolicy
    table = {
        "AES_CM_128_HMAC_SHA1_80": (P.AESCM_ENCRYPTION, 16, 14, 10, 10),
        "AES_CM_128_HMAC_SHA1_32": (P.AESCM_ENCRYPTION, 16, 14, 4, 10),
        "NULL_HMAC_SHA1_80": (P.NULL_ENCRYPTION, 0, 0, 10, 10),
        "NULL_HMAC_SHA1_32": (P.NULL_ENCRYPTION, 0, 0, 4, 10),
        "F8_128_HMAC_SHA1_80": (P.AESF8_ENCRYPTION, 16, 14, 10, 10),
        # ZRTP "2FS" Twofish policies (ZRTPTransformEngine.java:864-900: Twofish
        # with HMAC-SHA1 "HS80"/"HS32"; key length 128 or 256 bits)
        "TWOFISH_CM_128_HMAC_SHA1_80": (P.TWOFISH_ENCRYPTION, 16, 14, 10, 10),
        "TWOFISH_CM_128_HMAC_SHA1_32": (P.TWOFISH_ENCRYPTION, 16, 14, 4, 10),
        "TWOFISH_CM_256_HMAC_SHA1_80": (P.TWOFISH_ENCRYPTION, 32, 14, 10, 10),
        "TWOFISH_F8_128_HMAC_SHA1_80": (P.TWOFISHF8_ENCRYPTION, 16, 14, 10, 10),
        "TWOFISH_F8_256_HMAC_SHA1_80": (P.TWOFISHF8_ENCRYPTION, 32, 14, 10, 10),
        # AES-256-CM (RFC 6188): SRTPCryptoContext with encKeyLength 32
        "AES_256_CM_HMAC_SHA1_80": (P.AESCM_ENCRYPTION, 32, 14, 10, 10),
        "AES_256_CM_HMAC_SHA1_32": (P.AESCM_ENCRYPTION, 32, 14, 4, 10),
    }
    # ZRTP "SK32" / "SK64" Skein-MAC policies (ZRTPTransformEngine.java:867-909:
    # SKEIN_AUTHENTICATION with a 32-byte auth key, tag of srtpAuthTagLen / 8
    # bytes, one policy for SRTP and SRTCP) over AES-CM ("AES1"/"AES3") or
    # Twofish ("2FS1"/"2FS3")
    skein = {
        "AES_CM_128_SKEIN_32": (P.AESCM_ENCRYPTION, 16, 4),
        "AES_CM_128_SKEIN_64": (P.AESCM_ENCRYPTION, 16, 8),
        "AES_256_CM_SKEIN_64": (P.AESCM_ENCRYPTION, 32, 8),
        "TWOFISH_CM_128_SKEIN_32": (P.TWOFISH_ENCRYPTION, 16, 4),
        "TWOFISH_CM_256_SKEIN_64": (P.TWOFISH_ENCRYPTION, 32, 8),
    }
    # RFC 7714 AEAD profiles: NULL authentication (the 16-byte tag is the
    # cipher's own), no auth key, 12-byte salts; one policy for SRTP and SRTCP
    gcm = {"AEAD_AES_128_GCM": 16, "AEAD_AES_256_GCM": 32}
    if profile in gcm:
        return (P(P.AESGCM_ENCRYPTION, gcm[profile], P.NULL_AUTHENTICATION, 0, 16, 12),
                P(P.AESGCM_ENCRYPTION, gcm[profile], P.NULL_AUTHENTICATION, 0, 16, 12))
    if profile in skein:
        enc, klen, tag = skein[profile]
        pol = P(enc, klen, P.SKEIN_AUTHENTICATION, 32, tag, 14)
        return pol, P(enc, klen, P.SKEIN_AUTHENTICATION, 32, tag, 14)
    enc, klen, slen, rtp_tag, rtcp_tag = table[profile]
    return (P(enc, klen, P.HMACSHA1_AUTHENTICATION, 20, rtp_tag, slen),
            P(enc, klen, P.HMACSHA1_AUTHENTICATION, 20, rtcp_tag, slen))


class SRTPEngine:
    """One MI355X device's engine: HBM tables of session keys and contexts."""

    _default = {}
    _lock = threading.Lock()

    def __init__(self, device: int = 0, check_replay: bool = True, abort_on_error: bool = True,
                 max_contexts: int = 1 << 20, max_factories: int = 1 << 14,
                 max_transformers: int = 1 << 16, max_batch: int = 1 << 16):
        L = N.lib()
        o = N.EngineOpts()
        L.srtp_engine_opts_default(C.byref(o))
        o.device, o.check_replay, o.abort_on_error = device, int(check_replay), int(abort_on_error)
        o.max_contexts, o.max_factories = max_contexts, max_factories
        o.max_transformers, o.max_batch = max_transformers, max_batch
        h = C.c_void_p()
        N.check(L.srtp_engine_create(C.byref(o), C.byref(h)), None, "srtp_engine_create")
        self.h = h
        self.device = device
        # test hook: SRTP_TEST_DEBUG=<flags> puts every engine of a test run on
        # e.g. the split path (N.DEBUG_FORCE_WIDE) or the fused one (N.DEBUG_NO_WIDE)
        self._env_debug = int(os.environ.get("SRTP_TEST_DEBUG", "0"), 0)
        if self._env_debug:
            self.set_debug(0)

    @classmethod
    def default(cls, device: int = 0) -> "SRTPEngine":
        with cls._lock:
            if device not in cls._default:
                cls._default[device] = SRTPEngine(device)
            return cls._default[device]

    def close(self):
        if self.h:
            _rp_close_all(self)
            N.lib().srtp_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self, stream=None):
        N.check(N.lib().srtp_engine_sync(self.h, stream), self.h, "srtp_engine_sync")

    @property
    def stream_ptr(self) -> int:
        """hipStream_t of the engine's own stream (transform_device's default)."""
        return N.lib().srtp_engine_stream(self.h) or 0

    def set_timing(self, enable: bool) -> None:
        N.check(N.lib().srtp_engine_set_timing(self.h, int(enable)), self.h, "set_timing")

    def set_debug(self, flags: int) -> None:
        """Test hooks (srtp_engine_set_debug), e.g. N.DEBUG_FORCE_CHAIN_STALL."""
        flags = int(flags) | getattr(self, "_env_debug", 0)
        N.check(N.lib().srtp_engine_set_debug(self.h, flags), self.h, "set_debug")

    def enable_aead(self, on: bool = True) -> None:
        """srtp_engine_enable_aead: let new factories carry the RFC 7714 AES-GCM
        policy (profile_policies("AEAD_AES_128_GCM" / "AEAD_AES_256_GCM")); off
        on a new engine.  Existing GCM factories keep working when turned off."""
        N.check(N.lib().srtp_engine_enable_aead(self.h, int(bool(on))), self.h, "enable_aead")

    @property
    def trailer_room(self) -> int:
        """srtp_engine_trailer_room: the room the per-packet paths leave for
        protect's trailer -- 16, or 20 once enable_aead is on.  Aggregators and
        RawPacket batches sample it when they are created."""
        return int(N.lib().srtp_engine_trailer_room(self.h))

    def read_timing(self) -> dict:
        """{stage: (total ms, bundles)} since the last read (HIP events)."""
        ms = (C.c_double * len(N.STAGES))()
        cnt = (C.c_uint64 * len(N.STAGES))()
        N.check(N.lib().srtp_engine_read_timing(self.h, ms, cnt), self.h, "read_timing")
        return {name: (ms[i], cnt[i]) for i, name in enumerate(N.STAGES)}

    def num_contexts(self) -> int:
        return N.check(N.lib().srtp_engine_num_contexts(self.h), self.h, "num_contexts")

    def stats(self) -> dict:
        """srtp_engine_stats: cumulative per-status counts, ROC re-checks,
        repairs, context-table occupancy / overflow / rehashes."""
        st = N.Stats()
        N.check(N.lib().srtp_engine_stats(self.h, C.byref(st)), self.h, "stats")
        return st.as_dict()

    def gcm_stats(self) -> dict:
        """srtp_engine_gcm_stats: AES-GCM packets deciphered with their tag
        check (opened), of those put back as ciphertext after the walk
        (restored), and deciphered after the walk (late)."""
        st = N.GcmStats()
        N.check(N.lib().srtp_engine_gcm_stats(self.h, C.byref(st)), self.h, "gcm_stats")
        return st.as_dict()

    # -- control plane used by SRTPContextFactory / SRTPTransformer ----------
    def _factory_create(self, sender, key, salt, klen, slen, srtp, srtcp) -> int:
        fid = C.c_int32()
        rc = N.lib().srtp_factory_create(self.h, int(sender), key, klen, salt, slen, C.byref(srtp),
                                         C.byref(srtcp), C.byref(fid))
        N.check(rc, self.h, "SRTPContextFactory")
        return fid.value

    def _factory_close(self, fid: int) -> None:
        N.check(N.lib().srtp_factory_close(self.h, fid), self.h, "close")

    def _transformer_create(self, kind: int, fwd: int, rev: int) -> int:
        tid = C.c_int32()
        N.check(N.lib().srtp_transformer_create(self.h, kind, fwd, rev, C.byref(tid)), self.h,
                "transformer_create")
        return tid.value

    def _transformer_set_factory(self, tid: int, fid: int, forward: bool) -> None:
        N.check(N.lib().srtp_transformer_set_factory(self.h, tid, fid, int(forward)), self.h,
                "setFactory")

    def _transformer_close(self, tid: int) -> None:
        N.check(N.lib().srtp_transformer_close(self.h, tid), self.h, "close")

    def context_state(self, transformer: "_SRTPBase", ssrc: int) -> Optional[dict]:
        st = N.CtxState()
        rc = N.check(N.lib().srtp_get_context_state(self.h, transformer.tid, ssrc & 0xFFFFFFFF,
                                                    C.byref(st)), self.h, "get_context_state")
        if rc == 0:
            return None
        return {k: getattr(st, k) for k, _ in N.CtxState._fields_}

    def export_contexts(self, transformer: "_SRTPBase") -> dict:
        """{ssrc: state} of every context the transformer holds:
        ROC / s_l / replay window / SRTCP indices, to move a stream to another
        engine or GPU with srtp_set_context_state."""
        L = N.lib()
        cnt = C.c_uint32()
        N.check(L.srtp_export_contexts(self.h, transformer.tid, None, None, 0, C.byref(cnt)), self.h,
                "export_contexts")
        n = cnt.value
        ssrcs = (C.c_uint32 * max(n, 1))()
        states = (N.CtxState * max(n, 1))()
        N.check(L.srtp_export_contexts(self.h, transformer.tid, ssrcs, states, n, C.byref(cnt)),
                self.h, "export_contexts")
        return {int(ssrcs[i]): {k: getattr(states[i], k) for k, _ in N.CtxState._fields_}
                for i in range(min(n, cnt.value))}

    def import_context(self, transformer: "_SRTPBase", ssrc: int, state: dict,
                       forward: bool) -> None:
        """Create or overwrite the transformer's context for ssrc with an
        exported state, keyed by its forward or reverse factory."""
        st = N.CtxState(**{k: state.get(k, 0) for k, _ in N.CtxState._fields_})
        N.check(N.lib().srtp_set_context_state(self.h, transformer.tid, ssrc & 0xFFFFFFFF,
                                               int(forward), C.byref(st)), self.h, "import_context")

    # -- bundle entry points -------------------------------------------------
    def transform_host(self, reverse: bool, tid, seg: np.ndarray, off: np.ndarray,
                       length: np.ndarray, cap: np.ndarray, flags=None) -> np.ndarray:
        """Process a packed bundle held in host memory (copied to HBM and back).
        ``tid`` is one transformer id or an int32 array with one id per packet."""
        n = len(off)
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        assert length.dtype == np.uint32 and length.flags.c_contiguous and len(length) == n
        status = np.zeros(n, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            tids_p, tid0 = tids.ctypes.data, -1
        rc = N.lib().srtp_transform_host(
            self.h, int(reverse), tids_p, tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data,
            length.ctypes.data, cap.ctypes.data, None if fl is None else fl.ctypes.data,
            status.ctypes.data, n)
        N.check(rc, self.h, "srtp_transform_host")
        return status

    def transform_device(self, reverse: bool, tid, seg, off, length, cap, status, flags=None,
                         n: Optional[int] = None, stream=None) -> None:
        """Enqueue a bundle whose buffers are device tensors (torch, on this
        engine's GPU).  ``tid`` is an int or an int32 device tensor.  Async on
        ``stream`` (a torch.cuda.Stream or raw hipStream_t pointer); None =
        the device's default stream (torch's default stream too), ordered after
        the torch work that produced the tensors there.  ``stream_ptr`` is the
        engine's own stream (one hardware queue per engine)."""
        if n is None:
            n = off.numel()
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        rc = N.lib().srtp_transform_device(
            self.h, int(reverse), tids_p, tid0, seg.data_ptr(), off.data_ptr(), length.data_ptr(),
            cap.data_ptr(), None if flags is None else flags.data_ptr(), status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_transform_device")

    # -- receive with the ssrc-audio-level read on the device -------------------
    def transform_device_lvl(self, tid, seg, off, length, cap, status, level, flags=None, ext_ids=None,
                             ext_id: int = 0, n: Optional[int] = None, stream=None) -> None:
        """srtp_transform_device_lvl: :meth:`transform_device` with
        ``reverse=True`` and SsrcTransformEngine.reverseTransform
        (SsrcTransformEngine.java:226-274) in front of it, on the device.
        Entry i's ssrc-audio-level (RFC 6464, RawPacket.extractSsrcAudioLevel)
        is written to ``level[i]`` (an int8 tensor of n elements: 0..127, or
        -128 where the packet carries none) and an entry whose level is 127, a
        muted source, is unprotected as if the caller had flagged it
        ``N.PKT_FLAG_SILENCE``: authenticated, not deciphered.  ``ext_ids`` is
        a uint8 tensor with one negotiated extension ID per entry, or None for
        ``ext_id`` on every entry; an ID of 0 or above 127 reads nothing (pass
        0 for SRTCP entries).  The level is reported whatever the packet's
        SRTP status turns out to be; the reference, too, dispatches it before
        authentication.  Async on ``stream`` like :meth:`transform_device`."""
        if n is None:
            n = off.numel()
        if level.element_size() != 1 or level.numel() < n or not level.is_contiguous():
            raise ValueError("level: a contiguous tensor of n 1-byte elements")
        if ext_ids is not None and (ext_ids.element_size() != 1 or ext_ids.numel() < n or
                                    not ext_ids.is_contiguous()):
            raise ValueError("ext_ids: a contiguous tensor of n 1-byte elements")
        if not 0 <= int(ext_id) <= 255:
            raise ValueError("ext_id: a byte")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        rc = N.lib().srtp_transform_device_lvl(
            self.h, tids_p, tid0, seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(),
            None if flags is None else flags.data_ptr(), None if ext_ids is None else ext_ids.data_ptr(),
            int(ext_id), level.data_ptr(), status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_transform_device_lvl")

    def transform_host_lvl(self, tid, seg: np.ndarray, off: np.ndarray, length: np.ndarray, cap: np.ndarray,
                           flags=None, ext_ids=None, ext_id: int = 0):
        """srtp_transform_host_lvl: :meth:`transform_host` with
        ``reverse=True`` and the audio-level stage of
        :meth:`transform_device_lvl` in front (SsrcTransformEngine.java:226-274).
        ``ext_ids``: one uint8 ID per packet, or None for ``ext_id`` on every
        packet.  Returns ``(status, level)``, ``level`` an int8 array."""
        n = len(off)
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        assert length.dtype == np.uint32 and length.flags.c_contiguous and len(length) == n
        status = np.zeros(n, np.int32)
        level = np.full(n, N.AUDIO_LEVEL_NONE, np.int8)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        ids = None if ext_ids is None else np.ascontiguousarray(ext_ids, np.uint8)
        assert (fl is None or len(fl) == n) and (ids is None or len(ids) == n)
        if not 0 <= int(ext_id) <= 255:
            raise ValueError("ext_id: a byte")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            assert len(tids) == n
            tids_p, tid0 = tids.ctypes.data, -1
        rc = N.lib().srtp_transform_host_lvl(
            self.h, tids_p, tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data, length.ctypes.data,
            cap.ctypes.data, None if fl is None else fl.ctypes.data, None if ids is None else ids.ctypes.data,
            int(ext_id), level.ctypes.data, status.ctypes.data, n)
        N.check(rc, self.h, "srtp_transform_host_lvl")
        return status, level

    def audio_level_stats(self) -> dict:
        """srtp_engine_audio_level_stats: the _lvl calls, the entries whose
        bytes were read, the levels found and the entries flagged silent."""
        st = N.AudioLevelStats()
        N.check(N.lib().srtp_engine_audio_level_stats(self.h, C.byref(st)), self.h, "audio_level_stats")
        return st.as_dict()

    # -- fan-out: one packet to many peers -----------------------------------
    def fanout_device(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status,
                      src_status=None, flags=None, m: Optional[int] = None, n: Optional[int] = None,
                      stream=None) -> None:
        """srtp_fanout_device over torch tensors on this engine's GPU: the m
        sources (``src_seg`` uint8, ``src_off`` / ``src_len`` / ``src_cap``
        4-byte ints, ``src_status`` int32 or None) are expanded on the device
        into the n destination entries (entry j: a copy of source
        ``src_idx[j]`` in region ``off[j]`` / ``cap[j]`` of ``seg``) and
        protected as one bundle under ``tid`` (an int, or an int32 tensor with
        one transformer id per entry).  ``length`` and ``status`` are outputs.
        ``src_len`` / ``src_status`` may be the ``length`` / ``status`` tensors
        of a ``transform_device(reverse=True)`` enqueued before on the same
        stream.  Async on ``stream`` like :meth:`transform_device`."""
        self.fanout_device_rw(tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status, None,
                              src_status, flags, m, n, stream)

    def fanout_device_rw(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status,
                         rewrite, src_status=None, flags=None, m: Optional[int] = None, n: Optional[int] = None,
                         stream=None) -> None:
        """srtp_fanout_device_rw: :meth:`fanout_device` with one rewrite record
        per destination entry.  ``rewrite`` is a tensor on this engine's GPU
        that holds n x 16 bytes, 16-byte aligned (n records of
        ``N.FANOUT_REWRITE_DTYPE``: mask, ssrc, timestamp, seq, pt in host
        byte order), or None for :meth:`fanout_device` exactly.  Entry j's copy
        gets the fields its mask names (``N.REWRITE_SSRC`` / ``_SEQ`` /
        ``_TIMESTAMP`` / ``_PT``) before it is parsed: its SRTP context is the
        one of the rewritten SSRC.  Mask bits above 0xF are ignored here."""
        if m is None:
            m = src_off.numel()
        if n is None:
            n = off.numel()
        if rewrite is not None and rewrite.numel() * rewrite.element_size() < 16 * n:
            raise ValueError("fanout_device_rw: rewrite holds fewer than n records")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        rc = N.lib().srtp_fanout_device_rw(
            self.h, src_seg.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), src_cap.data_ptr(),
            None if src_status is None else src_status.data_ptr(), m, src_idx.data_ptr(), tids_p, tid0,
            seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(),
            None if flags is None else flags.data_ptr(), None if rewrite is None else rewrite.data_ptr(),
            status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_fanout_device" if rewrite is None else "srtp_fanout_device_rw")

    def fanout_device_ast(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status,
                          rewrite, stamp, src_status=None, flags=None, m: Optional[int] = None,
                          n: Optional[int] = None, stream=None) -> None:
        """srtp_fanout_device_ast: :meth:`fanout_device_rw` with one
        abs-send-time record per destination entry.  ``stamp`` is a tensor on
        this engine's GPU that holds n x 8 bytes, 8-byte aligned (n records of
        ``N.FANOUT_AST_DTYPE``: value, id, on), or None for
        :meth:`fanout_device_rw` exactly; ``rewrite`` may be None either way.
        Where entry j's record is on and its copy carries a one-byte
        header-extension element with that ID and len 2, found as
        AbsSendTimeEngine.replaceAbsSendTime finds it
        (AbsSendTimeEngine.java:86-152; the engine sits in front of SRTP,
        MediaStreamImpl.java:1018-1035), the element's three bytes become the
        low 24 bits of ``value``, big-endian, before the copy is protected."""
        if m is None:
            m = src_off.numel()
        if n is None:
            n = off.numel()
        if rewrite is not None and rewrite.numel() * rewrite.element_size() < 16 * n:
            raise ValueError("fanout_device_ast: rewrite holds fewer than n records")
        if stamp is not None and stamp.numel() * stamp.element_size() < 8 * n:
            raise ValueError("fanout_device_ast: stamp holds fewer than n records")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        rc = N.lib().srtp_fanout_device_ast(
            self.h, src_seg.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), src_cap.data_ptr(),
            None if src_status is None else src_status.data_ptr(), m, src_idx.data_ptr(), tids_p, tid0,
            seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(),
            None if flags is None else flags.data_ptr(), None if rewrite is None else rewrite.data_ptr(),
            None if stamp is None else stamp.data_ptr(), status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_fanout_device_ast")

    def fanout_device_pay(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status,
                          rewrite, stamp, pay, src_status=None, flags=None, m: Optional[int] = None,
                          n: Optional[int] = None, stream=None) -> None:
        """srtp_fanout_device_pay: :meth:`fanout_device_ast` with one payload
        record per destination entry.  ``pay`` is a tensor on this engine's
        GPU that holds n x 8 bytes, 8-byte aligned (n records of
        ``N.FANOUT_PAYLOAD_DTYPE``: at0, b0, at1, b1), or None for
        :meth:`fanout_device_ast` exactly; ``rewrite`` and ``stamp`` may each
        be None either way.  A patch writes its two bytes at packet bytes
        ``at``, ``at + 1`` of entry j's copy before the copy is protected --
        the RTX original sequence number, rewriteRTX's
        setOriginalSequenceNumber (ExtendedSequenceNumberInterval.java:261-284,
        RawPacket.java:1018-1022), or the FEC header's SN base, rewriteFEC's
        two stores (ExtendedSequenceNumberInterval.java:346-386).  It is on
        when ``at >= 12`` and the copy holds byte ``at``; a byte the copy does
        not hold is not written.  Patch 0, then patch 1, then the stamp."""
        if m is None:
            m = src_off.numel()
        if n is None:
            n = off.numel()
        if rewrite is not None and rewrite.numel() * rewrite.element_size() < 16 * n:
            raise ValueError("fanout_device_pay: rewrite holds fewer than n records")
        if stamp is not None and stamp.numel() * stamp.element_size() < 8 * n:
            raise ValueError("fanout_device_pay: stamp holds fewer than n records")
        if pay is not None and pay.numel() * pay.element_size() < 8 * n:
            raise ValueError("fanout_device_pay: pay holds fewer than n records")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        rc = N.lib().srtp_fanout_device_pay(
            self.h, src_seg.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), src_cap.data_ptr(),
            None if src_status is None else src_status.data_ptr(), m, src_idx.data_ptr(), tids_p, tid0,
            seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(),
            None if flags is None else flags.data_ptr(), None if rewrite is None else rewrite.data_ptr(),
            None if stamp is None else stamp.data_ptr(), None if pay is None else pay.data_ptr(),
            status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_fanout_device_pay")

    def fanout_device_red(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status,
                          rewrite, stamp, pay, red, red_out, src_status=None, flags=None, m: Optional[int] = None,
                          n: Optional[int] = None, stream=None) -> None:
        """srtp_fanout_device_red: :meth:`fanout_device_pay` with one RED
        (RFC 2198) record per destination entry.  ``red`` is a tensor on this
        engine's GPU that holds n x 4 bytes, 4-byte aligned (n records of
        ``N.FANOUT_RED_DTYPE``: mode, red_pt, reserved), or None for
        :meth:`fanout_device_pay` exactly; ``rewrite``, ``stamp`` and ``pay``
        may each be None either way.  ``N.RED_STRIP`` takes the one-byte RED
        header of a single-block packet whose PT is ``red_pt`` out of entry j's
        copy (REDFilterTransformEngine.java:95-145: length - 1), ``N.RED_WRAP``
        puts one in and makes ``red_pt`` the PT (REDTransformEngine.java:151-182:
        length + 1), ``N.RED_OFF`` leaves the entry to the other records.
        Where the reference throws the entry is dropped: it ends
        ``STATUS_SKIPPED``.  ``red_out`` (None, or an int8 tensor of n
        elements) gets what became of each entry: ``N.RED_UNTOUCHED``,
        ``N.RED_STRIPPED``, ``N.RED_WRAPPED`` or ``N.RED_DROPPED``.  RED runs
        first; the other records apply to the packet it left."""
        if m is None:
            m = src_off.numel()
        if n is None:
            n = off.numel()
        if rewrite is not None and rewrite.numel() * rewrite.element_size() < 16 * n:
            raise ValueError("fanout_device_red: rewrite holds fewer than n records")
        if stamp is not None and stamp.numel() * stamp.element_size() < 8 * n:
            raise ValueError("fanout_device_red: stamp holds fewer than n records")
        if pay is not None and pay.numel() * pay.element_size() < 8 * n:
            raise ValueError("fanout_device_red: pay holds fewer than n records")
        if red is not None and red.numel() * red.element_size() < 4 * n:
            raise ValueError("fanout_device_red: red holds fewer than n records")
        if red_out is not None and (red_out.element_size() != 1 or red_out.numel() < n):
            raise ValueError("fanout_device_red: red_out holds fewer than n 1-byte elements")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        rc = N.lib().srtp_fanout_device_red(
            self.h, src_seg.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), src_cap.data_ptr(),
            None if src_status is None else src_status.data_ptr(), m, src_idx.data_ptr(), tids_p, tid0,
            seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(),
            None if flags is None else flags.data_ptr(), None if rewrite is None else rewrite.data_ptr(),
            None if stamp is None else stamp.data_ptr(), None if pay is None else pay.data_ptr(),
            None if red is None else red.data_ptr(), None if red_out is None else red_out.data_ptr(),
            status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_fanout_device_red")

    def fanout_device_fec(self, tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, length, cap, status,
                          rewrite, stamp, pay, red, red_out, fec, members, fec_out, src_status=None, flags=None,
                          m: Optional[int] = None, n: Optional[int] = None, n_members: Optional[int] = None,
                          stream=None) -> None:
        """srtp_fanout_device_fec: :meth:`fanout_device_red` with one FEC
        record per destination entry.  ``fec`` is a tensor on this engine's GPU
        that holds n x 12 bytes, 4-byte aligned (n records of
        ``N.FANOUT_FEC_DTYPE``: first, ssrc, count, pt, red_pt, mode), or None
        for :meth:`fanout_device_red` exactly; ``members`` an int32 tensor of
        ``n_members`` indices of destination entries.  An entry whose record is
        on (``N.FEC_PLAIN``, ``N.FEC_RED``) has ``src_idx`` -1 and becomes the
        ulpfec packet (FECSender.java:319-412) over entries ``members[first ..
        first + count)`` as their other records left them, wrapped in RED
        (REDTransformEngine.java:151-182) for ``N.FEC_RED``, and is protected
        like any other entry; its own other records are ignored.  An entry the
        rule refuses (include/srtp_mi355x.h lists the causes) ends
        ``STATUS_SKIPPED``.  ``fec_out`` (None, or an int8 tensor of n
        elements) gets ``N.FEC_NONE``, ``N.FEC_MADE`` or ``N.FEC_REFUSED``."""
        if m is None:
            m = src_off.numel()
        if n is None:
            n = off.numel()
        if n_members is None:
            n_members = 0 if members is None else members.numel()
        for name, t, size in (("rewrite", rewrite, 16), ("stamp", stamp, 8), ("pay", pay, 8), ("red", red, 4),
                              ("fec", fec, 12)):
            if t is not None and t.numel() * t.element_size() < size * n:
                raise ValueError("fanout_device_fec: %s holds fewer than n records" % name)
        for name, t in (("red_out", red_out), ("fec_out", fec_out)):
            if t is not None and (t.element_size() != 1 or t.numel() < n):
                raise ValueError("fanout_device_fec: %s holds fewer than n 1-byte elements" % name)
        if members is not None and members.numel() * members.element_size() < 4 * n_members:
            raise ValueError("fanout_device_fec: members holds fewer than n_members indices")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids_p, tid0 = tid.data_ptr(), -1
        sp = getattr(stream, "cuda_stream", stream)
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = N.lib().srtp_fanout_device_fec(
            self.h, src_seg.data_ptr(), src_off.data_ptr(), src_len.data_ptr(), src_cap.data_ptr(), ptr(src_status),
            m, src_idx.data_ptr(), tids_p, tid0, seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(),
            ptr(flags), ptr(rewrite), ptr(stamp), ptr(pay), ptr(red), ptr(red_out), ptr(fec), ptr(members),
            n_members, ptr(fec_out), status.data_ptr(), n, sp)
        N.check(rc, self.h, "srtp_fanout_device_fec")

    def fanout_host(self, tid, src_seg: np.ndarray, src_off, src_len, src_cap, src_idx, seg: np.ndarray, off,
                    cap, src_status=None, flags=None):
        """srtp_fanout_host over numpy: only the source segment and the small
        arrays cross to the device.  ``seg`` is output only -- afterwards the
        bytes ``[off[j], off[j] + length[j])`` of the entries with status OK
        are defined, every other byte of it is unspecified.  Returns
        ``(length, status)``."""
        return self.fanout_host_rw(tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, cap, src_status, flags,
                                   None)

    def fanout_host_rw(self, tid, src_seg: np.ndarray, src_off, src_len, src_cap, src_idx, seg: np.ndarray, off,
                       cap, src_status=None, flags=None, rewrite=None):
        """srtp_fanout_host_rw: :meth:`fanout_host` with one rewrite record per
        destination entry, ``rewrite`` a numpy structured array of n records
        with dtype ``N.FANOUT_REWRITE_DTYPE`` (None: :meth:`fanout_host`
        exactly).  A mask with a bit above 0xF is refused (SRTP_EINVAL)."""
        assert src_seg.dtype == np.uint8 and src_seg.flags.c_contiguous
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous and seg.flags.writeable
        src_off = np.ascontiguousarray(src_off, np.uint32)
        src_len = np.ascontiguousarray(src_len, np.uint32)
        src_cap = np.ascontiguousarray(src_cap, np.uint32)
        src_idx = np.ascontiguousarray(src_idx, np.int32)
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        m, n = len(src_off), len(off)
        assert len(src_len) == m and len(src_cap) == m and len(src_idx) == n and len(cap) == n
        st_in = None if src_status is None else np.ascontiguousarray(src_status, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        assert (st_in is None or len(st_in) == m) and (fl is None or len(fl) == n)
        rw = None if rewrite is None else np.ascontiguousarray(rewrite, N.FANOUT_REWRITE_DTYPE)
        assert rw is None or len(rw) == n
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            assert len(tids) == n
            tids_p, tid0 = tids.ctypes.data, -1
        length = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        rc = N.lib().srtp_fanout_host_rw(
            self.h, src_seg.ctypes.data, src_seg.nbytes, src_off.ctypes.data, src_len.ctypes.data,
            src_cap.ctypes.data, None if st_in is None else st_in.ctypes.data, m, src_idx.ctypes.data, tids_p,
            tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data, length.ctypes.data, cap.ctypes.data,
            None if fl is None else fl.ctypes.data, None if rw is None else rw.ctypes.data, status.ctypes.data, n)
        N.check(rc, self.h, "srtp_fanout_host" if rw is None else "srtp_fanout_host_rw")
        return length, status

    def fanout_host_ast(self, tid, src_seg: np.ndarray, src_off, src_len, src_cap, src_idx, seg: np.ndarray, off,
                        cap, src_status=None, flags=None, rewrite=None, stamp=None):
        """srtp_fanout_host_ast: :meth:`fanout_host_rw` with one abs-send-time
        record per destination entry, ``stamp`` a numpy structured array of n
        records with dtype ``N.FANOUT_AST_DTYPE`` (None:
        :meth:`fanout_host_rw` exactly).  What a record does is
        :meth:`fanout_device_ast`'s (AbsSendTimeEngine.java:86-152,
        MediaStreamImpl.java:1018-1035)."""
        if stamp is None:
            return self.fanout_host_rw(tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, cap, src_status,
                                       flags, rewrite)
        assert src_seg.dtype == np.uint8 and src_seg.flags.c_contiguous
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous and seg.flags.writeable
        src_off = np.ascontiguousarray(src_off, np.uint32)
        src_len = np.ascontiguousarray(src_len, np.uint32)
        src_cap = np.ascontiguousarray(src_cap, np.uint32)
        src_idx = np.ascontiguousarray(src_idx, np.int32)
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        m, n = len(src_off), len(off)
        assert len(src_len) == m and len(src_cap) == m and len(src_idx) == n and len(cap) == n
        st_in = None if src_status is None else np.ascontiguousarray(src_status, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        assert (st_in is None or len(st_in) == m) and (fl is None or len(fl) == n)
        rw = None if rewrite is None else np.ascontiguousarray(rewrite, N.FANOUT_REWRITE_DTYPE)
        ast = np.ascontiguousarray(stamp, N.FANOUT_AST_DTYPE)
        assert (rw is None or len(rw) == n) and len(ast) == n
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            assert len(tids) == n
            tids_p, tid0 = tids.ctypes.data, -1
        length = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        rc = N.lib().srtp_fanout_host_ast(
            self.h, src_seg.ctypes.data, src_seg.nbytes, src_off.ctypes.data, src_len.ctypes.data,
            src_cap.ctypes.data, None if st_in is None else st_in.ctypes.data, m, src_idx.ctypes.data, tids_p,
            tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data, length.ctypes.data, cap.ctypes.data,
            None if fl is None else fl.ctypes.data, None if rw is None else rw.ctypes.data, ast.ctypes.data,
            status.ctypes.data, n)
        N.check(rc, self.h, "srtp_fanout_host_ast")
        return length, status

    def fanout_host_pay(self, tid, src_seg: np.ndarray, src_off, src_len, src_cap, src_idx, seg: np.ndarray, off,
                        cap, src_status=None, flags=None, rewrite=None, stamp=None, pay=None):
        """srtp_fanout_host_pay: :meth:`fanout_host_ast` with one payload
        record per destination entry, ``pay`` a numpy structured array of n
        records with dtype ``N.FANOUT_PAYLOAD_DTYPE`` (None:
        :meth:`fanout_host_ast` exactly); ``rewrite`` and ``stamp`` may each be
        None.  What a record does is :meth:`fanout_device_pay`'s
        (ExtendedSequenceNumberInterval.java:261-284 and :346-386)."""
        if pay is None:
            return self.fanout_host_ast(tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, cap, src_status,
                                        flags, rewrite, stamp)
        assert src_seg.dtype == np.uint8 and src_seg.flags.c_contiguous
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous and seg.flags.writeable
        src_off = np.ascontiguousarray(src_off, np.uint32)
        src_len = np.ascontiguousarray(src_len, np.uint32)
        src_cap = np.ascontiguousarray(src_cap, np.uint32)
        src_idx = np.ascontiguousarray(src_idx, np.int32)
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        m, n = len(src_off), len(off)
        assert len(src_len) == m and len(src_cap) == m and len(src_idx) == n and len(cap) == n
        st_in = None if src_status is None else np.ascontiguousarray(src_status, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        assert (st_in is None or len(st_in) == m) and (fl is None or len(fl) == n)
        rw = None if rewrite is None else np.ascontiguousarray(rewrite, N.FANOUT_REWRITE_DTYPE)
        ast = None if stamp is None else np.ascontiguousarray(stamp, N.FANOUT_AST_DTYPE)
        py = np.ascontiguousarray(pay, N.FANOUT_PAYLOAD_DTYPE)
        if len(py) < n:
            raise ValueError("fanout_host_pay: pay holds fewer than n records")
        assert (rw is None or len(rw) == n) and (ast is None or len(ast) == n)
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            assert len(tids) == n
            tids_p, tid0 = tids.ctypes.data, -1
        length = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        rc = N.lib().srtp_fanout_host_pay(
            self.h, src_seg.ctypes.data, src_seg.nbytes, src_off.ctypes.data, src_len.ctypes.data,
            src_cap.ctypes.data, None if st_in is None else st_in.ctypes.data, m, src_idx.ctypes.data, tids_p,
            tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data, length.ctypes.data, cap.ctypes.data,
            None if fl is None else fl.ctypes.data, None if rw is None else rw.ctypes.data,
            None if ast is None else ast.ctypes.data, py.ctypes.data, status.ctypes.data, n)
        N.check(rc, self.h, "srtp_fanout_host_pay")
        return length, status

    def fanout_host_red(self, tid, src_seg: np.ndarray, src_off, src_len, src_cap, src_idx, seg: np.ndarray, off,
                        cap, src_status=None, flags=None, rewrite=None, stamp=None, pay=None, red=None):
        """srtp_fanout_host_red: :meth:`fanout_host_pay` with one RED record
        per destination entry, ``red`` a numpy structured array of n records
        with dtype ``N.FANOUT_RED_DTYPE`` (None: :meth:`fanout_host_pay`
        exactly, every result code 0); ``rewrite``, ``stamp`` and ``pay`` may
        each be None.  What a record does is :meth:`fanout_device_red`'s
        (REDFilterTransformEngine.java:95-145, REDTransformEngine.java:151-182).
        A record with mode > 2, red_pt > 127 or non-zero reserved bytes is
        refused (SRTP_EINVAL).  Returns ``(length, status, red_out)``,
        ``red_out`` an int8 array."""
        if red is None:
            length, status = self.fanout_host_pay(tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off, cap,
                                                  src_status, flags, rewrite, stamp, pay)
            return length, status, np.zeros(len(status), np.int8)
        assert src_seg.dtype == np.uint8 and src_seg.flags.c_contiguous
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous and seg.flags.writeable
        src_off = np.ascontiguousarray(src_off, np.uint32)
        src_len = np.ascontiguousarray(src_len, np.uint32)
        src_cap = np.ascontiguousarray(src_cap, np.uint32)
        src_idx = np.ascontiguousarray(src_idx, np.int32)
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        m, n = len(src_off), len(off)
        assert len(src_len) == m and len(src_cap) == m and len(src_idx) == n and len(cap) == n
        st_in = None if src_status is None else np.ascontiguousarray(src_status, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        assert (st_in is None or len(st_in) == m) and (fl is None or len(fl) == n)
        rw = None if rewrite is None else np.ascontiguousarray(rewrite, N.FANOUT_REWRITE_DTYPE)
        ast = None if stamp is None else np.ascontiguousarray(stamp, N.FANOUT_AST_DTYPE)
        py = None if pay is None else np.ascontiguousarray(pay, N.FANOUT_PAYLOAD_DTYPE)
        rd = np.ascontiguousarray(red, N.FANOUT_RED_DTYPE)
        if len(rd) < n or (py is not None and len(py) < n):
            raise ValueError("fanout_host_red: fewer than n records")
        assert (rw is None or len(rw) == n) and (ast is None or len(ast) == n)
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            assert len(tids) == n
            tids_p, tid0 = tids.ctypes.data, -1
        length = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        red_out = np.zeros(n, np.int8)
        rc = N.lib().srtp_fanout_host_red(
            self.h, src_seg.ctypes.data, src_seg.nbytes, src_off.ctypes.data, src_len.ctypes.data,
            src_cap.ctypes.data, None if st_in is None else st_in.ctypes.data, m, src_idx.ctypes.data, tids_p,
            tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data, length.ctypes.data, cap.ctypes.data,
            None if fl is None else fl.ctypes.data, None if rw is None else rw.ctypes.data,
            None if ast is None else ast.ctypes.data, None if py is None else py.ctypes.data, rd.ctypes.data,
            red_out.ctypes.data, status.ctypes.data, n)
        N.check(rc, self.h, "srtp_fanout_host_red")
        return length, status, red_out

    def fanout_host_fec(self, tid, src_seg: np.ndarray, src_off, src_len, src_cap, src_idx, seg: np.ndarray, off,
                        cap, src_status=None, flags=None, rewrite=None, stamp=None, pay=None, red=None, fec=None,
                        members=None):
        """srtp_fanout_host_fec: :meth:`fanout_host_red` with one FEC record
        per destination entry, ``fec`` a numpy structured array of n records
        with dtype ``N.FANOUT_FEC_DTYPE`` and ``members`` an int32 array (None:
        :meth:`fanout_host_red` exactly, every FEC code 0).  What a record does
        is :meth:`fanout_device_fec`'s.  ``src_idx`` is -1 exactly for the
        entries whose record is on; a record or member that the rule would
        refuse for its fields or indices raises (SRTP_EINVAL).  Returns
        ``(length, status, red_out, fec_out)``."""
        if fec is None:
            length, status, ro = self.fanout_host_red(tid, src_seg, src_off, src_len, src_cap, src_idx, seg, off,
                                                      cap, src_status, flags, rewrite, stamp, pay, red)
            return length, status, ro, np.zeros(len(status), np.int8)
        assert src_seg.dtype == np.uint8 and src_seg.flags.c_contiguous
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous and seg.flags.writeable
        src_off = np.ascontiguousarray(src_off, np.uint32)
        src_len = np.ascontiguousarray(src_len, np.uint32)
        src_cap = np.ascontiguousarray(src_cap, np.uint32)
        src_idx = np.ascontiguousarray(src_idx, np.int32)
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        m, n = len(src_off), len(off)
        assert len(src_len) == m and len(src_cap) == m and len(src_idx) == n and len(cap) == n
        st_in = None if src_status is None else np.ascontiguousarray(src_status, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        assert (st_in is None or len(st_in) == m) and (fl is None or len(fl) == n)
        rw = None if rewrite is None else np.ascontiguousarray(rewrite, N.FANOUT_REWRITE_DTYPE)
        ast = None if stamp is None else np.ascontiguousarray(stamp, N.FANOUT_AST_DTYPE)
        py = None if pay is None else np.ascontiguousarray(pay, N.FANOUT_PAYLOAD_DTYPE)
        rd = None if red is None else np.ascontiguousarray(red, N.FANOUT_RED_DTYPE)
        fc = np.ascontiguousarray(fec, N.FANOUT_FEC_DTYPE)
        mem = np.ascontiguousarray(np.zeros(0, np.int32) if members is None else members, np.int32)
        for a in (rw, ast, py, rd, fc):
            if a is not None and len(a) < n:
                raise ValueError("fanout_host_fec: fewer than n records")
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            assert len(tids) == n
            tids_p, tid0 = tids.ctypes.data, -1
        length = np.zeros(n, np.uint32)
        status = np.zeros(n, np.int32)
        red_out = np.zeros(n, np.int8)
        fec_out = np.zeros(n, np.int8)
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = N.lib().srtp_fanout_host_fec(
            self.h, src_seg.ctypes.data, src_seg.nbytes, src_off.ctypes.data, src_len.ctypes.data,
            src_cap.ctypes.data, ptr(st_in), m, src_idx.ctypes.data, tids_p, tid0, seg.ctypes.data, seg.nbytes,
            off.ctypes.data, length.ctypes.data, cap.ctypes.data, ptr(fl), ptr(rw), ptr(ast), ptr(py), ptr(rd),
            red_out.ctypes.data, fc.ctypes.data, mem.ctypes.data if len(mem) else None, len(mem),
            fec_out.ctypes.data, status.ctypes.data, n)
        N.check(rc, self.h, "srtp_fanout_host_fec")
        return length, status, red_out, fec_out

    def fanout_fec_stats(self) -> dict:
        """srtp_engine_fanout_fec_stats: the _fec calls with records, the
        entries made and refused, and the member bytes XORed."""
        st = N.FanoutFecStats()
        N.check(N.lib().srtp_engine_fanout_fec_stats(self.h, C.byref(st)), self.h, "fanout_fec_stats")
        return st.as_dict()

    def fec_recover_device(self, seg, off, length, cap, status, rec, cand, out_seg, out_off, out_cap, out_len,
                           out_status, code, n: Optional[int] = None, n_rec: Optional[int] = None,
                           n_cand: Optional[int] = None, stream=None) -> None:
        """srtp_fec_recover_device: FECReceiver.Reconstructor (FECReceiver.java,
        setFecPacket :472-520 and recover :527-596) over the tables of a bundle
        that :meth:`transform_device` ``(reverse=True)`` has unprotected, on
        ``stream`` and with nothing read back.  Every argument is a tensor on
        this engine's GPU: ``rec`` holds n_rec x 16 bytes, 4-byte aligned
        (records of ``N.FEC_RECOVER_DTYPE``: fec, first, ssrc, count, on), and
        ``cand`` n_cand int32 entry indices; ``status`` may be None (every
        entry OK).  Record r recovers the one packet its FEC entry protects
        and ``cand[first .. first + count)`` lack, into ``out_seg`` at
        ``out_off[r]``; ``code`` (int8) gets ``N.FECRX_*``, ``out_len`` and
        ``out_status`` what :meth:`fanout_device` takes of a source."""
        n = off.numel() if n is None else n
        n_cand = (0 if cand is None else cand.numel()) if n_cand is None else n_cand
        if n_rec is None:
            n_rec = out_off.numel()
        if rec.numel() * rec.element_size() < 16 * n_rec:
            raise ValueError("fec_recover_device: rec holds fewer than n_rec records")
        if cand is not None and cand.numel() * cand.element_size() < 4 * n_cand:
            raise ValueError("fec_recover_device: cand holds fewer than n_cand indices")
        if code.element_size() != 1 or code.numel() < n_rec:
            raise ValueError("fec_recover_device: code holds fewer than n_rec 1-byte elements")
        for name, t in (("out_cap", out_cap), ("out_len", out_len), ("out_status", out_status)):
            if t.numel() * t.element_size() < 4 * n_rec:
                raise ValueError("fec_recover_device: %s holds fewer than n_rec elements" % name)
        sp = getattr(stream, "cuda_stream", stream)
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = N.lib().srtp_fec_recover_device(
            self.h, seg.data_ptr(), off.data_ptr(), length.data_ptr(), cap.data_ptr(), ptr(status), n,
            rec.data_ptr(), n_rec, ptr(cand), n_cand, out_seg.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(),
            out_len.data_ptr(), out_status.data_ptr(), code.data_ptr(), sp)
        N.check(rc, self.h, "srtp_fec_recover_device")

    def fec_recover_host(self, seg: np.ndarray, off, length, cap, rec, cand, out_seg: np.ndarray, out_off, out_cap,
                         status=None):
        """srtp_fec_recover_host over numpy: what :meth:`fec_recover_device`
        does, with the tables staged to the device and ``out_seg`` and the
        results copied back.  ``rec`` is a structured array of dtype
        ``N.FEC_RECOVER_DTYPE``, ``cand`` an int32 array.  A record or candidate
        index the rule would refuse raises (SRTP_EINVAL).  Returns ``(out_len,
        out_status, code)``."""
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous
        assert out_seg.dtype == np.uint8 and out_seg.flags.c_contiguous and out_seg.flags.writeable
        off = np.ascontiguousarray(off, np.uint32)
        length = np.ascontiguousarray(length, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        out_off = np.ascontiguousarray(out_off, np.uint32)
        out_cap = np.ascontiguousarray(out_cap, np.uint32)
        rc_ = np.ascontiguousarray(rec, N.FEC_RECOVER_DTYPE)
        cd = np.ascontiguousarray(np.zeros(0, np.int32) if cand is None else cand, np.int32)
        st = None if status is None else np.ascontiguousarray(status, np.int32)
        n, n_rec = len(off), len(rc_)
        assert len(length) == n and len(cap) == n and (st is None or len(st) == n)
        assert len(out_off) == n_rec and len(out_cap) == n_rec
        out_len = np.zeros(n_rec, np.uint32)
        out_status = np.zeros(n_rec, np.int32)
        code = np.zeros(n_rec, np.int8)
        rc = N.lib().srtp_fec_recover_host(
            self.h, seg.ctypes.data, seg.nbytes, off.ctypes.data, length.ctypes.data, cap.ctypes.data,
            None if st is None else st.ctypes.data, n, rc_.ctypes.data, n_rec, cd.ctypes.data if len(cd) else None,
            len(cd), out_seg.ctypes.data, out_seg.nbytes, out_off.ctypes.data, out_cap.ctypes.data,
            out_len.ctypes.data, out_status.ctypes.data, code.ctypes.data)
        N.check(rc, self.h, "srtp_fec_recover_host")
        return out_len, out_status, code

    def fec_recover_stats(self) -> dict:
        """srtp_engine_fec_recover_stats: the recover calls, the records that
        were on and how they ended, and the member bytes XORed."""
        st = N.FecRecoverStats()
        N.check(N.lib().srtp_engine_fec_recover_stats(self.h, C.byref(st)), self.h, "fec_recover_stats")
        return st.as_dict()

    def fanout_red_stats(self) -> dict:
        """srtp_engine_fanout_red_stats: the _red calls with records, and the
        entries they stripped, wrapped and dropped."""
        st = N.FanoutRedStats()
        N.check(N.lib().srtp_engine_fanout_red_stats(self.h, C.byref(st)), self.h, "fanout_red_stats")
        return st.as_dict()

    def fanout_stats(self) -> dict:
        """srtp_engine_fanout_stats: fan-out calls, their sources and
        destination entries, the entries skipped for their index or their
        source's status, and the source bytes fanout_host copied to the device."""
        st = N.FanoutStats()
        N.check(N.lib().srtp_engine_fanout_stats(self.h, C.byref(st)), self.h, "fanout_stats")
        return st.as_dict()


def host_register(arr: np.ndarray) -> None:
    """Pins ``arr``'s memory for DMA by every GPU (srtp_host_register): a
    long-lived buffer pool registered once, which the dispatcher then moves
    with no host copy (a one-shard bundle, or each shard's packets back to
    back).  Unregister before the array is freed."""
    assert arr.flags.c_contiguous and arr.nbytes > 0
    N.check(N.lib().srtp_host_register(arr.ctypes.data, arr.nbytes), None, "srtp_host_register")


def host_unregister(arr: np.ndarray) -> None:
    N.check(N.lib().srtp_host_unregister(arr.ctypes.data), None, "srtp_host_unregister")


class HostBuffer:
    """Pinned host memory of the engine's own (srtp_host_alloc), registered for
    in-place DMA like host_register's, at the full PCIe rate: ``array`` is a
    uint8 view of it.  close() frees it; no view may be used afterwards."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        N.check(N.lib().srtp_host_alloc(int(nbytes), C.byref(p)), None, "srtp_host_alloc")
        self._p = p
        self.array = np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(p.value))

    def close(self):
        if self._p:
            self.array = None
            N.check(N.lib().srtp_host_free(self._p), None, "srtp_host_free")
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_is_registered(arr: np.ndarray) -> bool:
    return bool(N.lib().srtp_host_is_registered(arr.ctypes.data, arr.nbytes))


class SRTPDispatcher:
    """In-process multi-GPU engine (srtp_dispatch_*, C ABI): one engine per
    shard on ``devices[i]`` (several shards may share a GPU), each bundle split
    by SSRC (shard = srtp_shard_of(SSRC)), results identical to one engine.
    Usable wherever an SRTPEngine is (``engine=`` of SRTPContextFactory)."""

    def __init__(self, devices: Sequence[int], check_replay: bool = True,
                 abort_on_error: bool = True, max_contexts: int = 1 << 20,
                 max_factories: int = 1 << 14, max_transformers: int = 1 << 16,
                 max_batch: int = 1 << 16):
        L = N.lib()
        o = N.EngineOpts()
        L.srtp_engine_opts_default(C.byref(o))
        o.check_replay, o.abort_on_error = int(check_replay), int(abort_on_error)
        o.max_contexts, o.max_factories = max_contexts, max_factories
        o.max_transformers, o.max_batch = max_transformers, max_batch
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        N.check(L.srtp_dispatch_create(devs, len(devices), C.byref(o), C.byref(h)), None,
                "srtp_dispatch_create")
        self.h = h
        self.devices = list(devices)

    @property
    def shards(self) -> int:
        return N.lib().srtp_dispatch_num_shards(self.h)

    def shard_of(self, ssrc: int) -> int:
        return N.lib().srtp_shard_of(ssrc & 0xFFFFFFFF, self.shards)

    def close(self):
        if self.h:
            _rp_close_all(self)
            N.lib().srtp_dispatch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        return N.check(rc, None, what, dispatch=self.h)

    def stats(self) -> dict:
        st = N.Stats()
        self._chk(N.lib().srtp_dispatch_stats(self.h, C.byref(st)), "stats")
        return st.as_dict()

    def gcm_stats(self) -> dict:
        """srtp_dispatch_gcm_stats: SRTPEngine.gcm_stats summed over the shards."""
        st = N.GcmStats()
        self._chk(N.lib().srtp_dispatch_gcm_stats(self.h, C.byref(st)), "gcm_stats")
        return st.as_dict()

    def enable_aead(self, on: bool = True) -> None:
        """srtp_dispatch_enable_aead: SRTPEngine.enable_aead on every shard."""
        self._chk(N.lib().srtp_dispatch_enable_aead(self.h, int(bool(on))), "enable_aead")

    def host_times(self) -> dict:
        """srtp_dispatch_host_times in ms (plan, pack, wait, scatter, total) and calls."""
        ns = (C.c_uint64 * 6)()
        self._chk(N.lib().srtp_dispatch_host_times(self.h, ns), "host_times")
        d = {k: ns[i] / 1e6 for i, k in enumerate(("plan_ms", "pack_ms", "wait_ms", "scatter_ms",
                                                    "total_ms"))}
        d["calls"] = int(ns[5])
        return d

    def context_state(self, transformer: "_SRTPBase", ssrc: int) -> Optional[dict]:
        st = N.CtxState()
        rc = self._chk(N.lib().srtp_dispatch_get_context_state(self.h, transformer.tid,
                                                               ssrc & 0xFFFFFFFF, C.byref(st)),
                       "get_context_state")
        if rc == 0:
            return None
        return {k: getattr(st, k) for k, _ in N.CtxState._fields_}

    def import_context(self, transformer: "_SRTPBase", ssrc: int, state: dict,
                       forward: bool) -> None:
        st = N.CtxState(**{k: state.get(k, 0) for k, _ in N.CtxState._fields_})
        self._chk(N.lib().srtp_dispatch_set_context_state(self.h, transformer.tid, ssrc & 0xFFFFFFFF,
                                                          int(forward), C.byref(st)),
                  "import_context")

    def _factory_create(self, sender, key, salt, klen, slen, srtp, srtcp) -> int:
        fid = C.c_int32()
        self._chk(N.lib().srtp_dispatch_factory_create(self.h, int(sender), key, klen, salt, slen,
                                                       C.byref(srtp), C.byref(srtcp), C.byref(fid)),
                  "SRTPContextFactory")
        return fid.value

    def _factory_close(self, fid: int) -> None:
        self._chk(N.lib().srtp_dispatch_factory_close(self.h, fid), "close")

    def _transformer_create(self, kind: int, fwd: int, rev: int) -> int:
        tid = C.c_int32()
        self._chk(N.lib().srtp_dispatch_transformer_create(self.h, kind, fwd, rev, C.byref(tid)),
                  "transformer_create")
        return tid.value

    def _transformer_set_factory(self, tid: int, fid: int, forward: bool) -> None:
        self._chk(N.lib().srtp_dispatch_transformer_set_factory(self.h, tid, fid, int(forward)),
                  "setFactory")

    def _transformer_close(self, tid: int) -> None:
        self._chk(N.lib().srtp_dispatch_transformer_close(self.h, tid), "close")

    def transform_host(self, reverse: bool, tid, seg: np.ndarray, off: np.ndarray,
                       length: np.ndarray, cap: np.ndarray, flags=None) -> np.ndarray:
        """As SRTPEngine.transform_host, split across the shards."""
        n = len(off)
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        assert length.dtype == np.uint32 and length.flags.c_contiguous and len(length) == n
        status = np.zeros(n, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            tids_p, tid0 = tids.ctypes.data, -1
        rc = N.lib().srtp_dispatch_transform_host(
            self.h, int(reverse), tids_p, tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data,
            length.ctypes.data, cap.ctypes.data, None if fl is None else fl.ctypes.data,
            status.ctypes.data, n)
        self._chk(rc, "srtp_dispatch_transform_host")
        return status

    def submit_host(self, reverse: bool, tid, seg: np.ndarray, off: np.ndarray,
                    length: np.ndarray, cap: np.ndarray, flags=None) -> "HostTicket":
        """srtp_dispatch_submit_host: transform_host without waiting.  The
        arrays (kept alive by the returned ticket) must not be touched until
        ``ticket.wait()`` (srtp_dispatch_wait_host) returns the statuses."""
        n = len(off)
        assert seg.dtype == np.uint8 and seg.flags.c_contiguous
        off = np.ascontiguousarray(off, np.uint32)
        cap = np.ascontiguousarray(cap, np.uint32)
        assert length.dtype == np.uint32 and length.flags.c_contiguous and len(length) == n
        status = np.zeros(n, np.int32)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint32)
        tids = None
        if np.isscalar(tid):
            tids_p, tid0 = None, int(tid)
        else:
            tids = np.ascontiguousarray(tid, np.int32)
            tids_p, tid0 = tids.ctypes.data, -1
        t = C.c_uint64()
        rc = N.lib().srtp_dispatch_submit_host(
            self.h, int(reverse), tids_p, tid0, seg.ctypes.data, seg.nbytes, off.ctypes.data,
            length.ctypes.data, cap.ctypes.data, None if fl is None else fl.ctypes.data,
            status.ctypes.data, n, C.byref(t))
        self._chk(rc, "srtp_dispatch_submit_host")
        return HostTicket(self, t.value, status, (seg, off, length, cap, fl, tids))


class HostTicket:
    """A host bundle in flight (SRTPDispatcher.submit_host)."""

    def __init__(self, d: SRTPDispatcher, ticket: int, status: np.ndarray, keep):
        self.d, self.ticket, self.status, self._keep = d, ticket, status, keep
        self.done = False

    def wait(self) -> np.ndarray:
        if not self.done:
            self.d._chk(N.lib().srtp_dispatch_wait_host(self.d.h, self.ticket), "srtp_dispatch_wait_host")
            self.done = True
            self._keep = None
        return self.status


class SRTPAggregator:
    """Per-packet submits from many threads -> bundles (srtp_aggregator_*,
    SURVEY.md 8f.2).  ``callback(cookie, status, data)`` runs on a dispatch
    thread once per packet, in bundle order; packets of one direction (and,
    over a dispatcher, of one shard) complete in the order they were
    accepted.  ``engine`` is an SRTPEngine or an SRTPDispatcher (one lane per
    shard, srtp_aggregator_create_dispatch).  Each packet is its own
    1-element RawPacket[] as in the reference's RTPConnector streams
    (RTPConnectorInputStream.java:425-452, RTPConnectorOutputStream.java
    :268-300,652-830), whatever the engine's abort_on_error.  ``callback``
    None: only synchronous ``transform`` calls.  ``seal_idle``: a lane with no
    bundle in flight seals at once (SRTP_AGG_SEAL_IDLE)."""

    def __init__(self, engine, callback, max_packets: int = 1 << 14,
                 max_bytes: int = 24 << 20, deadline_us: int = 1000, depth: int = 4,
                 seal_idle: bool = True):
        self.engine = engine
        o = N.AggregatorOpts(max_packets, max_bytes, deadline_us, depth,
                             N.AGG_SEAL_IDLE if seal_idle else 0)

        def _cb(user, cookie, status, data, length):
            callback(int(cookie), int(status), C.string_at(data, length) if length else b"")

        self._cb = N.AGG_CB(_cb) if callback is not None else N.AGG_CB()  # kept alive
        h = C.c_void_p()
        if isinstance(engine, SRTPDispatcher):
            rc = N.lib().srtp_aggregator_create_dispatch(engine.h, C.byref(o), self._cb, None,
                                                         C.byref(h))
            N.check(rc, None, "srtp_aggregator_create_dispatch")
        else:
            N.check(N.lib().srtp_aggregator_create(engine.h, C.byref(o), self._cb, None, C.byref(h)),
                    engine.h, "srtp_aggregator_create")
        self.h = h
        # the room behind a protect packet, sampled from the engine at creation
        # (srtp_aggregator_trailer_room): 16, or 20 with AES-GCM on
        self.trailer_room = int(N.lib().srtp_aggregator_trailer_room(h))

    def submit(self, reverse: bool, transformer: "_SRTPBase", data: bytes, flags: int = 0,
               cookie: int = 0) -> int:
        """0, or N.EFULL for a submit from a callback that found no free slot."""
        data = bytes(data)
        rc = N.lib().srtp_aggregator_submit(self.h, int(reverse), transformer.tid, data, len(data),
                                            flags, cookie)
        if rc == N.EFULL:
            return rc
        return N.check(rc, None, "submit")

    def transform(self, reverse: bool, transformer: "_SRTPBase", data: bytes, flags: int = 0):
        """Synchronous (srtp_aggregator_transform): (status, bytes) of one
        packet, sharing bundles with concurrent callers."""
        data = bytes(data)
        cap = len(data) if reverse else len(data) + self.trailer_room
        out = (C.c_uint8 * max(cap, 1))()
        st, ol = C.c_int32(), C.c_uint32()
        N.check(N.lib().srtp_aggregator_transform(self.h, int(reverse), transformer.tid, data, len(data),
                                                  len(data), cap, flags, out, C.byref(st), C.byref(ol)),
                None, "srtp_aggregator_transform")
        return int(st.value), bytes(out[:ol.value])

    def flush(self) -> None:
        N.check(N.lib().srtp_aggregator_flush(self.h), None, "flush")

    def stats(self) -> dict:
        a, c, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        N.lib().srtp_aggregator_stats(self.h, C.byref(a), C.byref(c), C.byref(b))
        return {"accepted": a.value, "completed": c.value, "bundles": b.value}

    def close(self) -> None:
        if self.h:
            N.lib().srtp_aggregator_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SRTPContextFactory:
    """SRTPContextFactory(sender, masterKey, masterSalt, srtpPolicy, srtcpPolicy)."""

    def __init__(self, sender: bool, masterKey: bytes, masterSalt: bytes, srtpPolicy: SRTPPolicy,
                 srtcpPolicy: SRTPPolicy, engine=None):
        self.engine = engine or SRTPEngine.default()
        key = (C.c_uint8 * len(masterKey)).from_buffer_copy(bytes(masterKey))
        salt = (C.c_uint8 * len(masterSalt)).from_buffer_copy(bytes(masterSalt))
        try:
            self.fid = self.engine._factory_create(sender, key, salt, len(masterKey),
                                                   len(masterSalt), srtpPolicy._c(),
                                                   srtcpPolicy._c())
        finally:
            C.memset(key, 0, len(masterKey))
            C.memset(salt, 0, len(masterSalt))
        self.sender = sender
        self.srtpPolicy, self.srtcpPolicy = srtpPolicy, srtcpPolicy

    def close(self):
        self.engine._factory_close(self.fid)


class RawPacket:
    """Packet view (nm/RawPacket.java): buffer, offset, length, flags."""

    FIXED_HEADER_SIZE = 12
    EXT_HEADER_SIZE = 4

    def __init__(self, buffer, offset: int = 0, length: Optional[int] = None, flags: int = 0):
        self.buffer = bytearray(buffer)
        self.offset = offset
        self.length = len(self.buffer) - offset if length is None else length
        self.flags = flags

    def getBuffer(self): return self.buffer
    def getOffset(self): return self.offset
    def getLength(self): return self.length
    def getFlags(self): return self.flags
    def setFlags(self, f): self.flags = f

    def data(self) -> bytes:
        return bytes(self.buffer[self.offset:self.offset + self.length])

    def readByte(self, off): return self.buffer[self.offset + off]

    def readInt(self, off):
        return int.from_bytes(self.buffer[self.offset + off:self.offset + off + 4], "big")

    def getSequenceNumber(self):
        return int.from_bytes(self.buffer[self.offset + 2:self.offset + 4], "big")

    def getSSRC(self): return self.readInt(8)
    def getRTCPSSRC(self): return self.readInt(4)

    def getHeaderLength(self):
        b0 = self.buffer[self.offset]
        h = 12 + 4 * (b0 & 0x0F)
        if b0 & 0x10:
            i = self.offset + 12 + 4 * (b0 & 0x0F) + 2
            hi = self.buffer[i] - 256 if self.buffer[i] >= 128 else self.buffer[i]
            h += 4 + ((hi << 8) | self.buffer[i + 1]) * 4
        return h

    def getPayloadLength(self): return self.length - self.getHeaderLength()

    def isInvalid(self):
        return len(self.buffer) < self.offset + self.length or self.length < 12


# largest trailer: SRTCP E|index (4) + 12-byte tag.  An engine with AES-GCM on
# needs 20 (SRTPEngine.trailer_room; pack's ``room``)
TRAILER_ROOM = 16


def block_encrypt(enc_type: int, key: bytes, block: bytes) -> bytes:
    """One block of the policy's cipher on the host (AES-128/256, Twofish)."""
    out = (C.c_uint8 * 16)()
    N.check(N.lib().srtp_block_encrypt(enc_type, bytes(key), len(key), bytes(block)[:16], out), None,
            "block_encrypt")
    return bytes(out)


def derive_session_keys_for(enc_type: int, masterKey: bytes, masterSalt: bytes, rtcp: bool = False):
    """Session keys with the policy's cipher as the PRF (Twofish for the ZRTP
    Twofish policies, AES otherwise).  AESGCM_ENCRYPTION: RFC 7714 11 -- a
    12-byte master salt, a 12-byte session salt (two zero bytes follow it) and
    a zeroed auth key."""
    mk = bytes(masterKey)
    klen = 32 if len(mk) >= 32 else 16
    enc, auth, salt = (C.c_uint8 * klen)(), (C.c_uint8 * 20)(), (C.c_uint8 * 14)()
    N.check(N.lib().srtp_derive_session_keys_for(enc_type, mk[:klen], klen, bytes(masterSalt)[:14],
                                                 int(rtcp), enc, auth, salt), None, "kdf")
    return bytes(enc), bytes(auth), bytes(salt)


def derive_session_keys_auth(enc_type: int, masterKey: bytes, masterSalt: bytes, rtcp: bool = False,
                             auth_len: int = 20):
    """Session keys with an auth key of `auth_len` bytes (ZRTP's Skein
    policies: 32, ZRTPTransformEngine.java:867-872)."""
    mk = bytes(masterKey)
    klen = 32 if len(mk) >= 32 else 16
    enc, auth, salt = (C.c_uint8 * klen)(), (C.c_uint8 * auth_len)(), (C.c_uint8 * 14)()
    N.check(N.lib().srtp_derive_session_keys_auth(enc_type, mk[:klen], klen, bytes(masterSalt)[:14],
                                                  int(rtcp), enc, auth, auth_len, salt), None, "kdf")
    return bytes(enc), bytes(auth), bytes(salt)


def aes_gcm(key: bytes, iv: bytes, aad: bytes, data: bytes, tag: Optional[bytes] = None):
    """The engine's host AES-GCM (srtp_aes_gcm; 12-byte IV, 16-byte tag).
    Without ``tag``: seals, returns (ciphertext, tag).  With it: opens, returns
    the plaintext, or None on a tag mismatch."""
    assert len(iv) == 12
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    t = (C.c_uint8 * 16).from_buffer_copy(bytes(tag) if tag is not None else bytes(16))
    rc = N.lib().srtp_aes_gcm(0 if tag is None else 1, bytes(key), len(key), bytes(iv), bytes(aad), len(aad),
                              buf, len(data), t)
    if rc == 1:
        return None
    N.check(rc, None, "aes_gcm")
    out = bytes(buf)[:len(data)]
    return (out, bytes(t)) if tag is None else out


def gf128_mul(a: bytes, b: bytes) -> bytes:
    """a * b in GF(2^128), 16-byte blocks in GCM's bit order (srtp_gf128_mul)."""
    out = (C.c_uint8 * 16)()
    assert len(a) == 16 and len(b) == 16
    N.check(N.lib().srtp_gf128_mul(bytes(a), bytes(b), out), None, "gf128_mul")
    return bytes(out)


def gcm_hpowers(h: bytes):
    """[h^1, ..., h^64] as 16-byte blocks (srtp_gcm_hpowers): the powers of the
    hash key the wave-per-packet GCM kernels multiply by."""
    out = (C.c_uint8 * 1024)()
    assert len(h) == 16
    N.check(N.lib().srtp_gcm_hpowers(bytes(h), out), None, "gcm_hpowers")
    return [bytes(out[16 * k:16 * k + 16]) for k in range(64)]


def aes_gcm_device(engine, key: bytes, seg, off, aad_len, length, iv, tag, result=None,
                   open: bool = False, n: Optional[int] = None, stream=None, wave: bool = False) -> None:
    """AES-GCM on the GPU for a batch of packets under one key
    (srtp_aes_gcm_device): the device twin of :func:`aes_gcm`.  All buffers are
    torch tensors on ``engine``'s GPU: packet i is ``seg[off[i] : off[i] +
    aad_len[i] + length[i]]`` (uint8; AAD first), ``off`` / ``aad_len`` /
    ``length`` uint32-sized ints (int32 tensors), ``iv`` n x 12 and ``tag``
    n x 16 bytes.  Seals in place and writes ``tag``; with ``open`` it checks
    ``tag`` instead: ``result[i]`` (int32) is 1 and the data untouched on a
    mismatch, else 0 and the data deciphered.  Async on ``stream`` like
    :meth:`SRTPEngine.transform_device`; touches none of the engine's state.
    ``wave``: a wave per packet instead of a lane (srtp_aes_gcm_device_ex with
    SRTP_GCM_BATCH_WAVE); the results are the same to the byte."""
    if n is None:
        n = off.numel()
    for t, size, what in ((off, 4, "off"), (aad_len, 4, "aad_len"), (length, 4, "length"),
                          (iv, 1, "iv"), (tag, 1, "tag"), (seg, 1, "seg")) + \
            (((result, 4, "result"),) if result is not None else ()):
        if t.element_size() != size or not t.is_contiguous():
            raise ValueError("%s: a contiguous tensor of %d-byte elements" % (what, size))
    if off.numel() < n or aad_len.numel() < n or length.numel() < n or iv.numel() < 12 * n or \
            tag.numel() < 16 * n or (result is not None and result.numel() < n):
        raise ValueError("an array is shorter than n packets")
    if open and result is None and n:
        raise ValueError("open needs a result tensor")
    sp = getattr(stream, "cuda_stream", stream)
    rc = N.lib().srtp_aes_gcm_device_ex(
        engine.h, int(bool(open)), bytes(key), len(key), seg.data_ptr(), off.data_ptr(), aad_len.data_ptr(),
        length.data_ptr(), iv.data_ptr(), tag.data_ptr(), None if result is None else result.data_ptr(), n,
        N.GCM_BATCH_WAVE if wave else 0, sp)
    N.check(rc, engine.h, "srtp_aes_gcm_device")


def skein512_mac(key: bytes, msg: bytes, out_bits: int = 512) -> bytes:
    """The engine's host Skein-512 (version 1.3): keyed like bccontrib's SkeinMac
    (plain hash for an empty key), out_bits output bits."""
    out = (C.c_uint8 * ((out_bits + 7) // 8))()
    N.check(N.lib().srtp_skein512_mac(bytes(key), len(key), out_bits, bytes(msg), len(msg), out), None,
            "skein512_mac")
    return bytes(out)


def derive_session_keys(masterKey: bytes, masterSalt: bytes, rtcp: bool = False):
    """The engine's host-side RFC 3711 4.3 key derivation (no GPU needed); a
    32-byte master key selects the AES-256 PRF and a 32-byte session key
    (RFC 6188 4.1)."""
    mk = bytes(masterKey)
    klen = 32 if len(mk) >= 32 else 16
    enc, auth, salt = (C.c_uint8 * klen)(), (C.c_uint8 * 20)(), (C.c_uint8 * 14)()
    N.check(N.lib().srtp_derive_session_keys_n(mk[:klen], klen, bytes(masterSalt)[:14], int(rtcp),
                                               enc, auth, salt), None, "kdf")
    return bytes(enc), bytes(auth), bytes(salt)


def pack(pkts: Sequence[Optional[RawPacket]], predicate=None, reverse: bool = False,
         room: int = TRAILER_ROOM):
    """RawPacket[] -> (seg, off, len, cap, flags): the marshalling a JNI shim
    does.  Each packet region is 16-byte aligned and holds the
    packet's buffer bytes from its offset; ``cap`` is the Java buffer's length
    after the offset, so RawPacket.isInvalid and the bounds the reference
    reads against (getHeaderLength's extension field, readRegionToBuff) are the
    same.  For protect, ``cap`` also leaves room for the trailer (the in-place
    form of RawPacket.append / grow), so a packet whose header-extension
    length field lies past its buffer reads the zero padding there instead of
    throwing (the one protect-side difference from the reference's
    AIOOBE); ``room`` is that room, the engine's ``trailer_room``.  ``None`` elements and packets the predicate rejects are flagged
    SKIP (SinglePacketTransformer.java:121-216 never hands them to the
    transformer)."""
    n = len(pkts)
    off = np.zeros(n, np.uint32)
    length = np.zeros(n, np.uint32)
    cap = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint32)
    pos = 0
    for i, p in enumerate(pkts):
        if p is None or (predicate is not None and not predicate(p)):
            flags[i] = N.PKT_FLAG_SKIP
            cap[i] = 16
        else:
            avail = len(p.buffer) - p.offset
            fits = p.length <= avail
            cap[i] = max(avail, p.length + room) if fits and not reverse else max(avail, 0)
            length[i] = p.length
            flags[i] = p.flags & (N.PKT_FLAG_DISCARD | N.PKT_FLAG_SILENCE)
        off[i] = pos
        pos += (int(cap[i]) + 15) & ~15
    seg = np.zeros(max(pos, 16), np.uint8)
    for i, p in enumerate(pkts):
        if p is not None and not (flags[i] & N.PKT_FLAG_SKIP):
            src = np.frombuffer(bytes(p.buffer[p.offset:]), np.uint8)
            seg[off[i]:off[i] + len(src)] = src
    return seg, off, length, cap, flags


class PacketTransformer:
    """transform/PacketTransformer.java:28-53"""

    def close(self):
        raise NotImplementedError

    def transform(self, pkts):
        raise NotImplementedError

    def reverseTransform(self, pkts):
        raise NotImplementedError


_rp_lock = threading.Lock()


def _rp_batch(engine) -> C.c_void_p:
    """The calling thread's srtp_rawpacket_batch on `engine` (an SRTPEngine or
    SRTPDispatcher): the staging of the C marshalling, one per thread as a
    JNI shim keeps one per Java thread."""
    with _rp_lock:
        tl = engine.__dict__.get("_rp_tls")
        if tl is None:
            tl = engine._rp_tls = threading.local()
            engine._rp_all = []
    h = getattr(tl, "h", None)
    if h is None:
        h = C.c_void_p()
        L = N.lib()
        if isinstance(engine, SRTPDispatcher):
            N.check(L.srtp_rawpacket_batch_create_dispatch(engine.h, C.byref(h)), None, "rawpacket")
        else:
            N.check(L.srtp_rawpacket_batch_create(engine.h, C.byref(h)), engine.h, "rawpacket")
        tl.h = h
        with _rp_lock:
            engine._rp_all.append(h)
    return h


def _rp_close_all(engine) -> None:
    agg = engine.__dict__.pop("_pkt_agg", None)
    if agg is not None:
        agg.close()
    with _rp_lock:
        for h in engine.__dict__.get("_rp_all", []):
            N.lib().srtp_rawpacket_batch_destroy(h)
        engine.__dict__["_rp_all"] = []
        engine.__dict__.pop("_rp_tls", None)


def _packet_aggregator(engine) -> "SRTPAggregator":
    """The engine's (or dispatcher's: one lane per shard) aggregator for
    per-packet calls, created on first use -- what the JNI shim keeps one of
    per process."""
    with _rp_lock:
        agg = engine.__dict__.get("_pkt_agg")
        if agg is None:
            agg = engine._pkt_agg = SRTPAggregator(engine, None, max_packets=4096, max_bytes=8 << 20,
                                                   deadline_us=500, depth=4, seal_idle=True)
    return agg


_grow_tls = threading.local()
_GROW = 65536 + 20


def _rawpacket_one(engine, reverse: bool, tid: int, pkt: "RawPacket"):
    """SinglePacketTransformer.transform / reverseTransform(RawPacket)
    (SinglePacketTransformer.java:113,169; SRTPTransformer.java:185-219,
    SRTCPTransformer.java:175-207) through srtp_rawpacket_transform_one: the
    packet joins the bundles of concurrent callers (srtp_aggregator_transform)
    and is written back as the reference leaves it.  Returns the packet or
    None (dropped); raises where the reference throws."""
    g = getattr(_grow_tls, "buf", None)
    if g is None:
        g = _grow_tls.buf = (C.c_uint8 * _GROW)()
    agg = _packet_aggregator(engine)
    buf = pkt.buffer if len(pkt.buffer) else bytearray(1)
    v = (C.c_char * len(buf)).from_buffer(buf)
    length, st, need = C.c_uint32(pkt.length), C.c_int32(), C.c_uint32()
    rc = N.lib().srtp_rawpacket_transform_one(
        agg.h, int(reverse), int(tid), C.addressof(v), len(pkt.buffer), pkt.offset, C.byref(length),
        pkt.flags & (N.PKT_FLAG_DISCARD | N.PKT_FLAG_SILENCE), C.byref(st), C.byref(need), g, _GROW)
    del v
    N.check(rc, None, "srtp_rawpacket_transform_one")
    if need.value:  # the reference's new byte[] (RawPacket.append / grow): the result at offset 0
        nb = bytearray(need.value)
        nb[:length.value] = bytes(g[:length.value])
        pkt.buffer, pkt.offset = nb, 0
    pkt.length = int(length.value)
    s = int(st.value)
    if s == N.STATUS_ERR_MALFORMED:
        raise SRTPTransformException("Failed to transform RawPacket! (malformed for SRTP)")
    return pkt if s == N.STATUS_OK else None


def _rawpacket_run(engine, reverse: bool, tids, pkts, predicate=None):
    """transform / reverseTransform(RawPacket[]) through the C marshalling
    (srtp_rawpacket_transform, libjitsi_amd/csrc/rawpacket.cpp), with what a
    JNI shim does around it: hand over each RawPacket's buffer, offset, length
    and flags; afterwards move a packet the reference gives a new buffer
    (RawPacket.append without room, RawPacket.grow: need_len) to a new buffer
    at offset 0, replace dropped elements with None, and rethrow a throw after
    the whole array was written back (SinglePacketTransformer.java:121-216).
    ``tids`` is one transformer id or one per packet (-1: no transformer)."""
    n = len(pkts)
    L = N.lib()
    bufs = (C.c_void_p * n)()
    buf_len = np.zeros(n, np.uint32)
    offset = np.zeros(n, np.uint32)
    length = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint32)
    views = []
    for i, p in enumerate(pkts):
        if p is None:
            continue
        if predicate is not None and not predicate(p):
            flags[i] = N.PKT_FLAG_SKIP
        else:
            flags[i] = p.flags & (N.PKT_FLAG_DISCARD | N.PKT_FLAG_SILENCE)
        buf = p.buffer if len(p.buffer) else bytearray(1)
        v = (C.c_char * len(buf)).from_buffer(buf)
        views.append(v)
        bufs[i] = C.addressof(v)
        buf_len[i] = len(p.buffer)
        offset[i] = p.offset
        length[i] = p.length
    status = np.zeros(n, np.int32)
    need = np.zeros(n, np.uint32)
    thrown = C.c_int32(-1)
    if np.isscalar(tids):
        tids_p, tid0 = None, int(tids)
    else:
        tids_a = np.ascontiguousarray(tids, np.int32)
        tids_p, tid0 = tids_a.ctypes.data, -1
    b = _rp_batch(engine)
    rc = L.srtp_rawpacket_transform(b, int(reverse), tids_p, tid0, bufs, buf_len.ctypes.data,
                                    offset.ctypes.data, length.ctypes.data, flags.ctypes.data,
                                    status.ctypes.data, need.ctypes.data, n, C.byref(thrown))
    del views
    N.check(rc, None, "srtp_rawpacket_transform")
    for i, p in enumerate(pkts):
        st = int(status[i])
        if p is None or st in (N.STATUS_SKIPPED, N.STATUS_NOT_PROCESSED):
            continue
        if need[i]:  # the reference's new byte[]: the result at offset 0
            data, dl = C.POINTER(C.c_uint8)(), C.c_uint32()
            N.check(L.srtp_rawpacket_result(b, i, C.byref(data), C.byref(dl)), None, "result")
            nb = bytearray(int(need[i]))
            nb[:dl.value] = C.string_at(data, dl.value)
            p.buffer, p.offset = nb, 0
        p.length = int(length[i])
        if st != N.STATUS_OK and st != N.STATUS_ERR_MALFORMED:
            pkts[i] = None
    if thrown.value >= 0:
        raise SRTPTransformException(
            f"Failed to transform RawPacket(s)! (packet {thrown.value}: malformed for SRTP)")
    return pkts


class _SRTPBase(PacketTransformer):
    KIND = N.KIND_RTP

    def __init__(self, forwardFactory: SRTPContextFactory,
                 reverseFactory: Optional[SRTPContextFactory] = None, packetPredicate=None):
        reverseFactory = reverseFactory or forwardFactory
        self.engine = forwardFactory.engine
        self.forwardFactory, self.reverseFactory = forwardFactory, reverseFactory
        self.packetPredicate = packetPredicate
        self.exceptionsInTransform = 0
        self.exceptionsInReverseTransform = 0
        self.tid = self.engine._transformer_create(self.KIND, forwardFactory.fid,
                                                   reverseFactory.fid)

    def _set_factory(self, factory: SRTPContextFactory, forward: bool):
        self.engine._transformer_set_factory(self.tid, factory.fid, forward)
        if forward:
            self.forwardFactory = factory
        else:
            self.reverseFactory = factory

    def close(self):
        self.engine._transformer_close(self.tid)

    def _count_exception(self, reverse):
        if reverse:
            self.exceptionsInReverseTransform += 1
        else:
            self.exceptionsInTransform += 1

    def _run(self, pkts, reverse):
        """RawPacket: SinglePacketTransformer's per-packet transform(RawPacket)
        (coalesced with concurrent callers).  An array of one element: the
        SinglePacketTransformer array loop over that per-packet call -- the
        connectors' 1-element arrays.  Longer arrays: one bundle
        (srtp_rawpacket_transform) with the loop's abort-on-throw."""
        if pkts is None:
            return None
        if isinstance(pkts, RawPacket):
            return _rawpacket_one(self.engine, reverse, self.tid, pkts)
        if len(pkts) == 0:
            return pkts
        if len(pkts) == 1:
            p = pkts[0]
            if p is not None and (self.packetPredicate is None or self.packetPredicate(p)):
                try:
                    pkts[0] = _rawpacket_one(self.engine, reverse, self.tid, p)
                except SRTPTransformException:
                    self._count_exception(reverse)
                    raise
            return pkts
        try:
            return _rawpacket_run(self.engine, reverse, self.tid, pkts, self.packetPredicate)
        except SRTPTransformException:
            self._count_exception(reverse)
            raise

    def transform(self, pkts):
        return self._run(pkts, False)

    def reverseTransform(self, pkts):
        return self._run(pkts, True)


class SRTPTransformer(_SRTPBase):
    """SRTPTransformer(forwardFactory, reverseFactory)"""

    KIND = N.KIND_RTP

    def setContextFactory(self, factory: SRTPContextFactory, forward: bool):
        self._set_factory(factory, forward)


class SRTCPTransformer(_SRTPBase):
    """SRTCPTransformer(forwardFactory, reverseFactory) or SRTCPTransformer(srtpTransformer)"""

    KIND = N.KIND_RTCP

    def __init__(self, forwardFactory, reverseFactory=None):
        if isinstance(forwardFactory, SRTPTransformer):
            t = forwardFactory
            forwardFactory, reverseFactory = t.forwardFactory, t.reverseFactory
        super().__init__(forwardFactory, reverseFactory)

    def updateFactory(self, factory: SRTPContextFactory, forward: bool):
        self._set_factory(factory, forward)


def fan_out(pkts: Sequence[Optional[RawPacket]], transformers: Sequence[_SRTPBase], exclusion=None):
    """One packet to many peers: what OutputDataStreamImpl.doWrite
    (rtp/translator/OutputDataStreamImpl.java:171-243) does with each packet --
    it loops over the streams and hands the same ``buf, off, len`` to each, and
    each stream's connector copies it and runs its own transformer's
    ``transform`` -- for a list of packets and the streams' transformers (all of
    one SRTPEngine), with the copies made on the GPU (srtp_fanout_host): each
    packet crosses to the device once.  Entries are processed in doWrite's
    order, packet by packet and, within a packet, stream by stream, as one
    bundle: toward each transformer the result is that of its
    ``transform(copies of pkts)``, except that a copy on which the reference
    would throw is answered with None instead of an exception (and, on an
    engine with abort_on_error, so are the later copies toward that
    transformer, SinglePacketTransformer.java:121-216).
    ``exclusion``: a transformer, or one (or None) per packet -- the stream the
    packet came from, which doWrite passes over (:193-194).  ``None`` packets
    are written to nobody.  The packets themselves are left as they are.
    Returns one list per transformer: element i is the protected copy of
    packet i as a new RawPacket, or None (not written, dropped, or thrown)."""
    return _fan_out(pkts, transformers, None, exclusion)


def fan_out_rw(pkts: Sequence[Optional[RawPacket]], transformers: Sequence[_SRTPBase], rewriters, exclusion=None):
    """:func:`fan_out` for a bridge whose per-peer send chain rewrites the
    packet in front of SRTP.  In the reference each stream's chain holds
    ptTransformEngine and ssrcRewritingEngine before the SRTP transformer
    (MediaStreamImpl.java:986-1035), and the rewriting engine gives the copy
    its target SSRC, sequence number, timestamp and payload type through
    RawPacket.setSSRC / setSequenceNumber / setTimestamp / setPayloadType
    (ExtendedSequenceNumberInterval.java:163-229, rewriteRTP).  ``rewriters``
    holds one rewriter or None per transformer.  A rewriter is a callable
    ``f(pkt)``; it is called for every copy that would be written toward its
    transformer (not for a None packet, the excluded stream or a copy the
    packetPredicate refuses), in doWrite's order: packet by packet and, within
    a packet, stream by stream -- so a stateful rewriter, such as the
    reference's, works.  It returns None -- the copy is not written
    (rewriteRTP returned null) -- or a mapping with any of ``ssrc``, ``seq``,
    ``timestamp``, ``pt``; an empty mapping leaves the copy unchanged.  The
    values are written into the copies on the GPU (srtp_fanout_host_rw), and
    each copy is protected under its rewritten SSRC and sequence number.  The
    packets themselves are left as they are.  Everything else is
    :func:`fan_out`'s."""
    transformers, rewriters = list(transformers), list(rewriters)
    if len(rewriters) != len(transformers):
        raise ValueError("fan_out_rw: one rewriter (or None) per transformer")
    return _fan_out(pkts, transformers, rewriters, exclusion)


def abs_send_time(ns: int) -> int:
    """AbsSendTimeEngine.setTimestamp's conversion (AbsSendTimeEngine.java:141-152) of a
    time in nanoseconds, ``ns >= 0``, to the 24 bits of abs-send-time: 6.18 fixed-point
    seconds, ``((ns // 1e9) % 64) << 18 | (ns % 1e9) * 2**18 // 1e9``."""
    ns = int(ns)
    if ns < 0:
        raise ValueError("abs_send_time: ns >= 0")
    b = 1000 * 1000 * 1000
    return ((((ns // b) % 64) << 18) | ((ns % b) * (1 << 18) // b)) & 0x00FFFFFF


def fan_out_ast(pkts: Sequence[Optional[RawPacket]], transformers: Sequence[_SRTPBase], rewriters, stampers,
                exclusion=None):
    """:func:`fan_out_rw` for streams that have abs-send-time negotiated.  In
    the reference the last engine in front of a stream's SRTP transformer is
    absSendTimeEngine (MediaStreamImpl.java:1018-1035), whose
    replaceAbsSendTime (AbsSendTimeEngine.java:86-152) walks the copy's one-byte
    header-extension elements and overwrites the three data bytes of the first
    element that carries the stream's abs-send-time ID (if its len field is 2)
    with the local send time.  ``stampers`` holds one stamper or None per
    transformer.  A stamper is a callable ``g(pkt)``, called like a rewriter --
    for every copy that would be written toward its transformer, after that
    transformer's rewriter, in doWrite's order -- that returns None (this copy
    is not stamped) or ``(ext_id, value)``: the stream's extension ID and the
    24-bit time (:func:`abs_send_time`).  The walk and the stamp happen on the
    GPU (srtp_fanout_host_ast), in the copy, before it is protected; a copy
    without such an element leaves unchanged.  ``rewriters`` as in
    :func:`fan_out_rw` (one or None per transformer).  Everything else is
    :func:`fan_out`'s."""
    transformers, rewriters, stampers = list(transformers), list(rewriters), list(stampers)
    if len(rewriters) != len(transformers):
        raise ValueError("fan_out_ast: one rewriter (or None) per transformer")
    if len(stampers) != len(transformers):
        raise ValueError("fan_out_ast: one stamper (or None) per transformer")
    return _fan_out(pkts, transformers, rewriters, exclusion, stampers)


def fec_sn_bytes(sn: int):
    """The two bytes rewriteFEC stores at ``off + 2`` and ``off + 3`` of an FEC
    header for the rewritten SN base ``sn``
    (ExtendedSequenceNumberInterval.java:383-384), **as Java evaluates them**:
    ``(byte) (snRewritenBase & 0xff00 >> 8)`` shifts before it masks, so it is
    ``snRewritenBase & 0xff`` -- both bytes are the low byte of ``sn``, and
    ``fec_sn_bytes(0x1234) == (0x34, 0x34)``.  :func:`fan_out_pay` writes what
    the reference writes; a caller who wants the big-endian number, or any
    other bytes, fills ``N.FANOUT_PAYLOAD_DTYPE`` records and calls
    :meth:`SRTPEngine.fanout_host_pay`: the record carries bytes and has no
    opinion."""
    sn = int(sn)
    return (sn & (0xFF00 >> 8)) & 0xFF, sn & 0x00FF


def fan_out_pay(pkts: Sequence[Optional[RawPacket]], transformers: Sequence[_SRTPBase], rewriters, stampers,
                exclusion=None):
    """:func:`fan_out_ast` for streams that carry RTX or FEC.  Besides the four
    header fields, ExtendedSequenceNumberInterval.rewriteRTP
    (ExtendedSequenceNumberInterval.java:163-229) writes two per-peer values
    into the payload before the SRTP transformer sees the packet, and a
    rewriter's mapping may carry them as two more keys:

    ``osn``: an int, the peer's rewritten number of the original packet.  It is
    written big-endian at ``pkt.getHeaderLength()`` of the source packet:
    rewriteRTX's ``setOriginalSequenceNumber`` (:261-284), which is
    ``writeShort(getHeaderLength(), sn)`` (RawPacket.java:1018-1022, 1334-1337).

    ``fec``: ``(off, sn)``, where ``off`` is the FEC header's offset from the
    packet's first byte (for a RED packet the matching block's, which the
    host's block walk finds).  The bytes at ``off + 2`` and ``off + 3`` become
    :func:`fec_sn_bytes` ``(sn)``: rewriteFEC's two stores (:346-386; rewriteRED,
    :307-333).

    Both may appear together (an FEC packet inside RTX): ``fec`` is written
    first, then ``osn``, rewriteRTP's order.  A header length or offset that
    does not fit 16 bits, or lies below byte 12, raises ``ValueError``.  The
    bytes are written into the copies on the GPU (srtp_fanout_host_pay) before
    they are protected; a byte the copy does not hold is not written.
    Everything else is :func:`fan_out_ast`'s."""
    transformers, rewriters, stampers = list(transformers), list(rewriters), list(stampers)
    if len(rewriters) != len(transformers):
        raise ValueError("fan_out_pay: one rewriter (or None) per transformer")
    if len(stampers) != len(transformers):
        raise ValueError("fan_out_pay: one stamper (or None) per transformer")
    return _fan_out(pkts, transformers, rewriters, exclusion, stampers, payload=True)


RED_OFF, RED_STRIP, RED_WRAP = N.RED_OFF, N.RED_STRIP, N.RED_WRAP


def fan_out_red(pkts: Sequence[Optional[RawPacket]], transformers: Sequence[_SRTPBase], rewriters, stampers, payers,
                reds, exclusion=None):
    """:func:`fan_out_pay` for a bridge whose peers differ in whether they
    negotiated RED (RFC 2198).  ``reds`` holds one ``(mode, red_pt)`` (or None)
    per transformer: ``RED_STRIP`` is REDFilterTransformEngine.transform
    (transform/REDFilterTransformEngine.java:95-145), which takes the one-byte
    RED header out of a single-block packet whose PT is ``red_pt``;
    ``RED_WRAP`` is REDTransformEngine.transform (transform/
    REDTransformEngine.java:151-182), which puts one in and makes ``red_pt`` the
    PT; ``RED_OFF`` or None leaves the peer's copies alone.  A packet on which
    the reference throws is lost for that peer (None), as there.

    ``payers`` holds one callable (or None) per transformer: ``payer(pkt)``
    returns None or a mapping with ``osn`` and / or ``fec``, :func:`fan_out_pay`'s
    two keys, here apart from the header fields so that a peer may have one
    without the other.  RED runs first (MediaStreamImpl.java:993-998): ``osn`` is
    written at the header's end, which RED does not move, and ``fec``'s offset
    counts in the packet RED left.  A rewriter's mapping may still carry both.

    The copies are made, changed and protected on the GPU
    (srtp_fanout_host_red).  Returns ``(out, codes)``: ``out`` as
    :func:`fan_out_pay`'s, ``codes[k][i]`` what RED did to packet i for
    transformer k (0 untouched, 1 stripped, 2 wrapped, -1 dropped)."""
    transformers, rewriters, stampers = list(transformers), list(rewriters), list(stampers)
    payers, reds = list(payers), list(reds)
    if len(rewriters) != len(transformers):
        raise ValueError("fan_out_red: one rewriter (or None) per transformer")
    if len(stampers) != len(transformers):
        raise ValueError("fan_out_red: one stamper (or None) per transformer")
    if len(payers) != len(transformers):
        raise ValueError("fan_out_red: one payer (or None) per transformer")
    if len(reds) != len(transformers):
        raise ValueError("fan_out_red: one (mode, red_pt) (or None) per transformer")
    for x in reds:
        if x is not None and not (int(x[0]) in (RED_OFF, RED_STRIP, RED_WRAP) and 0 <= int(x[1]) <= 127):
            raise ValueError("fan_out_red: a RED record of %r" % (x,))
    return _fan_out(pkts, transformers, rewriters, exclusion, stampers, payload=True, payers=payers, reds=reds)


class FecSender:
    """FECSender's state for one SSRC toward one peer (transform/fec/
    FECSender.java): ``counter`` media packets seen and ``nb_fec`` ulpfec
    packets made, kept across :func:`fan_out_fec` calls; ``rate`` media packets
    to a group (1..16, FECTransformEngine.java:236), ``pt`` the ulpfec payload
    type and ``red_pt`` the RED payload type the packet is wrapped in (None:
    sent plain)."""

    def __init__(self, ssrc: int, rate: int, pt: int, red_pt: Optional[int] = None):
        if not 1 <= int(rate) <= 16:
            raise ValueError("FecSender: a rate of %r" % (rate,))
        if not 0 <= int(pt) <= 127 or (red_pt is not None and not 0 <= int(red_pt) <= 127):
            raise ValueError("FecSender: a payload type above 127")
        self.ssrc, self.rate, self.pt = int(ssrc) & 0xFFFFFFFF, int(rate), int(pt)
        self.red_pt = None if red_pt is None else int(red_pt)
        self.counter = 0
        self.nb_fec = 0


def fan_out_fec(pkts: Sequence[Optional[RawPacket]], transformers: Sequence[_SRTPBase], rewriters, stampers, payers,
                reds, fecs, exclusion=None):
    """:func:`fan_out_red` for peers whose downlink is protected with ulpfec
    (RFC 5109).  ``fecs`` holds one :class:`FecSender` (or None) per
    transformer.  Every version-2 copy toward that transformer whose SSRC, as
    its rewriter left it, is the sender's, is a media packet of the sender: its
    (rewritten) sequence number is shifted by ``nb_fec``
    (FECSender.transformSingle's ``setSequenceNumber(seq + nbFec)``, :132), and
    after every ``rate`` of them an FEC entry follows, made on the GPU
    (srtp_fanout_host_fec, one call) from the copies as all their records left
    them -- FECSender.FECPacket's addMedia and finish (:319-412) over the
    packets the peer gets -- and protected behind them in the same context
    order.  A group still open at the end of the call is closed short; nothing
    is carried between calls but ``counter`` and ``nb_fec``.

    The ``fec`` key of a payer or rewriter keeps its meaning: it patches the SN
    base of an FEC packet that came from elsewhere (:func:`fan_out_pay`); it
    makes none.

    Returns ``(out, codes, fec)``: ``out`` and ``codes`` as
    :func:`fan_out_red`'s, ``fec[k]`` a list of ``(i, RawPacket or None)``: the
    FEC packet sent toward transformer k behind packet i (None where it was
    refused or not protected)."""
    transformers, rewriters, stampers = list(transformers), list(rewriters), list(stampers)
    payers, reds, fecs = list(payers), list(reds), list(fecs)
    for name, x in (("rewriter", rewriters), ("stamper", stampers), ("payer", payers), ("(mode, red_pt)", reds),
                    ("FecSender", fecs)):
        if len(x) != len(transformers):
            raise ValueError("fan_out_fec: one %s (or None) per transformer" % name)
    for x in reds:
        if x is not None and not (int(x[0]) in (RED_OFF, RED_STRIP, RED_WRAP) and 0 <= int(x[1]) <= 127):
            raise ValueError("fan_out_fec: a RED record of %r" % (x,))
    return _fan_out(pkts, transformers, rewriters, exclusion, stampers, payload=True, payers=payers, reds=reds,
                    fecs=fecs)


def _seq_cmp(a: int, b: int) -> int:
    """FECReceiver.seqNumComparator (transform/fec/FECReceiver.java:49-74)."""
    if a == b:
        return 0
    if a > b:
        return 1 if a - b < 32768 else -1
    return -1 if b - a < 32768 else 1


class FecReceiver:
    """FECReceiver's state for one SSRC (transform/fec/FECReceiver.java): the
    media packets (at most 64) and ulpfec packets (at most 32) kept across
    :meth:`reverse_transform` calls as host bytes by sequence number, ``nb_fec``
    ulpfec packets received and ``nb_recovered`` media packets recovered.
    ``ulpfec_pt`` is the ulpfec payload type.  The maps are the reference's
    TreeMaps under seqNumComparator (:49-74): the first key is the oldest of a
    set that spans fewer than 2^15 sequence numbers, as the Java comment
    demands of its input.  Every decision and every XOR is the GPU's
    (:meth:`SRTPEngine.fec_recover_host`, Reconstructor.setFecPacket :472-520
    and recover :527-596); ``engine`` defaults to :meth:`SRTPEngine.default`."""

    MEDIA_BUF_SIZE, FEC_BUF_SIZE = 64, 32  # :114-127

    def __init__(self, ssrc: int, ulpfec_pt: int, engine: Optional["SRTPEngine"] = None):
        if not 0 <= int(ulpfec_pt) <= 127:
            raise ValueError("FecReceiver: a payload type above 127")
        self.ssrc, self.ulpfec_pt = int(ssrc) & 0xFFFFFFFF, int(ulpfec_pt)
        self.engine = engine
        self.nb_fec = 0
        self.nb_recovered = 0
        self.media = {}  # sequence number -> bytes
        self.fec = {}

    @staticmethod
    def _first_key(d):
        return sorted(d, key=functools.cmp_to_key(_seq_cmp))[0]

    def _save_fec(self, data: bytes) -> None:
        """saveFec (:350-356)"""
        if len(self.fec) >= self.FEC_BUF_SIZE:
            del self.fec[self._first_key(self.fec)]
        self.fec[int.from_bytes(data[2:4], "big")] = data

    def _save_media(self, data: bytes) -> None:
        """saveMedia (:364-389)"""
        if len(self.media) >= self.MEDIA_BUF_SIZE:
            del self.media[self._first_key(self.media)]
        self.media[int.from_bytes(data[2:4], "big")] = data

    def _recover(self, keys):
        """One srtp_fec_recover_host call: a record per FEC packet of ``keys``, every kept media packet a
        candidate of each.  Returns (codes, packets)."""
        eng = self.engine if self.engine is not None else SRTPEngine.default()
        packets = list(self.media.values()) + [self.fec[k] for k in keys]
        m = len(self.media)
        up = lambda v: (v + 15) & ~15
        off = np.zeros(len(packets), np.uint32)
        off[1:] = np.cumsum([up(len(p)) for p in packets[:-1]])
        seg = np.zeros(int(off[-1]) + up(len(packets[-1])), np.uint8)
        for o, p in zip(off, packets):
            seg[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
        length = np.array([len(p) for p in packets], np.uint32)
        rec = np.zeros(len(keys), N.FEC_RECOVER_DTYPE)
        for r in range(len(keys)):
            rec[r] = (m + r, 0, self.ssrc, m, 1, 0)
        # a recovered packet is shorter than its FEC packet: the payload lies inside it
        out_cap = np.array([len(self.fec[k]) for k in keys], np.uint32)
        out_off = np.zeros(len(keys), np.uint32)
        out_off[1:] = np.cumsum([up(int(c)) for c in out_cap[:-1]])
        out_seg = np.zeros(int(out_off[-1]) + up(int(out_cap[-1])), np.uint8)
        out_len, out_status, code = eng.fec_recover_host(seg, off, length, length, rec, np.arange(m, dtype=np.int32),
                                                         out_seg, out_off, out_cap)
        got = [bytes(out_seg[int(o):int(o) + int(n)]) if c == N.FECRX_RECOVERED and s == N.STATUS_OK else None
               for o, n, s, c in zip(out_off, out_len, out_status, code)]
        return [int(c) for c in code], got

    def reverse_transform(self, pkts: Sequence[Optional[RawPacket]]):
        """FECReceiver.reverseTransform (:233-319) over packets that have been
        unprotected: ulpfec packets are counted, kept and taken out of the
        list, media packets are kept, and every kept ulpfec packet is asked, in
        sequence order, whether its group is complete (it is dropped), lacks
        exactly one packet (the packet is recovered, kept at once and put into
        the list's first empty slot, or appended) or more (it waits).  The
        reference's order -- a recovered packet is a media packet for the FEC
        packets behind it -- is kept by repeating the call: all pending records
        run at once, the results up to and including the first that recovered
        stand, and the records behind it run again."""
        out = list(pkts)
        for i, pkt in enumerate(out):
            if pkt is None:
                continue
            data = pkt.data()
            if (data[1] & 0x7F) == self.ulpfec_pt:
                self.nb_fec += 1
                out[i] = None
                self._save_fec(data)
            else:
                self._save_media(data)
        pending = sorted(self.fec, key=functools.cmp_to_key(_seq_cmp))
        remove = []
        while pending:
            codes, got = self._recover(pending)
            again = []
            for r, key in enumerate(pending):
                if codes[r] in (N.FECRX_COMPLETE, N.FECRX_PARTIAL, N.FECRX_RECOVERED):
                    remove.append(key)  # packetsToRemove (:274, :280)
                if codes[r] == N.FECRX_RECOVERED and got[r] is not None:
                    self.nb_recovered += 1
                    self._save_media(got[r])
                    rp = RawPacket(got[r], 0, len(got[r]))
                    if None in out:
                        out[out.index(None)] = rp
                    else:
                        out.append(rp)
                    again = pending[r + 1:]
                    break
            pending = again
        for key in remove:
            self.fec.pop(key, None)
        return out


def _fec_entries(pkts, T, flags, rewrite, fecs):
    """The FEC entries of one call: per transformer k with a sender, its media
    entries in order, their sequence numbers shifted in ``rewrite`` (made where
    it is None), a group closed after every ``rate``.  Returns ``(rewrite,
    groups)``, ``groups`` a list of ``(k, i_last, [entry indices])``."""
    groups = []
    for k, snd in enumerate(fecs):
        if snd is None:
            continue
        open_group = []
        for i, p in enumerate(pkts):
            j = i * T + k
            if p is None or flags[j] & N.PKT_FLAG_SKIP or p.length < 12 or (p.readByte(0) >> 6) != 2:
                continue
            rw_on = rewrite is not None
            ssrc = int(rewrite["ssrc"][j]) if rw_on and rewrite["mask"][j] & N.REWRITE_SSRC else p.getSSRC() & 0xFFFFFFFF
            if ssrc != snd.ssrc:
                continue
            if rewrite is None:
                rewrite = np.zeros(len(pkts) * T, N.FANOUT_REWRITE_DTYPE)
            seq = int(rewrite["seq"][j]) if rewrite["mask"][j] & N.REWRITE_SEQ else p.getSequenceNumber()
            rewrite["seq"][j] = (seq + snd.nb_fec) & 0xFFFF
            rewrite["mask"][j] |= N.REWRITE_SEQ
            snd.counter += 1
            open_group.append(j)
            if len(open_group) == snd.rate:
                groups.append((k, i, open_group))
                open_group = []
                snd.nb_fec += 1
        if open_group:  # closed short: nothing is carried between calls
            groups.append((k, open_group[-1] // T, open_group))
            snd.nb_fec += 1
    return rewrite, groups


def _pay_one(pay, j, r, p):
    """Entry j's payload record from the rewriter's mapping r: fec is patch 0, osn patch 1."""
    if "fec" in r:
        off, sn = r["fec"]
        if not 12 <= int(off) <= 0xFFFF - 2:
            raise ValueError("fan_out_pay: an FEC header at offset %r" % (off,))
        pay["at0"][j], pay["b0"][j] = int(off) + 2, fec_sn_bytes(sn)
    if "osn" in r:
        at = int(p.getHeaderLength())
        if not 12 <= at <= 0xFFFF:
            raise ValueError("fan_out_pay: a header length of %d" % at)
        pay["at1"][j], pay["b1"][j] = at, ((int(r["osn"]) >> 8) & 0xFF, int(r["osn"]) & 0xFF)


_REWRITE_FIELDS = (("ssrc", N.REWRITE_SSRC, 0xFFFFFFFF), ("seq", N.REWRITE_SEQ, 0xFFFF),
                   ("timestamp", N.REWRITE_TIMESTAMP, 0xFFFFFFFF), ("pt", N.REWRITE_PT, 0x7F))


def _stamp_one(stamp, j, g, p):
    """Entry j's abs-send-time record from stamper g (the engine behind the rewriter)."""
    if g is None:
        return
    r = g(p)
    if r is None:
        return
    ext_id, value = r
    if not 0 <= int(ext_id) <= 255:
        raise ValueError("fan_out_ast: a stamper returned the ID %r" % (ext_id,))
    stamp["id"][j], stamp["value"][j], stamp["on"][j] = int(ext_id), int(value) & 0x00FFFFFF, 1


def _fan_out(pkts, transformers, rewriters, exclusion, stampers=None, payload=False, payers=None, reds=None,
             fecs=None):
    pkts, transformers = list(pkts), list(transformers)
    out = [[None] * len(pkts) for _ in transformers]
    if not pkts or not transformers:
        codes = [[0] * len(pkts) for _ in transformers]
        return out if reds is None else (out, codes) if fecs is None else (out, codes, [[] for _ in transformers])
    eng = transformers[0].engine
    if not isinstance(eng, SRTPEngine) or any(t.engine is not eng for t in transformers):
        raise ValueError("fan_out: the transformers of one SRTPEngine")
    excl = list(exclusion) if isinstance(exclusion, (list, tuple)) else [exclusion] * len(pkts)
    room = eng.trailer_room
    src_seg, src_off, src_len, src_cap, src_flags = pack(pkts, reverse=True)
    src_status = np.where(src_flags & N.PKT_FLAG_SKIP, N.STATUS_SKIPPED, N.STATUS_OK).astype(np.int32)
    T = len(transformers)
    src_idx = np.repeat(np.arange(len(pkts), dtype=np.int32), T)
    tids = np.tile(np.array([t.tid for t in transformers], np.int32), len(pkts))
    # a copy's buffer holds the packet and the trailer (RawPacket.append / grow)
    cap = np.repeat(np.maximum(src_cap, src_len + room), T).astype(np.uint32)
    if reds is not None:  # a wrapped copy is one byte longer (REDTransformEngine allocates len + 1)
        cap += np.tile(np.array([x is not None and int(x[0]) == RED_WRAP for x in reds], np.uint32), len(pkts))
    flags = np.repeat(src_flags & (N.PKT_FLAG_DISCARD | N.PKT_FLAG_SILENCE), T).astype(np.uint32)
    for i, x in enumerate(excl):
        for k, t in enumerate(transformers):
            if x is t or (t.packetPredicate is not None and pkts[i] is not None
                          and not t.packetPredicate(pkts[i])):
                flags[i * T + k] |= N.PKT_FLAG_SKIP
    rewrite = stamp = pay = None
    if stampers is not None and any(g is not None for g in stampers):
        stamp = np.zeros(len(pkts) * T, N.FANOUT_AST_DTYPE)
    if (rewriters is not None and any(f is not None for f in rewriters)) or stamp is not None:
        if rewriters is not None and any(f is not None for f in rewriters):
            rewrite = np.zeros(len(pkts) * T, N.FANOUT_REWRITE_DTYPE)
            if payload:
                pay = np.zeros(len(pkts) * T, N.FANOUT_PAYLOAD_DTYPE)
        for i, p in enumerate(pkts):  # doWrite's order
            for k in range(T):
                j = i * T + k
                f = rewriters[k] if rewrite is not None else None
                g = stampers[k] if stamp is not None else None
                if p is None or flags[j] & N.PKT_FLAG_SKIP:
                    continue
                if f is None:
                    _stamp_one(stamp, j, g, p)
                    continue
                r = f(p)
                if r is None:
                    flags[j] |= N.PKT_FLAG_SKIP
                    continue
                unknown = set(r) - {name for name, _, _ in _REWRITE_FIELDS} - ({"osn", "fec"} if payload else set())
                if unknown:
                    raise ValueError("fan_out_rw: a rewriter returned %s" % sorted(unknown))
                if payload:
                    _pay_one(pay, j, r, p)
                for name, bit, lim in _REWRITE_FIELDS:
                    if name in r:
                        rewrite[name][j] = int(r[name]) & lim
                        rewrite["mask"][j] |= bit
                _stamp_one(stamp, j, g, p)
    if payers is not None and any(y is not None for y in payers):
        if pay is None:
            pay = np.zeros(len(pkts) * T, N.FANOUT_PAYLOAD_DTYPE)
        for i, p in enumerate(pkts):
            for k in range(T):
                j = i * T + k
                if p is None or flags[j] & N.PKT_FLAG_SKIP or payers[k] is None:
                    continue
                y = payers[k](p)
                if y is None:
                    continue
                if set(y) - {"osn", "fec"}:
                    raise ValueError("fan_out_red: a payer returned %s" % sorted(set(y) - {"osn", "fec"}))
                _pay_one(pay, j, y, p)
    n0, fec, members, groups = len(pkts) * T, None, None, []
    if fecs is not None:
        rewrite, groups = _fec_entries(pkts, T, flags, rewrite, fecs)
    if groups:  # the FEC entries stand behind the media entries: no source, the peer's transformer, room for
        g = len(groups)  # the 26 (27) header bytes less the 12 that are no payload
        grow = lambda a, dt: None if a is None else np.concatenate((a, np.zeros(g, dt)))
        rewrite, stamp, pay = (grow(rewrite, N.FANOUT_REWRITE_DTYPE), grow(stamp, N.FANOUT_AST_DTYPE),
                               grow(pay, N.FANOUT_PAYLOAD_DTYPE))
        fec = np.zeros(n0 + g, N.FANOUT_FEC_DTYPE)
        members = np.array([j for _, _, js in groups for j in js], np.int32)
        first = 0
        for x, (k, _, js) in enumerate(groups):
            snd = fecs[k]
            fec[n0 + x] = (first, snd.ssrc, len(js), snd.pt, snd.red_pt or 0,
                           N.FEC_PLAIN if snd.red_pt is None else N.FEC_RED)
            first += len(js)
        cap = np.concatenate((cap, [int(cap[js].max()) + 15 for _, _, js in groups])).astype(np.uint32)
        src_idx = np.concatenate((src_idx, np.full(g, -1, np.int32)))
        tids = np.concatenate((tids, [transformers[k].tid for k, _, _ in groups])).astype(np.int32)
        flags = np.concatenate((flags, np.zeros(g, np.uint32)))
    step = (cap.astype(np.int64) + 15) & ~15
    off = np.concatenate(([0], np.cumsum(step)[:-1])).astype(np.int64)
    if int(off[-1] + step[-1]) >= 1 << 32:
        raise ValueError("fan_out: more than 4 GiB of copies")
    seg = np.zeros(int(off[-1] + step[-1]), np.uint8)
    if pay is not None and not (pay["at0"].any() or pay["at1"].any()):
        pay = None  # no rewriter named a payload value: fan_out_ast's call
    codes = None
    if fecs is not None:
        red = None
        if any(x is not None and int(x[0]) != RED_OFF for x in reds):
            red = np.zeros(len(cap), N.FANOUT_RED_DTYPE)
            for k, x in enumerate(reds):
                if x is not None:
                    red["mode"][k:n0:T], red["red_pt"][k:n0:T] = int(x[0]), int(x[1])
        ln, st, ro, fo = eng.fanout_host_fec(tids, src_seg, src_off, src_len, src_cap, src_idx, seg,
                                             off.astype(np.uint32), cap, src_status, flags, rewrite, stamp, pay, red,
                                             fec, members)
        codes = [[int(ro[i * T + k]) for i in range(len(pkts))] for k in range(T)]
    elif reds is None:
        ln, st = eng.fanout_host_pay(tids, src_seg, src_off, src_len, src_cap, src_idx, seg, off.astype(np.uint32),
                                     cap, src_status, flags, rewrite, stamp, pay)
    else:
        red = None
        if any(x is not None and int(x[0]) != RED_OFF for x in reds):
            red = np.zeros(len(pkts) * T, N.FANOUT_RED_DTYPE)
            for k, x in enumerate(reds):
                if x is not None:
                    red["mode"][k::T], red["red_pt"][k::T] = int(x[0]), int(x[1])
        ln, st, ro = eng.fanout_host_red(tids, src_seg, src_off, src_len, src_cap, src_idx, seg,
                                         off.astype(np.uint32), cap, src_status, flags, rewrite, stamp, pay, red)
        codes = [[int(ro[i * T + k]) for i in range(len(pkts))] for k in range(T)]
    for j in np.nonzero(st[:n0] == N.STATUS_OK)[0]:
        i, k = divmod(int(j), T)
        o = int(off[j])
        out[k][i] = RawPacket(seg[o:o + int(ln[j])].tobytes(), 0, int(ln[j]), pkts[i].flags)
    if fecs is not None:
        made = [[] for _ in transformers]
        for x, (k, i, _) in enumerate(groups):
            j, o = n0 + x, int(off[n0 + x])
            ok = st[j] == N.STATUS_OK and fo[j] == N.FEC_MADE
            made[k].append((i, RawPacket(seg[o:o + int(ln[j])].tobytes(), 0, int(ln[j]), 0) if ok else None))
        return out, codes, made
    return out if reds is None else (out, codes)


def audio_level_job(pkt: bytes, length: int, cap: int, flags: int, ext_id: int):
    """srtp_audio_level_job: the rule k_audio_level compiles
    (libjitsi_amd/csrc/audio_level_job.h), on the host, over ``pkt``.  Returns
    ``(level, flags_out)``."""
    lv, fo = C.c_int8(), C.c_uint32()
    buf = bytes(pkt)
    N.check(N.lib().srtp_audio_level_job(buf, length, cap, flags, ext_id, C.byref(lv), C.byref(fo)), None,
            "srtp_audio_level_job")
    return lv.value, fo.value


def reverse_transform_levels(pkts, transformer: _SRTPBase, ext_id: int):
    """SsrcTransformEngine.reverseTransform (SsrcTransformEngine.java:226-274,
    dropMutedAudioSourceInReverseTransform false) and the stream's SRTP
    ``reverseTransform`` behind it (MediaStreamImpl.java:1037-1044) over the
    list ``pkts`` of RawPacket, in one bundle on the GPU
    (srtp_transform_host_lvl).  ``ext_id`` is the negotiated ssrc-audio-level
    extension ID (a Java byte: 1..127 is on).  As ``reverseTransform`` does, it
    works on the list in place: accepted packets are unprotected in their
    buffers, dropped ones become None, and a packet from a muted source (level
    127) gets ``FLAG_SILENCE`` in ``pkt.flags``, as the reference sets it, and
    is authenticated but not deciphered.  Returns, per packet, the ``(ssrc,
    127 - level, timestamp)`` tuple the reference hands to
    CsrcAudioLevelDispatcher.addLevels, or None where the level is negative
    (no such extension, or the packet was not read).  The level is reported
    whatever the packet's later SRTP status: the reference also dispatches it
    before authentication."""
    levels = [None] * len(pkts)
    if not len(pkts):
        return levels
    eng = transformer.engine
    if not isinstance(eng, SRTPEngine):
        raise ValueError("reverse_transform_levels: a transformer of an SRTPEngine")
    seg, off, length, cap, flags = pack(pkts, transformer.packetPredicate, reverse=True)
    status, level = eng.transform_host_lvl(transformer.tid, seg, off, length, cap, flags, None, int(ext_id) & 0xFF)
    thrown = -1
    for i, p in enumerate(pkts):
        st = int(status[i])
        if p is None or st == N.STATUS_SKIPPED:
            continue
        lv = int(level[i])
        if lv >= 0:  # at least the fixed header is there (audio_level_wanted)
            levels[i] = (p.readInt(8), 127 - lv, p.readInt(4))
        if lv == N.AUDIO_LEVEL_MUTED:
            p.flags |= N.PKT_FLAG_SILENCE
        if st == N.STATUS_NOT_PROCESSED:
            continue
        if st == N.STATUS_OK:
            o, nl = int(off[i]), int(length[i])
            p.buffer[p.offset:p.offset + nl] = seg[o:o + nl].tobytes()
            p.length = nl
        elif st == N.STATUS_ERR_MALFORMED:
            thrown = i if thrown < 0 else thrown
        else:
            pkts[i] = None
    if thrown >= 0:
        transformer._count_exception(True)
        raise SRTPTransformException(
            f"Failed to transform RawPacket(s)! (packet {thrown}: malformed for SRTP)")
    return levels


def transform_bundle(transformers: Sequence[Optional[_SRTPBase]], pkts, reverse: bool):
    """Process packets of many transformers in one GPU bundle (the batching the
    reference's 1-element arrays cannot express).  Equivalent to calling each
    transformer's transform()/reverseTransform() on its packets in order; a
    throw aborts the later packets of that transformer only, and is raised
    once every packet was written back."""
    eng = next(t for t in transformers if t is not None).engine
    pkts = list(pkts)
    masked = [p if t is not None else None for p, t in zip(pkts, transformers)]
    tids = np.array([t.tid if t is not None else -1 for t in transformers], np.int32)
    out = _rawpacket_run(eng, reverse, tids, masked)
    return [o if t is not None else p for o, p, t in zip(out, pkts, transformers)]
