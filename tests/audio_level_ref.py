"""SsrcTransformEngine.reverseTransform (SsrcTransformEngine.java:226-274, with
dropMutedAudioSourceInReverseTransform false, the default) restated in Python
over a bytearray that is exactly the packet, with Java's signed bytes and int
arithmetic, through the RawPacket methods it calls: extractSsrcAudioLevel
(RawPacket.java:305-318), getCsrcAudioLevel (:419-443), findExtension (:331-394),
getExtensionHeaderLength (:504-524), getExtensionLength (:544-556) and
getLengthForExtension (:640-648).  Where the reference has no defined answer the
answer here is "none", as libjitsi_amd/csrc/audio_level_job.h defines it: an
index past the packet (Java throws, or reads a larger buffer's stale bytes; here
an IndexError), and a two-byte-form element that is not the match and whose
length byte is negative (Java's offset walks backwards).  Shared by the
audio-level tests; it knows nothing of the engine."""

NONE = -128   # Byte.MIN_VALUE
MUTED = 127
FLAG_SILENCE = 0x4
FLAG_SKIP = 0x80000000


def sbyte(b):
    """A byte as Java reads it from a byte[]."""
    return b - 256 if b >= 128 else b


class _Backwards(Exception):
    pass


class Packet:
    """The RawPacket methods, offset 0, buffer = exactly the packet."""

    def __init__(self, buf):
        self.buffer = buf

    def b(self, i):
        if i < 0:
            raise IndexError(i)  # Java has no negative indices
        return sbyte(self.buffer[i])

    def getVersion(self):
        return (self.b(0) & 0xC0) >> 6

    def getExtensionBit(self):
        return (self.b(0) & 0x10) == 0x10

    def getCsrcCount(self):
        return self.b(0) & 0x0F

    def getExtensionLength(self):
        if not self.getExtensionBit():
            return 0
        i = 12 + self.getCsrcCount() * 4 + 2
        return ((self.b(i) << 8) | (self.b(i + 1) & 0xFF)) * 4

    def getExtensionHeaderLength(self):
        if not self.getExtensionBit():
            return -1
        i = 12 + self.getCsrcCount() * 4
        if self.b(i) == sbyte(0xBE) and self.b(i + 1) == sbyte(0xDE):
            return 1
        if self.b(i) == 0x10 and (self.b(i + 1) >> 4) == 0:
            return 2
        return -1

    def findExtension(self, extensionID):
        if not self.getExtensionBit() or self.getExtensionLength() == 0:
            return 0
        extOffset = 12 + self.getCsrcCount() * 4 + 4
        extensionEnd = extOffset + self.getExtensionLength()
        extHdrLen = self.getExtensionHeaderLength()
        if extHdrLen != 1 and extHdrLen != 2:
            return -1
        while extOffset < extensionEnd:
            if extHdrLen == 1:
                currType = self.b(extOffset) >> 4
                currLen = (self.b(extOffset) & 0x0F) + 1
                extOffset += 1
            else:
                currType = self.b(extOffset)
                currLen = self.b(extOffset + 1)
                extOffset += 2
            if currType == extensionID:
                return extOffset
            if currLen < 0:
                raise _Backwards()  # the defined deviation: the walk ends
            extOffset += currLen
        return -1

    def getLengthForExtension(self, contentStart):
        if self.getExtensionHeaderLength() == 1:
            return (self.b(contentStart - 1) & 0x0F) + 1
        return self.b(contentStart - 1)

    def getCsrcAudioLevel(self, csrcExtID, index, defaultValue):
        level = defaultValue
        if self.getExtensionBit() and self.getExtensionLength() != 0:
            levelsStart = self.findExtension(csrcExtID)
            if levelsStart != -1:
                levelsCount = self.getLengthForExtension(levelsStart)
                if levelsCount < index:
                    pass
                else:
                    level = sbyte(0x7F & self.b(levelsStart + index))
        return level

    def extractSsrcAudioLevel(self, ssrcExtID):
        return self.getCsrcAudioLevel(ssrcExtID, 0, NONE)


def extract(buf, ext_id):
    """extractSsrcAudioLevel over the bytes `buf` for the Java byte `ext_id`; none where Java has no answer."""
    try:
        return Packet(buf).extractSsrcAudioLevel(ext_id)
    except (IndexError, _Backwards):
        return NONE


def reverse_transform(buf, length, cap, flags, ext_id):
    """(level, flags) of one entry: buf the region's bytes, `length` the packet's, `cap` the buffer's after
    the offset, ext_id the record's byte 0..255 (a Java byte: >= 128 is negative, off)."""
    level = NONE
    jid = sbyte(ext_id & 0xFF)
    invalid = length < 12 or length > cap  # RawPacket.isInvalid, offset 0
    if not flags & FLAG_SKIP and jid > 0 and not invalid:
        pkt = bytearray(buf[:length])
        if Packet(pkt).getVersion() == 2:
            level = extract(pkt, jid)
            if level == MUTED:
                flags |= FLAG_SILENCE
    return level, flags


# ---- packets
def one_byte_body(elements):
    """(id, data) elements in the one-byte form; a bare int n is n padding bytes; padded to a word."""
    out = bytearray()
    for e in elements:
        if isinstance(e, int):
            out += bytes(e)
        else:
            eid, data = e
            out += bytes([((eid & 15) << 4) | (len(data) - 1)]) + bytes(data)
    out += bytes(-len(out) % 4)
    return bytes(out)


def two_byte_body(elements):
    """(id, data) or (id, data, length_byte) elements in the two-byte form; a bare int n is n padding bytes."""
    out = bytearray()
    for e in elements:
        if isinstance(e, int):
            out += bytes(e)
        else:
            eid, data = e[0], e[1]
            out += bytes([eid & 0xFF, e[2] if len(e) > 2 else len(data)]) + bytes(data)
    out += bytes(-len(out) % 4)
    return bytes(out)


def rtp(ssrc, seq, body, payload, cc=0, profile=0xBEDE, words=None, b0=None, pt=111, ts=0x01020304):
    """An RTP packet: fixed header, cc CSRCs, then (X set) the profile word, the length word and body."""
    if words is None:
        words = len(body) // 4
    first = (0x90 | cc) if b0 is None else b0
    hdr = bytes([first, pt]) + (seq & 0xFFFF).to_bytes(2, "big") + ts.to_bytes(4, "big") + ssrc.to_bytes(4, "big")
    csrc = b"".join((0xC0000000 + k).to_bytes(4, "big") for k in range(first & 15))
    ext = profile.to_bytes(2, "big") + (words & 0xFFFF).to_bytes(2, "big") + bytes(body) if first & 0x10 else b""
    return hdr + csrc + ext + bytes(payload)


def header_shapes(ext_id=1, level=0x7F):
    """[(name, build(ssrc, seq, payload) -> packet, wild)]: the header shapes the audio-level tests share, the
    element under `ext_id` with data byte `level`.  wild: the header claims what the packet does not hold, or
    is no RTP header at all (such a packet may throw in SRTP; the tests keep those apart)."""
    e, lv, hi = ext_id & 15, bytes([level]), ext_id & 0x7F
    other, long_ = (5, b"\x50\x51\x52"), (6, bytes(range(0x60, 0x70)))
    ob, tb = one_byte_body, two_byte_body
    out = [
        ("no_x", lambda s, q, p: rtp(s, q, b"", p, b0=0x80), False),
        ("x_zero_words", lambda s, q, p: rtp(s, q, b"", p, words=0), False),
        ("negative_words", lambda s, q, p: rtp(s, q, ob([(e, lv)]), p, words=0xFFFF), True),
        ("first", lambda s, q, p: rtp(s, q, ob([(e, lv), other]), p), False),
        ("second", lambda s, q, p: rtp(s, q, ob([other, (e, lv)]), p), False),
        ("last", lambda s, q, p: rtp(s, q, ob([other, long_, (e, lv)]), p), False),
        ("never_8_15", lambda s, q, p: rtp(s, q, ob([(8 | e, lv), (15, lv)]), p), False),
        ("pad1_swallows", lambda s, q, p: rtp(s, q, ob([1, (e, lv), (e, b"\x0A")]), p), False),
        ("pad2", lambda s, q, p: rtp(s, q, ob([2, (e, lv)]), p), False),
        ("v_bit", lambda s, q, p: rtp(s, q, ob([(e, bytes([level | 0x80]))]), p), False),
        ("two_byte", lambda s, q, p: rtp(s, q, tb([(20, b"abc"), (hi, lv)]), p, profile=0x1000), False),
        ("two_byte_high_id", lambda s, q, p: rtp(s, q, tb([(200, b"a"), (hi, lv)]), p, profile=0x100F), False),
        ("two_byte_other_80", lambda s, q, p: rtp(s, q, tb([(20, b"ab", 0xFE), (hi, lv)]), p, profile=0x1000), False),
        ("two_byte_match_80", lambda s, q, p: rtp(s, q, tb([(hi, lv, 0x80)]), p, profile=0x1000), False),
        ("profile_neither", lambda s, q, p: rtp(s, q, ob([(e, lv)]), p, profile=0x1010), False),
        ("cc1", lambda s, q, p: rtp(s, q, ob([other, (e, lv)]), p, cc=1), False),
        ("cc15", lambda s, q, p: rtp(s, q, ob([other, (e, lv)]), p, cc=15), False),        # the element past byte 64
        ("cc15_two_byte", lambda s, q, p: rtp(s, q, tb([(20, b"abc"), (hi, lv)]), p, cc=15, profile=0x1000), False),
        ("cc11_crosses_64", lambda s, q, p: rtp(s, q, ob([other, (e, lv)]), p, cc=11), False),  # element byte 64
        ("data_at_len", lambda s, q, p: rtp(s, q, ob([3]) + bytes([e << 4]), b"", words=2), True),
        ("words_past_end", lambda s, q, p: rtp(s, q, ob([other]), b"", words=40), True),
        ("version_1", lambda s, q, p: rtp(s, q, ob([(e, lv)]), p, b0=0x50), True),
        ("short", lambda s, q, p: rtp(s, q, b"", b"", b0=0x80)[:8], True),
    ]
    return out
