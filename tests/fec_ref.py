"""FECSender.FECPacket (transform/fec/FECSender.java:243-413) restated line by
line over Python bytearrays, and the receiver's side of RFC 5109 (section 9.2)
to show that what it makes recovers a lost packet.

``make(members, ssrc, pt, red_pt=None)`` is ``new FECPacket(ssrc, pt)``,
``addMedia`` on every member in order and ``finish()``; with ``red_pt`` the
result then goes through REDTransformEngine.transform (transform/
REDTransformEngine.java:151-182) as the chain has it (MediaStreamImpl.java:
988-996).  The restatement keeps what the Java does: "payload" is everything
behind the fixed 12 bytes, byte 12 is the plain XOR of the members' first bytes
(with an odd count the E bit comes out set), and the mask takes the members to
be consecutive."""

INITIAL_BUFFER_SIZE = 1500  # FECTransformEngine.INITIAL_BUFFER_SIZE
RTP_HDR_LEN, FEC_HDR_LEN = 12, 14


class FECPacket:
    def __init__(self, ssrc, payload_type):
        self.buf = bytearray(INITIAL_BUFFER_SIZE)
        self.length = INITIAL_BUFFER_SIZE
        self.ssrc, self.payload_type = ssrc, payload_type
        self.base, self.num_packets, self.protection_length = -1, 0, -1
        self.last_added_seq, self.last_added_ts = -1, -1

    def add_media(self, media):  # :319-380
        media = bytes(media)
        media_payload_len = len(media) - 12
        if len(self.buf) < media_payload_len + RTP_HDR_LEN + FEC_HDR_LEN:
            self.buf += bytes(media_payload_len + RTP_HDR_LEN + FEC_HDR_LEN - len(self.buf))
        buf = self.buf
        if self.base == -1:
            self.base = int.from_bytes(media[2:4], "big")
            buf[RTP_HDR_LEN:RTP_HDR_LEN + 8] = media[:8]
            buf[RTP_HDR_LEN + 8] = media_payload_len >> 8 & 0xFF
            buf[RTP_HDR_LEN + 9] = media_payload_len & 0xFF
            buf[RTP_HDR_LEN + FEC_HDR_LEN:RTP_HDR_LEN + FEC_HDR_LEN + media_payload_len] = media[12:]
        else:
            for i in range(8):
                buf[RTP_HDR_LEN + i] ^= media[i]
            buf[RTP_HDR_LEN + 8] ^= media_payload_len >> 8 & 0xFF
            buf[RTP_HDR_LEN + 9] ^= media_payload_len & 0xFF
            for i in range(media_payload_len):
                buf[RTP_HDR_LEN + FEC_HDR_LEN + i] ^= media[RTP_HDR_LEN + i]
        self.last_added_seq = int.from_bytes(media[2:4], "big")
        self.last_added_ts = int.from_bytes(media[4:8], "big")
        if media_payload_len > self.protection_length:
            self.protection_length = media_payload_len
        self.num_packets += 1

    def finish(self):  # :387-412
        buf = self.buf
        buf[0] = 0x80
        buf[1] = (buf[1] & 0x80) | (self.payload_type & 0x7F)                # setPayloadType
        buf[2:4] = ((self.last_added_seq + 1) & 0xFFFF).to_bytes(2, "big")   # setSequenceNumber: two writeByte
        buf[8:12] = (self.ssrc & 0xFFFFFFFF).to_bytes(4, "big")              # setSSRC
        buf[4:8] = (self.last_added_ts & 0xFFFFFFFF).to_bytes(4, "big")      # setTimestamp
        buf[RTP_HDR_LEN + 2] = self.base >> 8 & 0xFF
        buf[RTP_HDR_LEN + 3] = self.base & 0xFF
        buf[RTP_HDR_LEN + 10] = self.protection_length >> 8 & 0xFF
        buf[RTP_HDR_LEN + 11] = self.protection_length & 0xFF
        mask = ((1 << self.num_packets) - 1) << (16 - self.num_packets)
        buf[RTP_HDR_LEN + 12] = mask >> 8 & 0xFF
        buf[RTP_HDR_LEN + 13] = mask & 0xFF
        self.length = RTP_HDR_LEN + FEC_HDR_LEN + self.protection_length
        return bytes(buf[:self.length])


def red_wrap(pkt, red_pt):
    """REDTransformEngine.transform on a version-2 packet without CSRCs or extension (header length 12)."""
    assert pkt[0] == 0x80
    new = bytearray(len(pkt) + 1)
    new[:12] = pkt[:12]
    new[13:] = pkt[12:]
    new[12] = pkt[1] & 0x7F
    new[1] = (new[1] & 0x80) | (red_pt & 0x7F)
    return bytes(new)


def make(members, ssrc, pt, red_pt=None):
    assert 1 <= len(members) <= 16 and all(len(m) >= 12 for m in members)
    f = FECPacket(ssrc, pt)
    for m in members:
        f.add_media(m)
    out = f.finish()
    return out if red_pt is None else red_wrap(out, red_pt)


def recover(fec, others):
    """RFC 5109 section 9.2 for one level and the short mask: the media packet
    of the group that is not among ``others``, from the (plain) FEC packet and
    the group's other packets.  The SSRC is the FEC packet's (the sender gives
    both the same one)."""
    fh, level = fec[12:22], fec[22:26]
    base, plen = int.from_bytes(fh[2:4], "big"), int.from_bytes(level[0:2], "big")
    mask = int.from_bytes(level[2:4], "big")
    group = [(base + i) & 0xFFFF for i in range(16) if mask & (0x8000 >> i)]
    have = {int.from_bytes(o[2:4], "big") for o in others}
    missing = [s for s in group if s not in have]
    assert len(missing) == 1 and len(have) == len(group) - 1, (group, sorted(have))
    bits = bytearray(fh[0:2] + fh[4:8] + fh[8:10])  # the 80-bit recovery string less the SN base
    for o in others:
        for i, b in enumerate(o[0:2] + o[4:8] + (len(o) - 12).to_bytes(2, "big")):
            bits[i] ^= b
    length = int.from_bytes(bits[6:8], "big")
    payload = bytearray(fec[26:26 + plen]) + bytearray(max(length - plen, 0))
    for o in others:
        for i, b in enumerate(o[12:12 + len(payload)]):
            payload[i] ^= b
    head = bytes([0x80 | (bits[0] & 0x3F), bits[1]]) + missing[0].to_bytes(2, "big") + bytes(bits[2:6]) + fec[8:12]
    return head + bytes(payload[:length])
