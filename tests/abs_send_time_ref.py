"""AbsSendTimeEngine.transform / replaceAbsSendTime (AbsSendTimeEngine.java:46-130)
restated in Python over a bytearray that is exactly the packet -- the reference's
buf.length for a RawPacket whose buffer holds the packet and nothing else, which is
what the connector's copy is -- with Java's signed bytes and int arithmetic.  The
three bytes are the low 24 bits of `value`, big-endian, as setTimestamp writes its
own (:141-152).  Shared by the fan-out stamp tests; it knows nothing of the engine."""


def sbyte(b):
    """A byte as Java reads it from a byte[]."""
    return b - 256 if b >= 128 else b


def find(buf, ext_id):
    """The offset of the first byte replaceAbsSendTime would overwrite in `buf`
    for the extension ID `ext_id` (an int, as the reference's; -1 disables), or -1."""
    B = len(buf)
    if ext_id == -1 or B < 12:
        return -1
    if (buf[0] & 0xC0) >> 6 != 2 or not buf[0] & 0x10:  # getVersion() == RTPHeader.VERSION, getExtensionBit()
        return -1
    p = 12 + 4 * (buf[0] & 0x0F) + 2
    if p + 1 < B:
        lw = (sbyte(buf[p]) << 8) | sbyte(buf[p + 1])  # Python's ints shift and or as Java's do here
        nbytes = 4 * (1 + lw)
        p += 2
        inner = 0
        while p < B and inner < nbytes:
            eid = (buf[p] & 0xF0) >> 4
            ln = buf[p] & 0x0F
            if eid == ext_id:
                return p + 1 if ln == 2 and p + 3 < B else -1
            inner += 1 + ln + 1
            p += 1 + ln + 1
    return -1


def stamp(buf, ext_id, value):
    """replaceAbsSendTime on the bytearray `buf`; returns the offset stamped, or -1."""
    at = find(buf, ext_id)
    if at >= 0:
        buf[at] = (value >> 16) & 0xFF
        buf[at + 1] = (value >> 8) & 0xFF
        buf[at + 2] = value & 0xFF
    return at


def apply(buf, rec):
    """A record (value, id, on[, reserved]) as srtp_fanout_abs_send_time means it:
    off, or an ID no nibble equals, is the reference's engine disabled."""
    value, ext_id, on = int(rec[0]), int(rec[1]), int(rec[2])
    if not on or ext_id > 15:
        return -1
    return stamp(buf, ext_id, value & 0x00FFFFFF)


def one_byte_ext(elements, pad_to_word=True):
    """The body of a one-byte-header extension from (id, data) elements; a bare int n is n padding bytes."""
    out = bytearray()
    for e in elements:
        if isinstance(e, int):
            out += bytes(e)
        else:
            eid, data = e
            assert 1 <= len(data) <= 16
            out += bytes([(eid << 4) | (len(data) - 1)]) + bytes(data)
    while pad_to_word and len(out) % 4:
        out.append(0)
    return bytes(out)


def filler(front, eid=5):
    """Elements of ID eid that take `front` bytes in all (0, or 2 and more)."""
    assert front == 0 or front >= 2
    out = []
    while front:
        k = 17 if front >= 19 else 16 if front == 18 else front
        out.append((eid, bytes(range(0x40, 0x40 + k - 1))))
        front -= k
    return out


def low_words(body):
    """The body padded until its word count's low byte is below 0x80 (no byte of the length sign-extends)."""
    while (len(body) // 4) & 0xFF >= 0x80:
        body += bytes(4)
    return body


def rtp_ext(ssrc, seq, body, payload, cc=0, profile=0xBEDE, words=None, pt=96, ts=0x01020304, b0=None):
    """An RTP packet with X set: fixed header, cc CSRCs, the profile word, the
    length (words; by default the body's) and body, then the payload."""
    if words is None:
        assert len(body) % 4 == 0
        words = len(body) // 4
    first = (0x90 | cc) if b0 is None else b0
    hdr = bytes([first, pt]) + seq.to_bytes(2, "big") + ts.to_bytes(4, "big") + ssrc.to_bytes(4, "big")
    csrc = b"".join((0xC0000000 + k).to_bytes(4, "big") for k in range(cc))
    return hdr + csrc + profile.to_bytes(2, "big") + (words & 0xFFFF).to_bytes(2, "big") + bytes(body) + bytes(payload)
