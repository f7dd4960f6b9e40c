"""The reference's two RED (RFC 2198) engines of the send chain, restated in
Python from the Java source, statement by statement, over a Java-like byte
array that throws on an index outside it:

  strip  REDFilterTransformEngine.transform (transform/
         REDFilterTransformEngine.java:95-145) behind RTPPacketPredicate
         (AbstractRTPPacketPredicate.test, :53-97), over
         REDBlockIterator.getPrimaryBlock / isMultiBlock / initialize / next
         (codec/REDBlockIterator.java:118-318)
  wrap   REDTransformEngine.transform (transform/REDTransformEngine.java:151-182)
  both   RawPacket.getHeaderLength / getExtensionLength (RawPacket.java:602-614,
         544-556), getPayloadType (:760-763), setPayloadType (:1240-1247)

The packet is a RawPacket over a buffer that ends with its bytes (offset 0,
length = buffer.length), the convention of the fan-out rules.  An exception
leaves SinglePacketTransformer.transform (:194-210): the packet is lost.

``apply(buf, rec)`` -> ``(result, new_bytes)``: rec is ``(mode, red_pt)``;
result 0 untouched, 1 stripped, 2 wrapped, -1 dropped (new_bytes None)."""

OFF, STRIP, WRAP = 0, 1, 2


class JavaThrow(Exception):
    """ArrayIndexOutOfBoundsException / IndexOutOfBoundsException"""


def sbyte(v):
    v &= 0xFF
    return v - 256 if v >= 128 else v


class Buf:
    """byte[]: signed elements, bounds-checked"""

    def __init__(self, data):
        self.b = bytearray(data)

    def __len__(self):
        return len(self.b)

    def __getitem__(self, i):
        if not 0 <= i < len(self.b):
            raise JavaThrow("index %d of %d" % (i, len(self.b)))
        return sbyte(self.b[i])

    def __setitem__(self, i, v):
        if not 0 <= i < len(self.b):
            raise JavaThrow("index %d of %d" % (i, len(self.b)))
        self.b[i] = v & 0xFF


def arraycopy(src, src_pos, dst, dst_pos, length):
    if src_pos < 0 or dst_pos < 0 or length < 0 or src_pos + length > len(src) or dst_pos + length > len(dst):
        raise JavaThrow("arraycopy")
    dst.b[dst_pos:dst_pos + length] = bytes(src.b[src_pos:src_pos + length])


class Pkt:
    def __init__(self, data):
        self.buffer, self.offset, self.length = Buf(data), 0, len(data)

    def version(self):
        return ((self.buffer[self.offset] & 0xC0) & 0xFFFFFFFF) >> 6

    def extension_bit(self):
        return (self.buffer[self.offset] & 0x10) == 0x10

    def csrc_count(self):
        return self.buffer[self.offset] & 0x0F

    def extension_length(self):  # RawPacket.java:544-556
        if not self.extension_bit():
            return 0
        i = self.offset + 12 + self.csrc_count() * 4 + 2
        return ((self.buffer[i] << 8) | (self.buffer[i + 1] & 0xFF)) * 4

    def header_length(self):  # :602-614
        h = 12 + 4 * self.csrc_count()
        if self.extension_bit():
            h += 4 + self.extension_length()
        return h

    def payload_type(self):  # :760-763
        return sbyte(self.buffer[self.offset + 1] & 0x7F)

    def set_payload_type(self, pt):  # :1240-1247
        pt = sbyte(pt) & 0x7F
        self.buffer[self.offset + 1] = (self.buffer[self.offset + 1] & 0x80) | pt

    def bytes(self):
        return bytes(self.buffer.b[self.offset:self.offset + self.length])


def rtp_predicate(pkt):  # AbstractRTPPacketPredicate.test with rtcp == false
    if pkt.length >= 4 and pkt.version() == 2:
        pt = pkt.buffer[pkt.offset + 1] & 0xFF
        return not 200 <= pt <= 211
    return False


def is_multi_block(buffer, offset, length):  # REDBlockIterator.java:178-193
    if len(buffer) == 0:
        return False
    if offset < 0 or len(buffer) <= offset:
        return False
    return (buffer[offset] & 0x80) != 0


class BlockIterator:  # REDBlockIterator.java:202-317
    def __init__(self, buffer, offset, length):
        self.buffer, self.offset, self.length = buffer, offset, length
        self.cnt, self.off_header, self.off_payload = -1, -1, -1
        if len(buffer) == 0:
            return
        self.off_header = offset
        self.cnt = 0
        while (buffer[self.off_header] & 0x80) != 0:
            self.cnt += 1
            self.off_header += 4
        if len(buffer) >= self.off_header + 8:
            self.cnt += 1
        self.off_header = offset
        if self.cnt > 0:
            self.off_payload = self.off_header + (self.cnt - 1) * 4 + 1

    def has_next(self):
        return self.cnt > 0

    def next(self):
        self.cnt -= 1
        if len(self.buffer) <= self.off_header:
            return None
        block_pt = sbyte(self.buffer[self.off_header] & 0x7F)
        if self.has_next():
            if len(self.buffer) < self.off_header + 4:
                return None
            block_len = (self.buffer[self.off_header + 2] & 0x03) << 8 | self.buffer[self.off_header + 3]
            self.off_header += 4
            self.off_payload += block_len
        else:
            block_len = self.length - (self.off_payload + 1)
            self.off_header = -1
            self.off_payload = -1
        return (self.off_payload, block_len, block_pt)


def get_primary_block(buffer, offset, length):  # :118-166
    if is_multi_block(buffer, offset, length):
        block = None
        it = BlockIterator(buffer, offset, length)
        while it.has_next():
            block = it.next()
        return block
    if offset < 0 or length < 0 or len(buffer) < offset + length:
        return None
    block_pt = sbyte(buffer[offset] & 0x7F)
    block_off = offset + 1
    block_len = length - block_off
    if len(buffer) < block_off + block_len:
        return None
    return (block_off, block_len, block_pt)


def strip(pkt, red_pt):  # REDFilterTransformEngine.java:95-145, enabled
    if not rtp_predicate(pkt):
        return 0
    if red_pt == -1 or pkt.payload_type() != red_pt:
        return 0
    h = pkt.header_length()
    pb = get_primary_block(pkt.buffer, pkt.offset + h, pkt.length - h)
    if pb is None:
        return 0
    buf, hdr_len, off, length = pkt.buffer, pkt.header_length(), pkt.offset, pkt.length
    pkt.set_payload_type(pb[2])
    arraycopy(buf, off, buf, pb[0] - hdr_len, hdr_len)
    pkt.offset = pb[0] - hdr_len
    pkt.length = length - (pb[0] - hdr_len - off)
    return 1


def wrap(pkt, red_pt):  # REDTransformEngine.java:151-182
    if red_pt == -1:
        return 0
    if pkt.version() != 2:
        return 0
    buf, length, off, hdr_len = pkt.buffer, pkt.length, pkt.offset, pkt.header_length()
    new = buf
    if len(new) < length + 1:
        new = Buf(bytes(length + 1))
    arraycopy(buf, off, new, 0, hdr_len)
    arraycopy(buf, off + hdr_len, new, hdr_len + 1, length - hdr_len)
    new[hdr_len] = pkt.payload_type()
    pkt.buffer, pkt.offset, pkt.length = new, 0, length + 1
    pkt.set_payload_type(red_pt)
    return 2


def apply(buf, rec):
    """(result, new_bytes) for the packet ``buf`` (bytes) under rec = (mode, red_pt)."""
    mode, red_pt = int(rec[0]), int(rec[1])
    if mode not in (STRIP, WRAP) or not 0 <= red_pt <= 127 or len(buf) < 12:
        return 0, bytes(buf)
    pkt = Pkt(buf)
    try:
        result = strip(pkt, red_pt) if mode == STRIP else wrap(pkt, red_pt)
    except JavaThrow:
        return -1, None
    return result, pkt.bytes()
