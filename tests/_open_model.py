"""A pure-Python model of SsTable::open's parse over one file image (tpz_open_index /
tpz_open_metas), lifted from table.py's SsTable._read_bloom / open and
BlockMeta.decode_block_meta, and a builder of synthetic images. No GPU, no library."""
import struct

(OK, SHORT, BLOOM_RANGE, META_RANGE, META_TRUNCATED, BAD_EXTENTS, NO_BLOCKS, UNSUPPORTED) = range(8)
NONE = 2**64 - 1


class Parsed:
    """info: the d_info row (flags included); for an OK file ext (n + 1 offsets, the last one the
    meta offset), first_keys (n byte strings) and has_codec."""

    def __init__(self, info, ext=None, first_keys=None):
        self.info, self.ext, self.first_keys = info, ext, first_keys
        self.status = info[0]
        self.has_codec = bool(info[7] & 1)

    @property
    def first_pos(self):
        pos = [0]
        for k in self.first_keys:
            pos.append(pos[-1] + len(k))
        return pos


def parse(data: bytes) -> Parsed:
    ln = len(data)
    size = ln - 4 if ln >= 4 else 0

    def fail(status):
        return Parsed([status, size, 0, 0, 0, 0, 0, 0])

    if ln > 1 << 34:
        return fail(UNSUPPORTED)
    if ln < 8:                                   # _read_bloom: size < SIZEOF_U32 (or no trailer)
        return fail(SHORT)
    offset = struct.unpack(">I", data[size - 4:size])[0]
    bloom_off, flen = NONE, 0
    if size != offset + 4:
        if offset + 4 > size:
            return fail(BLOOM_RANGE)
        bloom_off, flen = offset, size - 4 - offset
    if offset < 4:
        return fail(META_RANGE)
    meta_off = struct.unpack(">I", data[offset - 4:offset])[0]
    if meta_off > offset - 4:
        return fail(META_RANGE)
    buf = data[meta_off:offset - 4]
    offs, keys, p = [], [], 0
    while p < len(buf):                          # decode_block_meta
        if p + 6 > len(buf):
            return fail(META_TRUNCATED)
        off, kl = struct.unpack(">IH", buf[p:p + 6])
        if p + 6 + kl > len(buf):
            return fail(META_TRUNCATED)
        offs.append(off)
        keys.append(bytes(buf[p + 6:p + 6 + kl]))
        p += 6 + kl
    ext = offs + [meta_off]
    if offs and any(b < a for a, b in zip(ext, ext[1:])):
        return fail(BAD_EXTENTS)
    if not offs:
        return fail(NO_BLOCKS)
    codec = any(b > a and data[b - 1] in (2, 3) for a, b in zip(ext, ext[1:]))
    return Parsed([OK, size, meta_off, len(buf), bloom_off, flen, len(offs), int(codec)], ext, keys)


def encode_metas(metas) -> bytes:
    return b"".join(struct.pack(">IH", off & 0xFFFFFFFF, len(k)) + k for off, k in metas)


def assemble(region: bytes, section: bytes, meta_off=None, filt=None, offset=None) -> bytes:
    """region | section | BE u32 meta offset | [filt] | BE u32 offset | 4 trailer bytes. meta_off
    and offset default to the true positions; filt None is a file without a bloom section
    (read_bloom: size == offset + 4). The trailer is filler (the parse never reads it)."""
    out = region + section + struct.pack(">I", len(region) if meta_off is None else meta_off)
    pos = len(out)
    out += filt or b""
    return out + struct.pack(">I", pos if offset is None else offset) + b"\xC4\xC3\xC2\xC1"


def build_image(metas, filt=None, block_lens=None, tags=None, fill=0xA5) -> bytes:
    """A file image whose meta section encodes `metas` ((offset, first_key) pairs, taken as they
    are). The data region is filler: blocks of `block_lens` bytes, each ending in its tag byte
    (1 by default); without block_lens it is as long as the largest offset."""
    if block_lens is None:
        region = bytes([fill]) * max([off for off, _ in metas] + [0])
    else:
        tags = tags or [1] * len(block_lens)
        region = b"".join(bytes([fill]) * (n - 1) + bytes([t]) if n else b""
                          for n, t in zip(block_lens, tags))
    return assemble(region, encode_metas(metas), filt=filt)


def regular_metas(block_lens, keys):
    offs, p = [], 0
    for n in block_lens:
        offs.append(p)
        p += n
    return list(zip(offs, keys))


def boundary_cases():
    """(name, image, status): one image per status class and at each boundary of the checks."""
    good = [(0, b"apple"), (10, b"berry"), (25, b"cherry")]
    sec = encode_metas(good)
    region = b"\x01" * 40
    c = [("len%d" % n, b"\x00" * n, SHORT) for n in (0, 3, 4, 7)]
    c += [("len8_offset0", struct.pack(">I", 0) + b"cccc", META_RANGE),
          ("len8_offset_max", b"\xFF" * 4 + b"cccc", BLOOM_RANGE),
          ("no_bloom", assemble(region, sec), OK),
          ("filter_1_byte", assemble(region, sec, filt=b"\x07"), OK),
          ("filter_61_bytes", assemble(region, sec, filt=bytes(range(61))), OK)]
    img = assemble(region, sec)
    size = len(img) - 4
    c += [("offset_size_minus_3", img[:size - 4] + struct.pack(">I", size - 3) + img[size:],
           BLOOM_RANGE),
          ("offset_3", assemble(b"", b"", filt=b"xyz", offset=3), META_RANGE),
          ("offset_4_empty_section", assemble(b"", b"", filt=b"xyz"), NO_BLOCKS),
          ("meta_off_at_end_of_section", assemble(region, sec, meta_off=len(region) + len(sec)),
           NO_BLOCKS),
          ("meta_off_one_past", assemble(region, sec, meta_off=len(region) + len(sec) + 1),
           META_RANGE)]
    for cut in range(1, 6):
        c.append(("header_cut_%d" % cut, assemble(region, sec + sec[:cut]), META_TRUNCATED))
    c += [("key_cut_by_one", assemble(region, sec[:-1]), META_TRUNCATED),
          ("decreasing_then_truncated",
           assemble(region, encode_metas([(20, b"a"), (10, b"b")]) + b"\x00\x00", filt=b"\x01"),
           META_TRUNCATED),
          ("decreasing", assemble(region, encode_metas([(20, b"a"), (10, b"b"), (30, b"c")])),
           BAD_EXTENTS),
          ("last_offset_past_meta_offset", assemble(region, encode_metas([(0, b"a"), (41, b"b")])),
           BAD_EXTENTS),
          ("key_len_0", assemble(region, encode_metas([(0, b""), (10, b""), (20, b"k")])), OK),
          ("key_len_65535",
           assemble(region, encode_metas([(0, b"a"), (10, bytes(range(256)) * 255 + b"z" * 255),
                                          (20, b"b")]), filt=b"\x05\x06"), OK)]
    return c
