"""Stream auditors for the two block codecs, in plain Python: every element of a snappy raw stream
(snap::raw's format: a varint length, literal and copy elements) and every sequence of a
size-prefixed LZ4 block (what compress::encode writes, src/block/compress.rs:66-77) is walked,
checked and listed, so that a test can ask what an encoder emitted and not only whether it decodes.

Nothing here shares code with the oracle's decoders (oracle/tpz_snappy.c, oracle/tpz_lz4.c): the
auditors and _oracle check each other (test_codec_audit.py). Test infrastructure only."""


class AuditError(ValueError):
    """The stream breaks a rule of its format (or, for LZ4, one of the encoder-side end rules)."""


def _append_copy(out: bytearray, off: int, ln: int) -> None:
    """ln bytes from `off` back, byte by byte as the formats define it (off < ln repeats)."""
    start = len(out) - off
    if off >= ln:
        out += out[start:start + ln]
    else:
        out += (bytes(out[start:]) * (ln // off + 1))[:ln]


def snappy_audit(stream):
    """(decoded bytes, elements) of a snappy raw stream; elements are ("lit", length,
    length bytes after the tag byte: 0 = inline) and ("copy1" | "copy2" | "copy4", offset,
    length). AuditError where the stream is not a minimal, exact snappy stream."""
    s = bytes(stream)
    want, shift, pos = 0, 0, 0
    while True:
        if pos >= len(s):
            raise AuditError("the varint preamble runs past the stream")
        if pos >= 5:
            raise AuditError("overlong varint: more than 5 bytes")
        b = s[pos]
        pos += 1
        want |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            if b == 0 and pos > 1:
                raise AuditError("non-minimal varint: a zero last byte")
            break
    if want >= 1 << 32:
        raise AuditError("overlong varint: %d does not fit 32 bits" % want)
    out = bytearray()
    elements = []
    while pos < len(s):
        if len(out) == want:
            raise AuditError("%d bytes left over after the preamble's %d bytes"
                             % (len(s) - pos, want))
        tag = s[pos]
        kind = tag & 3
        if kind == 0:
            ln, nb = (tag >> 2) + 1, 0
            if ln > 60:
                nb = ln - 60
                if pos + 1 + nb > len(s):
                    raise AuditError("a literal's length bytes run past the stream")
                ln = int.from_bytes(s[pos + 1:pos + 1 + nb], "little") + 1
            pos += 1 + nb
            if pos + ln > len(s):
                raise AuditError("a literal of %d bytes runs past the stream" % ln)
            if len(out) + ln > want:
                raise AuditError("a literal of %d bytes runs past the preamble's %d" % (ln, want))
            out += s[pos:pos + ln]
            pos += ln
            elements.append(("lit", ln, nb))
            continue
        hdr = (2, 3, 5)[kind - 1]
        if pos + hdr > len(s):
            raise AuditError("a copy's header runs past the stream")
        if kind == 1:
            ln = 4 + ((tag >> 2) & 7)
            off = (tag >> 5) << 8 | s[pos + 1]
        else:
            ln = (tag >> 2) + 1
            off = int.from_bytes(s[pos + 1:pos + hdr], "little")
        pos += hdr
        if off == 0:
            raise AuditError("a copy with offset 0")
        if off > len(out):
            raise AuditError("a copy's offset %d reaches before the %d bytes produced"
                             % (off, len(out)))
        if len(out) + ln > want:
            raise AuditError("a copy of %d bytes runs past the preamble's %d" % (ln, want))
        _append_copy(out, off, ln)
        elements.append(("copy%d" % (1, 2, 4)[kind - 1], off, ln))
    if len(out) != want:
        raise AuditError("the preamble says %d bytes, the elements produce %d" % (want, len(out)))
    return bytes(out), elements


def _lz4_length(s: bytes, pos: int, base: int):
    """A token nibble of 15 continued: (length, position after it, continuation bytes)."""
    n = 0
    while True:
        if pos >= len(s):
            raise AuditError("a length continuation runs past the block")
        b = s[pos]
        pos += 1
        n += 1
        base += b
        if b != 255:
            return base, pos, n


def lz4_audit(block, end_rules: bool = True):
    """(decoded bytes, sequences) of a u32 LE size followed by an LZ4 block; sequences are
    (literal_len, offset, match_len, literal continuation bytes, match continuation bytes), the
    last one with offset = match_len = 0. AuditError where the block is not an exact LZ4 block of
    that size and, with end_rules, where a match breaks what an encoder owes LZ4_decompress_safe:
    it starts at least 12 bytes and ends at least 5 bytes before the end of the output."""
    s = bytes(block)
    if len(s) < 4:
        raise AuditError("no size prefix")
    want = int.from_bytes(s[:4], "little")
    pos = 4
    out = bytearray()
    seqs = []
    while True:
        if pos >= len(s):
            raise AuditError("the last sequence carries a match" if seqs else "no sequence")
        token = s[pos]
        pos += 1
        ll, ll_ext = token >> 4, 0
        if ll == 15:
            ll, pos, ll_ext = _lz4_length(s, pos, 15)
        if pos + ll > len(s):
            raise AuditError("%d literals run past the block" % ll)
        if len(out) + ll > want:
            raise AuditError("%d literals run past the size prefix %d" % (ll, want))
        out += s[pos:pos + ll]
        pos += ll
        if pos == len(s):
            if token & 15:
                raise AuditError("the last sequence carries a match length")
            seqs.append((ll, 0, 0, ll_ext, 0))
            break
        if len(out) == want:
            raise AuditError("%d bytes left over after the size prefix's %d bytes"
                             % (len(s) - pos, want))
        if pos + 2 > len(s):
            raise AuditError("an offset runs past the block")
        off = s[pos] | s[pos + 1] << 8
        pos += 2
        ml, ml_ext = (token & 15) + 4, 0
        if ml == 19:
            ml, pos, ml_ext = _lz4_length(s, pos, 19)
        if off == 0:
            raise AuditError("a match with offset 0")
        if off > len(out):
            raise AuditError("a match's offset %d reaches before the %d bytes produced"
                             % (off, len(out)))
        if len(out) + ml > want:
            raise AuditError("a match of %d bytes runs past the size prefix %d" % (ml, want))
        if end_rules:
            if want < 13:
                raise AuditError("a match in a block of %d < 13 bytes" % want)
            if len(out) > want - 12:
                raise AuditError("a match starts at %d, past n - 12 = %d" % (len(out), want - 12))
            if len(out) + ml > want - 5:
                raise AuditError("a match ends at %d, past n - 5 = %d"
                                 % (len(out) + ml, want - 5))
        _append_copy(out, off, ml)
        seqs.append((ll, off, ml, ll_ext, ml_ext))
    if len(out) != want:
        raise AuditError("the size prefix says %d bytes, the sequences produce %d"
                         % (want, len(out)))
    return bytes(out), seqs


def snappy_matches(elements):
    """The matches of a snappy element list as (offset, [piece lengths]): consecutive copies of
    one offset that follow each other without a literal are one match cut into pieces."""
    out = []
    prev = None
    for e in elements:
        if e[0] == "lit":
            prev = None
            continue
        if prev is not None and prev == e[1]:
            out[-1][1].append(e[2])
        else:
            out.append((e[1], [e[2]]))
        prev = e[1]
    return out


def device_rules(items, codec: int) -> None:
    """What tpz_compress.hip (and the host encoders of tpz_host_builder.cpp) state about their own
    output, over snappy_audit's elements (codec 2) or lz4_audit's sequences (codec 3)."""
    if codec == 3:
        for i, (ll, off, ml, _le, _me) in enumerate(items[:-1]):
            if ml < 4:
                raise AuditError("sequence %d: a match of %d < 4 bytes" % (i, ml))
        return
    assert codec == 2, codec
    for i, e in enumerate(items):
        if e[0] == "copy4":
            raise AuditError("element %d: a copy-4" % i)
        if e[0] == "copy1" and not (4 <= e[2] <= 11 and e[1] < 2048):
            raise AuditError("element %d: copy-1 of %d bytes at offset %d" % (i, e[2], e[1]))
        if e[0] == "copy2" and not 1 <= e[2] <= 64:
            raise AuditError("element %d: copy-2 of %d bytes" % (i, e[2]))
    for off, pieces in snappy_matches(items):
        if min(pieces) < 4:
            raise AuditError("a match at offset %d cut into %r: a piece under 4" % (off, pieces))
