"""Inputs for the compressors' edge tests (test_codec_audit.py over the host encoders,
test_gpu_compress_edges.py over tpz_compress_blocks): families of batches with fixed seeds, each
aimed at a branch of the format, of the 4,352-byte staging window or of the per-wave hash table.

A block is payload + b"\\x01": the compressors read only the tag byte, so the m payload bytes are
exactly what the codec sees. Test infrastructure only."""
import numpy as np

WINDOW_MAX = 4336          # tpz_compress.hip's kCMaxStaged: longer payloads go out as one literal
HASH_BITS = 10             # its kHashBits
DEFAULT_CUS = 256          # an MI355X; the GPU tests pass the device's own count

TINY_M = range(0, 21)
WINDOW_M = (4320, 4331, 4332, 4333, 4334, 4335, 4336, 4337, 4338, 4352, 4353)
LENGTHS_A = (0, 1, 14, 15, 16, 59, 60, 61, 62, 255, 256, 257, 269, 270, 271, 524, 525, 526)
LENGTHS_M = (4, 5, 11, 12, 18, 19, 20, 59, 60, 63, 64, 65, 66, 67, 68, 69, 128, 273, 274, 275,
             528, 529, 530)
OFFSETS_D = (64, 65, 2047, 2048, 2049, 4000)
OFFSETS_RUN_P = (1, 2, 3, 5)          # distances 1, 2, 3 (and 5): a run, its copy overlaps itself
PERIODIC_P = (1, 2, 3, 7, 16, 63, 64)
PERIODIC_M = (256, 1000, 4336)
LONG_M = (4337, 16383, 16384, 65535, 65536, 65537, 70000, 1 << 24, (1 << 24) + 1)
COUNTS_N = (1, 15, 16, 17, 1023, 1024, 1025)


def tag1(payload) -> bytes:
    return bytes(payload) + b"\x01"


def batch(blocks):
    """(src uint8, ext uint64) of blocks back to back; src is exactly ext[-1] bytes long."""
    ext = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    return np.frombuffer(b"".join(blocks), np.uint8).copy(), ext


def _word(rng, p: int) -> bytes:
    """p distinct random bytes: repeated, its period is exactly p."""
    return bytes(rng.permutation(256)[:p].astype(np.uint8))


def _periodic(word: bytes, m: int) -> bytes:
    return (word * (m // len(word) + 1))[:m]


def _other(rng, not_this: int) -> int:
    v = int(rng.integers(0, 256))
    return v if v != not_this else (v + 1) & 255


def snappy_literal_block(data: bytes) -> bytes:
    """A valid tag-2 block by hand (one literal element), for the blocks a compressor passes on."""
    assert 0 < len(data) <= 60
    return bytes([len(data), (len(data) - 1) << 2]) + data + b"\x02"


# ---- tiny: the n < 4, n < 5, n < 12 and n = 12, 13 rules --------------------------------------
def tiny():
    blocks = []
    for m in TINY_M:
        blocks += [tag1(bytes(m)), tag1(bytes(range(1, m + 1))), tag1(_periodic(b"abc", m))]
    return blocks


# ---- window: the staging window's edge at every start residue ---------------------------------
def window_payload(m: int, seed: int = 11) -> bytes:
    """Period 7, the last 64 bytes repeating bytes 0..63: a match has to run to the last byte the
    codec allows."""
    p = bytearray(_periodic(_word(np.random.default_rng(seed), 7), m))
    p[-64:] = p[:64]
    return bytes(p)


def window():
    """(blocks, [(block index, m, residue)]): before every window block a tag-7 filler block of
    0..15 bytes brings its start to the residue; the last block is staged and ends inside a
    16-byte piece that the source does not fill (the staging loop's byte-wise tail)."""
    blocks, index, at = [], [], 0

    def add(m, r):
        nonlocal at
        fill = (r - at) % 16
        blocks.append(bytes(fill - 1) + b"\x07" if fill else b"")
        blocks.append(tag1(window_payload(m)))
        at += fill
        assert at % 16 == r
        index.append((len(blocks) - 1, m, r))
        at += m + 1

    for m in WINDOW_M:
        for r in range(16):
            add(m, r)
    add(4331, 2)
    start = at - 4332
    assert (start + 4331 + 15) // 16 * 16 > at      # the last 16-byte piece passes src_bytes
    return blocks, index


# ---- lengths: a literal of a bytes, then a match of M bytes, after a first match ---------------
def lengths_payload(rng, a: int, M: int) -> bytes:
    """R[:pre] | R[:32] | S(a) | R[40:40+M] | T(24): S[0] and T[0] are redrawn so that neither
    match extends by accident."""
    pre = max(128, 48 + M)
    R = rng.integers(0, 256, pre, dtype=np.uint8).tobytes()
    S = bytearray(rng.integers(0, 256, a, dtype=np.uint8).tobytes())
    T = bytearray(rng.integers(0, 256, 24, dtype=np.uint8).tobytes())
    if a:
        S[0] = _other(rng, R[32])
    T[0] = _other(rng, R[40 + M])
    return R + R[:32] + bytes(S) + R[40:40 + M] + bytes(T)


def lengths(seed: int = 7):
    """(blocks, [(a, M)])."""
    rng = np.random.default_rng(seed)
    cases = [(a, M) for a in LENGTHS_A for M in LENGTHS_M]
    return [tag1(lengths_payload(rng, a, M)) for a, M in cases], cases


# ---- offsets: copy-1 against copy-2 by offset and by length; overlapping copies ---------------
def _lone_bucket(p: bytes, at) -> bool:
    """No word of p other than those at the positions `at` shares the bucket of the word at at[0]
    (the finder's 4-byte hash; it keeps one position per bucket, so nothing clobbers that
    word's entry)."""
    arr = np.frombuffer(p, np.uint8).astype(np.uint64)
    words = arr[:-3] | arr[1:-2] << np.uint64(8) | arr[2:-1] << np.uint64(16) \
        | arr[3:] << np.uint64(24)
    h = ((words * np.uint64(0x1E35A7BD)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)
    return int(h[at[0]]) not in set(np.delete(h, at).tolist())


def offsets_payload(rng, D: int, L: int) -> bytes:
    """F0(70) | W(L) | F1(D - L) | W(L) | F2(24): the word W twice, D bytes apart, in random
    filler. W is redrawn until no other word of the payload falls into the bucket of W's first
    four bytes: the finder keeps one position per bucket, and 2,048 random words fill most of
    1,024 buckets, so a far match would otherwise be lost in nearly every draw."""
    F0 = rng.integers(0, 256, 70, dtype=np.uint8).tobytes()
    F1 = rng.integers(0, 256, D - L, dtype=np.uint8).tobytes()
    F2 = bytearray(rng.integers(0, 256, 24, dtype=np.uint8).tobytes())
    F2[0] = _other(rng, F1[0])                      # the match ends with W
    while True:
        W = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        p = F0 + W + F1 + W + bytes(F2)
        if _lone_bucket(p, [70, 70 + D]):
            return p


def offsets(seed: int = 13):
    """(blocks, [("far", D, L) | ("run", P, 600)])."""
    rng = np.random.default_rng(seed)
    blocks, cases = [], []
    for D in OFFSETS_D:
        for L in (8, 12):
            for _rep in range(3):
                blocks.append(tag1(offsets_payload(rng, D, L)))
                cases.append(("far", D, L))
    for P in OFFSETS_RUN_P:
        tail = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
        blocks.append(tag1(_periodic(_word(rng, P), 600) + tail))
        cases.append(("run", P, 600))
    return blocks, cases


# ---- ends: the last position a match may start at, from both sides ----------------------------
ENDS_K = range(3, 17)


def ends(seed: int = 31):
    """(blocks, [k]): W(8) | F(100) | (W | G)[:k], random bytes: the word W comes back k bytes
    before the end, cut short by the end, and nothing else repeats. Snappy may start a match
    there from k = 4 on, LZ4 from k = 12 on (and must stop it 5 bytes before the end)."""
    rng = np.random.default_rng(seed)
    blocks = []
    for k in ENDS_K:
        while True:
            W, F, G = (rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (8, 100, 16))
            p = W + F + (W + bytes([_other(rng, F[0])]) + G)[:k]
            if _lone_bucket(p + b"\0\0\0", [0, 108]):
                break
        blocks.append(tag1(p))
    return blocks, list(ENDS_K)


# ---- periodic ---------------------------------------------------------------------------------
def periodic(seed: int = 17):
    """(blocks, [(P, m)])."""
    rng = np.random.default_rng(seed)
    cases = [(P, m) for P in PERIODIC_P for m in PERIODIC_M]
    return [tag1(_periodic(_word(rng, P), m)) for P, m in cases], cases


# ---- long: the literal-only path past the window ----------------------------------------------
def long_blocks(seed: int = 19):
    """(blocks, [(m, "random" | "zeros")])."""
    rng = np.random.default_rng(seed)
    blocks, cases = [], []
    for m in LONG_M:
        blocks.append(tag1(rng.integers(0, 256, m, dtype=np.uint8).tobytes()))
        cases.append((m, "random"))
        blocks.append(tag1(bytes(m)))
        cases.append((m, "zeros"))
    return blocks, cases


# ---- reuse: more than two blocks per wave, each of another kind than the wave's last ----------
_WORDS = [b"key_", b"value_", b"user", b"0000", b"topaz", b"/a/b/", b"field=", b"\x00\x00\x01"]


def _textlike(rng, m: int) -> bytes:
    out = bytearray()
    while len(out) < m:
        out += _WORDS[int(rng.integers(0, len(_WORDS)))]
        out += b"%d" % int(rng.integers(0, 1000))
    return bytes(out[:m])


def reuse(num_cus: int = DEFAULT_CUS, seed: int = 23):
    """2 * 16 * num_cus + 37 blocks: a launch of num_cus workgroups of 16 waves gives every wave
    two blocks and some a third. Block i cycles through text-like bytes, random bytes, an empty
    block, a tag-2 block (passed on), 5,000 random bytes (the literal path) and zeros. With 256
    compute units a wave's stride of 4,096 blocks is 4 mod 6, so its blocks are of three kinds;
    with any count they differ in length."""
    rng = np.random.default_rng(seed)
    n = 2 * 16 * num_cus + 37
    big = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    blocks = []
    for i in range(n):
        m = int(rng.integers(0, 401))
        k = i % 6
        if k == 0:
            blocks.append(tag1(_textlike(rng, m)))
        elif k == 1:
            blocks.append(tag1(rng.integers(0, 256, m, dtype=np.uint8).tobytes()))
        elif k == 2:
            blocks.append(b"")
        elif k == 3:
            blocks.append(snappy_literal_block(_textlike(rng, 1 + m % 60)))
        elif k == 4:
            blocks.append(tag1(big[i % 64:] + big[:i % 64]))
        else:
            blocks.append(tag1(bytes(m)))
    return blocks


# ---- counts: the size scan and the pack kernel's short and empty blocks -----------------------
def counts(n: int, seed: int = 29):
    """n blocks of 0..40 bytes: tag-1 blocks (random, runs and empty payloads), empty blocks and
    blocks of other tags."""
    rng = np.random.default_rng(seed + n)
    blocks = []
    for i in range(n):
        m = int(rng.integers(0, 40))
        k = int(rng.integers(0, 6))
        if k == 0:
            blocks.append(b"")
        elif k == 1:
            blocks.append(rng.integers(0, 256, m, dtype=np.uint8).tobytes() + b"\x07")
        elif k == 2:
            blocks.append(tag1(bytes([i & 255]) * m))
        elif k == 3:
            blocks.append(tag1(b""))
        else:
            blocks.append(tag1(rng.integers(0, 256, m, dtype=np.uint8).tobytes()))
    return blocks


def all_batches(num_cus: int = DEFAULT_CUS):
    """Every family's blocks as {name: [block]} (the counts family once per block count)."""
    out = {"tiny": tiny(), "ends": ends()[0], "window": window()[0], "lengths": lengths()[0],
           "offsets": offsets()[0], "periodic": periodic()[0], "long": long_blocks()[0],
           "reuse": reuse(num_cus)}
    for n in COUNTS_N:
        out["counts%d" % n] = counts(n)
    return out
