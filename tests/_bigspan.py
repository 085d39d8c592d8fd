"""A sparse big device buffer for tests that put byte positions past 2^31 and 2^32, which fails
safe.

Every position of the C ABI is a u64 relative to a base pointer (d_src, d_keys, d_vals, d_dst,
d_base). A kernel that truncates one to 32 bits reads or writes at `pos mod 2^32`; one that
sign-extends it from 32 bits reads or writes at `pos - 2^32` (for positions in [2^31, 2^32) that is
a negative offset of down to -2^31 from the base). A BigSpan therefore covers

    [-2^31, 2^32 + 128 MiB)   around the base it hands to the kernels,

(PORCH bytes below the base, SPAN bytes from it), so that a position wrong in either way still
lands inside the one allocation: a wrong kernel produces wrong bytes (it reads the canary, or
writes where `untouched` sees it) and a failing assertion, not a fault on a shared machine. The
buffer is filled once with CANARY; a test places a few MiB of real data at a base chosen so that
an item of the workload straddles 2^31 or 2^32 (`base_for`, `base_at_boundary`), and the rest of
the buffer stays canary.

This is a plain module (no fixtures): the test modules that use it define their own
module-scoped fixtures around `BigSpan` and `need_room`.
"""
import numpy as np
import torch

PORCH = 1 << 31
SPAN = (1 << 32) + (128 << 20)
TAIL = 4096
CANARY = 0xC5
CHUNK = 256 << 20          # untouched() compares at most this many bytes at a time
LINES = (1 << 31, 1 << 32)


class BigSpan:
    """PORCH + SPAN + TAIL bytes of device memory filled with CANARY; `.ptr` is the address of byte
    PORCH (the base every kernel gets), `.view` the tensor from there on."""

    def __init__(self, dev):
        self.dev = dev
        self.buf = torch.empty(PORCH + SPAN + TAIL, dtype=torch.uint8, device=dev)
        self.buf.fill_(CANARY)
        self.view = self.buf[PORCH:]
        self.ptr = self.view.data_ptr()
        assert self.ptr == self.buf.data_ptr() + PORCH and self.ptr % 256 == 0

    def place(self, data, at: int) -> None:
        """Host bytes (bytes or a uint8 array) to view[at : at + len]."""
        a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
        a = np.ascontiguousarray(a, np.uint8)
        assert 0 <= at and at + a.size <= SPAN
        if a.size:
            self.view[at:at + a.size].copy_(torch.from_numpy(a.copy()))

    def read(self, lo: int, hi: int) -> np.ndarray:
        """view[lo : hi] on the host."""
        assert 0 <= lo <= hi <= SPAN + TAIL
        return self.view[lo:hi].cpu().numpy()

    def wipe(self, windows) -> None:
        """Puts the canary back over the given [lo, hi) windows (between runs of one test)."""
        for lo, hi in windows:
            if hi > lo:
                self.view[lo:hi].fill_(CANARY)

    def untouched(self, windows=()) -> bool:
        """True iff every byte outside the given [lo, hi) windows (relative to the base; the
        porch is [-PORCH, 0)) still holds CANARY. Compared in chunks of at most CHUNK bytes."""
        ws = sorted((max(int(lo), -PORCH), min(int(hi), SPAN + TAIL)) for lo, hi in windows
                    if hi > lo)
        gaps, at = [], -PORCH
        for lo, hi in ws:
            if lo > at:
                gaps.append((at, lo))
            at = max(at, hi)
        if at < SPAN + TAIL:
            gaps.append((at, SPAN + TAIL))
        bad = torch.zeros((), dtype=torch.int64, device=self.dev)
        for lo, hi in gaps:
            for c in range(lo, hi, CHUNK):
                part = self.buf[PORCH + c:PORCH + min(c + CHUNK, hi)]
                bad += (part != CANARY).sum()
        return int(bad.cpu()) == 0

    def free(self) -> None:
        self.view = None
        self.buf = None


def need_room(n_spans: int, extra: int = 4 << 30) -> None:
    """Asserts the device has room for n_spans BigSpans and `extra` bytes of ordinary tensors."""
    free, _total = torch.cuda.mem_get_info()
    need = n_spans * (PORCH + SPAN + TAIL) + extra
    assert free >= need, f"{free >> 20} MiB free on the device, the spans need {need >> 20} MiB"


def _starts(lens) -> np.ndarray:
    s = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(np.asarray(lens, np.int64), out=s[1:])
    return s


def assert_straddle(line: int, base: int, lens, j: int, boundary: bool = False) -> None:
    """The three-way split every case states: at least one whole item of the back-to-back layout
    at `base` lies below `line`, item j contains it (strictly inside; with `boundary`, starts
    exactly on it) and at least one whole item lies above."""
    s = _starts(lens) + base
    assert 1 <= j <= len(lens) - 2
    assert base >= 0 and s[-1] <= SPAN
    assert s[0] < s[j] <= line, "a whole (non-empty) item below the line"
    if boundary:
        assert s[j] == line < s[j + 1]
    else:
        assert s[j] < line < s[j + 1], (int(s[j]), line, int(s[j + 1]))
    assert line < s[j + 1] < s[-1], "a whole (non-empty) item above the line"


def base_for(line: int, lens, j: int, frac: float = 1 / 3, align: int = 16, odd: int = 0) -> int:
    """The base B (a multiple of 16; of `align`, itself one, when given; plus `odd` bytes for a
    column that is to start on no multiple of 16) at which item j of a back-to-back layout with
    lengths `lens` has `line` strictly inside it, about `frac` of the way in (as near to that as
    the alignment allows)."""
    s = _starts(lens)
    assert align % 16 == 0 and 0 <= odd < 16
    b = (line - int(s[j]) - int(lens[j] * frac)) // align * align + odd
    if b + int(s[j]) >= line:              # the item must start below the line
        b -= align
    while b + int(s[j + 1]) <= line:       # and end above it
        b += align
    assert b >= 0 and (b - odd) % align == 0
    assert_straddle(line, b, lens, j)
    return b


def base_at_boundary(line: int, lens, j: int) -> int:
    """The base at which item j starts exactly on `line` (a multiple of 16 only when the items
    before j sum to one)."""
    b = line - int(_starts(lens)[j])
    assert b >= 0
    assert_straddle(line, b, lens, j, boundary=True)
    return b
