"""Guard bands around the buffers of one call (tests/test_gpu_extents.py; proven able to fail without a GPU
by tests/test_extents_host.py).

A Layout puts every pointer argument of a call into ONE byte block: each buffer has exactly its documented
size and starts 256-byte aligned; buffers are separated, and the block is bracketed at both ends, by guard
bands.  A band's width is a condition, not a measurement: at least 64 KiB and at least one row of each of
the two buffers it touches (rounded up to 256), so an overrun by one element, one row or one cell still
lands inside it.

Bands, outputs and the workspace are pre-filled with a pattern byte; the inputs hold the caller's bytes.
guarded() runs the call once per pattern (0xFF: NaN as fp64, -1 as int32; 0x55: a large finite fp64, a
positive int32) and asserts
 1. every guard byte still holds the pattern,
 2. every input is bit-identical to what was uploaded,
 3. the outputs are bit-identical between the two patterns: a read outside a buffer, or of workspace bytes
    the call never wrote, that reaches a result shows here.
The module knows nothing of the GPU: a block is anything with .image() (the bytes now, as numpy) made by a
`make_block(image)` callable; NumpyBlock is the host one, test_gpu_extents.py has the torch one."""
import numpy as np

BAND_MIN = 64 * 1024
ALIGN = 256
PATTERNS = (0xFF, 0x55)
IN, OUT, WS = "in", "out", "ws"


def _up(x, a=ALIGN):
    return (x + a - 1) // a * a


class Buf:
    """One pointer argument: name, exact size in bytes, bytes of one row, role (IN / OUT / WS) and, for an
    output, the dtype its bytes are read back as."""

    def __init__(self, name, nbytes, row, role, dtype=np.uint8):
        assert nbytes > 0 and row > 0, (name, nbytes, row)
        self.name, self.nbytes, self.row, self.role, self.dtype = name, int(nbytes), int(row), role, np.dtype(dtype)


class Layout:
    def __init__(self, bufs):
        self.bufs = list(bufs)
        assert len(set(b.name for b in self.bufs)) == len(self.bufs)
        self.off, self.bands = {}, []            # name -> offset; (begin, end, name before, name after)
        o = 0                                    # end of the previous buffer: a band begins at its very next byte
        for i, b in enumerate(self.bufs + [None]):
            prev = self.bufs[i - 1] if i else None
            e = _up(o + max(BAND_MIN, prev.row if prev else 0, b.row if b else 0))
            self.bands.append((o, e, prev.name if prev else "<start of block>", b.name if b else "<end of block>"))
            if b is not None:
                self.off[b.name] = e
                o = e + b.nbytes
        self.total = e

    def image(self, pattern, inputs):
        """the block's bytes before the call: pattern everywhere, the inputs' bytes in their buffers"""
        img = np.full(self.total, pattern, dtype=np.uint8)
        for b in self.bufs:
            if b.role == IN:
                raw = np.ascontiguousarray(inputs[b.name]).view(np.uint8).reshape(-1)
                assert raw.size == b.nbytes, "%s: %d bytes given, %d documented" % (b.name, raw.size, b.nbytes)
                img[self.off[b.name]:self.off[b.name] + b.nbytes] = raw
        assert set(inputs) == set(b.name for b in self.bufs if b.role == IN)
        return img

    def check(self, before, after, pattern):
        """assertions 1 and 2 on the block's bytes before and after the call"""
        assert before.shape == after.shape == (self.total,)
        for s, e, a, c in self.bands:
            hit = np.nonzero(after[s:e] != pattern)[0]
            if hit.size:
                raise AssertionError(
                    "guard band between %s and %s (pattern 0x%02X) was written: %d byte(s), first at %d bytes behind "
                    "the end of %s (%d bytes before %s), last at %d behind it" % (
                        a, c, pattern, hit.size, hit[0], a, e - s - hit[0], c, hit[-1]))
        for b in self.bufs:
            if b.role == IN:
                o = self.off[b.name]
                hit = np.nonzero(after[o:o + b.nbytes] != before[o:o + b.nbytes])[0]
                if hit.size:
                    raise AssertionError("input %s was written: %d byte(s), first at offset %d, last at %d" % (
                        b.name, hit.size, hit[0], hit[-1]))

    def outputs(self, img):
        return {b.name: img[self.off[b.name]:self.off[b.name] + b.nbytes].copy().view(b.dtype)
                for b in self.bufs if b.role == OUT}


def same_bits(a, b, what):
    """two dicts of outputs hold the same bytes (NaN payloads included)"""
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        x, y = np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)
        assert x.dtype == y.dtype and x.size == y.size, (what, k)
        hit = np.nonzero(x.view(np.uint8) != y.view(np.uint8))[0]
        if hit.size:
            i = hit[0] // x.dtype.itemsize
            raise AssertionError("output %s differs between %s: %d byte(s), first at element %d (%s against %s)" % (
                k, what, hit.size, i, x[i], y[i]))


class NumpyBlock:
    """a host block (the fake kernels of tests/test_extents_host.py write into .a)"""

    def __init__(self, image):
        self.a = image.copy()

    def image(self):
        return self.a.copy()


def guarded(layout, inputs, call, make_block=NumpyBlock, patterns=PATTERNS):
    """call(block, layout.off) once per pattern on a fresh block; assertions 1 to 3; -> the outputs"""
    outs = []
    for pat in patterns:
        before = layout.image(pat, inputs)
        block = make_block(before)
        call(block, layout.off)
        after = block.image()
        layout.check(before, after, pat)
        outs.append(layout.outputs(after))
    for o in outs[1:]:
        same_bits(outs[0], o, "the fill patterns " + " and ".join("0x%02X" % p for p in patterns))
    return outs[0]
