"""The guard-band checker of tests/extents.py can fail: on numpy blocks and fake "kernels", each of its
assertions fires, and names the right buffer, for a write one element past an output, one element before it, a
write into an input and a result copied from a band; and a well-behaved kernel passes.  No GPU."""
import numpy as np
import pytest

import extents as X

T, N = 9, 3


def _layout():
    return X.Layout([X.Buf("d_y", 8 * T, 8 * T, X.IN),
                     X.Buf("d_theta", 8 * N * 4, 8 * 4, X.OUT, np.float64),
                     X.Buf("d_n_iter", 4 * N, 4 * N, X.OUT, np.int32),
                     X.Buf("ws", 1000, 1000, X.WS),
                     X.Buf("d_lik", 8 * N, 8 * N, X.OUT, np.float64)])


def _inputs():
    return {"d_y": np.arange(T, dtype=np.float64)}


def _f64(block, off, count=None):
    """the block's bytes from `off` on as doubles (a view the fake kernels write through)"""
    n = (block.a.size - off) // 8 if count is None else count
    return block.a[off:off + 8 * n].view(np.float64)


def good(block, off):
    y = _f64(block, off["d_y"], T)
    _f64(block, off["d_theta"], N * 4)[:] = np.repeat(y[:N], 4) * 2
    block.a[off["d_n_iter"]:off["d_n_iter"] + 4 * N].view(np.int32)[:] = 7
    block.a[off["ws"]:off["ws"] + 1000] = 3                          # (a workspace may hold anything afterwards)
    _f64(block, off["d_lik"], N)[:] = y[-N:]


def test_layout_meets_its_conditions():
    L = _layout()
    ends = {b.name: L.off[b.name] + b.nbytes for b in L.bufs}
    assert all(o % 256 == 0 for o in L.off.values())
    assert len(L.bands) == len(L.bufs) + 1 and L.bands[0][0] == 0 and L.bands[-1][1] == L.total
    for (s, e, a, c), nxt in zip(L.bands, L.bufs + [None]):
        assert e - s >= X.BAND_MIN
        assert s == ends.get(a, 0)                                   # not one byte of slack outside a band
        assert e == (L.off[nxt.name] if nxt else L.total)
    wide = X.Layout([X.Buf("a", 8 * 100000, 8 * 100000, X.OUT, np.float64), X.Buf("b", 8, 8, X.OUT, np.float64)])
    assert all(e - s >= 800000 for s, e, _, _ in wide.bands[:2]) and wide.bands[2][1] - wide.bands[2][0] >= X.BAND_MIN
    with pytest.raises(AssertionError, match="documented"):
        L.image(0xFF, {"d_y": np.zeros(T + 1)})


def test_a_well_behaved_kernel_passes():
    out = X.guarded(_layout(), _inputs(), good)
    assert np.array_equal(out["d_theta"], np.repeat(np.arange(N), 4) * 2.0)
    assert np.array_equal(out["d_n_iter"], np.full(N, 7)) and np.array_equal(out["d_lik"], np.arange(T - N, T))
    assert set(out) == {"d_theta", "d_n_iter", "d_lik"}


def test_a_write_one_element_past_an_output_fires():
    def k(block, off):
        good(block, off)
        _f64(block, off["d_theta"])[N * 4] = 1.0
    with pytest.raises(AssertionError, match=r"between d_theta and d_n_iter .*: 8 byte\(s\), first at 0 bytes behind"):
        X.guarded(_layout(), _inputs(), k)

    def k4(block, off):                                              # ... and past an int output that ends off 256
        good(block, off)
        block.a[off["d_n_iter"]:].view(np.int32)[N] = 1
    with pytest.raises(AssertionError, match=r"between d_n_iter and ws .*: 4 byte\(s\), first at 0 bytes behind"):
        X.guarded(_layout(), _inputs(), k4)

    def kend(block, off):                                            # ... and past the last buffer
        good(block, off)
        _f64(block, off["d_lik"])[N] = 1.0
    with pytest.raises(AssertionError, match=r"between d_lik and <end of block>"):
        X.guarded(_layout(), _inputs(), kend)


def test_a_write_one_element_before_an_output_fires():
    def k(block, off):
        good(block, off)
        block.a[off["d_theta"] - 8:off["d_theta"]].view(np.float64)[0] = 1.0
    with pytest.raises(AssertionError, match=r"between d_y and d_theta .*: 8 byte\(s\).*\(8 bytes before d_theta\)"):
        X.guarded(_layout(), _inputs(), k)

    def kfirst(block, off):
        good(block, off)
        block.a[off["d_y"] - 1] = 0
    with pytest.raises(AssertionError, match=r"between <start of block> and d_y .*\(1 bytes before d_y\)"):
        X.guarded(_layout(), _inputs(), kfirst)


def test_a_row_past_a_buffer_still_lands_in_the_band():
    def k(block, off):
        good(block, off)
        _f64(block, off["d_theta"])[(N + 1) * 4 - 1] = 1.0           # the last element of the row behind the last
    with pytest.raises(AssertionError, match=r"between d_theta and d_n_iter .*first at 24 bytes behind"):
        X.guarded(_layout(), _inputs(), k)


def test_a_write_into_an_input_fires():
    def k(block, off):
        good(block, off)
        _f64(block, off["d_y"], T)[2] = -1.0
    with pytest.raises(AssertionError, match=r"input d_y was written: 2 byte\(s\), first at offset 22, last at 23"):
        X.guarded(_layout(), _inputs(), k)

    def same_value(block, off):                                      # (rewriting the same bytes is not a change)
        good(block, off)
        _f64(block, off["d_y"], T)[2] = 2.0
    X.guarded(_layout(), _inputs(), same_value)


def test_a_result_copied_from_a_band_fires():
    def k(block, off):
        good(block, off)
        _f64(block, off["d_lik"], N)[1] = _f64(block, off["d_y"])[T]        # y[T]: one element past the input
    with pytest.raises(AssertionError, match=r"output d_lik differs between the fill patterns 0xFF and 0x55: .*element 1 "):
        X.guarded(_layout(), _inputs(), k)

    def kws(block, off):                                             # ... and from workspace bytes nobody wrote
        stale = block.a[off["ws"] + 8:off["ws"] + 12].view(np.int32)[0]
        good(block, off)
        block.a[off["d_n_iter"]:off["d_n_iter"] + 4 * N].view(np.int32)[2] = stale
    with pytest.raises(AssertionError, match=r"output d_n_iter differs between the fill patterns .*element 2 \(-1 against"):
        X.guarded(_layout(), _inputs(), kws)

    def kout(block, off):                                            # ... and an output element left unwritten
        keep = _f64(block, off["d_theta"], N * 4)[5]
        good(block, off)
        _f64(block, off["d_theta"], N * 4)[5] = keep
    with pytest.raises(AssertionError, match=r"output d_theta differs .*element 5 "):
        X.guarded(_layout(), _inputs(), kout)


def test_same_bits_sees_nan_payloads_and_signed_zeros():
    a = {"x": np.array([0.0, np.nan])}
    X.same_bits(a, {"x": np.array([0.0, np.nan])}, "two runs")
    with pytest.raises(AssertionError, match="output x differs between two runs"):
        X.same_bits(a, {"x": np.array([-0.0, np.nan])}, "two runs")
    other = np.array([0.0, np.nan])
    other.view(np.uint64)[1] ^= 1
    with pytest.raises(AssertionError, match="element 1"):
        X.same_bits(a, {"x": other}, "two runs")
