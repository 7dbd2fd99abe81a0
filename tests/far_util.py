"""Where the rows of tests/test_far_offsets_kernels_gpu.py sit in memory.  Plain Python: tests/test_far_util_cpu.py checks every
placement (the rows themselves are tests/far_cases.py's).

Placement.  One buffer of BUF_BYTES (2^33 + 2^20) is addressed from BASE_BYTES (2^19) into it - the base pointer a kernel receives -
so that an index which 32 bits turn into a small NEGATIVE number still lands inside the allocation.  In elements from that base:

  row A (near)        a small odd start
  row B (far)         2-byte kinds: element 2^32 + k; 4-byte kinds: element 2^30 + k (byte offset 2^32 + 4 k); k odd
  row C (straddling)  starts CROSS_BEFORE = 700 elements before the same line and runs across it

`truncations(e, itemsize)` lists where element e turns up when its element index or its byte offset passes through 32 bits, unsigned
or sign-extended; `decoys(start, count, itemsize)` the windows a whole row turns up in.  The GPU module fills every such window with
other samples (a source) or sentinels (a destination), so a truncated index reads wrong data or damages a sentinel and an assert
reports it; nothing leaves the allocation.  Rows, decoys and the guard windows of WINDOW elements around them never overlap."""
import collections

import numpy as np

LINE = 1 << 32
BUF_BYTES = (1 << 33) + (1 << 20)
BASE_BYTES = 1 << 19
WINDOW = 1024
CROSS_BEFORE = 700
CROSS_MIN = 1500            # a straddling row holds at least this many elements
ITEMSIZE = {"int16": 2, "float16": 2, "float32": 4, "int32": 4}
NP_OF = {"int16": np.int16, "float16": np.float16, "float32": np.float32, "int32": np.int32}


def _u32(v):
    return v & 0xFFFFFFFF


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def truncations(e, itemsize):
    """the element indices other than e itself that element e becomes when its index (first two) or its byte offset (last two) is
    cut to 32 bits, unsigned and signed"""
    found = {_u32(e), _s32(e), _u32(e * itemsize) // itemsize, _s32(e * itemsize) // itemsize}
    found.discard(e)
    return sorted(found)


def decoys(start, count, itemsize):
    """[(start, count)] of the windows in which the row [start, start + count) turns up under truncations(): the row is cut where
    its index or its byte offset crosses a multiple of 2^31, and each piece lands as one contiguous window"""
    step = (1 << 31) // itemsize
    cuts = [start] + [c for c in range((start // step + 1) * step, start + count, step)] + [start + count]
    found = set()
    for a, b in zip(cuts[:-1], cuts[1:]):
        for cut in (lambda e: _u32(e), lambda e: _s32(e), lambda e: _u32(e * itemsize) // itemsize, lambda e: _s32(e * itemsize) // itemsize):
            lo, hi = cut(a), cut(b - 1)
            assert hi - lo == b - 1 - a, "a piece lands in one window"
            if lo != a:
                found.add((lo, b - a))
    return sorted(found)


def far_element(itemsize):
    """the first element whose byte offset needs more than 32 bits (4-byte kinds) or whose index does (2-byte kinds)"""
    return LINE if itemsize == 2 else LINE // itemsize


Layout = collections.namedtuple("Layout", "itemsize starts counts decoys")


def layout(itemsize, counts):
    """counts: the elements of rows A, B, C -> Layout(starts (A, B, C) in elements from the base, decoys [(start, count)])"""
    n_a, n_b, n_c = counts
    assert n_c >= CROSS_MIN and itemsize in (2, 4)
    far = far_element(itemsize)
    c = far - CROSS_BEFORE
    cursor = n_c - CROSS_BEFORE + 2 * WINDOW                # behind C's low decoy
    k_b = cursor | 1
    cursor = k_b + n_b + 2 * WINDOW                         # behind B's decoy
    k_a = cursor | 1
    starts = (k_a, far + k_b, c)
    merged = []                                             # windows that touch or overlap become one
    for s, n in sorted(set(decoys(starts[1], n_b, itemsize) + decoys(c, n_c, itemsize) + decoys(k_a, n_a, itemsize))):
        if merged and s <= merged[-1][0] + merged[-1][1]:
            merged[-1] = (merged[-1][0], max(merged[-1][1], s + n - merged[-1][0]))
        else:
            merged.append((s, n))
    return Layout(itemsize, starts, tuple(counts), merged)


def check_layout(lay):
    """every row, every decoy and the guard window around each lies inside the buffer, and no two of them overlap (a decoy may
    repeat); rows B and C are far, and each has a decoy"""
    lo, hi = -(BASE_BYTES // lay.itemsize), (BUF_BYTES - BASE_BYTES) // lay.itemsize
    spans = [(s, s + n, "row") for s, n in zip(lay.starts, lay.counts)] + [(s, s + n, "decoy") for s, n in lay.decoys]
    for a, b, what in spans:
        assert lo + WINDOW <= a - WINDOW and b + WINDOW <= hi - WINDOW, "%s [%d, %d) and its guards leave the buffer" % (what, a, b)
    for i, (a, b, _) in enumerate(spans):
        for c, d, _ in spans[i + 1:]:
            assert b + 2 * WINDOW <= c or d + 2 * WINDOW <= a, "[%d, %d) and [%d, %d) are closer than two guard windows" % (a, b, c, d)
    far = far_element(lay.itemsize)
    assert lay.starts[0] & 1 and lay.starts[1] & 1 and lay.starts[0] < (1 << 20)
    assert lay.starts[1] >= far and lay.starts[1] * lay.itemsize >= LINE
    assert lay.starts[2] == far - CROSS_BEFORE and lay.starts[2] + lay.counts[2] >= far + CROSS_MIN - CROSS_BEFORE
    for q in (1, 2):                                        # every element of a far row has its landing spots inside decoys
        s, n = lay.starts[q], lay.counts[q]
        for e in {s, s + CROSS_BEFORE - 1, s + CROSS_BEFORE, s + n - 1} if q == 2 else {s, s + n - 1}:
            spots = truncations(e, lay.itemsize)
            assert spots, "element %d is not far" % e
            for t in spots:
                assert any(a <= t < a + m for a, m in lay.decoys), "element %d lands at %d, outside every decoy" % (e, t)
    return True
