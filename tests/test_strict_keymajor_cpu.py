"""The region of a strict launch's key-major order and the functions that map a key index to its
bin (narwhal_amd/csrc/nw_strict_keymajor.hpp: km_region_plan, km_block_t, km_shift, km_bin),
read through tools/libnw_hostcheck.so (hc_keymajor_layout, hc_keymajor_bin): the parts
are in order, disjoint and aligned and sized for the slices test_strict_layout_cpu.py uses; the
bins are monotonic groups of equal size that fit the histogram, with the last bin kept for items
without a live key."""
import ctypes

import pytest

from test_hostcheck import hc  # noqa: F401  (the library fixture)
from test_strict_layout_cpu import SHAPES

BLOCK, BINS, CHUNK = 256, 1024, 16384
PLAN = ["hist", "cursor", "perm", "pslot", "bytes"]
BLOCK_FIELDS = {"npos": 0, "placed": 8, "bins": 16, "slices": 24, "size": 256}
NO_KEY = 0xFFFFFFFF


def _layout(hc, slice_):  # noqa: F811
    out = (ctypes.c_uint64 * 32)()
    hc.hc_keymajor_layout.restype = ctypes.c_int
    hc.hc_keymajor_layout.argtypes = [ctypes.c_uint64, ctypes.c_void_p]
    n = hc.hc_keymajor_layout(slice_, out)
    assert n == len(PLAN) + 3 + len(BLOCK_FIELDS)
    v = [int(x) for x in out[:n]]
    return dict(zip(PLAN, v[:5])), v[5:8], dict(zip(BLOCK_FIELDS, v[8:]))


def _bin(hc, kk, space):  # noqa: F811
    shift = ctypes.c_uint32()
    hc.hc_keymajor_bin.restype = ctypes.c_uint32
    hc.hc_keymajor_bin.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return int(hc.hc_keymajor_bin(kk, space, ctypes.byref(shift))), int(shift.value)


@pytest.mark.parametrize("slice_", sorted({s for s, _, _ in SHAPES}))
def test_region_plan(hc, slice_):  # noqa: F811
    r, (clear, bins, chunk), blk = _layout(hc, slice_)
    assert (bins, chunk) == (BINS, CHUNK) and blk == BLOCK_FIELDS
    want = {"hist": BLOCK, "cursor": BLOCK + 4 * BINS, "perm": BLOCK + 8 * BINS}
    want["pslot"] = want["perm"] + 4 * slice_
    want["bytes"] = want["pslot"] + 4 * slice_
    assert r == want
    # in order and disjoint: each part ends where the next begins, or before it
    sizes = {"hist": 4 * BINS, "cursor": 4 * BINS, "perm": 4 * slice_, "pslot": 4 * slice_}
    assert blk["size"] <= r["hist"]                      # the block comes first
    for part, nxt in zip(PLAN, PLAN[1:]):
        assert r[part] + sizes[part] <= r[nxt], (part, nxt)
    assert all(r[part] % 8 == 0 for part in PLAN)
    # what a launch clears: the block and the histogram (and the cursors), nothing per item
    assert r["hist"] + 4 * BINS <= clear <= r["perm"]
    assert 32 <= blk["size"] and blk["slices"] + 8 <= blk["size"]


@pytest.mark.parametrize("space", [1, 2, 40, 1022, 1023, 1024, 2046, 2047, 4096, 8192, 16384,
                                   8192 + (1 << 20), 0xFFFFFFFF])
def test_bins(hc, space):  # noqa: F811
    _, shift = _bin(hc, 0, space)
    # the smallest shift at which the live indices fall into the BINS - 1 key bins
    assert (space - 1) >> shift < BINS - 1
    assert shift == 0 or (space - 1) >> (shift - 1) >= BINS - 1
    probes = sorted(k for k in {0, 1, space // 2, space - 1, (1 << shift) - 1, 1 << shift}
                    if k < space)
    last = -1
    for kk in probes:
        b, s = _bin(hc, kk, space)
        assert s == shift and b == kk >> shift and last <= b < BINS - 1
        last = b
    # no live key: the index past the space, any index beyond it, kNoKey
    for kk in {space, min(space + 5, NO_KEY), NO_KEY}:
        assert _bin(hc, kk, space)[0] == BINS - 1


def test_bins_without_live_keys(hc):  # noqa: F811
    assert _bin(hc, 0, 0) == (BINS - 1, 0) and _bin(hc, NO_KEY, 0) == (BINS - 1, 0)

