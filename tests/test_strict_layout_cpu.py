"""The two device regions of an unkeyed two-pass strict launch and their counter blocks
(narwhal_amd/csrc/nw_strict_layout.hpp: strict_region_plan, comb_region_plan, triage_block_t,
comb_block_t), read through tools/libnw_hostcheck.so (hc_strict_layout). Every offset is pinned
to the formula written out here, the parts are in order and disjoint, the tables are 256-byte
aligned, and the block fields sit where the kernels and the counters' reader expect them."""
import ctypes

import pytest

from test_hostcheck import hc  # noqa: F401  (the library fixture)

PLANES, BLOCK, KEY_TAB = 42, 2048, 1024
# the 8-bit comb tables of one key: 32 tables of 129 entries of 128 bytes, then 2 + 32 points of
# 160 bytes (key_tables_bytes); a region without hot keys still holds room for one key
KEY_TABLES_8 = 128 * 32 * 129 + 160 * (2 + 32)
SHAPES = [(64, 0, 0), (64, 64, 0), (64, 64, 1), (192, 256, 3), (1 << 24, 1 << 20, 8192)]
STRICT = ["list", "keyslot", "block", "slots", "kflags", "ktabs", "bytes"]
COMB = ["todo", "uses", "hotidx", "match", "hotrow", "hok", "tabs", "bytes"]
TRIAGE_BLOCK = {"count": 0, "nkeys": 4, "keys_tabulated": 8, "with_slot": 1024, "size": 2048}
COMB_BLOCK = {"nhot": 0, "todo_count": 4, "nlive": 8, "hot_keys": 16, "checked": 24, "listed": 32,
              "matched": 40, "laddered": 48, "lane_checked": 1024, "lane_reg_items": 1280,
              "lane_reg_passed": 1536, "lane_settled": 1792, "size": 2048}
KEY_STAT_LANES, COMB_STAT_LANES = 128, 32


def _layout(hc, slice_, key_slots, hot_cap):  # noqa: F811
    out = (ctypes.c_uint64 * 64)()
    hc.hc_strict_layout.restype = ctypes.c_int
    hc.hc_strict_layout.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p]
    n = hc.hc_strict_layout(slice_, key_slots, hot_cap, out)
    assert n == len(STRICT) + len(COMB) + len(TRIAGE_BLOCK) + len(COMB_BLOCK)
    v = [int(x) for x in out[:n]]
    a, b, c = len(STRICT), len(STRICT) + len(COMB), len(STRICT) + len(COMB) + len(TRIAGE_BLOCK)
    return (dict(zip(STRICT, v[:a])), dict(zip(COMB, v[a:b])), dict(zip(TRIAGE_BLOCK, v[b:c])),
            dict(zip(COMB_BLOCK, v[c:])))


@pytest.mark.parametrize("slice_,key_slots,hot_cap", SHAPES)
def test_region_plans(hc, slice_, key_slots, hot_cap):  # noqa: F811
    r, c, _, _ = _layout(hc, slice_, key_slots, hot_cap)
    want_r = {"list": 4 * PLANES * slice_}
    want_r["keyslot"] = want_r["list"] + 4 * slice_
    want_r["block"] = want_r["keyslot"] + 4 * slice_
    want_r["slots"] = want_r["block"] + BLOCK
    want_r["kflags"] = want_r["slots"] + 4 * key_slots
    want_r["ktabs"] = want_r["kflags"] + 4 * key_slots + 256
    want_r["bytes"] = want_r["ktabs"] + KEY_TAB * key_slots
    assert r == want_r
    want_c = {"todo": BLOCK}
    want_c["uses"] = want_c["todo"] + 4 * slice_
    want_c["hotidx"] = want_c["uses"] + 4 * key_slots
    want_c["match"] = want_c["hotidx"] + 4 * key_slots
    want_c["hotrow"] = want_c["match"] + 4 * key_slots
    want_c["hok"] = want_c["hotrow"] + 4 * hot_cap
    want_c["tabs"] = (want_c["hok"] + 4 * hot_cap + 255) // 256 * 256
    want_c["bytes"] = want_c["tabs"] + KEY_TABLES_8 * max(hot_cap, 1)
    assert c == want_c
    # in order and disjoint: each part ends where the next begins, or before it
    sizes_r = {"list": 4 * slice_, "keyslot": 4 * slice_, "block": BLOCK, "slots": 4 * key_slots,
               "kflags": 4 * key_slots, "ktabs": KEY_TAB * key_slots}
    assert 0 < 4 * PLANES * slice_ <= r["list"]          # the planes come first
    for part, nxt in zip(STRICT, STRICT[1:]):
        assert r[part] + sizes_r[part] <= r[nxt], (part, nxt)
    sizes_c = {"todo": 4 * slice_, "uses": 4 * key_slots, "hotidx": 4 * key_slots,
               "match": 4 * key_slots, "hotrow": 4 * hot_cap, "hok": 4 * hot_cap,
               "tabs": KEY_TABLES_8 * hot_cap}
    assert BLOCK <= c["todo"]                            # the block comes first
    for part, nxt in zip(COMB, COMB[1:]):
        assert c[part] + sizes_c[part] <= c[nxt], (part, nxt)
    assert r["ktabs"] % 256 == 0 and c["tabs"] % 256 == 0
    assert r["block"] % 8 == 0


def test_block_fields(hc):  # noqa: F811
    _, _, tb, cb = _layout(hc, 64, 64, 1)
    assert tb == TRIAGE_BLOCK and cb == COMB_BLOCK
    assert tb["size"] == cb["size"] == BLOCK
    # the lane arrays fit: 64-bit counters, back to back, the last one ending with the block
    assert tb["with_slot"] + 8 * KEY_STAT_LANES == tb["size"]
    lanes = ["lane_checked", "lane_reg_items", "lane_reg_passed", "lane_settled"]
    for a, b in zip(lanes, lanes[1:] + ["size"]):
        assert cb[a] + 8 * COMB_STAT_LANES == cb[b]
