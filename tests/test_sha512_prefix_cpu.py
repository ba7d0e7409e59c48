"""sha512_prefix_lane<8> (narwhal_amd/csrc/nw_sha512.hpp), the lane function that hashes
prefix || M for signing over messages of any length, compiled for the CPU with the two gfx950
builtins it uses stated as plain functions (tools/prefix_lane_san.cpp, a stand-alone program under
AddressSanitizer / UBSan): the digest at every length 0 .. 400 and every start alignment against
hashlib, and no read outside the aligned dwords that hold a message byte (none at all for an
empty message). No GPU."""
import hashlib
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_length_and_alignment():
    r = subprocess.run(["make", "-s", "tools/prefix_lane_san"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "tools/prefix_lane_san"), "400"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    P = b"".join(struct.pack("<I", (0x0F1E2D3C * (j + 2) + 41) & 0xFFFFFFFF) for j in range(8))
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 401 * 4
    seen, bad = set(), []
    for line in lines:
        ln, al, hx = line.split()
        ln, al = int(ln), int(al)
        seen.add((ln, al))
        msg = bytes((i * 113 + ln * 5 + al) & 255 for i in range(ln))
        if hashlib.sha512(P + msg).hexdigest() != hx:
            bad.append((ln, al))
    assert not bad, bad[:16]
    assert seen == {(ln, al) for ln in range(401) for al in range(4)}
