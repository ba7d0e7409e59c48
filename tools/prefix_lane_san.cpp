// sha512_prefix_lane<8> (narwhal_amd/csrc/nw_sha512.hpp: SHA-512 of a 32-byte prefix followed by
// msg on one lane, the hash behind r of signing over messages of any length) compiled for the CPU
// under AddressSanitizer / UBSan, as a stand-alone program (make tools/prefix_lane_san; the
// stand-in for the HIP header is tools/hram_san/hip/hip_runtime.h). For every length 0 .. max
// (argv[1], default 400) and every start alignment 0 .. 3 it hashes a message that lies in a heap
// block of exactly the aligned dwords that hold a message byte (none for an empty message: the
// pointer is then 32 bytes past a 16-byte block), so a read outside the rule of load_block_tail
// stops the program, and prints "len align digest"; tests/test_sha512_prefix_cpu.py compares with
// hashlib.
#include <stdio.h>
#include <stdlib.h>

#include "nw_sha512.hpp"

int main(int argc, char** argv) {
  const int max_len = argc > 1 ? atoi(argv[1]) : 400;
  uint32_t P[8];
  for (int j = 0; j < 8; ++j) P[j] = 0x0f1e2d3cu * (uint32_t)(j + 2) + 41u;
  for (int len = 0; len <= max_len; ++len)
    for (int al = 0; al < 4; ++al) {
      uint8_t* buf;
      uint8_t* msg;
      if (len == 0) {
        buf = (uint8_t*)malloc(16);
        msg = buf + 48 + al;
      } else {
        buf = (uint8_t*)malloc(((size_t)al + (size_t)len + 3) & ~(size_t)3);
        msg = buf + al;
      }
      for (int i = 0; i < len; ++i) msg[i] = (uint8_t)(i * 113 + len * 5 + al);
      uint32_t x[16];
      nw::sha512_prefix_lane<8>(x, P, msg, (uint64_t)len);
      printf("%d %d ", len, al);
      for (int i = 0; i < 64; ++i) printf("%02x", ((const uint8_t*)x)[i]);
      printf("\n");
      free(buf);
    }
  return 0;
}
