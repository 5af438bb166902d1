// The host digests of lcpc_amd/csrc/host_crypto.cpp (what lcpc_verify hashes opened columns and path nodes with) over a fixed byte
// pattern, for tests/test_host_digests.py to compare with hashlib: reads message lengths from stdin, one per line, and writes
// "<len> <blake3 hex> <sha3-256 hex> <blake2b hex>" per length.  msg[i] = (7 i + 3) mod 256 behind `len` bytes that are exactly
// as long as asked (a heap buffer of that size, so a read past the end is an AddressSanitizer finding).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_crypto.h"

static void hex(const uint8_t* d, int n) {
  for (int i = 0; i < n; i++) printf("%02x", d[i]);
}

int main() {
  unsigned long long len;
  while (scanf("%llu", &len) == 1) {
    uint8_t* msg = (uint8_t*)malloc(len ? len : 1);
    if (!msg) return 2;
    for (unsigned long long i = 0; i < len; i++) msg[i] = (uint8_t)(7 * i + 3);
    uint8_t b3[32], s3[32], b2[64];
    lcpc::blake3_host(msg, len, b3);
    lcpc::sha3_256_host(msg, len, s3);
    lcpc::blake2b_host(msg, len, b2);
    printf("%llu ", len); hex(b3, 32); printf(" "); hex(s3, 32); printf(" "); hex(b2, 64); printf("\n");
    free(msg);
  }
  return 0;
}
