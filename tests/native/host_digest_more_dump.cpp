// keccak256_host and sha256_host of lcpc_amd/csrc/host_crypto.cpp (what lcpc_verify hashes opened columns and path nodes with under
// LCPC_HASH_KECCAK256 / LCPC_HASH_SHA256) over a fixed byte pattern, for tests/test_host_digests_more.py to compare with its
// references: reads message lengths from stdin, one per line, and writes "<len> <keccak-256 hex> <sha-256 hex> <sha3-256 hex>" per
// length (SHA3-256 rides along: the same sponge with the other domain byte must keep its digests).  msg[i] = (7 i + 3) mod 256 in a
// heap buffer exactly as long as asked, so a read past the end is an AddressSanitizer finding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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
    uint8_t k[32], s2[32], s3[32];
    lcpc::keccak256_host(msg, len, k);
    lcpc::sha256_host(msg, len, s2);
    lcpc::sha3_256_host(msg, len, s3);
    printf("%llu ", len); hex(k, 32); printf(" "); hex(s2, 32); printf(" "); hex(s3, 32); printf("\n");
    free(msg);
  }
  return 0;
}
