// lcpc_amd/csrc/sha256.hip -- SHA-256 column hash and Merkle tree (LcCommit<Sha256, E>) for gfx950: the chain template of chain_dev.h
// over Sha256Chain (sha256_dev.h).
#include "sha256_dev.h"
#include "chain_dev.h"

namespace lcpc {
LCPC_CHAIN_LAUNCHERS(, Sha256Chain)
}  // namespace lcpc
