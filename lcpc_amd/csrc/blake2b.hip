// lcpc_amd/csrc/blake2b.hip -- BLAKE2b-512 column hash and Merkle tree (LcCommit<Blake2b, E>) for gfx950: the chain template of
// chain_dev.h over Blake2bChain (blake2b_dev.h).  LcCommit.hashes is [2 np2 - 1][16] words for a BLAKE2b encoder.
#include "blake2b_dev.h"
#include "chain_dev.h"

namespace lcpc {
LCPC_CHAIN_LAUNCHERS(, Blake2bChain)
}  // namespace lcpc
