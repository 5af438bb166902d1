// lcpc_amd/csrc/sha3.hip -- SHA3-256 and Keccak-256 column hash and Merkle tree (LcCommit<Sha3_256, E>, LcCommit<Keccak256, E>) for
// gfx950: the chain template of chain_dev.h over KeccakChain<DOM> (keccak_dev.h).  The two differ in one constant, the byte DOM that
// opens the padding: 0x06 for SHA3-256 (FIPS 202), 0x01 for Keccak-256 (the pre-FIPS padding, the EVM's KECCAK256).
#include "keccak_dev.h"
#include "chain_dev.h"

namespace lcpc {
LCPC_CHAIN_LAUNCHERS(, KeccakChain<kc::KC_DOM_SHA3>)
LCPC_CHAIN_LAUNCHERS(, KeccakChain<kc::KC_DOM_KECCAK>)
}  // namespace lcpc
