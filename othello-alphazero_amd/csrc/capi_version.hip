// C ABI, what the library is: its ABI version and the hashes of the sources
// it was built from. The only unit that carries the hashes, so the only one
// rebuilt whenever any source changes (build.py).

#include <cstring>

#include "../../include/othello_mcts_amd.h"

extern "C" {

int oamd_abi_version(void) { return OAMD_ABI_VERSION; }

// build.py passes the source hashes (othello_mcts/provenance.py)
#ifndef OAMD_SOURCE_HASH_ALL
#define OAMD_SOURCE_HASH_ALL "unknown"
#define OAMD_SOURCE_HASH_RESNET "unknown"
#define OAMD_SOURCE_HASH_TREE "unknown"
#endif
const char* oamd_source_hash(const char* family) {
    if (!family) return nullptr;
    if (!std::strcmp(family, "all")) return OAMD_SOURCE_HASH_ALL;
    if (!std::strcmp(family, "resnet")) return OAMD_SOURCE_HASH_RESNET;
    if (!std::strcmp(family, "tree")) return OAMD_SOURCE_HASH_TREE;
    return nullptr;
}

}  // extern "C"
