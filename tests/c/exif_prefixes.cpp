// Every prefix of each file named on the command line through ik::exif_orientation, each
// prefix in a heap block of exactly its length so that a read at or past bytes + len is
// an AddressSanitizer report.  A stand-alone host program (ik_exif.h needs no HIP):
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o exif_prefixes tests/c/exif_prefixes.cpp && ./exif_prefixes FILE...
//
// Prints each file's orientation and the set of values its prefixes gave; exit status 1
// when a prefix gives a value outside 1..8.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rust-image-transform_amd/csrc/ik_exif.h"

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::perror(argv[a]); return 2; }
        std::vector<unsigned char> all;
        unsigned char chunk[4096];
        for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) all.insert(all.end(), chunk, chunk + n);
        std::fclose(f);
        unsigned seen = 0;
        for (size_t k = 0; k <= all.size(); ++k) {
            unsigned char* p = static_cast<unsigned char*>(std::malloc(k ? k : 1));
            if (k) std::memcpy(p, all.data(), k);
            const int v = ik::exif_orientation(p, k);
            std::free(p);
            if (v < 1 || v > 8) { std::printf("%s: prefix %zu gives %d\n", argv[a], k, v); bad = 1; }
            else seen |= 1u << v;
        }
        std::printf("%s: %zu bytes, orientation %d, prefix values mask 0x%x\n", argv[a], all.size(),
                    ik::exif_orientation(all.data(), all.size()), seen);
    }
    return bad;
}
