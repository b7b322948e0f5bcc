// create3_words.cpp — TEST-ONLY: prints what the message builders of a CREATE3 job (vgen_amd/csrc/core/hash.h, compiled for the host)
// make of inputs given on the command line, for tests/test_create3.py to hold against bytes laid out in Python.
//   create3_words guard <guard hex or -> <24-byte prefix hex> <counter>   -> the 26 words after create3_guard_place_counter, then
//                                                                            the 8 words of keccak256_guard_digest
//   create3_words shift <20-byte factory hex> <32-byte hash hex> <32-byte digest hex>
//                                                                         -> the 22 words after create3_place_digest
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../vgen_amd/csrc/core/hash.h"

static std::vector<uint8_t> unhex(const char *s) {
    std::vector<uint8_t> out;
    if (!strcmp(s, "-")) return out;
    for (size_t i = 0; i + 1 < strlen(s); i += 2) out.push_back((uint8_t)strtoul(std::string(s + i, 2).c_str(), nullptr, 16));
    return out;
}

int main(int argc, char **argv) {
    using namespace vg;
    if (argc == 5 && !strcmp(argv[1], "guard")) {
        const std::vector<uint8_t> g = unhex(argv[2]), pre = unhex(argv[3]);
        if (g.size() > 64 || pre.size() != 24) return 2;
        const unsigned long long counter = strtoull(argv[4], nullptr, 0);
        u32 w[26], d[8];
        create3_guard_message(g.data(), (int)g.size(), pre.data(), w);
        create3_guard_place_counter(w, (u32)g.size() + 24u, counter);
        keccak256_guard_digest(w, d);
        for (int i = 0; i < 26; i++) printf("%08x ", w[i]);
        for (int i = 0; i < 8; i++) printf("%08x ", d[i]);
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "shift")) {
        const std::vector<uint8_t> f = unhex(argv[2]), h = unhex(argv[3]), dg = unhex(argv[4]);
        if (f.size() != 20 || h.size() != 32 || dg.size() != 32) return 2;
        const uint8_t zero[32] = {0};
        u32 m[22], d[8];
        memcpy(d, dg.data(), 32);   // the digest's words in memory order, as the block leaves them (little-endian host)
        create2_message(f.data(), zero, h.data(), m);
        create3_place_digest(m, d);
        for (int i = 0; i < 22; i++) printf("%08x ", m[i]);
        printf("\n");
        return 0;
    }
    return 2;
}
