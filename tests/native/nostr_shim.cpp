// nostr_shim.cpp — host build (g++) of what the kernels evaluate for the Nostr format (VGF_NOSTR): the prefilter
// (core/filter_eval.h filter_eval_npub, with and without the filter's checksum tables) and the on-device automaton
// (core/dfa_eval.h dfa_match_npub) on payloads the test chooses, beside the exact automaton on the host-encoded string.
// (tests/test_nostr.py)
#include <string.h>

#include <string>

#include "../../vgen_amd/csrc/core/dfa_eval.h"
#include "../../vgen_amd/csrc/core/filter_eval.h"
#include "../../vgen_amd/csrc/host/encode.h"
#include "../../vgen_amd/csrc/host/filter.h"

using namespace vg;

extern "C" {

// Compiles `pattern` for the format and judges n payloads of 32 bytes.  out_flags[i]: bit 0 = the device test accepts (kinds 1 - 3:
// filter_eval_npub; kind 4: dfa_match_npub), bit 1 = the exact automaton accepts the npub string, bit 2 = the device test without
// the checksum tables (the step-by-step polymod) accepts.  info: kind, count, flags, has checksum tables.  -1 on a pattern error.
int nostr_filter_check(const char *pattern, int ci, const unsigned char *payloads, int n, unsigned char *out_flags, unsigned *info) {
    vgen_filter f;
    std::string err;
    if (!filter_compile(pattern, ci != 0, VGF_NOSTR, f, err)) return -1;
    info[0] = f.dev.kind;
    info[1] = f.dev.count;
    info[2] = f.dev.flags;
    info[3] = f.dev.chk_lut ? 1u : 0u;
    DevFilter bare = f.dev;
    bare.chk_lut = nullptr;
    for (int i = 0; i < n; i++) {
        u32 pl[8];
        memcpy(pl, payloads + 32 * i, 32);
        int dev, dev_bare;
        if (f.dev.kind == DEVF_DFA) {
            dev = dev_bare = dfa_match_npub(f.dfa_blob.data(), pl) ? 1 : 0;
        } else {
            dev = filter_eval_npub(&f.dev, pl) ? 1 : 0;
            dev_bare = filter_eval_npub(&bare, pl) ? 1 : 0;
        }
        const std::string addr = address_from_payload(VGF_NOSTR, payloads + 32 * i);
        out_flags[i] = (unsigned char)(dev | ((f.dfa.is_match(addr) ? 1 : 0) << 1) | (dev_bare << 2));
    }
    return 0;
}

}
