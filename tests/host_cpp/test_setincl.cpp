// Host build of csrc/zkv_setincl.h (the keccak-256 Merkle hashes of the RISC Zero set-inclusion path): one request per input line, one
// 32-byte digest in hex per output line.  tests/test_risc0_set_inclusion_host.py feeds it the hash cases of
// tests/golden/set_inclusion_cases.json, once as a plain build and once under -fsanitize=address,undefined.
//   K <msg | ->            keccak256 of a message of fewer than 136 bytes
//   L <claim>              leaf = keccak256("LEAF_TAG" || claim)
//   N <a> <b>              node(a, b)
//   W <claim> <path | ->   the walk from the claim's leaf over the path's siblings (any depth)
//   J <id> <root>          sha256(id || root)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_setincl.h"

using namespace zkv;

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> v;
    if (!strcmp(s, "-")) return v;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        unsigned b;
        if (sscanf(s + i, "%2x", &b) != 1) { fprintf(stderr, "bad hex\n"); exit(2); }
        v.push_back((uint8_t)b);
    }
    return v;
}
static void words_le(const std::vector<uint8_t>& b, uint32_t w[8]) { SiblingBytes{b.data()}(0, w); }
static void words_be(const std::vector<uint8_t>& b, uint32_t w[8]) { for (int j = 0; j < 8; j++) w[j] = load_be32(b.data() + 4 * j); }
static void put_le(const uint32_t w[8]) {
    for (int j = 0; j < 8; j++) for (int k = 0; k < 4; k++) printf("%02x", (w[j] >> (8 * k)) & 255u);
    printf("\n");
}
static void put_be(const uint32_t w[8]) {
    for (int j = 0; j < 8; j++) printf("%08x", w[j]);
    printf("\n");
}

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<char*> tok;
        for (char* t = strtok(line, " \r\n"); t; t = strtok(nullptr, " \r\n")) tok.push_back(t);
        if (tok.empty()) continue;
        uint32_t a[8], b[8], out[8];
        const char op = tok[0][0];
        if (op == 'K' && tok.size() == 2) {
            // an exact-size heap copy, so that a read past the message is a sanitizer finding
            std::vector<uint8_t> m = unhex(tok[1]);
            if (m.size() >= 136) return 2;
            uint8_t* exact = m.empty() ? nullptr : new uint8_t[m.size()];
            if (exact) memcpy(exact, m.data(), m.size());
            keccak256_short(exact, (uint32_t)m.size(), out);
            delete[] exact;
            put_le(out);
        } else if (op == 'L' && tok.size() == 2) {
            std::vector<uint8_t> c = unhex(tok[1]);
            if (c.size() != 32) return 2;
            words_be(c, a);
            setincl_leaf(a, out);
            put_le(out);
        } else if (op == 'N' && tok.size() == 3) {
            std::vector<uint8_t> x = unhex(tok[1]), y = unhex(tok[2]);
            if (x.size() != 32 || y.size() != 32) return 2;
            words_le(x, a); words_le(y, b);
            setincl_node(a, b, out);
            put_le(out);
        } else if (op == 'W' && tok.size() == 3) {
            std::vector<uint8_t> c = unhex(tok[1]), p = unhex(tok[2]);
            if (c.size() != 32 || p.size() % 32) return 2;
            words_be(c, a);
            setincl_leaf(a, out);
            uint8_t* exact = p.empty() ? nullptr : new uint8_t[p.size()];
            if (exact) memcpy(exact, p.data(), p.size());
            setincl_walk(out, (uint32_t)(p.size() / 32), SiblingBytes{exact});
            delete[] exact;
            put_le(out);
        } else if (op == 'J' && tok.size() == 3) {
            std::vector<uint8_t> id = unhex(tok[1]), r = unhex(tok[2]);
            if (id.size() != 32 || r.size() != 32) return 2;
            words_be(id, a); words_le(r, b);
            setincl_root_journal(a, b, out);
            put_be(out);
        } else {
            fprintf(stderr, "bad request\n");
            return 2;
        }
    }
    return 0;
}
