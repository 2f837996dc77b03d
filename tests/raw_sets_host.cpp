// csrc/raw_setup.h on the host: the bookkeeping of raw sets -- the union of the parts the sets of a context have (raw_union_add), the bytes a
// set-per-slot kernel stages for a set in the union's form (raw_staged_as), the set's entry of the set table (raw_set_entry) and what selects
// the kernel of a mixed launch (raw_union_stages) -- for every pair (set, union) of the eight states table x stage x map of an 8-bit, a
// 10-bit, a packed 12-bit layout.  Needs no input: the values are made here, from a fixed generator.
//
// Held for every pair: a set whose own form is the union's stages raw_staged's bytes; a set without a colour stage in a union with one stages
// the identity curve, then its table; a set that stages nothing of its own (8 bits, nothing set) stages the identity table; the entry's
// matrix is the set's or 1024 I, its pedestals the set's or zeros; the sizes are the union kernel's (256 for the curve + 4 << bits).
// Exit code 4 and a line on stderr: a case differs.  Prints "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "raw_setup.h"

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static int fail(const char* what, int layout, int s, int u) {
    std::fprintf(stderr, "layout %d, set state %d, union state %d: %s\n", layout, s, u, what);
    return 4;
}

static lt::RawSetup make(int layout, int state) {
    lt::RawSetup r;
    r.layout = layout;
    if (state & 1) {
        std::vector<uint8_t> t(r.table_bytes());
        for (auto& b : t) b = (uint8_t)(rnd() >> 24);
        r.set_table(t.data());
    }
    if (state & 2) {
        int16_t m[9];
        uint8_t c[256];
        for (auto& v : m) v = (int16_t)(rnd() >> 16);
        for (auto& v : c) v = (uint8_t)(rnd() >> 24);
        r.set_color(m, c);
    }
    if (state & 4) {
        std::vector<uint16_t> mesh(4 * 2 * 3);
        for (auto& v : mesh) v = (uint16_t)(rnd() >> 16);
        const int32_t blk[4] = {1, 2, 3, 4};
        r.set_shading(mesh.data(), 3, 2, blk);
    }
    return r;
}

int main() {
    int cases = 0;
    for (int layout : {17, 33, 54}) {
        const int bits = lt::raw_sample_bits(layout);
        std::vector<uint8_t> ident_table((size_t)4 << bits);
        lt::raw_default_table(bits, ident_table.data());
        for (int s = 0; s < 8; ++s)
            for (int o = 0; o < 8; ++o) {
                const lt::RawSetup a = make(layout, s), b = make(layout, o);
                lt::RawUnion u;
                lt::raw_union_add(u, a);
                lt::raw_union_add(u, b);
                const int us = s | o;
                if (u.color != ((us & 2) != 0) || u.shade != ((us & 4) != 0)) return fail("the union's parts", layout, s, us);
                if (u.staged != (bits > 8 || us != 0)) return fail("whether the union stages", layout, s, us);
                const lt::RawStages k = lt::raw_union_stages(layout, u, reinterpret_cast<const lt::RawSetEntry*>(&u));
                if (!u.staged) {
                    if (k.table) return fail("a kernel where nothing is staged", layout, s, us);
                    ++cases;
                    continue;
                }
                if (!k.table || k.bits != bits || k.color != u.color || (k.gains != nullptr) != u.shade || k.pack != lt::raw_pack(layout))
                    return fail("what selects the kernel", layout, s, us);
                const std::vector<uint8_t> t = lt::raw_staged_as(a, u.color);
                const size_t head = u.color ? 256 : 0;
                if (t.size() != head + ((size_t)4 << bits)) return fail("the staged size", layout, s, us);
                if (a.color == u.color && lt::raw_staged_size(a) && t != lt::raw_staged(a)) return fail("its own form is not raw_staged's", layout, s, us);
                for (size_t i = 0; i < head; ++i)
                    if (t[i] != (a.color ? a.curve[i] : (uint8_t)i)) return fail("the curve", layout, s, us);
                if (std::memcmp(t.data() + head, a.has_table ? a.table.data() : ident_table.data(), (size_t)4 << bits)) return fail("the table", layout, s, us);
                const uint32_t tab = 0;
                const uint16_t gain = 0;
                const lt::RawSetEntry e = lt::raw_set_entry(a, &tab, &gain);
                if (e.table != &tab || e.gains != &gain) return fail("the entry's pointers", layout, s, us);
                for (int i = 0; i < 9; ++i)
                    if (e.cm.m[i] != (a.color ? a.ccm[i] : (i % 4 == 0 ? 1024 : 0))) return fail("the entry's matrix", layout, s, us);
                for (int i = 0; i < 4; ++i)
                    if (e.blk.b[i] != (a.shade ? a.black.b[i] : 0)) return fail("the entry's pedestals", layout, s, us);
                ++cases;
            }
    }
    std::printf("ok %d\n", cases);
    return 0;
}
