// csrc/raw_setup.h on the host: for every case of CASES.bin, the RawSetup built the way the setters and the one-shot converters build it
// (set_table / set_color / set_shading), the bytes a raw kernel stages for it (raw_staged, raw_staged_size) and what a launch is given
// (raw_stages), against what the test wrote from the Python definitions.
//
//   raw_setup_host CASES.bin
//
// CASES.bin, little-endian, case after case until the end of the file:
//   int32 layout, table, stage, map         the raw layout's number and which parts are set (0 / 1)
//   int32 bits, pack, staged                what is expected: RawStages::bits and ::pack, the number of staged bytes (0: none, table null)
//   uint8 table[4 << bits]; int16 ccm[9]; uint8 curve[256]; int32 black[4]; uint16 mesh[4][2][3]     read whether set or not
//   uint8 expected[staged]
// Table, mesh and the expected bytes live in heap blocks of exactly their size (the sanitizer build: a read outside them is an error).  The
// device pointers of the holder are two host addresses that nobody follows.  Exit code 4 and a line on stderr: a case differs.  Prints
// "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "raw_setup.h"

template <class T>
static T* read_block(FILE* f, size_t count) {
    if (count == 0) return nullptr;
    T* p = static_cast<T*>(std::malloc(count * sizeof(T)));
    if (!p || std::fread(p, sizeof(T), count, f) != count) std::exit(2);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    static uint32_t device_table[1];
    static uint16_t device_gain[1];
    int32_t head[7];
    int cases = 0;
    while (std::fread(head, sizeof head, 1, f) == 1) {
        const int layout = head[0], bits = head[4], pack = head[5];
        const bool table = head[1] != 0, stage = head[2] != 0, map = head[3] != 0;
        const size_t staged = (size_t)head[6];
        if (bits != 8 && bits != 10 && bits != 12) return 2;
        uint8_t* lut = read_block<uint8_t>(f, (size_t)4 << bits);
        int16_t* ccm = read_block<int16_t>(f, 9);
        uint8_t* curve = read_block<uint8_t>(f, 256);
        int32_t* black = read_block<int32_t>(f, 4);
        uint16_t* mesh = read_block<uint16_t>(f, 4 * 2 * 3);
        uint8_t* want = read_block<uint8_t>(f, staged);

        lt::RawSetup s;
        s.layout = layout;
        // every part set and taken back once first: what is staged is a function of what is set NOW
        s.set_table(lut), s.set_color(ccm, curve), s.set_shading(mesh, 3, 2, black);
        s.set_table(nullptr), s.color = false, s.drop_shading();
        if (map) s.set_shading(mesh, 3, 2, black);
        if (stage) s.set_color(ccm, curve);
        if (table) s.set_table(lut);
        std::free(lut), std::free(ccm), std::free(curve), std::free(black), std::free(mesh);      // (the value holds copies)

        const std::vector<uint8_t> got = lt::raw_staged(s);
        lt::RawDevice d;
        d.table = device_table, d.table_bytes = got.size(), d.gain = device_gain;
        const lt::RawStages r = lt::raw_stages(s, d);
        const bool same = got.size() == staged && lt::raw_staged_size(s) == staged && (staged == 0 || std::memcmp(got.data(), want, staged) == 0);
        const bool fields = r.bits == bits && r.pack == pack && r.color == stage && (r.table != nullptr) == (staged != 0) &&
                            r.table == (staged ? device_table : nullptr) && r.gains == (map ? device_gain : nullptr);
        std::free(want);
        if (!same || !fields) {
            std::fprintf(stderr, "case %d (layout %d, table %d, stage %d, map %d): staged %zu bytes (expected %zu), %s; bits %d pack %d color %d table %s gains %s\n",
                         cases, layout, (int)table, (int)stage, (int)map, got.size(), staged, same ? "equal" : "DIFFERENT", r.bits, r.pack, (int)r.color,
                         r.table ? "set" : "null", r.gains ? "set" : "null");
            return 4;
        }
        ++cases;
    }
    std::fclose(f);
    // a layout that is not raw stages nothing and launches the plain kernels, whatever the value held before
    lt::RawSetup none;
    none.layout = 1;
    lt::RawDevice d;
    d.table = device_table, d.gain = device_gain;
    const lt::RawStages r = lt::raw_stages(none, d);
    if (lt::raw_staged_size(none) != 0 || !lt::raw_staged(none).empty() || r.table || r.gains || r.color || r.bits != 8 || r.pack != -1) return 4;
    std::printf("ok %d\n", cases);
    return 0;
}
