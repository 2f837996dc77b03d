// What the frames of a raw Bayer layout are conditioned with -- raw table, colour stage, shading map -- as a host value (RawSetup), the bytes a
// raw kernel stages for it (raw_staged) and what a launch is given (raw_stages): plain inline functions without HIP types, for lt_raw.cpp, which
// writes the value to the device (raw_commit), and for a host program (tests/raw_setup_host.cpp) that checks every state with the system
// compiler.  The states, table x stage x map for 8-bit and for 10- / 12-bit layouts: DESIGN.md section 4.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace lt {

// The 10- / 12-bit raw Bayer layouts (32 .. 35, 48 .. 51; pattern = layout & 3): the bits of a sample, 0 for every other layout.  Their frames
// are one plane of 16-bit little-endian words and they are always launched with a table (RawStages).
// Layouts 36 .. 39 / 52 .. 55 (bit 2 set) are the same samples MIPI-packed, one plane of bytes: raw_pack says which packing (mipi_arith.h), -1: none.
inline int raw_wide_bits(int layout) { return layout >= 32 && layout <= 39 ? 10 : layout >= 48 && layout <= 55 ? 12 : 0; }
inline int raw_pack(int layout) { return raw_wide_bits(layout) && (layout & 4) ? (layout >= 48 ? 1 : 0) : -1; }
// the bytes of a row of w sites of a raw layout with 10- / 12-bit samples
inline int raw_wide_row_bytes(int layout, int w) { return raw_pack(layout) == 0 ? w + (w >> 2) : raw_pack(layout) == 1 ? w + (w >> 1) : 2 * w; }
// the bits of a sample of ANY raw layout (8-bit raw Bayer: 16 .. 19), 0 for every other layout
inline int raw_sample_bits(int layout) { return layout >= 16 && layout <= 19 ? 8 : raw_wide_bits(layout); }

// What a launch of the front end over raw Bayer frames runs around the demosaic (`raw`, in the launchers of lt_internal.h; raw_stages, below), and
// the one argument of the raw kernels -- k_raw_walk_rows, k_raw_rows_rgb<.., STAGES>, launched in place of the plain ones whenever there is a table:
//   table  device memory, what the kernel stages in LDS: the raw table the samples are looked up in (lt_set_raw_lut: uint8[4][256], phase-major;
//          lt_set_raw_lut_wide: uint8[4][1 << bits]), behind the 256 bytes of the output curve where there is a colour stage.  Null: no raw
//          kernel, 8-bit frames go through the plain demosaic (10- / 12-bit frames always have a table)
//   bits   of a sample: 8, or 10 / 12 (16-bit little-endian words)
//   color  the colour stage (lt_set_raw_color; bayer_arith.h: color_px) on every demosaiced pixel; cm: its matrix, Q10, row-major
//   gains  not null: the lens-shading correction (lt_set_raw_shading; shade_arith.h) of every sample before its lookup -- device memory, the
//          gain of every site, uint16[h][w] (Q12) and 16 bytes of padding (launch_shade_expand); blk: the pedestal of each colour phase
struct RawColorMat { int32_t m[9]; };
struct RawShadeBlack { int32_t b[4]; };
//   pack   -1, or the packing of 10- / 12-bit samples (mipi_arith.h: 0 RAW10, five bytes for four sites; 1 RAW12, three bytes for two): the
//          kernels' packed forms, k_mipi_walk_rows, k_mipi_rows_rgb<.., STAGES, PACK>
struct RawStages {
    const uint32_t* table = nullptr;
    int bits = 8;
    bool color = false;
    RawColorMat cm = {};
    int pack = -1;                           // (in what was padding: every other member lies where it lay)
    const uint16_t* gains = nullptr;
    RawShadeBlack blk = {};
};

// Everything the frames of `layout` are conditioned with.  Which parts are set decides which kernels are launched; their content never does.
struct RawSetup {
    int layout = 0;                          // a raw layout, or any other one: then nothing below is set
    bool has_table = false;                  // lt_set_raw_lut / lt_set_raw_lut_wide: uint8[4][1 << bits], phase-major
    std::vector<uint8_t> table;
    bool color = false;                      // lt_set_raw_color: the colour-correction matrix (Q10, row-major) and the output curve
    int16_t ccm[9] = {1024, 0, 0, 0, 1024, 0, 0, 0, 1024};
    uint8_t curve[256] = {0};
    bool shade = false;                      // lt_set_raw_shading: the mesh, uint16[4][mesh_h][mesh_w], and the pedestals by colour phase
    std::vector<uint16_t> mesh;
    int mesh_w = 0, mesh_h = 0;
    RawShadeBlack black = {};

    int bits() const { return raw_sample_bits(layout); }
    size_t table_bytes() const { return (size_t)4 << bits(); }
    void set_table(const uint8_t* lut) {     // null: none (8 bits) / the default (10, 12 bits)
        has_table = lut != nullptr;
        table.assign(lut, lut ? lut + table_bytes() : lut);
    }
    void set_color(const int16_t* m, const uint8_t* t) {     // null: the identity, each
        static const int16_t ident[9] = {1024, 0, 0, 0, 1024, 0, 0, 0, 1024};
        color = true;
        std::memcpy(ccm, m ? m : ident, sizeof ccm);
        for (int i = 0; i < 256; ++i) curve[i] = t ? t[i] : (uint8_t)i;
    }
    void set_shading(const uint16_t* m, int mw, int mh, const int32_t* blk) {     // blk null: zeros
        shade = true;
        mesh.assign(m, m + (size_t)4 * mw * mh);
        mesh_w = mw, mesh_h = mh;
        for (int p = 0; p < 4; ++p) black.b[p] = blk ? blk[p] : 0;
    }
    void drop_shading() {
        shade = false, mesh_w = mesh_h = 0, black = {};
        mesh.clear();
    }
};

// The table in effect where none is set, 4 << bits bytes: 8 bits the identity; 10 / 12 bits full scale to full scale, rounded --
// utils.raw_lut(bits=..) with its defaults, in integers (floor(255 s / m + 1 / 2) = (510 s + m) / (2 m), m = 2^bits - 1).
inline void raw_default_table(int bits, uint8_t* lut) {
    const uint32_t n = 1u << bits, m = n - 1u;
    for (uint32_t p = 0; p < 4; ++p)
        for (uint32_t v = 0; v < n; ++v) lut[p * n + v] = bits == 8 ? (uint8_t)v : (uint8_t)((510u * v + m) / (2u * m));
}

// How many bytes a raw kernel stages for `s` (RawStages::table), 0: none, the plain kernels of the layout run -- no raw layout at all, or 8-bit
// frames with nothing set.  The ONE place that decides it.
inline size_t raw_staged_size(const RawSetup& s) {
    if (s.bits() == 0 || (s.bits() == 8 && !s.has_table && !s.color && !s.shade)) return 0;
    return (s.color ? 256 : 0) + s.table_bytes();
}
// ... and the bytes: the curve's 256 where there is a colour stage, then the table -- the caller's, or the default (8 bits: the identity, which
// a stage or a map brings along)
inline std::vector<uint8_t> raw_staged(const RawSetup& s) {
    std::vector<uint8_t> t(raw_staged_size(s));
    if (t.empty()) return t;
    const size_t head = s.color ? 256 : 0;
    if (s.color) std::memcpy(t.data(), s.curve, 256);
    if (s.has_table) std::memcpy(t.data() + head, s.table.data(), s.table_bytes());
    else raw_default_table(s.bits(), t.data() + head);
    return t;
}

// Raw sets (lt_add_raw_set): a context holds several RawSetups, one per kind of camera, and a launch whose slots mix sets runs ONE kernel --
// the stages of the UNION of the parts the sets have.  A set that lacks a part runs that part's identity, each exact in the integer
// definitions: the identity table (8 bits), the matrix 1024 I with the identity curve, a plane of unit gains (Q12 4096) with pedestals 0.
struct RawUnion {
    bool staged = false;                     // some set stages a table: the raw kernels run
    bool color = false, shade = false;
};
inline void raw_union_add(RawUnion& u, const RawSetup& s) {
    u.staged = u.staged || raw_staged_size(s) != 0;
    u.color = u.color || s.color;
    u.shade = u.shade || s.shade;
}
// the bytes a set-per-slot kernel stages for `s` in a launch with (or without) a colour stage: raw_staged's, the identity curve in front of
// them where the launch has a stage and `s` has none, the identity table where `s` stages nothing of its own
inline std::vector<uint8_t> raw_staged_as(const RawSetup& s, bool color) {
    if (s.bits() == 0) return {};
    if (s.color == color && raw_staged_size(s)) return raw_staged(s);
    RawSetup u;                              // (without the mesh: nothing here reads it)
    u.layout = s.layout, u.has_table = s.has_table, u.table = s.table;
    if (s.color) u.set_color(s.ccm, s.curve);
    else if (color) u.set_color(nullptr, nullptr);
    std::vector<uint8_t> t((color ? 256 : 0) + u.table_bytes());
    if (color) std::memcpy(t.data(), u.curve, 256);
    if (u.has_table) std::memcpy(t.data() + (color ? 256 : 0), u.table.data(), u.table_bytes());
    else raw_default_table(u.bits(), t.data() + (color ? 256 : 0));
    return t;
}
// One set as the set-per-slot kernels find it: entry `id` of the context's table of raw sets (device memory, rewritten behind a full
// synchronisation whenever a set changes).  What RawStages holds by value, per set: the staged bytes (raw_staged_as the union), the gain
// plane (the set's, or the one plane of unit gains that all sets without a map share), the matrix and the pedestals.  A slot's set is
// wave-uniform: an entry arrives by scalar loads.
struct RawSetEntry {
    const uint32_t* table;
    const uint16_t* gains;
    RawColorMat cm;
    RawShadeBlack blk;
    int32_t pad[3];
};
static_assert(sizeof(RawSetEntry) == 80, "RawSetEntry: 80 bytes");
inline RawSetEntry raw_set_entry(const RawSetup& s, const uint32_t* table, const uint16_t* gains) {
    RawSetEntry e{};
    e.table = table, e.gains = gains;
    for (int i = 0; i < 9; ++i) e.cm.m[i] = s.color ? s.ccm[i] : (i % 4 == 0 ? 1024 : 0);
    if (s.shade) e.blk = s.black;
    return e;
}
// What selects the kernel of a launch that mixes the sets of `u` (layout: the context's).  Its pointers only say "there is one" -- a
// set-per-slot kernel reads its slot's entry, never them -- so both are the set table's address.
inline RawStages raw_union_stages(int layout, const RawUnion& u, const RawSetEntry* sets) {
    RawStages r;
    if (raw_sample_bits(layout) == 0 || !u.staged) return r;
    r.bits = raw_sample_bits(layout);
    r.pack = raw_pack(layout);
    r.table = reinterpret_cast<const uint32_t*>(sets);
    r.color = u.color;
    r.gains = u.shade ? reinterpret_cast<const uint16_t*>(sets) : nullptr;
    return r;
}

// What a RawSetup is on the device: ONE buffer of what the kernels stage (raw_staged; reallocated only when that size changes, kept until the
// owner goes -- also while nothing is staged) and the gain plane that k_shade_expand makes of the mesh -- uint16[h][w] and 16 bytes of
// padding, allocated by the first map, freed when the map is removed.  Written by raw_commit and freed by raw_release alone (lt_raw.cpp).
struct RawDevice {
    uint32_t* table = nullptr;
    size_t table_bytes = 0;
    uint16_t* gain = nullptr;
};

// What a launch over frames conditioned with `s`, committed to `d`, is given.
inline RawStages raw_stages(const RawSetup& s, const RawDevice& d) {
    RawStages r;
    if (s.bits() == 0) return r;
    r.bits = s.bits();
    r.pack = raw_pack(s.layout);
    r.table = raw_staged_size(s) ? d.table : nullptr;
    r.color = s.color;
    for (int i = 0; i < 9; ++i) r.cm.m[i] = s.ccm[i];
    r.gains = s.shade ? d.gain : nullptr;
    r.blk = s.black;
    return r;
}

}  // namespace lt
