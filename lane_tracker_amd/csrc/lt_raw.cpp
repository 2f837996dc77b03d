// What the raw Bayer frames of liblane_tracker_amd.so are conditioned with: raw table, colour stage, shading map.  The three are ONE host value
// (RawSetup, raw_setup.h), written to the device in one place (raw_commit), for the contexts' setters -- each edits a copy of the context's value
// and adopts it -- and for the one-shot converters, which commit a value of their own for the length of a call.  With them what reads the
// same state: the getters, lt_get_raw_shading_plane, lt_raw_stats.  DESIGN.md section 4 holds the table of states.  See lt_ctx.h.
#include <algorithm>
#include <cstring>
#include <vector>

#include "lt_ctx.h"
#include "shade_arith.h"
#include "stats_arith.h"

using namespace lt;

// ---- checks ----------------------------------------------------------------------------------------------------------------------------
// Raw Bayer: whole 2 x 2 blocks, and a 4 x 4 window of bytes (the neighbourhoods of a sample's four taps) inside the plane; MIPI-packed RAW10
// holds four sites in five bytes, so a row is whole groups
int lt::check_raw_size(int layout, int h, int w) {
    if (h < 4 || w < 4 || (h & 1) || (w & 1)) return fail(LT_ERR_INVALID, "raw Bayer frames need an even width and height of at least 4, got %dx%d", w, h);
    if (raw_packing(layout) == 0 && (w & 3)) return fail(LT_ERR_INVALID, "MIPI-packed RAW10 frames need a width that is a multiple of 4, got %dx%d", w, h);
    return LT_OK;
}
int lt::check_one_shot_size(int layout, int h, int w) {
    if (int rc = is_raw_mosaic(layout) ? check_raw_size(layout, h, w) : 0) return rc;
    if (h > 16384 || w > 16384) return fail(LT_ERR_INVALID, "bad image size (at most 16384 x 16384)");
    return LT_OK;
}
static int check_shading(int layout, int mesh_w, int mesh_h, const int32_t* black) {
    if (mesh_w < sa::MESH_MIN || mesh_w > sa::MESH_MAX || mesh_h < sa::MESH_MIN || mesh_h > sa::MESH_MAX)
        return fail(LT_ERR_INVALID, "a shading mesh has 2 .. 64 nodes a side, got %d x %d", mesh_w, mesh_h);
    const int smax = (1 << raw_sample_bits(layout)) - 1;
    for (int p = 0; black && p < 4; ++p)
        if (black[p] < 0 || black[p] > smax) return fail(LT_ERR_INVALID, "black[%d] = %d is outside 0 .. %d", p, (int)black[p], smax);
    return LT_OK;
}
static int check_wide(lt_ctx* c, size_t entries) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (!is_bayer_wide(c->in_layout)) return fail(LT_ERR_STATE, "a wide raw table belongs to 10- / 12-bit raw Bayer input: this context's input format is another layout");
    if (entries != (size_t)1 << raw_bits(c->in_layout))
        return fail(LT_ERR_INVALID, "a %d-bit raw table has %d entries per colour phase, got %zu", raw_bits(c->in_layout), 1 << raw_bits(c->in_layout), entries);
    return LT_OK;
}

// ---- the value on the device -------------------------------------------------------------------------------------------------------------
// mesh (host) -> a gain plane of h x w sites and 16 bytes of padding at *plane (device memory, allocated here where it is null), on `st`
static int expand_mesh(hipStream_t st, const uint16_t* mesh, int mesh_w, int mesh_h, int layout, int h, int w, uint16_t** plane) {
    const size_t nodes = (size_t)4 * mesh_w * mesh_h;
    DevBuf<uint16_t> d_mesh;
    int rc;
    if ((rc = d_mesh.alloc(nodes)) || (!*plane && (rc = dev_alloc(plane, (size_t)h * w + 8)))) return rc;
    hipError_t e = hipMemcpyAsync(d_mesh.p, mesh, nodes * sizeof(uint16_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(*plane + (size_t)h * w, 0, 16, st);
    if (e == hipSuccess) {
        launch_shade_expand(st, d_mesh.p, mesh_w, mesh_h, layout & 3, *plane, h, w);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "expanding the shading mesh failed: %s", hipGetErrorString(e));
    return LT_OK;
}

int lt::raw_commit(RawSetup& s, RawDevice& d, bool new_map, hipStream_t st, int h, int w) {
    const std::vector<uint8_t> t = raw_staged(s);
    int rc;
    if (!t.empty()) {
        if (d.table_bytes != t.size()) {
            uint32_t* p = nullptr;
            if ((rc = dev_alloc(&p, t.size() / 4))) return rc;
            dev_free(d.table);
            d.table = p, d.table_bytes = t.size();
        }
        HIP_TRY(hipMemcpy(d.table, t.data(), t.size(), hipMemcpyHostToDevice));
    }
    if (!s.shade) dev_free(d.gain);
    else if (new_map && (rc = expand_mesh(st, s.mesh.data(), s.mesh_w, s.mesh_h, s.layout, h, w, &d.gain))) {
        s.drop_shading();                    // (the plane of a map that was set may hold part of the new one by now)
        dev_free(d.gain);
        return rc;
    }
    return LT_OK;
}

void lt::raw_release(RawDevice& d) {
    dev_free(d.table);
    dev_free(d.gain);
    d.table_bytes = 0;
}

// ---- the setters: validate, then edit ---------------------------------------------------------------------------------------------------
// Set-up or occasional calls (between windows), behind everything the context has in flight; what is launched afterwards reads the new
// value.  Planes and camera frames computed with the old one stay what they are: the slots' front ends are marked as not run, so that a re-run
// (lt_mask_rerun) computes them again.  c->raw := change(a copy of c->raw), on the device first (raw_commit: an error with nothing written
// keeps the old value; a failed expansion has taken the map out of the copy, which is adopted).
// The table of raw sets as the set-per-slot kernels read it, := the sets as they are now -- behind every change of a set, with nothing in
// flight.  One set: nothing to write.  An error leaves the context without a table (raw_sets_ok), so that a launch that mixes sets is refused
// and none reads a stale entry.
static int raw_sets_refresh(lt_ctx* c) {
    const int k = raw_set_count(c);
    RawUnion u;
    for (int id = 0; id < k; ++id) raw_union_add(u, raw_set_of(c, id));
    c->raw_union = u;
    if (k == 1) return LT_OK;
    auto drop = [&](int code) {
        dev_free(c->d_raw_sets);
        return code;
    };
    int rc;
    if (!c->d_raw_sets && (rc = dev_alloc(&c->d_raw_sets, (size_t)LT_MAX_CALIBRATIONS))) return rc;
    const int H = c->calib.img_h, W = c->calib.img_w;
    bool need_unit = false;
    for (int id = 0; id < k; ++id) need_unit = need_unit || (u.shade && !raw_set_of(c, id).shade);
    if (need_unit && !c->d_unit_gain) {                        // Q12 1.0 at every site (the 16 bytes of padding included: never used)
        const std::vector<uint16_t> unit((size_t)H * W + 8, (uint16_t)4096);
        if ((rc = dev_alloc(&c->d_unit_gain, unit.size()))) return drop(rc);
        if (hipMemcpy(c->d_unit_gain, unit.data(), unit.size() * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) {
            dev_free(c->d_unit_gain);
            return drop(fail(LT_ERR_HIP, "writing the plane of unit gains failed: %s", hipGetErrorString(hipGetLastError())));
        }
    }
    if (!need_unit) dev_free(c->d_unit_gain);
    c->union_table.resize((size_t)k);
    std::vector<RawSetEntry> ent((size_t)k);
    for (int id = 0; id < k; ++id) {
        const RawSetup& s = raw_set_of(c, id);
        const RawDevice& d = raw_dev_of(c, id);
        lt_ctx::UnionTable& ut = c->union_table[(size_t)id];
        const uint32_t* table = nullptr;
        if (u.staged && s.color == u.color && raw_staged_size(s)) {     // its own bytes are the union's form
            table = d.table;
            dev_free(ut.p), ut.bytes = 0;
        } else if (u.staged) {
            const std::vector<uint8_t> t = raw_staged_as(s, u.color);
            if (ut.bytes != t.size()) {
                dev_free(ut.p), ut.bytes = 0;
                if ((rc = dev_alloc(&ut.p, t.size() / 4))) return drop(rc);
                ut.bytes = t.size();
            }
            if (hipMemcpy(ut.p, t.data(), t.size(), hipMemcpyHostToDevice) != hipSuccess)
                return drop(fail(LT_ERR_HIP, "writing a raw set's table failed: %s", hipGetErrorString(hipGetLastError())));
            table = ut.p;
        }
        ent[(size_t)id] = raw_set_entry(s, table, s.shade ? d.gain : c->d_unit_gain);
    }
    if (hipMemcpy(c->d_raw_sets, ent.data(), ent.size() * sizeof(RawSetEntry), hipMemcpyHostToDevice) != hipSuccess)
        return drop(fail(LT_ERR_HIP, "writing the table of raw sets failed: %s", hipGetErrorString(hipGetLastError())));
    return LT_OK;
}

void lt::raw_sets_release(lt_ctx* c) {
    for (auto& q : c->raw_more) raw_release(q.d);
    c->raw_more.clear();
    for (auto& t : c->union_table) dev_free(t.p);
    c->union_table.clear();
    dev_free(c->d_raw_sets);
    dev_free(c->d_unit_gain);
    std::fill(c->slot_raw.begin(), c->slot_raw.end(), (uint8_t)0);
    c->raw_union = RawUnion{};
}

static int check_set(lt_ctx* c, int id) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (id < 0 || id >= raw_set_count(c)) return fail(LT_ERR_INVALID, "raw set %d out of range (the context has %d)", id, raw_set_count(c));
    return LT_OK;
}

// set `id` := change(a copy of it)
template <class F>
static int edit(lt_ctx* c, int id, bool new_map, F change) {
    int rc;
    if ((rc = check_set(c, id))) return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    RawSetup& cur = id > 0 ? c->raw_more[(size_t)id - 1].s : c->raw;
    RawDevice& dev = id > 0 ? c->raw_more[(size_t)id - 1].d : c->raw_dev;
    RawSetup next = cur;
    change(next);
    rc = raw_commit(next, dev, new_map, c->stream, c->calib.img_h, c->calib.img_w);
    if (rc != LT_OK && !(new_map && !next.shade)) return rc;
    cur = std::move(next);
    for (size_t i = 0; i < c->front_ok.size(); ++i)
        if (slot_raw_set(c, (int)i) == id) c->front_ok[i] = 0;
    const int rrc = raw_sets_refresh(c);
    return rc ? rc : rrc;
}

// (the sets beyond 0 are of the old layout: they go)
int lt::raw_take_layout(lt_ctx* c, int layout) {
    if (c && !c->raw_more.empty()) {
        int rc;
        if ((rc = set_device(c)) || (rc = sync_all(c))) return rc;
        raw_sets_release(c);
        std::fill(c->front_ok.begin(), c->front_ok.end(), (uint8_t)0);
    }
    return edit(c, 0, false, [&](RawSetup& s) {
        RawSetup next;
        next.layout = layout;
        if (is_bayer(layout) && is_bayer(s.layout) && s.has_table) next.table.swap(s.table), next.has_table = true;     // a raw table belongs to raw Bayer input
        s = std::move(next);
    });
}

// ---- raw sets ------------------------------------------------------------------------------------------------------------------------------
// A new set, a copy of set 0's value at this moment, committed to device buffers of its own.
int lt_add_raw_set(lt_ctx* c, int* id) {
    if (!c || !id) return fail(LT_ERR_INVALID, "null argument");
    if (!is_raw_mosaic(c->in_layout)) return fail(LT_ERR_STATE, "raw sets condition raw Bayer input: this context's input format is another layout");
    if (raw_set_count(c) >= LT_MAX_CALIBRATIONS) return fail(LT_ERR_CAPACITY, "a context holds at most %d raw sets", LT_MAX_CALIBRATIONS);
    int rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    lt_ctx::RawSet q;
    q.s = c->raw;
    if ((rc = raw_commit(q.s, q.d, q.s.shade, c->stream, c->calib.img_h, c->calib.img_w))) {
        raw_release(q.d);
        return rc;
    }
    c->raw_more.push_back(std::move(q));
    if ((rc = raw_sets_refresh(c))) {
        raw_release(c->raw_more.back().d);
        c->raw_more.pop_back();
        (void)raw_sets_refresh(c);
        return rc;
    }
    *id = raw_set_count(c) - 1;
    return LT_OK;
}

int lt_raw_set_count(lt_ctx* c, int* count) {
    if (!c || !count) return fail(LT_ERR_INVALID, "null argument");
    *count = raw_set_count(c);
    return LT_OK;
}

int lt_set_slot_raw_sets(lt_ctx* c, int first, int n, const int32_t* ids) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (n > 0 && !ids) return fail(LT_ERR_INVALID, "null ids");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= raw_set_count(c))
            return fail(LT_ERR_INVALID, "slot %d: raw set %d out of range (the context has %d)", first + i, ids[i], raw_set_count(c));
    // (as lt_set_slot_calibrations: a launch carries the sets of its slots by value; a slot that changes set has planes made with another's)
    for (int i = 0; i < n; ++i) {
        const size_t s = (size_t)(first + i);
        if (c->slot_raw[s] == (uint8_t)ids[i]) continue;
        c->slot_raw[s] = (uint8_t)ids[i];
        front_stale(c, first + i, 1);
    }
    return LT_OK;
}

int lt_get_slot_raw_sets(lt_ctx* c, int first, int n, int32_t* ids) {
    int rc = check_slots(c, first, n);
    if (rc) return rc;
    if (n > 0 && !ids) return fail(LT_ERR_INVALID, "null ids");
    for (int i = 0; i < n; ++i) ids[i] = slot_raw_set(c, first + i);
    return LT_OK;
}

int lt_last_raw_walk_form(lt_ctx* c) { return c ? c->last_raw_walk_form : -1; }

// ---- the setters and getters, of set `id`; the entry points without an id are set 0's -----------------------------------------------------
// the table of any raw layout: uint8[4][entries], entries = 1 << bits
static int check_entries(lt_ctx* c, size_t entries) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (is_bayer_wide(c->in_layout)) return check_wide(c, entries);
    if (!is_bayer(c->in_layout)) return fail(LT_ERR_STATE, "a raw table conditions raw Bayer input: this context's input format is another layout");
    if (entries != 256) return fail(LT_ERR_INVALID, "an 8-bit raw table has 256 entries per colour phase, got %zu", entries);
    return LT_OK;
}
static int set_table(lt_ctx* c, int id, const uint8_t* lut) {
    return edit(c, id, false, [&](RawSetup& s) { s.set_table(lut); });     // (8 bits, null under a map or a stage: the identity stays staged)
}

int lt_set_raw_lut_of(lt_ctx* c, int id, const uint8_t* lut, size_t entries) {
    int rc = check_entries(c, entries);
    if (!rc) rc = check_set(c, id);
    return rc ? rc : set_table(c, id, lut);
}

// 8 bits: the table where one is set (is_set); 10 / 12 bits: the table in effect, is_set = 1
int lt_get_raw_lut_of(lt_ctx* c, int id, uint8_t* lut, size_t entries, int* is_set) {
    int rc = check_entries(c, entries);
    if (!rc) rc = check_set(c, id);
    if (rc) return rc;
    const RawSetup& s = raw_set_of(c, id);
    const bool wide = is_bayer_wide(c->in_layout);
    if (is_set) *is_set = wide || s.has_table ? 1 : 0;
    if (lut && s.has_table) std::memcpy(lut, s.table.data(), s.table.size());
    else if (lut && wide) raw_default_table(s.bits(), lut);
    return LT_OK;
}

int lt_set_raw_lut(lt_ctx* c, const uint8_t* lut) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (is_bayer_wide(c->in_layout)) return fail(LT_ERR_STATE, "a 10- / 12-bit raw Bayer context takes its table through lt_set_raw_lut_wide");
    if (!is_bayer(c->in_layout)) return fail(LT_ERR_STATE, "a raw table conditions raw Bayer input: this context's input format is another layout");
    return set_table(c, 0, lut);
}

int lt_get_raw_lut(lt_ctx* c, uint8_t* lut, int* is_set) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    const bool set = is_bayer(c->in_layout) && c->raw.has_table;
    if (is_set) *is_set = set ? 1 : 0;
    if (lut && set) std::memcpy(lut, c->raw.table.data(), c->raw.table.size());
    return LT_OK;
}

// The table of a 10- / 12-bit context: uint8[4][1 << bits], always one (null: the default again)
int lt_set_raw_lut_wide(lt_ctx* c, const uint8_t* lut, size_t entries) {
    const int rc = check_wide(c, entries);
    return rc ? rc : set_table(c, 0, lut);
}

int lt_get_raw_lut_wide(lt_ctx* c, uint8_t* lut, size_t entries) {
    const int rc = check_wide(c, entries);
    return rc ? rc : lt_get_raw_lut_of(c, 0, lut, entries, nullptr);
}

// enable = 0 removes the stage (ccm and curve are not read)
int lt_set_raw_color_of(lt_ctx* c, int id, const int16_t* ccm, const uint8_t* curve, int enable) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (!is_raw_mosaic(c->in_layout)) return fail(LT_ERR_STATE, "a colour stage follows the demosaic of raw Bayer input: this context's input format is another layout");
    return edit(c, id, false, [&](RawSetup& s) {
        if (enable) s.set_color(ccm, curve);
        else s.color = false;
    });
}
int lt_set_raw_color(lt_ctx* c, const int16_t* ccm, const uint8_t* curve, int enable) { return lt_set_raw_color_of(c, 0, ccm, curve, enable); }

int lt_get_raw_color_of(lt_ctx* c, int id, int16_t* ccm, uint8_t* curve, int* is_set) {
    if (int rc = check_set(c, id)) return rc;
    const RawSetup& s = raw_set_of(c, id);
    if (is_set) *is_set = s.color ? 1 : 0;
    if (ccm && s.color) std::memcpy(ccm, s.ccm, sizeof s.ccm);
    if (curve && s.color) std::memcpy(curve, s.curve, sizeof s.curve);
    return LT_OK;
}
int lt_get_raw_color(lt_ctx* c, int16_t* ccm, uint8_t* curve, int* is_set) { return lt_get_raw_color_of(c, 0, ccm, curve, is_set); }

// enable = 0 removes the map (mesh and black are not read) and frees the gain plane
int lt_set_raw_shading_of(lt_ctx* c, int id, const uint16_t* mesh, int mesh_w, int mesh_h, const int32_t* black, int enable) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (!is_raw_mosaic(c->in_layout)) return fail(LT_ERR_STATE, "lens shading corrects raw Bayer input: this context's input format is another layout");
    int rc;
    if (enable) {
        if (!mesh) return fail(LT_ERR_INVALID, "null mesh");
        if ((rc = check_shading(c->in_layout, mesh_w, mesh_h, black))) return rc;
    }
    return edit(c, id, enable != 0, [&](RawSetup& s) {
        if (enable) s.set_shading(mesh, mesh_w, mesh_h, black);
        else s.drop_shading();
    });
}
int lt_set_raw_shading(lt_ctx* c, const uint16_t* mesh, int mesh_w, int mesh_h, const int32_t* black, int enable) {
    return lt_set_raw_shading_of(c, 0, mesh, mesh_w, mesh_h, black, enable);
}

int lt_get_raw_shading_of(lt_ctx* c, int id, uint16_t* mesh, int* mesh_w, int* mesh_h, int32_t* black, int* is_set) {
    if (int rc = check_set(c, id)) return rc;
    const RawSetup& s = raw_set_of(c, id);
    if (is_set) *is_set = s.shade ? 1 : 0;
    if (mesh_w) *mesh_w = s.mesh_w;
    if (mesh_h) *mesh_h = s.mesh_h;
    if (mesh && s.shade) std::memcpy(mesh, s.mesh.data(), s.mesh.size() * sizeof(uint16_t));
    if (black && s.shade) std::memcpy(black, s.black.b, sizeof s.black.b);
    return LT_OK;
}
int lt_get_raw_shading(lt_ctx* c, uint16_t* mesh, int* mesh_w, int* mesh_h, int32_t* black, int* is_set) {
    return lt_get_raw_shading_of(c, 0, mesh, mesh_w, mesh_h, black, is_set);
}

int lt_get_raw_shading_plane_of(lt_ctx* c, int id, uint16_t* plane) {
    if (!c || !plane) return fail(LT_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_set(c, id))) return rc;
    if (!raw_set_of(c, id).shade) return fail(LT_ERR_STATE, "this context has no shading map (lt_set_raw_shading)");
    if ((rc = set_device(c))) return rc;
    HIP_TRY(hipMemcpy(plane, raw_dev_of(c, id).gain, (size_t)c->calib.img_h * c->calib.img_w * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return LT_OK;
}
int lt_get_raw_shading_plane(lt_ctx* c, uint16_t* plane) { return lt_get_raw_shading_plane_of(c, 0, plane); }

// ---- raw statistics (lt_raw_stats) ---------------------------------------------------------------------------------------------
// Occasional, like the setters: behind everything the context has in flight, on the context's stream, and the host waits for it.  It
// reads the slots' frames and writes its own scratch: nothing a later call reads changes.
int lt_raw_stats(lt_ctx* c, int first, int n, const lt_raw_stats_params* p, uint32_t* hist, uint32_t* zone_count, uint64_t* zone_sum, int32_t* rect) {
    if (!c) return fail(LT_ERR_INVALID, "null context");
    if (!is_raw_mosaic(c->in_layout)) return fail(LT_ERR_STATE, "raw statistics are taken of raw Bayer input: this context's input format is another layout");
    if (!p) return fail(LT_ERR_INVALID, "null parameters");
    if (first < 0 || n < 0 || first > c->capacity || n > c->capacity - first)
        return fail(LT_ERR_INVALID, "slots [%d, %d) outside reserved capacity %d", first, first + n, c->capacity);
    const int H = c->calib.img_h, W = c->calib.img_w, bits = raw_sample_bits(c->in_layout), smax = (1 << bits) - 1;
    int in0 = 0, in1 = 0, d0 = 0, d1 = 0, rc;
    if ((rc = lt_get_input_rows(c, &in0, &in1))) return rc;
    st::default_rows(in0, in1, &d0, &d1);
    const int row0 = p->row1 == 0 ? d0 : p->row0, row1 = p->row1 == 0 ? d1 : p->row1;
    const int col0 = p->col1 == 0 ? 0 : p->col0, col1 = p->col1 == 0 ? W : p->col1;
    if (((row0 | row1 | col0 | col1) & 1) || row0 < 0 || row0 >= row1 || row1 > H || col0 < 0 || col0 >= col1 || col1 > W)
        return fail(LT_ERR_INVALID, "rows [%d, %d), columns [%d, %d): a rectangle of statistics has even bounds inside the %d x %d frame and is not empty",
                    row0, row1, col0, col1, W, H);
    const int ncy = (row1 - row0) / 2, ncx = (col1 - col0) / 2;
    if (p->grid_h < 1 || p->grid_h > std::min(st::GRID_MAX, ncy) || p->grid_w < 1 || p->grid_w > std::min(st::GRID_MAX, ncx))
        return fail(LT_ERR_INVALID, "a grid of %d x %d zones: each side is 1 .. 64 and at most the rectangle's %d x %d cells", p->grid_w, p->grid_h, ncx, ncy);
    for (int k = 0; k < 4; ++k)
        if (p->lo[k] < 0 || p->lo[k] > smax || p->hi[k] < 0 || p->hi[k] > smax)
            return fail(LT_ERR_INVALID, "lo[%d] = %d, hi[%d] = %d: the bounds of %d-bit samples lie in 0 .. %d", k, (int)p->lo[k], k, (int)p->hi[k], bits, smax);
    auto is_attached = [&](int i) { return i < (int)c->attached.size() && c->attached[(size_t)i] != 0; };
    if (row0 < in0 || row1 > in1)
        for (int i = first; i < first + n; ++i)
            if (!is_attached(i) && !(i < (int)c->frame_full.size() && c->frame_full[(size_t)i]))
                return fail(LT_ERR_STATE, "slot %d holds only the rows the path reads, [%d, %d): rows [%d, %d) were never uploaded into it", i, in0, in1, row0, row1);
    if (rect) rect[0] = row0, rect[1] = row1, rect[2] = col0, rect[3] = col1;
    if (n == 0) return LT_OK;
    if ((rc = set_device(c))) return rc;
    if ((rc = sync_all(c))) return rc;
    const size_t bins = (size_t)1 << bits, zones = (size_t)p->grid_h * p->grid_w;
    const size_t sum_bytes = (size_t)n * zones * 4 * sizeof(uint64_t), hist_bytes = (size_t)n * 4 * bins * sizeof(uint32_t),
                 count_bytes = (size_t)n * zones * sizeof(uint32_t), need = sum_bytes + hist_bytes + count_bytes;
    if (need > c->stats_bytes) {
        dev_free(c->d_stats);
        c->stats_bytes = 0;
        if ((rc = dev_alloc(&c->d_stats, need))) return rc;
        c->stats_bytes = need;
    }
    RawStatsJob job{};
    job.pattern = c->in_layout & 3, job.bits = bits, job.pack = raw_packing(c->in_layout);
    job.img_w = W;
    job.row0 = row0, job.col0 = col0, job.ncy = ncy, job.ncx = ncx, job.grid_h = p->grid_h, job.grid_w = p->grid_w;
    for (int k = 0; k < 4; ++k) job.lo[k] = p->lo[k], job.hi[k] = p->hi[k];
    unsigned long long* d_sum = reinterpret_cast<unsigned long long*>(c->d_stats);
    uint32_t* d_hist = reinterpret_cast<uint32_t*>(c->d_stats + sum_bytes);
    uint32_t* d_count = reinterpret_cast<uint32_t*>(c->d_stats + sum_bytes + hist_bytes);
    HIP_TRY(hipMemsetAsync(c->d_stats, 0, need, c->stream));
    for (int a = first; a < first + n;) {                        // runs of slots with one kind of source and one raw set
        int b = a + 1;
        while (b < first + n && is_attached(b) == is_attached(a) && slot_raw_set(c, b) == slot_raw_set(c, a)) ++b;
        const RawStages raw = raw_stages_of(c, slot_raw_set(c, a));      // (the slots' map as the front end reads it)
        job.gains = raw.gains;
        job.blk = raw.blk;
        job.zone_sum = d_sum + (size_t)(a - first) * zones * 4;
        job.hist = d_hist + (size_t)(a - first) * 4 * bins;
        job.zone_count = d_count + (size_t)(a - first) * zones;
        launch_raw_stats(c->stream, is_attached(a) ? FrameSource::surfaces(c->d_surf) : FrameSource::slots(slot_yuv(c, a), c->yuv_stride), a, b - a, job);
        a = b;
    }
    HIP_TRY(hipGetLastError());
    if (zone_sum) HIP_TRY(hipMemcpyAsync(zone_sum, d_sum, sum_bytes, hipMemcpyDeviceToHost, c->stream));
    if (hist) HIP_TRY(hipMemcpyAsync(hist, d_hist, hist_bytes, hipMemcpyDeviceToHost, c->stream));
    if (zone_count) HIP_TRY(hipMemcpyAsync(zone_count, d_count, count_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LT_OK;
}

// ---- one host frame -> RGB, on the device ---------------------------------------------------------------------------------------------
// The one-shot converters validate their arguments and describe their frame's conditioning as a RawSetup; convert_once does the rest.
int lt::convert_once(lt_ctx* c, const char* what, const void* frame, size_t in_bytes, int h, int w, YuvCoef k, RawSetup raw, uint8_t* out_rgb) {
    int rc;
    if ((rc = set_device(c))) return rc;
    const size_t out_bytes = (size_t)h * w * 3;
    DevBuf<uint8_t> d_in, d_out;
    struct Held : RawDevice { ~Held() { raw_release(*this); } } dev;
    if ((rc = d_in.alloc(in_bytes)) || (rc = d_out.alloc(out_bytes))) return rc;
    if ((rc = raw_commit(raw, dev, raw.shade, c->stream, h, w))) return rc;
    hipError_t e = hipMemcpyAsync(d_in.p, frame, in_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_yuv_rows_to_rgb(c->stream, raw.layout, d_in.p, in_bytes, k, d_out.p, out_bytes, h, w, 0, h, 1, raw_stages(raw, dev));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_rgb, d_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(LT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return LT_OK;
}

// one 8-bit raw Bayer host frame of any even size from 4 x 4 (h w bytes) -> RGB: the bilinear demosaic of bayer_arith.h
int lt_bayer_to_rgb(lt_ctx* c, const uint8_t* frame, int h, int w, int layout, uint8_t* out_rgb) {
    if (!c || !frame || !out_rgb) return fail(LT_ERR_INVALID, "null argument");
    if (!is_bayer(layout)) return fail(LT_ERR_INVALID, "lt_bayer_to_rgb takes the raw Bayer layouts (16 .. 19)");
    int rc = check_one_shot_size(layout, h, w);
    if (rc) return rc;
    RawSetup raw;
    raw.layout = layout;
    return convert_once(c, "raw Bayer conversion", frame, (size_t)h * w, h, w, YuvCoef{}, raw, out_rgb);
}

// one 10- / 12-bit raw Bayer host frame (h w 16-bit words) -> RGB: every sample looked up in `lut` (null: the default table), then the
// bilinear demosaic -- lt_bayer_to_rgb's twin
int lt_raw16_to_rgb(lt_ctx* c, const uint16_t* frame, int h, int w, int layout, const uint8_t* lut, uint8_t* out_rgb) {
    if (!c || !frame || !out_rgb) return fail(LT_ERR_INVALID, "null argument");
    if (!is_bayer_wide(layout) || raw_packing(layout) >= 0) return fail(LT_ERR_INVALID, "lt_raw16_to_rgb takes the 10- and 12-bit raw Bayer layouts (32 .. 35, 48 .. 51)");
    int rc = check_one_shot_size(layout, h, w);
    if (rc) return rc;
    RawSetup raw;
    raw.layout = layout;
    raw.set_table(lut);
    return convert_once(c, "raw Bayer conversion", frame, (size_t)h * w * 2, h, w, YuvCoef{}, raw, out_rgb);
}

// One raw Bayer host frame in any of the twelve raw layouts -> RGB behind its table, on behalf of `fn`: every sample shaded (mesh not null:
// the map and its pedestals), looked up in `lut` (8-bit: null is the identity; 10 / 12 bits: null is the default table) and demosaiced, then
// -- `color` -- matrix and curve (null: the identity each).
static int raw_to_rgb(lt_ctx* c, const char* fn, const void* frame, int h, int w, int layout, const uint8_t* lut, size_t lut_entries, bool color,
                      const int16_t* ccm, const uint8_t* curve, const uint16_t* mesh, int mesh_w, int mesh_h, const int32_t* black, uint8_t* out_rgb) {
    if (!c || !frame || !out_rgb) return fail(LT_ERR_INVALID, "null argument");
    if (!is_raw_mosaic(layout)) return fail(LT_ERR_INVALID, "%s takes the raw Bayer layouts (16 .. 19, 32 .. 35, 48 .. 51)", fn);
    const size_t entries = (size_t)1 << raw_sample_bits(layout);
    if (lut && lut_entries != entries) return fail(LT_ERR_INVALID, "the raw table of this layout has %zu entries per colour phase, got %zu", entries, lut_entries);
    int rc = check_one_shot_size(layout, h, w);
    if (rc) return rc;
    if (mesh && (rc = check_shading(layout, mesh_w, mesh_h, black))) return rc;
    RawSetup raw;
    raw.layout = layout;
    raw.set_table(lut);
    if (color) raw.set_color(ccm, curve);
    if (mesh) raw.set_shading(mesh, mesh_w, mesh_h, black);
    return convert_once(c, "raw Bayer conversion", frame, (size_t)h * (size_t)one_plane_row_bytes(layout, w), h, w, YuvCoef{}, raw, out_rgb);
}

// lt_bayer_to_rgb / lt_raw16_to_rgb behind a raw table and with the colour stage: the raw row kernels with STAGES 2 and 3 alone
int lt_raw_to_rgb_color(lt_ctx* c, const void* frame, int h, int w, int layout, const uint8_t* lut, size_t lut_entries, const int16_t* ccm,
                        const uint8_t* curve, uint8_t* out_rgb) {
    return raw_to_rgb(c, "lt_raw_to_rgb_color", frame, h, w, layout, lut, lut_entries, true, ccm, curve, nullptr, 0, 0, nullptr, out_rgb);
}

// lt_raw_to_rgb_color behind a shading map (mesh = null: none); without ccm and curve there is no colour stage either -- the raw row
// kernels with STAGES 4 .. 7 alone
int lt_raw_to_rgb_shaded(lt_ctx* c, const void* frame, int h, int w, int layout, const uint8_t* lut, size_t lut_entries, const int16_t* ccm,
                         const uint8_t* curve, const uint16_t* mesh, int mesh_w, int mesh_h, const int32_t* black, uint8_t* out_rgb) {
    if (!mesh) return lt_raw_to_rgb_color(c, frame, h, w, layout, lut, lut_entries, ccm, curve, out_rgb);
    return raw_to_rgb(c, "lt_raw_to_rgb_shaded", frame, h, w, layout, lut, lut_entries, ccm || curve, ccm, curve, mesh, mesh_w, mesh_h, black, out_rgb);
}
