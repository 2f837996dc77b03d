// The mask chain: filter_lane_points() of lane_tracker.py:210-238 on the R and Lab-b planes of a run of slots, in the device
// memory of a MaskArena (lt_ctx.h).  Three steps; what one leaves for the next is a value:
// tophats() -> which form ran (TophatForm); thresholds() -> what the merged plane is (MergeInputs, lt_internal.h); open().
// A new kernel form is one more TophatForm, or one more route in thresholds() that fills a MergeInputs.  Nothing here reads a
// switch: the launchers' alternatives are theirs (k_*.hip).
#include "lt_ctx.h"

namespace lt {

int validate_filter(const lt_filter_params* p) {
    if (!p) return fail(LT_ERR_INVALID, "null filter params");
    if (p->filter_type != 0 && p->filter_type != 1)
        return fail(LT_ERR_INVALID, "Unexpected filter mode. Expected modes are 'bilateral' or 'neighborhood'.");
    if (p->ksize_r < 1 || p->ksize_b < 1 || (p->mask_noise && p->ksize_noise < 1))
        return fail(LT_ERR_INVALID, "filter sizes must be >= 1");
    if (p->filter_type == 1 && ((p->ksize_r & 1) == 0 || (p->ksize_b & 1) == 0))
        return fail(LT_ERR_INVALID, "'neighborhood' block sizes must be odd (cv2.adaptiveThreshold requirement)");
    if (p->ksize_r > 128 || p->ksize_b > 128 || p->ksize_noise > 128)
        return fail(LT_ERR_INVALID, "filter size too large (max 128)");
    return LT_OK;
}

namespace {

enum TophatForm {
    TH_NONE,     // 'neighborhood': the thresholds read the R and Lab-b planes themselves
    TH_BRUTE,    // direct footprint evaluation (debugging aid of the experiments build, LT_TOPHAT_BRUTE=1; still on the GPU)
    TH_PAIR,     // one or two frames: both planes' erodes in one launch, both top-hats in the next
    TH_BATCH     // four launches of the decomposed kernels, one stage each
};

// one call of the chain: the slots' addresses in the arena and the decisions the three steps share
struct Chain {
    MaskArena& a;
    const ChainEnv& env;
    hipStream_t s;
    const lt_filter_params* p;
    const int first, n, h, w;
    const bool u8_mask;
    const size_t ps = a.plane_bytes, off = (size_t)first * ps;
    uint8_t *R = a.d_plane[P_R] + off, *B = a.d_plane[P_B] + off, *thR = a.d_plane[P_THR] + off, *thB = a.d_plane[P_THB] + off, *t0 = a.d_plane[P_T0] + off;
    unsigned long long *mbits = a.d_bits_merged + (size_t)first * a.bits_stride, *ebits = a.d_bits_eroded + (size_t)first * a.bits_stride;
    // The walking threshold kernels (a call of walk_min_pixels or more, window sizes they have) read the top-hat planes with a
    // padded row pitch: the dilate launches write them so.  The greenery mask, mask_noise, rides along: a third walk with
    // window 65 over the raw Lab-b plane, which the 55x55 top-hat launch leaves in the padded layout (bpad).
    bool walk = false;
    int tophat_path = 0;
    uint8_t *thRd = thR, *thBd = thB, *bpad = nullptr;
    int dpitch = 0;

    int scratch(int idx, uint8_t*& q) {      // a plane the arena allocates on first use
        const int rc = a.ensure_plane(idx);
        if (!rc) q = a.d_plane[idx] + off;
        return rc;
    }

    int choose_walk(int call_frames) {
        walk = p->filter_type == 0 && !env.brute_tophat && a.walk_planes() && (long long)call_frames * h * w >= env.walk_min_pixels &&
               bilateral_walk_supported(p->ksize_r, p->C_r, p->ksize_b, p->C_b, h, w, a.th_pitch, a.th_pad_bytes) &&
               (!p->mask_noise || noise_walk_supported(p->ksize_noise, p->C_noise, h, w, a.th_pitch, a.th_pad_bytes));
        if (p->filter_type != 0) return LT_OK;
        if (env.threshold_path) *env.threshold_path = walk ? 1 : 0;
        if (env.threshold_form) *env.threshold_form = walk ? 1 : 0;   // thresholds() says which of the two long forms
        for (int i = first; i < first + n && i < (int)a.th_padded.size(); ++i) a.th_padded[(size_t)i] = walk ? 1 : 0;
        if (!walk) return LT_OK;
        dpitch = a.th_pitch;
        thRd = a.d_th_pad[0] + (size_t)first * a.th_pad_bytes;
        thBd = a.d_th_pad[1] + (size_t)first * a.th_pad_bytes;
        if (p->mask_noise) {
            const int rc = a.ensure_noise_buffers();
            if (rc) return rc;
            bpad = a.d_b_pad + (size_t)first * a.th_pad_bytes;
        }
        return LT_OK;
    }

    // the 55x55 top-hat of the Lab-b plane; with the greenery mask it also leaves the raw plane in the padded layout
    int tophat_b(const MorphZone& zone, int* form) {
        if (bpad && launch_morph_runs(s, t0, thBd, B, h, w, 55, true, ps, n, dpitch, a.th_pad_bytes, bpad, zone, form)) return LT_OK;
        launch_morph_runs(s, t0, thBd, B, h, w, 55, true, ps, n, dpitch, a.th_pad_bytes, nullptr, zone, form);
        if (bpad)   // that kernel form does not exist for this geometry / A-B switch: plain strided copies
            for (int i = 0; i < n; ++i)
                HIP_TRY(hipMemcpy2DAsync(bpad + (size_t)i * a.th_pad_bytes, (size_t)a.th_pitch, B + (size_t)i * ps, (size_t)w, (size_t)w,
                                         (size_t)h, hipMemcpyDeviceToDevice, s));
        return LT_OK;
    }

    int tophats(TophatForm& form) {
        lt_ctx* const tm = env.timing;
        form = p->filter_type != 0 ? TH_NONE : env.brute_tophat ? TH_BRUTE : (n <= 2 && !tm && !walk) ? TH_PAIR : TH_BATCH;
        if (form == TH_BRUTE) {
            { StageScope t(tm, ST_ERODE_R, s);  launch_morph_ellipse(s, R, t0, nullptr, h, w, *env.se29, false, ps, n); }
            { StageScope t(tm, ST_TOPHAT_R, s); launch_morph_ellipse(s, t0, thR, R, h, w, *env.se29, true, ps, n); }
            { StageScope t(tm, ST_ERODE_B, s);  launch_morph_ellipse(s, B, t0, nullptr, h, w, *env.se55, false, ps, n); }
            { StageScope t(tm, ST_TOPHAT_B, s); launch_morph_ellipse(s, t0, thB, B, h, w, *env.se55, true, ps, n); }
        } else if (form == TH_PAIR) {
            // One or two frames cannot fill the chip (a few hundred waves per top-hat kernel), and the two planes' top-hats do not
            // depend on each other: the 55x55 erode of the Lab-b plane and the 29x29 erode of the R plane are ONE launch, the two
            // top-hats the next (k_morph_one_pair).  (Round 5 ran the R plane's chain on a side stream: a fork, a join that cost the
            // frame 11-12 us of signalling, and three more launches.)  The eroded R plane has a scratch of its own, one lane per stream.
            { const int rc = a.ensure_side_scratch(); if (rc) return rc; }
            int lane = MaskArena::SIDE_LANES - 1;
            for (int i = 0; env.streams && i < (int)env.streams->size() && i < MaskArena::SIDE_LANES - 1; ++i)
                if ((*env.streams)[(size_t)i] == s) { lane = i; break; }
            uint8_t* ts = a.d_side_scratch + (size_t)lane * 2 * ps;
            if (launch_morph_one_pair(s, B, t0, nullptr, R, ts, nullptr, h, w, false, ps, n, 0, 0)) {
                if (!launch_morph_one_pair(s, t0, thB, B, ts, thR, R, h, w, true, ps, n, 0, 0)) {
                    launch_morph_runs(s, t0, thB, B, h, w, 55, true, ps, n);
                    launch_morph_runs(s, ts, thR, R, h, w, 29, true, ps, n);
                }
            } else {             // (a geometry the one-frame kernel does not take: an image width that is not a multiple of four)
                launch_morph_runs(s, R, t0, nullptr, h, w, 29, false, ps, n);
                launch_morph_runs(s, t0, thR, R, h, w, 29, true, ps, n);
                launch_morph_runs(s, B, t0, nullptr, h, w, 55, false, ps, n);
                launch_morph_runs(s, t0, thB, B, h, w, 55, true, ps, n);
            }
        } else if (form == TH_BATCH) {
            // the split-band walks' boundary zones, per slot: the four launches run one behind the other on s and share them
            MorphZone zone;
            if (n > 2) {   // (one or two frames: launch_morph_runs takes k_morph_one, which needs none)
                const int rc = a.ensure_zone_scratch();
                if (rc) return rc;
                zone.base = a.d_zone + (size_t)first * a.zone_stride;
                zone.stride_dwords = a.zone_stride;
            }
            int f29e = 0, f29d = 0, f55e = 0, f55d = 0;
            { StageScope t(tm, ST_ERODE_R, s);  launch_morph_runs(s, R, t0, nullptr, h, w, 29, false, ps, n, 0, 0, nullptr, zone, &f29e); }
            { StageScope t(tm, ST_TOPHAT_R, s); launch_morph_runs(s, t0, thRd, R, h, w, 29, true, ps, n, dpitch, a.th_pad_bytes, nullptr, zone, &f29d); }
            { StageScope t(tm, ST_ERODE_B, s);  launch_morph_runs(s, B, t0, nullptr, h, w, 55, false, ps, n, 0, 0, nullptr, zone, &f55e); }
            { StageScope t(tm, ST_TOPHAT_B, s); const int rc = tophat_b(zone, &f55d); if (rc) return rc; }
            tophat_path = (f29e && f29d ? 1 : 0) | (f55e && f55d ? 2 : 0);
        }
        if (env.tophat_path && p->filter_type == 0) *env.tophat_path = tophat_path;
        return LT_OK;
    }

    // One early return per route that leaves bit planes; the two per-plane routes at the end leave u8 verdicts for pack_merge().
    int thresholds(TophatForm form, MergeInputs& in) {
        const size_t bs = a.bits_stride;
        const int noise = p->mask_noise ? 1 : 0;
        in = MergeInputs{};
        in.dst = mbits;                              // every route leaves its first (or only) term there
        uint8_t *t1 = nullptr, *t2 = nullptr;
        if (p->filter_type == 0) {
            StageScope t(env.timing, ST_THRESHOLD, s);   // both bilateral thresholds and the greenery mask
            if (walk) {
                // the long walks: four partial planes (R horizontal, R vertical, b horizontal, b vertical), and the greenery mask as two more
                unsigned long long *tbits = a.d_bits_tmp + (size_t)first * bs, *ubits = a.d_bits_tmp2 + (size_t)first * bs;
                // as i8 matrix products (k_threshold_mma.hip); the running-sum walks where that launcher stands aside
                int rc = launch_bilateral_mma(s, thRd, p->ksize_r, p->C_r, thBd, p->ksize_b, p->C_b, mbits, ebits, tbits, ubits, h, w, a.th_pitch,
                                              a.th_pad_bytes, bs, n);
                if (env.threshold_form) *env.threshold_form = rc == 0 ? 2 : 1;
                if (rc > 0)
                    rc = launch_bilateral_walk(s, thRd, p->ksize_r, p->C_r, thBd, p->ksize_b, p->C_b, mbits, ebits, tbits, ubits, h, w, a.th_pitch,
                                               a.th_pad_bytes, bs, n);
                if (rc) return fail(LT_ERR_STATE, "the bilateral walk refused parameters its own predicate accepted");
                in.more[0] = ebits, in.more[1] = tbits, in.more[2] = ubits, in.n_more = 3;
                if (!noise) return LT_OK;
                unsigned long long *n1 = a.d_bits_n1 + (size_t)first * bs, *n2 = a.d_bits_n2 + (size_t)first * bs;
                if (launch_noise_walk(s, bpad, p->ksize_noise, p->C_noise, p->noise_thresh, n1, n2, h, w, a.th_pitch, a.th_pad_bytes, bs, n))
                    return fail(LT_ERR_STATE, "the greenery-mask walk refused parameters its own predicate accepted");
                in.and0 = n1; in.and1 = n2;
                return LT_OK;
            }
            // One or two frames (process()): both planes' thresholds in ONE launch with the H and the V phases of a tile in workgroups
            // of their own (one frame: 81 tiles on 256 CUs) -- H verdicts of both planes into mbits, V verdicts into ebits.
            // (refused when the packed arithmetic does not fit the parameters: one workgroup per tile below)
            if (form == TH_PAIR && !noise &&
                launch_bilateral_bits(s, thR, p->ksize_r, p->C_r, thB, p->ksize_b, p->C_b, B, p->ksize_noise, p->C_noise, p->noise_thresh, 0,
                                      mbits, h, w, ps, bs, n, ebits) == 0) {
                in.more[0] = ebits, in.n_more = 1;
                return LT_OK;
            }
            if (launch_bilateral_bits(s, thR, p->ksize_r, p->C_r, thB, p->ksize_b, p->C_b, B, p->ksize_noise, p->C_noise, p->noise_thresh, noise,
                                      mbits, h, w, ps, bs, n) == 0)
                return LT_OK;                        // merged inside the tile kernel
            // tile + halo exceeds the LDS: one plane at a time
            { int rc = scratch(P_T1, t1); if (!rc) rc = scratch(P_T2, t2); if (rc) return rc; }
            launch_bilateral(s, thR, t1, h, w, p->ksize_r, p->C_r, 0, 255, 0, ps, n);
            launch_bilateral(s, thB, t2, h, w, p->ksize_b, p->C_b, 0, 255, 0, ps, n);
        } else {
            StageScope t(env.timing, ST_THRESHOLD, s);
            // running box sums, both planes in one launch, a bit plane each; the per-pixel window kernel for what that does not
            // take (window > 63, a width that is not a multiple of 4, the greenery mask)
            const bool box = !noise && launch_adaptive_walk(s, R, p->ksize_r, p->C_r, mbits, B, p->ksize_b, p->C_b, ebits, h, w, ps, bs, n);
            if (env.adaptive_path) *env.adaptive_path = box ? 1 : 0;
            if (box) {
                in.more[0] = ebits, in.n_more = 1;
                return LT_OK;
            }
            { int rc = scratch(P_T1, t1); if (!rc) rc = scratch(P_T2, t2); if (rc) return rc; }
            launch_adaptive_mean(s, R, t1, h, w, p->ksize_r, p->C_r, ps, n);
            launch_adaptive_mean(s, B, t2, h, w, p->ksize_b, p->C_b, ps, n);
        }
        return pack_merge(t1, t2);
    }

    // u8 verdicts of the two planes (+ the greenery term, thresholded here) -> the merged bit plane
    int pack_merge(uint8_t* t1, uint8_t* t2) {
        uint8_t* t3 = nullptr;
        { const int rc = scratch(P_T3, t3); if (rc) return rc; }
        if (p->mask_noise) {
            StageScope t(env.timing, ST_THRESHOLD, s);
            launch_bilateral(s, B, t3, h, w, p->ksize_noise, p->C_noise, 0, 255, 0, ps, n);
        }
        StageScope t(env.timing, ST_MERGE, s);
        launch_pack_merge(s, t1, t2, B, t3, p->noise_thresh, p->mask_noise ? 1 : 0, mbits, h, w, ps, a.bits_stride, n);
        return LT_OK;
    }

    void open(const MergeInputs& in, uint8_t* mask) {
        StageScope t(env.timing, ST_OPEN, s);
        const size_t bs = a.bits_stride;
        unsigned long long* obits = u8_mask ? nullptr : a.d_bits_open + (size_t)first * bs;
        auto said = [&](int form) { if (env.open_form) *env.open_form = form; };   // lt_last_open_form: the branch taken
        // 16 frames or more: one pass over the words, a wave walking down the rows -- for partial planes.  A plane that is merged
        // already has never taken that kernel (it went to the launcher with the arena's two spare planes beside it, which the
        // launcher refuses): it takes the separate kernels below, and k_merge_open5<1> has no caller.  Kept as found: this file
        // launches what its predecessor launched.
        if (!u8_mask && n >= 16 && in.n_more > 0 && launch_merge_open5(s, in, obits, h, w, bs, n)) return said(1);
        // a few frames are latency-bound and better off with the wide, shallow kernels: the OR and the open in one launch of small
        // workgroups (the one-frame chain is made of launch gaps: three kernels of 5 us here)
        if (!u8_mask && n <= 4 && launch_or_open5_small(s, in, obits, h, w, bs, n)) return said(2);
        said(0);
        launch_or4_bits(s, in, h, w, bs, n);
        if (u8_mask) launch_open5_bits(s, in.dst, ebits, mask, h, w, ps, bs, n);
        else launch_open5_to_bits(s, in.dst, ebits, obits, h, w, bs, n);
    }
};

}  // namespace

int run_mask_chain(MaskArena& a, const ChainEnv& env, hipStream_t s, int first, int n, const lt_filter_params* p, int h, int w,
                   int call_frames, bool u8_mask) {
    Chain c{a, env, s, p, first, n, h, w, u8_mask};
    uint8_t* mask = nullptr;
    int rc;
    if (u8_mask && (rc = c.scratch(P_MASK, mask))) return rc;
    if ((rc = c.choose_walk(call_frames))) return rc;
    TophatForm form;
    MergeInputs merged;
    if ((rc = c.tophats(form)) || (rc = c.thresholds(form, merged))) return rc;
    if (!merge_planes(merged)) return fail(LT_ERR_STATE, "the mask chain's thresholds left no valid merge");
    c.open(merged, mask);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

}  // namespace lt
