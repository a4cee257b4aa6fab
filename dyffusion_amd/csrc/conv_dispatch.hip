// Which kernel form a conv takes (host only, no kernels): one admission predicate per form, which reads the layer's ConvW for the
// fragment order the form streams, conv_choose_form, and the three launch entry points of conv.h, which choose and then call the
// chosen form's launcher.
// Parameters INSIDE a form (split-K factors, tile-row counts, igemm2's SH3 switch) stay with that form's launcher.
#include "conv.h"

#include <algorithm>
#include <initializer_list>

// ------------------------------------------------------------------------------------------------ admission rules, one per form
// Each returns the form's fragment-ordered weights when the form takes the conv, null when it does not.  They read the switch table
// and the ConvW they were given and nothing else; the ladders below fix the ORDER in which they are asked.
namespace {

long long form_rows(const ConvArgs& a) { return a.n_sel > 0 ? a.n_sel : a.n; }  // rows the form is chosen for (ConvArgs::n_sel)
// the ConvArgs a form's *_supported predicate is asked with: the pointer it would be launched with in place
ConvArgs with_up_frag(ConvArgs a, const el16_t* f) { a.wpk_up_frag = f; return a; }
ConvArgs with_frag(ConvArgs a, const ConvW& w) { a.wpk_frag = w.frag; return a; }  // pack_conv_frag order
const el16_t* halo_of(const ConvW& w, HaloOrder order) { return w.halo_order == order ? w.halo : nullptr; }
bool halo3_on() { return dyf_form_int("DYF_HALO3", 1) != 0; }  // the 3x3 / s1 and the 4x4 / s2 form of the 256-channel-block halo kernel
bool igemm2_on() { return dyf_form_int("DYF_IGEMM2", 1) != 0; }

// fused x2-upsample conv on the halo kernel from 32 x 32 low-res planes on; below that (dec2: 16 x 16, 2 tiles per image) the
// materialised upsample + plain 3x3 halo conv is still slightly ahead (7 715 vs 7 690 fields/s with DYF_HALO_MIN_PLANE=16: 640
// workgroups of the fused form fill 1.25 rounds of the 512 resident ones)
bool up_halo_admits(const ConvArgs& a) {
    const int halo_min = dyf_form_int("DYF_HALO_MIN_PLANE", 32);
    return a.up2x && dyf_form_int("DYF_UP_HALO", 1) != 0 && a.h >= halo_min && a.w >= halo_min && conv_up_halo_supported(a);
}

// plain 3x3 / s1 convs with cout % 256 == 0 on 8x16-tileable planes: the halo kernel (one window DMA per chunk instead of one gather
// per tap); DYF_HALO3=0 disables, DYF_HALO3_MIN_TILES sets the smallest launch (measured at NB = 80, enc3 with 320 tiles 115 -> 94 us;
// round 4, with the rows forms: from 80 tiles on -- NS at 7 / 10 / 25 rows +3.4 / +5.7 / +2.5 % against the 256 of rounds 1-3, nothing
// lost at 4 or 80 rows; 64 costs 2.4 % at 4 rows)
const el16_t* halo3_admits(const ConvArgs& a, const ConvW& w) {
    if (!(!a.up2x && a.kh == 3 && a.kw == 3 && a.cout % 256 == 0 && a.out_f32 == nullptr && a.residual == nullptr) || !halo3_on()) return nullptr;
    const ConvArgs b = with_up_frag(a, halo_of(w, HaloOrder::Halo3_256));
    const long long tiles3 = (form_rows(a) * a.h * a.w / 128) * (a.cout / 256);
    return b.wpk_up_frag && tiles3 >= dyf_form_int("DYF_HALO3_MIN_TILES", 80) && conv_halo3_supported(b) ? b.wpk_up_frag : nullptr;
}

// 3x3 / s1 convs with 64 or 128 (any multiple of 64 that is not one of 256) output channels -- the ResNet-UNet levels -- on planes of
// any size: SP = 5 of the halo kernel, when the 16 x 32 tiles cover the plane reasonably (>= 60 %: not 15 x 15) and the launch has
// enough of them.  DYF_HALO5=0 disables, DYF_HALO5_MIN_TILES sets the smallest launch (64 tiles since round 4: with the GroupNorm
// fused into this form a small launch also saves the three GroupNorm kernels behind the implicit-GEMM fallback -- OISST shapes at
// 38 / 75 rows +5.8 / +3 % against the 256 of round 3).  (A residual is only added by the fused-GroupNorm epilogue: the plain ladder
// asks with residual == nullptr.)
const el16_t* halo5_admits(const ConvArgs& a, const ConvW& w) {
    if (!(!a.up2x && a.kh == 3 && a.kw == 3 && a.stride == 1 && a.cout % 64 == 0 && a.cout % 256 != 0 && a.out_f32 == nullptr)) return nullptr;
    if (dyf_form_int("DYF_HALO5", 1) == 0) return nullptr;
    const ConvArgs b = with_up_frag(a, halo_of(w, HaloOrder::Halo3_64));
    const long long ty = (a.h + 15) / 16, tx = (a.w + 31) / 32;
    const long long tiles5 = form_rows(a) * ty * tx * (a.cout / 64);
    const bool covers = 10ll * a.h * a.w >= 6ll * ty * 16 * tx * 32;
    return b.wpk_up_frag && covers && tiles5 >= dyf_form_int("DYF_HALO5_MIN_TILES", 64) && conv_halo5_supported(b) ? b.wpk_up_frag : nullptr;
}

const el16_t* enc0_stem_admits(const ConvArgs& a, const ConvW& w) {  // enc0 on the fused stem: HBM-bound, its own persistent kernel
    if (!conv_enc0_stem_supported(a) || !halo_of(w, HaloOrder::Enc0Stem)) return nullptr;
    return a.pix_pitch0 == 8 ? w.enc0_p8 : w.halo;  // (supported: pitch 16 or 8)
}

const el16_t* halo_s2_admits(const ConvArgs& a, const ConvW& w) {  // 4x4 / s2 convs: the halo kernel on the space-to-depth view
    if (!(!a.up2x && a.kh == 4 && a.kw == 4 && a.stride == 2 && a.cout % 128 == 0 && a.c1 == 0 && a.out_f32 == nullptr &&
          a.residual == nullptr && a.pix_pitch0 == 0) || !halo3_on())
        return nullptr;
    const ConvArgs b = with_up_frag(a, halo_of(w, HaloOrder::S2));
    // (its own switch since round 5; DYF_HALO3_MIN_TILES still applies when unset)
    const long long min_tiles3 = dyf_form_int("DYF_HALO_S2_MIN_TILES", dyf_form_int("DYF_HALO3_MIN_TILES", 80));
    // cout % 256 == 0: 8 x 16 tiles x 256 channels; else 16 x 16 tiles x 128 channels
    const long long pix = form_rows(a) * a.ho * a.wo;
    const long long tiles3 = a.cout % 256 == 0 ? (pix / 128) * (a.cout / 256) : (pix / 256) * (a.cout / 128);
    return b.wpk_up_frag && tiles3 >= min_tiles3 && conv_halo_s2_supported(b) ? b.wpk_up_frag : nullptr;
}

// tiles of conv_igemm2_kernel: 256 pixels x 128 channels (cout % 128 == 0), else 256 x 64
long long igemm2_tiles(const ConvArgs& a) {
    return ((form_rows(a) * a.ho * a.wo + 255) / 256) * (a.cout % 128 == 0 ? a.cout / 128 : a.cout / 64);
}

// 256 x 128 tiles pay off once they fill the chip (2 workgroups x 256 CUs); below that the 128 x 128 form's finer tiles win
// (measured at NB = 50: dec2/enc2 with 400 tiles +9 %/+4 %, enc3 with 200 tiles -20 %); tests force the form on small problems
const el16_t* igemm2_admits(const ConvArgs& a, const ConvW& w) {
    if (!(!a.up2x && igemm2_on() && a.cout % 64 == 0)) return nullptr;
    const ConvArgs b = with_frag(a, w);
    return igemm2_tiles(a) >= dyf_form_int("DYF_IGEMM2_MIN_TILES", 384) && conv_igemm2_supported(b) ? b.wpk_frag : nullptr;
}

// few rows: 1x1 / 2x2-s2 convs whose 128 x 128 tiles would not even fill a quarter of the chip (the split-K regime of
// launch_conv_igemm) run on conv_skinny_kernel -- K split over the four waves of a 32 x 32 tile, one launch (DYF_SKINNY=0 disables).
// (64 tiles of 128 x 128: NS at 1 / 4 / 7 / 10 rows +10.6 / +4 / +2 / +1 %, nothing lost at 25 / 38; at 128 the 25- and 38-row
// rollouts lose 2.5 %)
const el16_t* skinny_admits(const ConvArgs& a, const ConvW& w) {
    if (!(!a.up2x && a.cout % 128 == 0) || dyf_form_int("DYF_SKINNY", 1) == 0) return nullptr;
    const long long tiles128 = ((form_rows(a) * a.ho * a.wo + 127) / 128) * (a.cout / 128);
    const ConvArgs b = with_frag(a, w);
    return tiles128 <= dyf_form_int("DYF_SKINNY_MAX_TILES", 64) && conv_skinny_supported(b) ? b.wpk_frag : nullptr;
}

// ---- GroupNorm fused into the conv (gn_fused.h): a form is used when a sample's statistics slots are few enough to sweep
const int GN_FUSE_MAX_SLOTS = 64;  // gn_fuse_sweep<16>: 4 slot classes x 16
bool gn_slots_fit(int slots, int max_slots) { return slots <= GN_FUSE_MAX_SLOTS && slots <= max_slots; }

// conv_gn16_kernel, 16 x 16-pixel tiles x 64 channels, three workgroups per CU, ONE slot per tile (conv_gn16.hip; DYF_GN16=0: off),
// when the tiles cover the plane reasonably (planes that fill less than 60 % of their tiles are left to the other forms;
// DYF_GN16_ANY_PLANE=1: the tests' tiny planes) and the launch has DYF_GN16_MIN_TILES of them.
// c256 -- the 256-channel level on SMALL planes (15 x 15 at OISST: one tile per sample): four 64-channel column blocks per sample
// instead of conv_igemm2_kernel<2, true>'s 256-pixel x 128-channel tiles -- half the K chain per workgroup, more than twice the
// workgroups (400 against 176 at 100 rows).  Its fragments are ConvW::frag64, planes above DYF_GN16_C256_MAX_PLANE pixels are
// left to igemm2, DYF_GN16_C256=0: off
const el16_t* gn16_admits(const ConvArgs& a, const ConvW& w, bool c256) {
    if (dyf_form_int("DYF_GN16", 1) == 0 || (c256 && dyf_form_int("DYF_GN16_C256", 1) == 0)) return nullptr;
    const ConvArgs b = with_up_frag(a, c256 ? w.frag64 : halo_of(w, HaloOrder::Halo3_64));
    const int slots16 = conv_gn16_slots(a.h, a.w);
    const long long tiles16 = form_rows(a) * slots16 * (a.cout / 64);
    const bool covers16 = 10ll * a.h * a.w >= 6ll * slots16 * 256 || dyf_form_int("DYF_GN16_ANY_PLANE", 0) != 0;
    const bool plane_ok = !c256 || (long long)a.h * a.w <= dyf_form_int("DYF_GN16_C256_MAX_PLANE", 1024);
    return b.wpk_up_frag && covers16 && plane_ok && tiles16 >= dyf_form_int("DYF_GN16_MIN_TILES", 64) &&
                   gn_slots_fit(slots16, a.gnf.max_slots) && conv_gn16_supported(b) ? b.wpk_up_frag : nullptr;
}

// conv_igemm2_kernel<2, true>; sets c->gn_slots / c->bm.  Un-fused, the 256 x 128 tiles pay off from 384 tiles on (igemm2_admits); fused,
// the form also saves the three GroupNorm launches behind it (statistics, finalise, apply: 15 us of launches at small batches): taken
// from 32 tiles on.  Measured at the end of round 4, OISST shapes, fields/s with the threshold at 256 (the first choice) / 64 / 16:
// 300 rows 4 154 / 4 165 / 4 181, 150 rows 3 568 / 3 626 / 3 631, 75 rows 2 360 / 2 494 / 2 479, 38 rows 1 548 / 1 619 / 1 654, 16 rows
// 811 / 811 / 791 (32: 818) -- DYF_GN_FUSE_MIN_TILES overrides, DYF_IGEMM2_MIN_TILES (tests) wins
const el16_t* igemm2_fused_admits(const ConvArgs& a, const ConvW& w, ConvChoice* c) {
    const GnFuse& G = a.gnf;
    if (!(igemm2_on() && a.cout % 128 == 0)) return nullptr;
    const ConvArgs b = with_frag(a, w);
    if (!conv_igemm2_supported(b)) return nullptr;
    const long long tiles2 = igemm2_tiles(a);
    const long long min_tiles = dyf_form_int("DYF_IGEMM2_MIN_TILES", dyf_form_int("DYF_GN_FUSE_MIN_TILES", 32));
    // flattened-M tiles cut a sample into 128-row slabs at (n * plane) % 128: unless plane % 128 == 0 (or the tiles are 2-D) the
    // fp32 partial sums of a sample are grouped by its POSITION in the launch, and (mean, 1/std) differ in the last bits between
    // batch offsets / ranks -- not acceptable to a batch_invariant engine, which then takes the three-kernel path
    const bool position_free = conv_igemm2_tile2d(a.ho, a.wo) || (a.ho * a.wo) % 128 == 0;
    if (G.invariant && !position_free) return nullptr;
    // few tiles: the 128-pixel tile form (half the K chain per wave, twice the workgroups) while the 256-pixel tiles would leave
    // CUs idle -- DYF_IGEMM2_BM128_BELOW tiles (0 = never); not for batch_invariant engines whose planes are not slab-aligned
    // (the same position argument as above, with 64-row slabs)
    const long long bm128_below = dyf_form_int("DYF_IGEMM2_BM128_BELOW", 224);  // read per launch (parity test)
    const int slots128 = conv_igemm2_gn_slots_bm128(a.ho, a.wo), slots = conv_igemm2_gn_slots(a.ho, a.wo);
    const bool free128 = (a.wo % 16 == 0 && a.ho % 8 == 0) || (a.ho * a.wo) % 64 == 0;
    if (tiles2 >= min_tiles && tiles2 < bm128_below && slots128 > 0 && gn_slots_fit(slots128, G.max_slots) && (!G.invariant || free128))
        c->gn_slots = slots128, c->bm = 128;
    else if (tiles2 >= min_tiles && slots > 0 && gn_slots_fit(slots, G.max_slots))
        c->gn_slots = slots, c->bm = 256;
    else
        return nullptr;
    return b.wpk_frag;
}

// ------------------------------------------------------------------------------------------------ the two ladders
ConvChoice choose_plain(const ConvArgs& a, const ConvW& w, bool mfma, bool stats) {
    const ConvChoice invalid{ConvForm::Invalid, nullptr, 0, 0};
    const el16_t* const h5 = mfma && a.residual == nullptr ? halo5_admits(a, w) : nullptr;
    // a fused nearest upsample exists in ONE form: refuse rather than read a low-resolution tensor as the full-size one
    if (a.up_nearest && !(h5 && a.h % 2 == 0 && a.w % 2 == 0 && a.c1 == 0)) return invalid;
    // the direct kernel has no fused-upsample form: caller materialises
    if (!mfma) return a.up2x ? invalid : ConvChoice{ConvForm::Direct, nullptr, 0, 0};
    // sparse-column form: only the halo kernel writes the compact output tensor
    if (a.up2x && a.up_cols) return conv_up_halo_supported(a) ? ConvChoice{ConvForm::UpHalo, nullptr, 0, 0} : invalid;
    if (up_halo_admits(a)) return {ConvForm::UpHalo, nullptr, 0, 0};
    if (const el16_t* f = halo3_admits(a, w))  // its rows form where that serves the plane
        return {dyf_form_int("DYF_HALO_ROWS", 1) != 0 && conv_halo_rows3_supported(a) ? ConvForm::Rows3 : ConvForm::Halo3, f, 0, 0};
    if (h5)  // with the statistics of the raw conv output where the caller asked for them
        return {ConvForm::Halo5, h5, stats && a.act == ACT_NONE && a.drop.mode == 0 ? conv_halo5_gn_slots(a.h, a.w) : 0, 0};
    if (const el16_t* f = enc0_stem_admits(a, w)) return {ConvForm::Enc0Stem, f, 0, 0};
    if (const el16_t* f = halo_s2_admits(a, w)) return {ConvForm::HaloS2, f, 0, 0};
    if (const el16_t* f = igemm2_admits(a, w)) return {ConvForm::Igemm2, f, 0, 0};
    if (const el16_t* f = skinny_admits(a, w)) return {ConvForm::Skinny, f, 0, 0};
    return {a.cout % 128 == 0 ? ConvForm::Igemm128 : ConvForm::Igemm256x64, nullptr, 0, 0};
}

// The fused forms are used exactly where the un-fused launch would have taken conv_up_halo_kernel<5> / conv_igemm2_kernel<2> (same
// tile rules), with conv_gn16_kernel in front of them.  (DYF_GN_FUSED=0 is read per engine, dyf_engine_create: the caller then
// never asks)
ConvChoice choose_gn_fused(const ConvArgs& a, const ConvW& w, bool mfma) {
    ConvChoice c{ConvForm::None, nullptr, 0, 0};
    const GnFuse& G = a.gnf;
    if (!mfma || G.gran == nullptr || G.epoch == nullptr || a.act != ACT_SILU || a.drop.mode == 2 || a.out_el16 == nullptr ||
        a.out_f32 != nullptr || a.up2x)
        return c;
    const int cpg = G.groups > 0 ? a.cout / G.groups : 0;
    if (cpg < 8 || cpg % 8 != 0 || 64 % cpg != 0 || cpg * G.groups != a.cout) return c;  // a group lies inside one 64-channel block
    const bool conv3 = a.kh == 3 && a.kw == 3 && a.stride == 1 && a.pad == 1;
    if (conv3 && a.cout % 64 == 0) {
        if (const el16_t* f = gn16_admits(a, w, a.cout % 256 == 0)) return {ConvForm::Gn16, f, conv_gn16_slots(a.h, a.w), 0};
        const int slots = conv_halo5_gn_slots(a.h, a.w);  // 16 x 32 tiles: conv_up_halo_kernel<5, 2>
        if (const el16_t* f = gn_slots_fit(slots, G.max_slots) ? halo5_admits(a, w) : nullptr) return {ConvForm::Halo5, f, slots, 0};
    }
    if ((c.frag = igemm2_fused_admits(a, w, &c))) c.form = ConvForm::Igemm2;
    return c;
}

// choose-then-launch for the three entry points: the choice's fields go into the ConvArgs, the form's own launcher does the rest
hipError_t launch_chosen(ConvArgs& a, const ConvChoice& c, hipStream_t stream) {
    switch (c.form) {
    case ConvForm::Invalid: return hipErrorInvalidValue;
    case ConvForm::None: return hipSuccess;
    case ConvForm::Direct: return launch_conv_direct(a, stream);
    case ConvForm::Igemm128:
    case ConvForm::Igemm256x64: return launch_conv_igemm(a, stream);
    case ConvForm::UpHalo: return launch_conv_up_halo(a, stream);
    case ConvForm::Halo3: a.wpk_up_frag = c.frag; return launch_conv_halo3(a, stream);
    case ConvForm::Rows3: a.wpk_up_frag = c.frag; return launch_conv_halo_rows3(a, stream);
    case ConvForm::Halo5: a.wpk_up_frag = c.frag; return launch_conv_halo5(a, stream);
    case ConvForm::HaloS2: a.wpk_up_frag = c.frag; return launch_conv_halo_s2(a, stream);
    case ConvForm::Gn16: a.wpk_up_frag = c.frag; return launch_conv_gn16(a, stream);
    case ConvForm::Enc0Stem: return launch_conv_enc0_stem(a, c.frag, stream);
    case ConvForm::Igemm2: a.wpk_frag = c.frag; return launch_conv_igemm2(a, stream);
    case ConvForm::Skinny: a.wpk_frag = c.frag; return launch_conv_skinny(a, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

ConvChoice conv_choose_form(const ConvArgs& a, const ConvW& w, int path, ConvWant want) {
    const bool mfma = path == 1 && conv_mfma_supported(a);
    const ConvChoice c = want == ConvWant::GnFused ? choose_gn_fused(a, w, mfma) : choose_plain(a, w, mfma, want == ConvWant::Stats);
    // a source that holds fewer samples than the output (ConvArgs::src0_rows), or the 8-channel stem, is read correctly by one form only
    if (((a.src0_rows > 0 && a.src0_rows != a.n) || a.pix_pitch0 == 8) && c.form != ConvForm::Enc0Stem) return {ConvForm::Invalid, nullptr, 0, 0};
    return c;
}

bool conv_plain3x3_takes_halo5(const ConvArgs& a, const ConvW& w) {
    return a.gn_part == nullptr && a.gnf.gran == nullptr && conv_choose_form(a, w, 1, ConvWant::Plain).form == ConvForm::Halo5;
}

int conv_gn_fused_max_slots(int h, int w) {
    int best = 0;
    for (int s : {conv_halo5_gn_slots(h, w), conv_gn16_slots(h, w), conv_igemm2_gn_slots(h, w), conv_igemm2_gn_slots_bm128(h, w)})
        if (gn_slots_fit(s, GN_FUSE_MAX_SLOTS)) best = std::max(best, s);
    return best;
}

hipError_t launch_conv(const ConvArgs& a, const ConvW& w, int path, hipStream_t stream) {
    return launch_conv_stats(a, w, path, stream, nullptr);
}

// (statistics are only produced when the caller can learn whether they were: gn_slots != null)
hipError_t launch_conv_stats(const ConvArgs& a_in, const ConvW& w, int path, hipStream_t stream, int* gn_slots) {
    if (gn_slots) *gn_slots = 0;
    ConvArgs a = a_in;
    a.wpk = w.wpk;
    a.gn_part = nullptr;  // only a form that produces statistics sees the buffer
    a.gn_slots = 0;
    const bool stats = gn_slots != nullptr && a_in.gn_part != nullptr;
    const ConvChoice c = conv_choose_form(a, w, path, stats ? ConvWant::Stats : ConvWant::Plain);
    if (c.gn_slots > 0) {
        a.gn_part = a_in.gn_part;
        a.gn_slots = c.gn_slots;
        *gn_slots = c.gn_slots;
    }
    return launch_chosen(a, c, stream);
}

hipError_t launch_conv_gn_fused(const ConvArgs& a_in, const ConvW& w, int path, hipStream_t stream, bool* fused) {
    ConvArgs a = a_in;
    a.wpk = w.wpk;
    a.gn_part = nullptr;
    a.gn_slots = 0;
    const ConvChoice c = conv_choose_form(a, w, path, ConvWant::GnFused);
    *fused = c.form != ConvForm::None;
    a.gnf.slots = c.gn_slots;
    if (c.bm) a.gnf.bm = c.bm;
    return launch_chosen(a, c, stream);
}
