#include "executor_internal.h"

#include <cstdint>
#include <sstream>
#include <stdexcept>
#include <string>

#include "igemm_tiles.h"
#include "kernels.h"


namespace ie {

void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

// Kernel operand for a planned view.  A chunk instance of the pipelined host path (PlanInstance::batch_off > 0) addresses its
// image range inside the parent's buffers: same layout, pointer advanced by batch_off images.
TensorArg make_arg(const PlanInstance& pi, const View& v) {
    TensorArg t;
    char* base = reinterpret_cast<char*>(pi.buffers.at(size_t(v.buf)));
    t.n = int(v.n); t.h = int(v.h); t.w = int(v.w); t.c = int(v.c);
    t.f16 = v.f16 ? 1 : 0;
    t.f8 = v.f8 ? 1 : 0;
    const int64_t esize = v.esize();
    if (v.nchw) {
        t.sw = 1; t.sh = v.w; t.sc = v.h * v.w; t.sn = v.c * v.h * v.w;
        t.p = reinterpret_cast<float*>(base + pi.batch_off * t.sn * esize);
    } else {
        t.sc = 1; t.sw = v.pitch; t.sh = v.w * v.pitch; t.sn = v.h * v.w * v.pitch;
        t.p = reinterpret_cast<float*>(base + (v.c_off + pi.batch_off * t.sn) * esize);
    }
    return t;
}


LnArgs MakeLnArgs(const PlanInstance& pi, const Step& s, const float* weights) {
    LnArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.gamma = s.w_off >= 0 ? weights + s.w_off : nullptr;
    a.beta = s.bias_off >= 0 ? weights + s.bias_off : nullptr;
    a.eps = s.ln_eps;
    a.rms = s.rms ? 1 : 0;
    return a;
}

GnArgs MakeGnArgs(const PlanInstance& pi, const Step& s, const float* weights) {
    GnArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.gamma = s.w_off >= 0 ? weights + s.w_off : nullptr;
    a.beta = s.bias_off >= 0 ? weights + s.bias_off : nullptr;
    a.groups = s.gn_groups;
    a.eps = s.ln_eps;
    a.act = int(s.act.kind); a.act_a = s.act.a; a.act_b = s.act.b;
    a.workspace = pi.workspace;
    a.workspace_floats = pi.workspace_floats;
    return a;
}

EmbedArgs MakeEmbedArgs(const PlanInstance& pi, const Step& s, const float* weights) {
    EmbedArgs a;
    a.ids = reinterpret_cast<const int64_t*>(make_arg(pi, s.in).p);
    a.tids = s.has_in2 ? reinterpret_cast<const int64_t*>(make_arg(pi, s.in2).p) : nullptr;
    a.out = make_arg(pi, s.out);
    a.word = s.w_off >= 0 ? weights + s.w_off : nullptr;
    a.type = s.w2_off >= 0 ? weights + s.w2_off : nullptr;
    a.pos = s.emb_pos_off >= 0 ? weights + s.emb_pos_off : nullptr;
    a.gamma = s.bias_off >= 0 ? weights + s.bias_off : nullptr;
    a.beta = s.bias2_off >= 0 ? weights + s.bias2_off : nullptr;
    a.vocab = int(s.emb_vocab);
    a.types = int(s.emb_types);
    a.eps = s.ln_eps;
    return a;
}

AttnArgs MakeAttnArgs(const PlanInstance& pi, const Step& s, const float* weights) {
    AttnArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.heads = s.heads;
    a.head_dim = s.head_dim;
    a.scale = s.attn_scale;
    if (s.key_mask && s.has_in2) {
        a.mask = reinterpret_cast<const int64_t*>(make_arg(pi, s.in2).p);
        a.mask_sn = s.in2.pitch;
        a.mask_value = s.mask_value;
    }
    a.causal = s.causal ? 1 : 0;
    a.kv_heads = s.kv_heads;
    if (s.rope) {
        a.rope_cos = weights + s.w_off;
        a.rope_sin = weights + s.w2_off;
    }
    return a;
}

// A kv_append step or a decode attention step (kernels_decode.hip): the cache views are dense fp32 [N][Hkv][rows][hd] graph inputs / outputs
DecodeArgs MakeDecodeArgs(const PlanInstance& pi, const Step& s, const float* weights) {
    DecodeArgs a;
    a.in = make_arg(pi, s.in);
    if (s.kind == StepKind::Attention) a.out = make_arg(pi, s.out);
    auto cache = [&](const View& v) -> float* { return v.buf >= 0 ? make_arg(pi, v).p : nullptr; };
    a.past_k = cache(s.past_k);
    a.past_v = cache(s.past_v);
    a.present_k = cache(s.present_k);
    a.present_v = cache(s.present_v);
    if (s.inplace) {       // bound to a resident cache: past and present are the layer's storage there, the graph's own cache buffers stay unused
        const KvBinding* kv = pi.kv.get();
        if (!kv || s.kv_layer < 0 || s.kv_layer >= kv->layers) throw std::runtime_error("internal error: in-place step " + s.name + " without its cache layer");
        a.past_k = a.present_k = kv->k[size_t(s.kv_layer)];
        a.past_v = a.present_v = kv->v[size_t(s.kv_layer)];
        a.cache_rows = kv->capacity;
        a.lens = kv->d_lens;
        a.news = kv->d_lens + kv->batch;
    }
    a.heads = s.heads;
    a.kv_heads = s.kv_heads > 0 ? s.kv_heads : s.heads;
    a.head_dim = s.head_dim;
    a.past_len = s.past_len;
    a.new_len = int(s.in.w);
    a.scale = s.attn_scale;
    if (s.key_mask && s.has_in2) {
        a.mask = reinterpret_cast<const int64_t*>(make_arg(pi, s.in2).p);
        a.mask_sn = s.in2.pitch;
        a.mask_value = s.mask_value;
    }
    if (s.rope) {
        a.rope_cos = weights + s.w_off;
        a.rope_sin = weights + s.w2_off;
        a.rope_rows = s.rope_rows;
        if (s.pos.buf >= 0) {
            a.pos = reinterpret_cast<const int64_t*>(make_arg(pi, s.pos).p);
            a.pos_sn = s.pos.pitch;
        }
    }
    a.splits = s.splits > 0 ? s.splits : 1;
    a.workspace = pi.workspace;
    a.workspace_floats = pi.workspace_floats;
    return a;
}

WinAttnArgs MakeWinAttnArgs(const PlanInstance& pi, const Step& s, const float* weights) {
    WinAttnArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.heads = s.heads;
    a.head_dim = s.head_dim;
    a.scale = s.attn_scale;
    a.wh = s.win_h; a.ww = s.win_w; a.sh = s.shift_h; a.sw = s.shift_w;
    a.bias = s.w_off >= 0 ? weights + s.w_off : nullptr;
    a.mask = s.masked && s.w2_off >= 0 ? weights + s.w2_off : nullptr;
    return a;
}

namespace {

// A view's shape and strides as make_arg lays them out, without a buffer (kernel labels of steps outside a plan instance)
TensorArg view_strides(const View& v) {
    TensorArg t;
    t.n = int(v.n); t.h = int(v.h); t.w = int(v.w); t.c = int(v.c);
    t.f16 = v.f16 ? 1 : 0;
    t.f8 = v.f8 ? 1 : 0;
    if (v.nchw) { t.sw = 1; t.sh = v.w; t.sc = v.h * v.w; t.sn = v.c * v.h * v.w; }
    else { t.sc = 1; t.sw = v.pitch; t.sh = v.w * v.pitch; t.sn = v.h * v.w * v.pitch; }
    return t;
}

ResizeArgs MakeResizeArgs(const PlanInstance& pi, const Step& s) {
    ResizeArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.mode = int(s.rs_mode);
    a.coord = int(s.rs_coord);
    a.nearest = int(s.rs_nearest);
    a.scale_h = s.rs_scale_h;
    a.scale_w = s.rs_scale_w;
    return a;
}



// ---- the kernel families of the conv steps: one row per family, read by the tune-file codes, the hand-over (LaunchedStep), the launch (LaunchStep),
// the search (TuneStep) and the labels (kernel_label) ------------------------------------------------------------------------------------------
std::string tile_label(const char* prefix, int tile) { return prefix + std::to_string(tile) + ">"; }

std::string igemm_label(const Step& s) {
    const IgemmTile& T = kIgemmTiles[s.tile];
    return std::string(s.in.f16 ? "conv_igemm_f16_kernel<" : "conv_igemm_kernel<") + std::to_string(T.bm) + "x" + std::to_string(T.bn) +
           (T.kg > 1 ? "x" + std::to_string(T.kg) + "kg" : std::string()) + (T.deep ? ",deep" : "") + (s.algo == ConvAlgo::IgemmVec ? ",vec" : ",scalar") +
           (s.splitk > 1 ? ",splitk" + std::to_string(s.splitk) : std::string()) + ">";
}
std::string raster_label(const Step& s) { return "conv3x3_raster_kernel<t" + std::to_string(s.tile) + (s.splitk > 1 ? ",splitk" + std::to_string(s.splitk) : std::string()) + ">"; }
std::string direct_label(const Step& s) {       // one launcher family, three kernels (kernels_direct.hip): report the one that runs
    return tile_label(s.tile >= 10 ? "conv1x1_as_kernel<f32,t" : s.tile >= kNumDirectBaseTiles ? "conv_win_kernel<f32,t" : s.in.f16 ? "conv_direct_kernel<f16,t" : "conv_direct_kernel<f32,t",
                      s.tile);
}
std::string dw_label(const Step& s) {
    static const int px[kNumConvDwTiles] = {0, 1, 2, 4};
    const bool act = s.act.kind != ActKind::None || s.pre_act.kind != ActKind::None;
    return s.tile == 0 ? std::string("conv_dw_generic_kernel")
                       : std::string("conv_dw_kernel<") + (s.out.f16 ? "f16,k" : "f32,k") + std::to_string(s.kh) + ",s" + std::to_string(s.sh) + ",px" +
                             std::to_string(DwLanePixels(px[s.tile], s.out.f16, s.kh, s.sh, act)) + (act ? ",act>" : ">");
}
std::string grouped_label(const Step& s) {
    const int cfg = GroupedCfgFor(s.in.c, s.out.c, s.group);
    if (s.tile == 0 || cfg < 0) return "conv_grouped_generic_kernel";
    const GroupedCfg& c = kGroupedCfgs[cfg];
    return std::string("conv_grouped_kernel<") + (s.out.f16 ? "f16,c" : "f32,c") + std::to_string(c.cpg) + ",o" + std::to_string(c.opb) + "x" + std::to_string(c.gpb) + ",px" +
           std::to_string(kGroupedPx[s.tile]) + ">";
}
std::string convt_label(const Step& s) {
    return s.tile == 0 ? std::string("convt_generic_kernel")
                       : std::string("convt_phase_kernel<") + (s.out.f16 ? "f16,px" : "f32,px") + std::to_string(32 * kConvtPixelBlocks[s.tile]) + ">";
}

void launch_igemm(const ConvArgs& a, const Step& s, hipStream_t st) {
    if (s.in.f16) check(LaunchConvIgemmF16(a, s.tile, s.splitk, st), "conv_igemm_f16");
    else check(LaunchConvIgemm(a, s.tile, s.algo == ConvAlgo::IgemmVec ? 1 : 0, s.splitk, st), "conv_igemm");
}

constexpr ConvFamily kConvFamilies[] = {
    {ConvAlgo::IgemmVec, 0, kNumIgemmTiles, 0, true, nullptr, launch_igemm, false, true, true, ConvAlgo::IgemmVec, igemm_label},
    {ConvAlgo::Raster3x3, 100, kNumConvRasterTiles, 0, true, [](const ConvArgs& a, const Step& s) { return ConvRasterEligible(a, s.tile); },
     [](const ConvArgs& a, const Step& s, hipStream_t st) { check(LaunchConvRaster3x3(a, s.tile, s.splitk, st), "conv3x3_raster"); }, false, true, false, ConvAlgo::IgemmVec, raster_label},
    {ConvAlgo::Ws1x1, 200, kNumConvWs32Tiles, kNumConvWs16Tiles, true, [](const ConvArgs& a, const Step& s) { return s.in.f16 ? ConvWsEligible(a, s.tile) : ConvWs32Eligible(a, s.tile); },
     [](const ConvArgs& a, const Step& s, hipStream_t st) {
         if (s.in.f16) check(LaunchConvWs1x1F16(a, s.tile, st), "conv1x1_ws_f16");
         else check(LaunchConvWs1x1F32(a, s.tile, st), "conv1x1_ws_f32");
     }, true, false, false, ConvAlgo::IgemmVec, [](const Step& s) { return tile_label(s.in.f16 ? "conv1x1_ws_f16_kernel<t" : "conv1x1_ws_f32_kernel<t", s.tile); }},
    {ConvAlgo::Ws3x3, 300, kNumConvWs3Tiles, 0, true, [](const ConvArgs& a, const Step& s) { return ConvWs3Eligible(a, s.tile); },
     [](const ConvArgs& a, const Step& s, hipStream_t st) { check(LaunchConvWs3x3F16(a, s.tile, st), "conv3x3_ws_f16"); }, false, false, false, ConvAlgo::IgemmVec,
     [](const Step& s) { return tile_label("conv3x3_ws_f16_kernel<t", s.tile); }},
    {ConvAlgo::Direct, 400, kNumConvDirectTiles, 0, true, [](const ConvArgs& a, const Step& s) { return ConvDirectEligible(a, s.tile); },
     [](const ConvArgs& a, const Step& s, hipStream_t st) { check(LaunchConvDirect(a, s.tile, st), "conv_direct"); }, false, false, false, ConvAlgo::IgemmVec, direct_label},
    {ConvAlgo::Wino3x3, 500, kNumConvWinoTiles, 0, true, [](const ConvArgs& a, const Step& s) { return ConvWinoEligible(a, s.tile); },
     [](const ConvArgs& a, const Step& s, hipStream_t st) { check(LaunchConvWino3x3(a, s.tile, st), "conv3x3_wino"); }, false, false, false, ConvAlgo::IgemmVec,
     [](const Step& s) { return tile_label(s.tile >= 8 ? "conv3x3_wino_x6_kernel<t" : "conv3x3_wino_kernel<t", s.tile); }},
    {ConvAlgo::X6, 600, kNumConvX6Tiles, 0, true, [](const ConvArgs& a, const Step& s) { return ConvX6Eligible(a, s.tile); },
     [](const ConvArgs& a, const Step& s, hipStream_t st) { check(LaunchConvX6(a, s.tile, st), "conv1x1_x6"); }, false, false, false, ConvAlgo::IgemmVec,
     [](const Step& s) { return tile_label("conv1x1_x6_kernel<t", s.tile); }},
    {ConvAlgo::Depthwise, 700, kNumConvDwTiles, 0, false, nullptr, nullptr, false, false, false, ConvAlgo::Depthwise, dw_label},
    {ConvAlgo::Grouped, 800, kNumConvGroupedTiles, 0, false, nullptr, nullptr, false, false, false, ConvAlgo::Grouped, grouped_label},
    {ConvAlgo::Transposed, 900, kNumConvtTiles, 0, false, nullptr, nullptr, false, false, false, ConvAlgo::Transposed, convt_label},
    {ConvAlgo::IgemmScalar, -1, kNumIgemmTiles, 0, false, nullptr, launch_igemm, false, true, true, ConvAlgo::IgemmScalar, igemm_label},
    {ConvAlgo::Stem, -1, 1, 0, false, [](const ConvArgs& a, const Step&) { return ConvStemEligible(a); },
     [](const ConvArgs& a, const Step&, hipStream_t st) { check(LaunchConvStem(a, st), "conv_stem"); }, false, false, false, ConvAlgo::IgemmScalar,
     [](const Step& s) { return std::string(s.out.f8 ? "conv_stem_kernel<f16,e4m3 out>" : (s.out.f16 ? "conv_stem_kernel<f16>" : "conv_stem_kernel<f32>")); }},
    {ConvAlgo::Naive, -1, 1, 0, false, nullptr, [](const ConvArgs& a, const Step&, hipStream_t st) { check(LaunchConvNaive(a, st), "conv_naive"); }, false, false, true, ConvAlgo::Naive,
     [](const Step&) { return std::string("conv_naive_kernel"); }},
};
constexpr int coded_families() {               // the leading rows: the ones with tune-file codes, by rising base (conv_families_ok holds the rest to base -1)
    int n = 0;
    while (n < int(sizeof(kConvFamilies) / sizeof(kConvFamilies[0])) && kConvFamilies[n].base >= 0) ++n;
    return n;
}
constexpr int kNumCodedFamilies = coded_families();

constexpr bool conv_families_ok() {
    constexpr int n = int(sizeof(kConvFamilies) / sizeof(kConvFamilies[0]));
    for (int i = 0; i < n; ++i) {
        const ConvFamily& f = kConvFamilies[i];
        if (i >= kNumCodedFamilies) { if (f.base != -1) return false; continue; }
        if (f.base != 100 * i) return false;                                                        // 0, 100, ..., 900: files written before this table must load
        if (f.base + family_tiles(f) > (i + 1 < kNumCodedFamilies ? kConvFamilies[i + 1].base : kLnTuneCode)) return false;      // every tile below the next base
    }
    return true;
}
static_assert(conv_families_ok(), "tune-file code bases must stay 0, 100, ..., 900, rising, every tile count below the next base and below kLnTuneCode");

}  // namespace

constexpr const char* kTuneFileTag = "# ie-tune-v2";
// the tile tables the codes of a file index into: the dense families' counts in the order of their bases, then the fp8, fused and pooled kernels'
std::string tune_file_header() {
    std::ostringstream o;
    o << kTuneFileTag;
    for (const ConvFamily& f : kConvFamilies) {
        if (!f.in_header) continue;
        o << ' ' << f.tiles;
        if (f.tiles16) o << ' ' << f.tiles16;
    }
    o << ' ' << kNumConvWs8Tiles << ' ' << kNumConvWs38Tiles << ' ' << kNumConvDenseFusedTiles << ' ' << kNumConvPooledTiles;
    return o.str();
}

const ConvFamily& conv_family(ConvAlgo algo) {
    for (const auto& f : kConvFamilies) if (f.algo == algo) return f;
    throw std::runtime_error("internal error: conv algorithm " + std::to_string(int(algo)) + " has no kernel family");
}

const ConvFamily& tune_family(int code) {
    const ConvFamily* f = &kConvFamilies[0];
    for (int i = 0; i < kNumCodedFamilies; ++i) if (code >= kConvFamilies[i].base) f = &kConvFamilies[i];
    return *f;
}

int tune_code(ConvAlgo algo, int tile) {
    for (int i = 1; i < kNumCodedFamilies; ++i) if (kConvFamilies[i].algo == algo) return kConvFamilies[i].base + tile;
    return tile;
}

// Kernel arguments of a dense-block chain step (kernels_block.hip) from its parts: (1x1, 3x3) pairs on one concat buffer.
bool DeviceModel::MakeBlockArgs(const PlanInstance& pi, const Step& s, DenseBlockArgs* out) const {
    if (s.parts.size() < 2 || s.parts.size() % 2 || s.parts.size() / 2 > size_t(kMaxBlockLayers) || !w_->d_weights16 || !w_->d_weights16_frag) return false;
    DenseBlockArgs b;
    const Step& f1 = s.parts[0];
    const TensorArg xin = make_arg(pi, f1.in);
    b.x = reinterpret_cast<_Float16*>(xin.p) - f1.in.c_off;           // pixel row start of the concat buffer (this plan instance's image range)
    b.pitch = int(f1.in.pitch);
    b.in_coff = int(f1.in.c_off);
    b.n = int(f1.in.n); b.h = int(f1.in.h); b.w = int(f1.in.w);
    b.wfrag16 = static_cast<const _Float16*>(w_->d_weights16_frag);
    b.w16 = static_cast<const _Float16*>(w_->d_weights16);
    b.w32 = w_->d_weights;
    b.w16_bytes = uint64_t(w_->weight_floats) * 2;
    b.nlayers = int(s.parts.size() / 2);
    auto u = [](int64_t off) { return off >= 0 ? unsigned(off) : 0xffffffffu; };
    for (int l = 0; l < b.nlayers; ++l) {
        const Step& c1 = s.parts[size_t(2 * l)];
        const Step& c3 = s.parts[size_t(2 * l + 1)];
        bool have1 = false, have3 = false;
        for (const auto& fr : w_->frag16_regions) { have1 = have1 || fr.w_off == c1.w_off; have3 = have3 || fr.w_off == c3.w_off; }
        if (!have1 || !have3 || c1.w_off >= (int64_t(1) << 31) || c3.w_off >= (int64_t(1) << 31)) return false;
        DenseBlockLayer& L = b.layer[l];
        L.K = int(c1.in.c);
        L.out_coff = int(c3.out.c_off);
        L.w1 = unsigned(c1.w_off);
        L.w3 = unsigned(c3.w_off);
        L.ps = u(c1.pre_scale_off);
        L.pt = u(c1.pre_shift_off);
        L.b1 = u(c1.bias_off);
        L.b3 = u(c3.bias_off);
        L.flags = (c1.pre_relu ? 1 : 0) | (c1.relu ? 2 : 0) | (c3.relu ? 4 : 0);
    }
    *out = b;
    return true;
}

ConvArgs DeviceModel::MakeConvArgs(const PlanInstance& pi, const Step& s) const {
    const float* wb = w_->d_weights;
    auto wp = [&](int64_t off) -> const float* { return off >= 0 ? wb + off : nullptr; };
    ConvArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    if (s.has_in2) a.res = make_arg(pi, s.in2);
    a.w = wp(s.w_off);
    a.w16 = w_->d_weights16 && s.w_off >= 0 ? static_cast<const char*>(w_->d_weights16) + s.w_off * 2 : nullptr;
    a.wfrag = w_->d_weights_frag && s.w_off >= 0 && s.out.c % 16 == 0 && s.in.c % 16 == 0 && s.kh * s.kw <= 49 ? w_->d_weights_frag + s.w_off : nullptr;
    a.bias = wp(s.bias_off);
    a.pre_scale = wp(s.pre_scale_off);
    a.pre_shift = wp(s.pre_shift_off);
    if (w_->d_weights16 && s.pre_scale_off >= 0) {
        a.pre_scale16 = static_cast<const char*>(w_->d_weights16) + s.pre_scale_off * 2;
        a.pre_shift16 = static_cast<const char*>(w_->d_weights16) + s.pre_shift_off * 2;
    }
    a.kh = s.kh; a.kw = s.kw; a.sh = s.sh; a.sw = s.sw; a.pt = s.pt; a.pl = s.pl;
    a.dh = int16_t(s.dh); a.dw = int16_t(s.dw);
    a.pre_relu = s.pre_relu; a.relu = s.relu;
    a.workspace = pi.workspace;
    a.workspace_floats = pi.workspace_floats;
    a.counters = pi.counters;
    a.num_counters = pi.counters ? kNumCounters : 0;
    if (s.algo == ConvAlgo::X6) {                    // the split kernel reads its three bf16 planes through `w16`
        a.w16 = nullptr;
        for (const auto& xr : w_->x6_regions)
            if (xr.w_off == s.w_off && w_->d_weights_x6) a.w16 = static_cast<const char*>(w_->d_weights_x6) + xr.byte_off;
    }
    if (s.algo == ConvAlgo::Wino3x3) {               // the Winograd kernel reads the transformed weights through `wfrag`
        a.wfrag = nullptr;
        a.w16 = nullptr;
        for (const auto& wr : w_->wino_regions)
            if (wr.w_off == s.w_off && w_->d_weights_wino) {
                a.wfrag = w_->d_weights_wino + wr.u_off;
                a.w16 = w_->d_weights_wino_x6 ? static_cast<const char*>(w_->d_weights_wino_x6) + wr.u_off * 6 : nullptr;
            }
    }
    if (s.out.f8 || s.in.f8) {       // fp8 mode: e4m3 weights, per-channel epilogue multipliers, tensor scales
        const DeviceWeights& W = *w_;
        a.out_qscale = 1.0f / W.scale_of(s.idx);
        a.res_scale = W.scale_of(s.in2_src);
        for (const auto& fc : W.f8_convs)
            if (fc.w_off == s.w_off) {
                a.w8 = static_cast<const char*>(W.d_weights8) + fc.w_off;
                a.escale = W.d_f8_aux + fc.aux_off + (fc.cout + 3) / 4 * 4;
            }
        if (s.algo == ConvAlgo::DualF8 && s.parts.size() == 2) {       // the projection conv rides along as a second GEMM
            const Step& pj = s.parts[0];
            a.in2 = make_arg(pi, pj.in);
            a.sh2 = pj.sh; a.sw2 = pj.sw;
            a.bias_b = wp(pj.bias_off);
            for (const auto& fc : W.f8_convs)
                if (fc.w_off == pj.w_off) {
                    a.w8b = static_cast<const char*>(W.d_weights8) + fc.w_off;
                    a.escale_b = W.d_f8_aux + fc.aux_off + (fc.cout + 3) / 4 * 4;
                }
        }
    }
    return a;
}

DwArgs DeviceModel::MakeDwArgs(const PlanInstance& pi, const Step& s) const {
    const float* wb = w_->d_weights;
    auto wp = [&](int64_t off) -> const float* { return off >= 0 ? wb + off : nullptr; };
    DwArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    if (s.has_in2) a.res = make_arg(pi, s.in2);
    a.w = wp(s.w_off);
    a.bias = wp(s.bias_off);
    a.pre_scale = wp(s.pre_scale_off);
    a.pre_shift = wp(s.pre_shift_off);
    a.pre_relu = s.pre_relu;
    a.pre_hi = s.pre_hi;
    a.kh = s.kh; a.kw = s.kw; a.sh = s.sh; a.sw = s.sw; a.pt = s.pt; a.pl = s.pl;
    a.relu = s.relu;
    a.lo = s.lo;
    a.hi = s.hi;
    a.act = int(s.act.kind); a.act_a = s.act.a; a.act_b = s.act.b;
    a.pre_act = int(s.pre_act.kind); a.pre_act_a = s.pre_act.a; a.pre_act_b = s.pre_act.b;
    return a;
}

GroupedArgs DeviceModel::MakeGroupedArgs(const PlanInstance& pi, const Step& s) const {
    GroupedArgs a;
    static_cast<DwArgs&>(a) = MakeDwArgs(pi, s);
    a.w16 = w_->d_weights16 && s.w_off >= 0 ? static_cast<const char*>(w_->d_weights16) + s.w_off * 2 : nullptr;
    a.groups = s.group;
    return a;
}

ConvtArgs DeviceModel::MakeConvtArgs(const PlanInstance& pi, const Step& s) const {
    ConvtArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.w = s.w_off >= 0 ? w_->d_weights + s.w_off : nullptr;
    a.w16 = w_->d_weights16 && s.w_off >= 0 ? static_cast<const char*>(w_->d_weights16) + s.w_off * 2 : nullptr;
    a.bias = s.bias_off >= 0 ? w_->d_weights + s.bias_off : nullptr;
    a.kh = s.kh; a.kw = s.kw; a.sh = s.sh; a.sw = s.sw; a.pt = s.pt; a.pl = s.pl; a.pb = s.pb; a.pr = s.pr; a.oph = s.oph; a.opw = s.opw;
    a.relu = s.relu;
    return a;
}

SeArgs DeviceModel::MakeSeArgs(const PlanInstance& pi, const Step& s) const {
    const float* wb = w_->d_weights;
    auto wp = [&](int64_t off) -> const float* { return off >= 0 ? wb + off : nullptr; };
    SeArgs a;
    a.in = make_arg(pi, s.in);
    a.out = make_arg(pi, s.out);
    a.w1 = wp(s.w_off);
    a.b1 = wp(s.bias_off);
    a.w2t = wp(s.w2_off);
    a.b2 = wp(s.bias2_off);
    a.mid = s.se_mid;
    a.act1 = int(s.se_act1.kind); a.act1_a = s.se_act1.a; a.act1_b = s.se_act1.b;
    a.act = int(s.act.kind); a.act_a = s.act.a; a.act_b = s.act.b;
    a.chunks = s.se_chunks;
    a.workspace = pi.workspace;
    a.workspace_floats = pi.workspace_floats;
    return a;
}

// The second conv's operands of a fused dense-layer step (kernels_fused.hip): what ConvDenseFusedEligible is asked and LaunchConvDenseFused is given
FusedArgs DeviceModel::MakeFusedArgs(const PlanInstance& pi, const Step& s) const {
    const Step& s3 = s.parts.at(0);
    FusedArgs f;
    f.in3 = make_arg(pi, s3.in);
    f.out3 = make_arg(pi, s3.out);
    f.wfrag3 = w_->d_weights_frag && s3.w_off >= 0 ? w_->d_weights_frag + s3.w_off : nullptr;
    f.bias3 = s3.bias_off >= 0 ? w_->d_weights + s3.bias_off : nullptr;
    f.relu3 = s3.relu;
    return f;
}

// The step that really runs when `s` is launched: `s` itself, or -- a specialised launcher that declines this operand set (alignment,
// LDS budget, a missing weight mirror ...) -- the hand-over step, built in `scratch`.  LaunchStep launches what this returns and
// Profile() labels it, so a declined step is reported under the kernel that ran.
const Step& DeviceModel::LaunchedStep(const PlanInstance& pi, const Step& s, Step& scratch) const {
    auto with_tile = [&](int tile) -> const Step& {
        if (tile == s.tile) return s;
        scratch = s;
        scratch.tile = tile;
        return scratch;
    };
    bool ok = true;
    if (s.kind == StepKind::Attention && !s.parts.empty() && s.tile == 0) return s;      // a decode step on tile 0: its parts
    if (TiledFamily(pi, s, [&](const auto& a, auto eligible, auto, TiledNames) { ok = s.tile == 0 || eligible(a, s.tile); }))
        return with_tile(ok ? s.tile : 0);           // the generic kernel takes every step of its family
    if (s.kind != StepKind::Conv) return s;
    switch (s.algo) {
        case ConvAlgo::StemPool:        // tile 0: the two plain steps
            return with_tile(s.tile != 0 && ConvStemPoolEligible(MakeConvArgs(pi, s)) ? s.tile : 0);
        case ConvAlgo::DenseBlock: {    // tile 0: the 2n plain steps
            DenseBlockArgs b;
            return with_tile(s.tile != 0 && MakeBlockArgs(pi, s, &b) && DenseBlockEligible(b) ? s.tile : 0);
        }
        case ConvAlgo::DenseFused:      // tile 0: the two plain steps
            return with_tile(s.tile != 0 && ConvDenseFusedEligible(MakeConvArgs(pi, s), MakeFusedArgs(pi, s), s.tile) ? s.tile : 0);
        case ConvAlgo::DualF8: return s;
        case ConvAlgo::IgemmF8: {       // a weights-stationary launcher that declines these operands hands the step to the tiled fp8 kernel
            const int t8 = s.tile;
            if (t8 < kWs8Code) return s;
            const ConvArgs a = MakeConvArgs(pi, s);
            const bool ok8 = t8 >= kWs38Code ? ConvWs38Eligible(a, t8 - kWs38Code) : ConvWs8Eligible(a, t8 - kWs8Code);
            return with_tile(ok8 ? t8 : (s.base_tile < kNumConvF8Tiles ? s.base_tile : 3));
        }
        default: {                      // the dense families: the tiled kernel takes every dense conv
            const ConvFamily& f = conv_family(s.algo);
            if (!f.probe) return s;
            ConvArgs a = MakeConvArgs(pi, s);
            if (!f.res_epilogue) a.res = TensorArg();
            if (f.probe(a, s)) return s;
            scratch = s;
            scratch.algo = f.fallback;
            scratch.tile = s.base_tile;
            scratch.splitk = 1;
            return scratch;
        }
    }
}

// Tile 0 of a fused step: its parts, each launched (and handed over) like a step of the plan
void DeviceModel::LaunchParts(const PlanInstance& pi, const Step& s, hipStream_t stream_) {
    for (const Step& q : s.parts) LaunchStep(pi, q, stream_);
}

void DeviceModel::LaunchStep(const PlanInstance& pi, const Step& s_in, hipStream_t stream_) {
    Step handed;
    const Step& s = LaunchedStep(pi, s_in, handed);
    const float* wb = w_->d_weights;
    auto wp = [&](int64_t off) -> const float* { return off >= 0 ? wb + off : nullptr; };
    if (s.kind == StepKind::Embed && (s.out.f8 || !s.in.i64)) throw std::runtime_error("internal error: the embed kernels take int64 ids and write floats or halfs");
    if (s.kind == StepKind::Conv && s.algo == ConvAlgo::Transposed && (s.has_in2 || s.pre_scale_off >= 0))
        throw std::runtime_error("internal error: transposed conv " + s.name + " with a prologue or a residual");
    // a decode step on tile 0 (or one whose tile 4 declined): kv_append, then the attention over `present`
    if (s.kind == StepKind::Attention && !s.parts.empty() && s.tile == 0) { LaunchParts(pi, s, stream_); return; }
    if (TiledFamily(pi, s, [&](const auto& a, auto, auto launch, TiledNames names) {
            if (names.fp8_noun && (s.in.f8 || s.out.f8)) throw std::runtime_error(std::string("internal error: fp8 tensor reached the ") + names.fp8_noun + " kernels");
            check(launch(a, s.tile, stream_), names.label);
        }))
        return;
    switch (s.kind) {
        case StepKind::Conv: {
            if (s.algo == ConvAlgo::DualF8) {
                if (s.in.f8) {          // fp8 plan: the two GEMMs of one launch; e4m3 tensors never reach another kernel
                    if (!w_->f8_ready) throw std::runtime_error("fp8 precision: scales are not calibrated yet");
                    const ConvArgs a = MakeConvArgs(pi, s);
                    const int t = s.tile >= kWs8Code ? s.tile - kWs8Code : 1;
                    if (a.in2.p == nullptr || !ConvWs8Eligible(a, t)) throw std::runtime_error("fp8 precision: the projection-shortcut step " + s.name + " cannot run on the dual 1x1 kernel");
                    check(LaunchConvWs1x1F8(a, t, stream_), "conv1x1_ws_f8(dual)");
                } else {                // the fp16 plan of the fp8 calibration: the same step list, the two plain convs
                    LaunchParts(pi, s, stream_);
                }
                break;
            }
            if (s.algo == ConvAlgo::StemPool) {
                // the stem conv and the max pool behind it in one launch (out = the pooled tensor); tile 0: the two plain steps
                if (s.tile != 0) check(LaunchConvStemPool(MakeConvArgs(pi, s), stream_), "conv_stem_pool");
                else LaunchParts(pi, s, stream_);
                break;
            }
            if (s.algo == ConvAlgo::DenseBlock) {
                DenseBlockArgs b;
                if (s.tile != 0 && MakeBlockArgs(pi, s, &b)) check(LaunchDenseBlockF16(b, stream_), "dense_block_f16");
                else LaunchParts(pi, s, stream_);
                break;
            }
            if (s.algo == ConvAlgo::DenseFused) {
                // one launch for the 3x3 of dense layer L and the 1x1 of layer L+1; tile 0: the two plain steps
                if (s.tile != 0) check(LaunchConvDenseFused(MakeConvArgs(pi, s), MakeFusedArgs(pi, s), s.tile, stream_), "conv_dense_fused");
                else LaunchParts(pi, s, stream_);
                break;
            }
            ConvArgs a = MakeConvArgs(pi, s);
            if (s.algo == ConvAlgo::IgemmF8) {
                // e4m3 tensors: only the fp8 kernel may touch them; a declined launch is an error, never a hand-over to a kernel that
                // would read the bytes as floats
                if (!w_->f8_ready) throw std::runtime_error("fp8 precision: scales are not calibrated yet");
                const int t8 = s.tile;
                if (t8 >= kWs38Code) check(LaunchConvWs3x3F8(a, t8 - kWs38Code, stream_), "conv3x3_ws_f8");        // weights-stationary 3x3 (kernels_ws8.hip)
                else if (t8 >= kWs8Code) check(LaunchConvWs1x1F8(a, t8 - kWs8Code, stream_), "conv1x1_ws_f8");   // weights-stationary 1x1
                else check(LaunchConvIgemmF8(a, t8, stream_), "conv_igemm_f8");
                break;
            }
            const ConvFamily& f = conv_family(s.algo);
            if (a.in.f8 || a.res.f8 || (a.out.f8 && s_in.algo != ConvAlgo::Stem)) throw std::runtime_error("internal error: fp8 tensor reached a non-fp8 conv kernel");
            if ((s.dh != 1 || s.dw != 1) && !f.dilation) throw std::runtime_error("internal error: dilated conv " + s.name + " reached a kernel without dilation");
            // A fused residual Add lives in the epilogue of the families that say so (the weights-stationary 1x1); any other kernel runs the conv without
            // its ReLU and adds the shortcut in place afterwards.
            const TensorArg res = a.res;
            const int relu = a.relu;
            const bool split_res = res.p != nullptr && !f.res_epilogue;
            if (split_res) { a.res = TensorArg(); a.relu = 0; }
            f.launch(a, s, stream_);
            if (split_res) {
                EltArgs e;
                e.a = a.out; e.b = res; e.out = a.out; e.relu = relu;
                check(LaunchEltwise(e, stream_), "eltwise(residual)");
            }
            break;
        }
        case StepKind::Pool: {
            PoolArgs a;
            a.in = make_arg(pi, s.in);
            a.out = make_arg(pi, s.out);
            a.kh = s.kh; a.kw = s.kw; a.sh = s.sh; a.sw = s.sw; a.pt = s.pt; a.pl = s.pl; a.pb = s.pb; a.pr = s.pr;
            a.is_max = s.pool_max; a.count_include_pad = s.count_include_pad;
            a.pre_scale = wp(s.pre_scale_off); a.pre_shift = wp(s.pre_shift_off); a.pre_relu = s.pre_relu;
            if (a.in.f8 || a.out.f8) {
                a.in_scale = w_->scale_of(s.in_src);
                a.out_qscale = 1.0f / w_->scale_of(s.idx);
                check(LaunchPoolF8(a, stream_), "pool_f8");
                break;
            }
            check(LaunchPool(a, stream_), "pool");
            break;
        }
        case StepKind::GlobalAvgPool:
            if (s.in.f8) {
                check(LaunchGlobalAvgPoolF8(make_arg(pi, s.in), make_arg(pi, s.out), w_->scale_of(s.in_src), stream_), "global_avg_pool_f8");
                break;
            }
            check(LaunchGlobalAvgPool(make_arg(pi, s.in), make_arg(pi, s.out), wp(s.pre_scale_off), wp(s.pre_shift_off),
                                      s.pre_relu, stream_, int(s.pre_act.kind), s.pre_act.a, s.pre_act.b), "global_avg_pool");
            break;
        case StepKind::Eltwise: {
            if (s.in.f8 || s.out.f8) throw std::runtime_error("internal error: fp8 tensor reached the eltwise kernel");
            EltArgs a;
            a.a = make_arg(pi, s.in);
            if (s.has_in2) a.b = make_arg(pi, s.in2);
            a.out = make_arg(pi, s.out);
            a.scale = wp(s.pre_scale_off);
            a.shift = wp(s.pre_shift_off);
            a.relu = s.relu;
            a.lo = s.lo;
            a.hi = s.hi;
            a.act = int(s.act.kind); a.act_a = s.act.a; a.act_b = s.act.b;
            a.pre_act = int(s.pre_act.kind); a.pre_act_a = s.pre_act.a; a.pre_act_b = s.pre_act.b;
            a.b_mul = s.mul;
            a.b_bcast = s.has_in2 && s.in2.h * s.in2.w == 1 && s.out.h * s.out.w > 1;
            check(LaunchEltwise(a, stream_), "eltwise");
            break;
        }
        case StepKind::SqueezeExcite: {
            if (s.in.f8 || s.out.f8) throw std::runtime_error("internal error: fp8 tensor reached the squeeze-excite kernels");
            const SeArgs a = MakeSeArgs(pi, s);
            if (!SqueezeExciteEligible(a)) throw std::runtime_error("squeeze-excite step " + s.name + ": the kernels decline its operands");
            check(LaunchSqueezeExcite(a, stream_), "squeeze_excite");
            break;
        }
        case StepKind::Copy:
            if (s.in.f8 || s.out.f8) throw std::runtime_error("internal error: fp8 tensor reached the copy kernel");
            check(LaunchCopy(make_arg(pi, s.in), make_arg(pi, s.out), stream_), "copy");
            break;
        case StepKind::Resize: {
            if (s.in.f8 || s.out.f8) throw std::runtime_error("internal error: fp8 tensor reached the resize kernels");
            const ResizeArgs a = MakeResizeArgs(pi, s);
            check(LaunchResize(a, ResizePath(a), stream_), "resize");
            break;
        }
        case StepKind::TokenAssemble: {
            if (s.in.f8 || s.out.f8) throw std::runtime_error("internal error: fp8 tensor reached the token kernels");
            TokenAssembleArgs a;
            a.in = make_arg(pi, s.in);
            a.out = make_arg(pi, s.out);
            a.cls = wp(s.w_off);
            a.pos = wp(s.bias_off);
            check(LaunchTokenAssemble(a, stream_), "token_assemble");
            break;
        }
        case StepKind::LayerNorm: case StepKind::GroupNorm: case StepKind::Embed: case StepKind::Attention: case StepKind::WindowAttention:
            break;      // (launched through TiledFamily above)
        case StepKind::KvAppend: {
            if (s.in.f8) throw std::runtime_error("internal error: fp8 tensor reached the kv_append kernel");
            const DecodeArgs a = MakeDecodeArgs(pi, s, wb);
            if (!KvAppendEligible(a)) throw std::runtime_error("kv_append step " + s.name + ": the kernel declines its operands");
            check(LaunchKvAppend(a, stream_), "kv_append");
            break;
        }
        case StepKind::PatchMerge: {
            if (s.in.f8 || s.out.f8) throw std::runtime_error("internal error: fp8 tensor reached the patch-merge kernel");
            PatchMergeArgs a;
            a.in = make_arg(pi, s.in);
            a.out = make_arg(pi, s.out);
            check(LaunchPatchMerge(a, stream_), "patch_merge");
            break;
        }
    }
}

std::string kernel_label(const Step& s) {
    switch (s.kind) {
        case StepKind::Conv:
            // the fused and fp8 steps name what they launch themselves; every other conv is labelled by its family's row
            if (s.algo == ConvAlgo::DenseBlock) return s.tile != 0 ? "dense_block_f16_kernel<" + std::to_string(s.parts.size() / 2) + " layers>" : "dense_block_parts<" + std::to_string(s.parts.size()) + " launches>";
            if (s.algo == ConvAlgo::DenseFused && s.tile == 0) return "dense_fused_parts<2 launches>";
            if (s.algo == ConvAlgo::DenseFused) return tile_label(s.tile == 4 || s.tile == 5 ? "conv_dense_fused_ws_kernel<t" : "conv_dense_fused_kernel<t", s.tile);
            if (s.algo == ConvAlgo::DualF8) return s.in.f8 ? tile_label("conv1x1_ws_f8_kernel<dual,t", s.tile >= kWs8Code ? s.tile - kWs8Code : 1) : "dual_f8_parts<2 launches>";
            if (s.algo == ConvAlgo::IgemmF8 && s.tile >= kWs38Code) return tile_label("conv3x3_ws_f8_kernel<t", s.tile - kWs38Code);
            if (s.algo == ConvAlgo::IgemmF8 && s.tile >= kWs8Code) return tile_label("conv1x1_ws_f8_kernel<t", s.tile - kWs8Code);
            if (s.algo == ConvAlgo::IgemmF8)
                return "conv_igemm_f8_kernel<" + std::to_string(kIgemmTiles[s.tile].bm) + "x" + std::to_string(kIgemmTiles[s.tile].bn) + ">";
            if (s.algo == ConvAlgo::StemPool) return s.tile != 0 ? (s.out.f8 ? "conv_stem_kernel<f16,pool,e4m3 out>" : (s.out.f16 ? "conv_stem_kernel<f16,pool>" : "conv_stem_kernel<f32,pool>")) : "stem + pool (2 launches)";
            return conv_family(s.algo).label(s);
        case StepKind::Pool: return s.in.f8 ? "pool_f8_kernel" : "pool_kernel";
        case StepKind::GlobalAvgPool: return s.in.f8 ? "gap_f8_kernel" : "gap_kernel";
        case StepKind::Eltwise: return "eltwise_kernel";
        case StepKind::Copy: return "copy_kernel";
        case StepKind::Resize: {
            static const char* const names[3] = {"resize_generic_kernel", "resize_vec_kernel<", "resize_nchw_kernel<"};
            ResizeArgs a;
            a.in = view_strides(s.in);
            a.out = view_strides(s.out);
            if (s.in.c_off % (s.in.f16 ? 8 : 4)) a.in.p = reinterpret_cast<float*>(uintptr_t(4));    // (a misaligned view: the launcher sees its address)
            if (s.out.c_off % (s.out.f16 ? 8 : 4)) a.out.p = reinterpret_cast<float*>(uintptr_t(4));
            const int path = ResizePath(a);
            return path == 0 ? std::string(names[0]) : std::string(names[path]) + (s.in.f16 ? "f16>" : "f32>");
        }
        case StepKind::LayerNorm: {
            const std::string stem = s.rms ? "rmsnorm" : "layernorm";
            return s.tile == 0 ? stem + "_generic_kernel" : stem + "_kernel<" + (s.out.f16 ? "f16," : "f32,") + std::to_string(kLnLanes[s.tile]) + ">";
        }
        case StepKind::GroupNorm: {
            static const char* const acts[] = {"none", "sigmoid", "", "silu", "", "relu"};
            const std::string t = s.out.f16 ? "f16" : "f32";
            return s.tile == 0 ? std::string("groupnorm_generic_kernel")
                               : "groupnorm_stats_kernel<" + t + "> + groupnorm_apply_kernel<" + t + "," + acts[int(s.act.kind)] + ">";
        }
        case StepKind::Embed: {
            const std::string stem = s.bias_off >= 0 ? "embed_ln" : "embed_sum";       // (no gamma: the sum alone)
            return s.tile == 0 ? stem + "_generic_kernel" : stem + "_kernel<" + (s.out.f16 ? "f16," : "f32,") + std::to_string(kLnLanes[s.tile]) + ">";
        }
        case StepKind::TokenAssemble: return std::string("token_assemble_kernel<") + (s.out.f16 ? "f16>" : "f32>");
        case StepKind::KvAppend: return std::string(s.inplace ? "kv_append_rows_kernel<" : "kv_append_kernel<") + (s.in.f16 ? "f16" : "f32") + (s.inplace ? ",inplace>" : ">");
        case StepKind::Attention:
            if (s.past_len > 0 && s.inplace) {     // a step bound to a resident cache: the in-place forms
                const std::string t = s.out.f16 ? "f16" : "f32";
                if (s.tile == kAttnExtendTile) return "kv_append_rows_kernel + attention_extend_kernel<" + t + "," + std::to_string(s.head_dim) + ",inplace>" + (s.splits > 1 ? " + attention_extend_combine_kernel" : "");
                if (s.tile == kAttnDecodeTile) return "attention_decode_kernel<" + t + "," + std::to_string(s.head_dim) + ",inplace>" + (s.splits > 1 ? " + attention_decode_combine_kernel" : "");
                return std::string(s.parts.empty() ? "" : "kv_append_rows_kernel + ") + "attention_inplace_generic_kernel<" + t + ">";
            }
            if (s.past_len > 0) {
                if (s.tile == kAttnExtendTile) return std::string("kv_append_kernel + attention_extend_kernel<") + (s.out.f16 ? "f16," : "f32,") + std::to_string(s.head_dim) + ">" + (s.splits > 1 ? " + attention_extend_combine_kernel" : "");
                if (s.tile == kAttnDecodeTile) return std::string("attention_decode_kernel<") + (s.out.f16 ? "f16," : "f32,") + std::to_string(s.head_dim) + ">" + (s.splits > 1 ? " + attention_decode_combine_kernel" : "");
                return std::string(s.parts.empty() ? "" : "kv_append_kernel + ") + (s.in.w > 1 ? "attention_extend_generic_kernel<" : "attention_decode_generic_kernel<") + (s.out.f16 ? "f16>" : "f32>");
            }
            if (s.tile == 2) return std::string("attention_stream_kernel<") + (s.out.f16 ? "f16," : "f32,") + std::to_string(s.head_dim) + (s.rope ? ",causal,rope>" : s.causal ? ",causal>" : ">");
            if (s.tile == 3) return std::string("attention_chunk_kernel<") + (s.out.f16 ? "f16," : "f32,") + std::to_string(s.head_dim) + (s.rope ? ",causal,rope>" : s.causal ? ",causal>" : ">");
            return s.tile == 0 ? std::string(s.key_mask ? "attention_generic_kernel<mask>" : s.causal ? "attention_generic_kernel<causal>" : "attention_generic_kernel")
                               : std::string("attention_mfma_kernel<") + (s.out.f16 ? "f16," : "f32,") + std::to_string(s.head_dim) +
                                     (s.key_mask ? ",mask>" : s.rope ? ",causal,rope>" : s.causal ? ",causal>" : ">");
        case StepKind::WindowAttention:
            return s.tile == 0 ? std::string("window_attention_generic_kernel")
                               : std::string("window_attention_mfma_kernel<") + (s.out.f16 ? "f16," : "f32,") + std::to_string(s.head_dim) + ">";
        case StepKind::PatchMerge: {
            const bool vec = !s.in.nchw && !s.out.nchw && PatchMergeVec(s.in.f16, s.out.f16, s.in.c, s.in.pitch, s.in.c_off, s.out.pitch, s.out.c_off);
            return std::string("patch_merge_kernel<") + (vec ? (s.out.f16 ? "f16,8>" : "f32,4>") : (s.out.f16 ? "f16,1>" : "f32,1>"));
        }
        case StepKind::SqueezeExcite: return std::string("se_squeeze_kernel + se_fc1_kernel + se_fc2_kernel + se_apply_kernel<") + (s.out.f16 ? "f16>" : "f32>");
    }
    return "?";
}


}  // namespace ie
