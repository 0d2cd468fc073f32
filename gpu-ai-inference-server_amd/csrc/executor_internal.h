// What executor.cpp (instances, capture, run, profile, host path), launch.cpp (kernel arguments, the kernel-family table, hand-over, launch, labels)
// and tune.cpp (tune file, load-time search, paired transitions) share beyond executor.h.
#pragma once

#include "executor.h"

namespace ie {

#pragma GCC visibility push(hidden)      // shared by the library's own files only: none of this is exported

constexpr int kNumCounters = 1 << 16;

void check(hipError_t e, const char* what);
TensorArg make_arg(const PlanInstance& pi, const View& v);
LnArgs MakeLnArgs(const PlanInstance& pi, const Step& s, const float* weights);
GnArgs MakeGnArgs(const PlanInstance& pi, const Step& s, const float* weights);
EmbedArgs MakeEmbedArgs(const PlanInstance& pi, const Step& s, const float* weights);
AttnArgs MakeAttnArgs(const PlanInstance& pi, const Step& s, const float* weights);
DecodeArgs MakeDecodeArgs(const PlanInstance& pi, const Step& s, const float* weights);
WinAttnArgs MakeWinAttnArgs(const PlanInstance& pi, const Step& s, const float* weights);
std::string kernel_label(const Step& s);

// A family that runs a dense conv on ConvArgs has a launcher; the tiled implicit GEMM takes every such conv, the others probe their operands first and
// hand a step they decline to `fallback` (tile = the step's base_tile, split-K 1).  The depthwise / grouped / transposed rows only hold their tune-file
// codes and label here: their arguments are not ConvArgs, TiledFamily launches them.
struct ConvFamily {
    ConvAlgo algo;
    int base;                 // tune-file code = base + tile.  -1: no codes of its own (a scalar-staging step stores its tile under base 0 like the vector
                              // staging, whichever the step has; naive and stem steps are never tuned)
    int tiles, tiles16;       // tile count; tiles16: of the fp16 kernel where one algo and one code base stand for two kernels (0: one count)
    bool in_header;           // the first line of a tune file names the tile count(s): a file written under other counts is ignored as a whole.  The
                              // rows that came later (depthwise, grouped, transposed) are not named; naming one more row invalidates every file written so far
    bool (*probe)(const ConvArgs&, const Step&);                  // nullptr: takes every step
    void (*launch)(const ConvArgs&, const Step&, hipStream_t);
    bool res_epilogue;        // false: probed and launched with `res` cleared and without the ReLU; LaunchStep adds the shortcut in a second kernel
    bool splitk, dilation;    // takes Step::splitk; may run a dilated conv
    ConvAlgo fallback;
    std::string (*label)(const Step&);
};
// the table's lookups (launch.cpp)
constexpr int family_tiles(const ConvFamily& f) { return f.tiles > f.tiles16 ? f.tiles : f.tiles16; }
const ConvFamily& conv_family(ConvAlgo algo);            // the row of an algorithm that has one (throws for the fused and fp8 steps)
const ConvFamily& tune_family(int code);                 // the row whose codes hold `code`: the last base at or below it
int tune_code(ConvAlgo algo, int tile);
std::string tune_file_header();                          // the first line of a tune file: its tag and the tile counts its codes index into

// Tune-file codes of the conv choices: base + tile of one kernel family, the family of a code is the last base at or below it.  Codes
// below 100 are tiles of the tiled implicit GEMM in whichever staging (vec / scalar) the step has.  fp8 plans store their run-time
// Step::tile (kernels.h kWs8Code, kWs38Code), which lies inside the ranges of the raster and weights-stationary 1x1 codes.
// kLnTuneCode + tile: a layer_norm step's kernel variant.  Not a conv, so it is no row of the table: tune_code_valid and the layer-norm
// branch of TuneStep know its range.
constexpr int kLnTuneCode = 1000;
inline bool ln_tune_code(int t) { return t >= kLnTuneCode && t < kLnTuneCode + kNumLnTiles; }
// kPoolConvTuneCode + c: how a transition's pool, conv and entry-conv steps launch (PairTransitions).  c = 0: every step on its own; 1 + t: pool + conv
// on tile t of conv1x1_pooled_kernel, the entry conv on its own; 1 + kNumConvPooledTiles + t: all three on tile t with the chained second conv
constexpr int kPoolConvTuneCode = 1100;
inline bool pool_conv_tune_code(int t) { return t >= kPoolConvTuneCode && t <= kPoolConvTuneCode + 2 * kNumConvPooledTiles; }


void load_tune_file(const std::string& path, std::map<std::vector<int64_t>, std::pair<int, int>>& cache);      // (tune.cpp)

#pragma GCC visibility pop

// The families with one contract: tile 0 is a generic kernel that takes every step of the family, tiles 1 .. n-1 are variants behind
// eligible(args, tile), launch(args, tile, stream) runs either.  f(args, eligible, launch, names) is called for a step of such a family; false: `s` is
// of none.  LaunchedStep hands over through this, LaunchStep launches through it, TuneTiles searches through it.
template <class F>
bool DeviceModel::TiledFamily(const PlanInstance& pi, const Step& s, F&& f) const {
    const float* wb = w_->d_weights;
    switch (s.kind) {
        case StepKind::LayerNorm: f(MakeLnArgs(pi, s, wb), LayerNormEligible, LaunchLayerNorm, TiledNames{"layer_norm", "layer-norm"}); return true;
        case StepKind::GroupNorm: f(MakeGnArgs(pi, s, wb), GroupNormEligible, LaunchGroupNorm, TiledNames{"group_norm", "group-norm"}); return true;
        case StepKind::Embed: f(MakeEmbedArgs(pi, s, wb), EmbedEligible, LaunchEmbed, TiledNames{"embed", nullptr}); return true;
        case StepKind::Attention:
            // a decode step (a past): its own two tiles, 0 = the generic kernel over `present` and kAttnDecodeTile; the step that carries the parts runs them at tile 0
            if (s.past_len > 0) { f(MakeDecodeArgs(pi, s, wb), AttentionDecodeEligible, LaunchAttentionDecode, TiledNames{"attention_decode", "attention"}); return true; }
            f(MakeAttnArgs(pi, s, wb), AttentionEligible, LaunchAttention, TiledNames{"attention", "attention"});
            return true;
        case StepKind::WindowAttention: f(MakeWinAttnArgs(pi, s, wb), WindowAttentionEligible, LaunchWindowAttention, TiledNames{"window_attention", "window-attention"}); return true;
        case StepKind::Conv:
            if (s.algo == ConvAlgo::Depthwise) { f(MakeDwArgs(pi, s), ConvDwEligible, LaunchConvDw, TiledNames{"conv_dw", nullptr}); return true; }
            if (s.algo == ConvAlgo::Grouped) { f(MakeGroupedArgs(pi, s), ConvGroupedEligible, LaunchConvGrouped, TiledNames{"conv_grouped", nullptr}); return true; }
            if (s.algo == ConvAlgo::Transposed) { f(MakeConvtArgs(pi, s), ConvTransposedEligible, LaunchConvTransposed, TiledNames{"conv_transposed", nullptr}); return true; }
            return false;
        default: return false;
    }
}

}  // namespace ie
