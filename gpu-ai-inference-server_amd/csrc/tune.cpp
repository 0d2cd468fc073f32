#include "executor_internal.h"
#include "env.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <unistd.h>
#include <sstream>

#include "igemm_tiles.h"
#include "kernels.h"


namespace ie {
namespace {

bool tune_code_valid(int t) {
    return (t >= 0 && t - tune_family(t).base < family_tiles(tune_family(t))) || ln_tune_code(t) || pool_conv_tune_code(t) || (t >= kWs8Code && t < kWs8Code + kNumConvWs8Tiles) ||
           (t >= kWs38Code && t < kWs38Code + kNumConvWs38Tiles);
}

}  // namespace

// "<signature ints> : <encoded tile> <splitk>" per line behind a header naming the tile tables the numbers index into; a file
// written by an engine with other tables is ignored as a whole.
void load_tune_file(const std::string& path, std::map<std::vector<int64_t>, std::pair<int, int>>& cache) {
    std::ifstream f(path);
    std::string line;
    if (!f || !std::getline(f, line) || line != tune_file_header()) return;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::vector<int64_t> key;
        std::string tok;
        bool ok = true;
        while (is >> tok && tok != ":") {
            char* endp = nullptr;
            const long long v = std::strtoll(tok.c_str(), &endp, 10);
            if (!endp || *endp) { ok = false; break; }
            key.push_back(v);
        }
        int t = -1, sp = 0;
        if (ok && (is >> t >> sp) && tune_code_valid(t) && sp >= 1 && sp <= 64 &&
            key.size() >= 6)          // (the fused steps have short signatures: stem + pool 7 numbers, dense block 10, dual 9)
            cache[key] = {t, sp};
    }
}

// One top-level Autotune call: the timing events and the L2 scrub buffer (freed on every way out), the cache accessors, and whether a
// choice was searched (the tune file is then saved once, at the end).  The parts of a fused step are tuned with the same context.
struct DeviceModel::TuneContext {
    DeviceWeights& w;
    bool allow_search, log;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    void* scrub = nullptr;                 // nullptr: the hot protocol
    bool searched = false;
    static constexpr size_t kScrubBytes = size_t(64) << 20;       // > 8 x 4 MiB of L2
    ~TuneContext() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (scrub) (void)hipFree(scrub);
    }
    bool lookup(const std::vector<int64_t>& key, std::pair<int, int>* choice) {     // (encoded tile, split-K) of a signature
        std::lock_guard<std::mutex> g(w.tune_mu);
        auto hit = w.tune_cache.find(key);
        if (hit == w.tune_cache.end()) return false;
        *choice = hit->second;
        return true;
    }
    void store(const std::vector<int64_t>& key, int code, int splitk) {
        std::lock_guard<std::mutex> g(w.tune_mu);
        w.tune_cache[key] = {code, splitk};
        w.tune_dirty = true;
        searched = true;
    }
};

// Kernel choice per conv step of pi.plan.steps[0, nsteps): an exact hit in the device's cache, else (allow_search) the exhaustive
// timed search, else the cached choice of the same conv at the nearest pixel count (within 2x), else the planner's default.
void DeviceModel::Autotune(PlanInstance& pi, size_t nsteps, bool allow_search) {
    TuneContext ctx{*w_, allow_search, env_.flag("IE_TUNE_LOG")};
    check(hipEventCreate(&ctx.e0), "hipEventCreate");
    check(hipEventCreate(&ctx.e1), "hipEventCreate");
    if (const char* e = env_.get("IE_TUNE_HOT"); allow_search && !(e && std::atoi(e) != 0))
        if (hipMalloc(&ctx.scrub, TuneContext::kScrubBytes) != hipSuccess) { ctx.scrub = nullptr; (void)hipGetLastError(); }
    for (size_t si = 0; si < nsteps && si < pi.plan.steps.size(); ++si) TuneStep(ctx, pi, pi.plan.steps[si]);
    if (nsteps >= pi.plan.steps.size()) PairTransitions(&ctx, pi);      // (a chunk instance runs head steps only: nothing is paired there)
    if (ctx.searched) SaveTuneCache();
}

// Best time in ms of one trial step: a warm launch, then cold -- three rounds of L2 scrub + one timed launch: in the real
// forward a layer finds neither its weights nor its input in L2 (the other layers ran in between), back-to-back repeats would flatter
// every kernel that re-reads operands from L2 -- or hot (IE_TUNE_HOT=1, or no scrub buffer): two timed triples.
float DeviceModel::TimeTrial(TuneContext& ctx, const PlanInstance& pi, const Step& trial) {
    const float best = TimeLaunches(ctx, [&] { LaunchStep(pi, trial, stream_); });
    if (ctx.log)
        std::fprintf(stderr, "[ie-tune] M=%lld N=%lld K=%lld algo=%d tile=%d splitk=%d: %.4f ms\n", static_cast<long long>(trial.out.n * trial.out.h * trial.out.w),
                     static_cast<long long>(trial.out.c), static_cast<long long>(trial.kh * trial.kw * trial.in.c), int(trial.algo), trial.tile, trial.splitk, best);
    return best;
}

// The same protocol for any launch sequence (a step, or the launches of a candidate that covers several steps)
float DeviceModel::TimeLaunches(TuneContext& ctx, const std::function<void()>& launch) {
    auto timed = [&](int launches) {
        check(hipEventRecord(ctx.e0, stream_), "hipEventRecord");
        for (int r = 0; r < launches; ++r) launch();
        check(hipEventRecord(ctx.e1, stream_), "hipEventRecord");
        check(hipEventSynchronize(ctx.e1), "hipEventSynchronize");
        float ms = 0;
        check(hipEventElapsedTime(&ms, ctx.e0, ctx.e1), "hipEventElapsedTime");
        return ms;
    };
    launch();                                        // warm
    float best = 1e30f;
    for (int rep = 0; rep < (ctx.scrub ? 3 : 2); ++rep) {
        if (ctx.scrub) check(hipMemsetAsync(ctx.scrub, 0, TuneContext::kScrubBytes, stream_), "hipMemsetAsync(scrub)");
        best = std::min(best, timed(ctx.scrub ? 1 : 3));
    }
    return best;
}

// The tile of a step of a generic-plus-variants family (TiledFamily): the cached code under `key`, else (allow_search) the fastest of the eligible tiles
// 0 .. ntiles-1, stored as code_base + tile.  A cached code of another family leaves the planner's tile; ties keep the earlier tile; with no eligible
// tile the planner's stays.
void DeviceModel::TuneTiles(TuneContext& ctx, const PlanInstance& pi, Step& s, const std::vector<int64_t>& key, int code_base, int ntiles) {
    std::pair<int, int> hit{-1, 0};
    if (ctx.lookup(key, &hit)) {
        if (hit.first >= code_base && hit.first < code_base + ntiles) s.tile = hit.first - code_base;
        return;
    }
    if (!ctx.allow_search) return;
    float best = 1e30f;
    int best_t = s.tile;
    TiledFamily(pi, s, [&](const auto& a, auto eligible, auto, TiledNames) {
        for (int t = 0; t < ntiles; ++t)
            if (eligible(a, t)) {
                Step trial = s;
                trial.tile = t;
                if (const float ms = TimeTrial(ctx, pi, trial); ms < best) { best = ms; best_t = t; }
            }
    });
    s.tile = best_t;
    ctx.store(key, code_base + best_t, 1);
}

// A fused step's parts (tile 0) against its fused tiles 1 .. last_tile that can(tile) admits: one timed choice, cached under `key` (`search` false: only a
// cached choice is taken).  A fused tile replaces the best so far when its time is below margin x that time (or_equal: or equal to it).
template <class Can>
void DeviceModel::TuneFusedChoice(TuneContext& ctx, const PlanInstance& pi, Step& s, const std::vector<int64_t>& key, int last_tile, bool search, float margin, bool or_equal,
                                  Can&& can) {
    std::pair<int, int> hit{-1, 0};
    int choice = ctx.lookup(key, &hit) ? hit.first : -1;
    if (choice < 0 && ctx.allow_search && search) {
        auto time_tile = [&](int t) {
            Step trial = s;
            trial.tile = t;
            return TimeTrial(ctx, pi, trial);
        };
        float best = time_tile(0);
        choice = 0;
        for (int t = 1; t <= last_tile; ++t)
            if (can(t))
                if (const float ms = time_tile(t); ms < best * margin || (or_equal && ms == best * margin)) { best = ms; choice = t; }
        ctx.store(key, choice, 1);
    }
    if (choice >= 0) s.tile = choice;
}

void DeviceModel::TuneStep(TuneContext& ctx, const PlanInstance& pi, Step& s) {
    if (s.kind == StepKind::LayerNorm) {
        // the generic kernel and the lane-group variants that hold the row (tune-file codes kLnTuneCode + tile)
        // (the channel offsets decide which tiles are eligible: they are part of the signature)
        TuneTiles(ctx, pi, s, {s.in.n * s.in.h * s.in.w, s.in.c, s.in.pitch, s.out.pitch, s.in.c_off, s.out.c_off, int64_t(s.in.f16), int64_t(s.out.f16), kLnTuneCode, s.rms ? 2 : s.bias_off >= 0},
                  kLnTuneCode, kNumLnTiles);
        return;
    }
    if (s.kind != StepKind::Conv || s.algo == ConvAlgo::Naive || s.algo == ConvAlgo::Stem) return;
    std::pair<int, int> hit{-1, 0};
    auto time_tile = [&](int t) {
        Step trial = s;
        trial.tile = t;
        return TimeTrial(ctx, pi, trial);
    };
    if (s.algo == ConvAlgo::DualF8) {
        if (!s.in.f8) return;                  // (a calibration plan: never tuned)
        const std::vector<int64_t> key = {s.out.n * s.out.h * s.out.w, s.out.c, s.in.c, s.parts.size() == 2 ? s.parts[0].in.c : 0, s.parts.size() == 2 ? s.parts[0].sh : 0,
                                          s.in.pitch, s.out.pitch, int64_t(ConvAlgo::DualF8), s.bias_off >= 0};
        if (ctx.lookup(key, &hit)) { s.tile = hit.first; return; }
        if (!ctx.allow_search || !w_->f8_ready) return;
        const ConvArgs a = MakeConvArgs(pi, s);
        float best = 1e30f;
        int best_t = kWs8Code + 1;             // (tile 0 is not a candidate)
        for (int t = 1; t < kNumConvWs8Tiles; ++t)
            if (ConvWs8Eligible(a, t))
                if (const float ms = time_tile(kWs8Code + t); ms < best) { best = ms; best_t = kWs8Code + t; }
        s.tile = best_t;
        ctx.store(key, best_t, 1);
        return;
    }
    if (s.algo == ConvAlgo::StemPool) {
        // fused vs the two launches (tile 1 / 0); within the timer's noise (5 %) the single launch wins: it moves a third of the bytes
        const bool can = ConvStemPoolEligible(MakeConvArgs(pi, s));
        TuneFusedChoice(ctx, pi, s, {s.in.n, s.in.h, s.in.w, s.out.c, s.out.pitch, s.out.f8 ? 2 : (s.out.f16 ? 1 : 0), int64_t(ConvAlgo::StemPool)}, 1,
                        can && !(s.out.f8 && !w_->f8_ready), 1.05f, true, [](int) { return true; });
        if (!can) s.tile = 0;
        return;
    }
    // the parts of a fused step get their own kernel choices (what runs when the fused launcher declines, and the yardstick), tuned in
    // place: they address the parent's buffers like every step (make_arg reads only buffers and batch_off)
    if (s.algo == ConvAlgo::DenseBlock || s.algo == ConvAlgo::DenseFused)
        for (Step& q : s.parts) TuneStep(ctx, pi, q);
    if (s.algo == ConvAlgo::DenseBlock) {
        // chain vs parts (tile 1 = one launch, 0 = the 2n plain launches); the chain wins a tie
        DenseBlockArgs b;
        const bool can = MakeBlockArgs(pi, s, &b) && DenseBlockEligible(b);
        TuneFusedChoice(ctx, pi, s, {s.in.n * s.in.h * s.in.w, int64_t(s.parts.size()), s.in.c, s.in.h, s.in.w, s.in.pitch, s.in.c_off, int64_t(ConvAlgo::DenseBlock),
                                     s.pre_scale_off >= 0, s.bias_off >= 0}, 1, can, 1.0f, true, [](int) { return true; });
        if (!can) s.tile = 0;
        return;
    }
    if (s.algo == ConvAlgo::DenseFused) {
        // fused vs split (tile 1 .. kNumConvDenseFusedTiles = fused tile variants of kernels_fused.hip, 0 = the two plain launches: what runs when
        // ConvDenseFusedEligible declines); the earlier candidate wins a tie
        const Step& p3 = s.parts[0];
        TuneFusedChoice(ctx, pi, s, {s.out.n * s.out.h * s.out.w, s.out.c, s.in.c, 1, 1, 1, 1, 0, 0, s.in.h, s.in.w, s.in.pitch, s.out.pitch, 0, int64_t(ConvAlgo::DenseFused),
                                     s.pre_scale_off >= 0, s.bias_off >= 0, p3.in.c, p3.in.pitch}, kNumConvDenseFusedTiles, true, 1.0f, false,
                        [&](int t) { return ConvDenseFusedEligible(MakeConvArgs(pi, s), MakeFusedArgs(pi, s), t); });      // (built when a search asks, not on a cache hit)
        return;
    }
    // depthwise, grouped and transposed convs: the generic kernel and the family's variants (tune-file codes 700 / 800 / 900 + tile); nothing else may run them
    if (s.algo == ConvAlgo::Depthwise) {
        TuneTiles(ctx, pi, s, {s.out.n * s.out.h * s.out.w, s.out.c, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.in.h, s.in.w, s.in.pitch, s.out.pitch,
                               s.in.nchw ? 2 : int64_t(s.in.f16), int64_t(ConvAlgo::Depthwise), s.pre_scale_off >= 0, s.has_in2},
                  conv_family(s.algo).base, conv_family(s.algo).tiles);
        return;
    }
    if (s.algo == ConvAlgo::Grouped) {
        TuneTiles(ctx, pi, s, {s.out.n * s.out.h * s.out.w, s.out.c, s.in.c, s.group, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.in.h, s.in.w, s.in.pitch,
                               s.out.pitch, s.in.nchw ? 2 : int64_t(s.in.f16), int64_t(ConvAlgo::Grouped), s.pre_scale_off >= 0, s.has_in2},
                  conv_family(s.algo).base, conv_family(s.algo).tiles);
        return;
    }
    if (s.algo == ConvAlgo::Transposed) {
        TuneTiles(ctx, pi, s, {s.in.n * s.in.h * s.in.w, s.out.c, s.in.c, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.pb, s.pr, s.oph, s.opw, s.in.h, s.in.w,
                               s.in.pitch, s.out.pitch, s.in.nchw ? 2 : int64_t(s.in.f16), int64_t(ConvAlgo::Transposed), s.bias_off >= 0},
                  conv_family(s.algo).base, conv_family(s.algo).tiles);
        return;
    }
    const int64_t M = s.out.n * s.out.h * s.out.w, N = s.out.c;
    if (s.algo == ConvAlgo::IgemmF8) {
        // fp8 convs: the tiled implicit GEMM's tiles, then the weights-stationary 1x1 kernel's, then the 3x3's
        const std::vector<int64_t> key = {M, N, s.in.c, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.in.h, s.in.w, s.in.pitch, s.out.pitch, 0, int64_t(s.algo), 0,
                                          s.bias_off >= 0, 8, s.has_in2};
        if (ctx.lookup(key, &hit)) { s.tile = hit.first; return; }
        if (!ctx.allow_search || !w_->f8_ready) return;
        const ConvArgs a = MakeConvArgs(pi, s);
        float best = 1e30f;
        int best_t = s.tile;
        auto consider = [&](int t) { if (const float ms = time_tile(t); ms < best) { best = ms; best_t = t; } };
        for (int t = 0; t < kNumConvF8Tiles; ++t) if (!(kIgemmTiles[t].bn > 32 && N <= 32)) consider(t);
        for (int t = 0; t < kNumConvWs8Tiles; ++t) if (ConvWs8Eligible(a, t)) consider(kWs8Code + t);
        for (int t = 0; t < kNumConvWs38Tiles; ++t) if (ConvWs38Eligible(a, t)) consider(kWs38Code + t);
        s.tile = best_t;
        ctx.store(key, best_t, 1);
        return;
    }
    const Step planned = s;                    // the planner's default, kept when nothing better is known
    // the planner's default may already name a specialised kernel: the search starts from the tiled implicit GEMM either way
    if (conv_family(s.algo).fallback != s.algo) {
        s.algo = conv_family(s.algo).fallback;
        s.tile = s.base_tile;
        s.splitk = 1;
    }
    const int64_t bk = s.in.f16 ? 2 * kIgemmBK : kIgemmBK;
    const int64_t KT = s.algo == ConvAlgo::IgemmVec ? int64_t(s.kh) * s.kw * ((s.in.c + bk - 1) / bk)
                                                   : (int64_t(s.kh) * s.kw * s.in.c + kIgemmBK - 1) / kIgemmBK;
    std::vector<int64_t> key = {M, N, s.in.c, s.kh, s.kw, s.sh, s.sw, s.pt, s.pl, s.in.h, s.in.w, s.in.pitch, s.out.pitch,
                                s.in.nchw, int64_t(s.algo), s.pre_scale_off >= 0, s.bias_off >= 0};
    if (s.in.f16 || s.out.f16) { key.push_back(s.in.f16); key.push_back(s.out.f16); }   // fp32 signatures keep 17 entries
    if (s.has_in2) key.push_back(1);              // a fused residual changes which kernels apply (18 / 20 entries)
    const bool dil = s.dh != 1 || s.dw != 1;
    if (dil) key.insert(key.end(), {-1, s.dh, s.dw});   // dilated convs: -1 (no other signature has a negative entry) and the dilation
    // Split-K admissibility (sp > 1) of the two families that split, for the search and for a choice taken from another pixel count
    auto igemm_split_ok = [&](const IgemmTile& T, int sp) {
        const int64_t wgs = ((M + T.bm - 1) / T.bm) * ((N + T.bn - 1) / T.bn);
        if (T.kg > 1 && ((!two_pass_splitk_ && !s.in.f16) || KT / (sp * T.kg) < 2)) return false;
        return KT / sp >= 2 && int64_t(sp) * wgs * T.bm * T.bn <= pi.workspace_floats && wgs <= kNumCounters && wgs * sp <= 8192 && wgs < 1024;
    };
    auto raster_split_ok = [&](int sp) {
        const int64_t chunks = (s.in.c + kIgemmBK - 1) / kIgemmBK, Mr = s.in.n * (s.in.h + 1) * (s.in.w + 1);
        return sp <= chunks && Mr / 64 * sp <= 16384 && int64_t(sp) * (M + 256) * (N + 64) * 2 <= pi.workspace_floats;
    };
    bool exact = ctx.lookup(key, &hit);
    if (!exact && !ctx.allow_search) {
        // nearest pixel count of the same conv (every other field of the signature equal), at most 2x away
        double best_d = 1.0;        // |log2(M' / M)| <= 1
        std::lock_guard<std::mutex> g(w_->tune_mu);
        for (const auto& kv : w_->tune_cache) {
            if (kv.first.size() != key.size() || !std::equal(kv.first.begin() + 1, kv.first.end(), key.begin() + 1)) continue;
            const double d = std::fabs(std::log2(double(kv.first[0]) / double(M)));
            if (d <= best_d) { best_d = d; hit = kv.second; }
        }
    }
    if (exact || hit.first >= 0) {
        const ConvFamily& f = tune_family(hit.first);
        int sp = hit.second;
        if (!exact && sp > 1 && !(f.splitk && (f.base == 0 ? igemm_split_ok(kIgemmTiles[hit.first], sp) : raster_split_ok(sp))))
            sp = 1;                             // split-K slabs must fit this instance's workspace at this pixel count
        if (f.base != 0) s.algo = f.algo;
        s.tile = hit.first - f.base;
        s.splitk = sp;
        return;
    }
    if (!ctx.allow_search) { s = planned; return; }
    float best = 1e30f;
    Step chosen = s;
    auto consider = [&](ConvAlgo algo, int t, int sp) {
        Step trial = s;
        trial.algo = algo;
        trial.tile = t;
        trial.splitk = sp;
        if (const float ms = TimeTrial(ctx, pi, trial); ms < best) { best = ms; chosen = trial; }
    };
    // A specialised family's tiles: admit(tile, eligible, operands) for every tile of the kernel this precision runs, probed on the operands its launch
    // will get (`res` cleared where the family has no residual epilogue).  The pre-conditions stay here, next to each family, and so does the order:
    // raster, Winograd, bf16x6, direct, weights-stationary 1x1, 3x3, then the tiled GEMM -- the earlier trial wins a tie.
    auto each_tile = [&](ConvAlgo algo, auto&& admit) {
        const ConvFamily& f = conv_family(algo);
        Step probe = s;
        probe.algo = algo;
        ConvArgs a = MakeConvArgs(pi, probe);
        if (!f.res_epilogue) a.res = TensorArg();
        for (probe.tile = 0; probe.tile < (s.in.f16 && f.tiles16 ? f.tiles16 : f.tiles); ++probe.tile) admit(probe.tile, f.probe(a, probe), a);
    };
    const bool from_igemm = !dil && s.algo == ConvAlgo::IgemmVec;       // (a dilated conv only has the implicit GEMM's base tiles: every other family reads adjacent taps)
    const bool f32 = !s.in.f16 && !s.out.f16;
    // LDS-window kernel for 3x3/s1/p1 convs without an activation prologue
    if (from_igemm && f32 && s.kh == 3 && s.kw == 3 && s.sh == 1 && s.sw == 1 && s.pt == 1 && s.pl == 1 && s.pb == 1 && s.pr == 1 && s.pre_scale_off < 0)
        each_tile(ConvAlgo::Raster3x3, [&](int t, bool ok, const ConvArgs&) {
            if (!ok || (ConvRasterTileBn(t) > 32 && N <= 32)) return;
            for (int sp : {1, 2, 4, 8})
                if (sp == 1 || raster_split_ok(sp)) consider(ConvAlgo::Raster3x3, t, sp);
        });
    // Winograd F(2x2, 3x3): 2.25x fewer MACs for the 32-channel 3x3 convs on even-sized images
    if (from_igemm && f32 && s.kh == 3 && s.kw == 3 && s.out.c == 32 && !s.has_in2)
        each_tile(ConvAlgo::Wino3x3, [&](int t, bool ok, const ConvArgs& probe) {
            if (ok) consider(ConvAlgo::Wino3x3, t, 1);
            else if (ctx.log)
                std::fprintf(stderr, "[ie-tune] M=%lld wino tile %d ineligible: wfrag=%p in(c=%d h=%d w=%d sw=%lld sh=%lld sn=%lld p=%p) out(c=%d sw=%lld p=%p) bias=%p pre=%p\n",
                             static_cast<long long>(M), t, (const void*)probe.wfrag, probe.in.c, probe.in.h, probe.in.w, (long long)probe.in.sw, (long long)probe.in.sh,
                             (long long)probe.in.sn, (void*)probe.in.p, probe.out.c, (long long)probe.out.sw, (void*)probe.out.p, (const void*)probe.bias, (const void*)probe.pre_scale);
        });
    // bf16x6 (opt-in): the 1x1 convs on the bf16 matrix pipe with exactly split operands
    if (from_igemm && w_->d_weights_x6 && f32 && s.kh == 1 && s.kw == 1 && !s.has_in2)
        each_tile(ConvAlgo::X6, [&](int t, bool ok, const ConvArgs&) { if (ok) consider(ConvAlgo::X6, t, 1); });
    // the kernels_direct.hip family (every variant checks its own pixel-count / shape limits): K split over the waves with
    // operands straight from global memory, LDS-window tiles, activations-stationary 1x1, window + streamed weights
    if (from_igemm) each_tile(ConvAlgo::Direct, [&](int t, bool ok, const ConvArgs&) { if (ok) consider(ConvAlgo::Direct, t, 1); });
    // 1x1/s1: weights-stationary streaming kernel (either precision)
    if (from_igemm && s.kh == 1 && s.kw == 1) each_tile(ConvAlgo::Ws1x1, [&](int t, bool ok, const ConvArgs&) { if (ok) consider(ConvAlgo::Ws1x1, t, 1); });
    if (from_igemm && s.in.f16 && s.kh == 3 && s.kw == 3) each_tile(ConvAlgo::Ws3x3, [&](int t, bool ok, const ConvArgs&) { if (ok) consider(ConvAlgo::Ws3x3, t, 1); });
    static const int kSplits[] = {1, 2, 3, 4, 6, 8, 12, 16, 24};
    for (int t = 0; t < kNumIgemmTiles; ++t) {
        const IgemmTile& T = kIgemmTiles[t];
        if (dil && t >= kNumIgemmBaseTiles) continue;
        if ((T.bn > 32 && N <= 32) || (T.bn > 64 && N <= 64)) continue;
        if ((T.kg > 1 || T.deep) && (s.algo != ConvAlgo::IgemmVec || KT < 2 * T.kg)) continue;
        if (T.deep && s.in.f16) continue;         // the fp16 kernel has no deep-prefetch variants
        if (T.deep && ((M + T.bm - 1) / T.bm) * ((N + T.bn - 1) / T.bn) > 1024) continue;       // the deep-prefetch variants target grids that cannot fill the chip
        for (int sp : kSplits)
            if (sp == 1 || igemm_split_ok(T, sp)) consider(s.algo, t, sp);
    }
    s = chosen;
    ctx.store(key, tune_code(s.algo, s.tile), s.splitk);
}

// Whole-file rewrite through a temporary + rename, so a reader (another process loading the same model) never sees a torn file
// and concurrent writers cannot interleave lines.
void DeviceModel::SaveTuneCache() {
    std::lock_guard<std::mutex> g(w_->tune_mu);
    if (w_->tune_cache_path.empty() || !w_->tune_dirty) return;
    const std::string tmp = w_->tune_cache_path + ".tmp" + std::to_string(long(getpid())) + "." + std::to_string(device_);
    {
        std::ofstream f(tmp, std::ios::trunc);
        if (!f) return;                                   // read-only model directory: keep the choices in memory only
        f << tune_file_header() << '\n';
        for (auto& kv : w_->tune_cache) {
            for (auto v : kv.first) f << v << ' ';
            f << ": " << kv.second.first << ' ' << kv.second.second << '\n';
        }
        if (!f.good()) { f.close(); std::remove(tmp.c_str()); return; }
    }
    if (std::rename(tmp.c_str(), w_->tune_cache_path.c_str()) != 0) std::remove(tmp.c_str());
    else w_->tune_dirty = false;
}

// ---- transitions in one launch (kernels_trans.hip) ------------------------------------------------------------------------------------
namespace {

bool same_view(const View& a, const View& b) {
    return a.buf == b.buf && a.n == b.n && a.c == b.c && a.h == b.h && a.w == b.w && a.c_off == b.c_off && a.pitch == b.pitch && a.nchw == b.nchw && a.f16 == b.f16 &&
           a.f8 == b.f8;
}
bool views_overlap(const View& a, const View& b) {
    return a.buf == b.buf && (a.nchw || b.nchw || (a.c_off < b.c_off + b.c && b.c_off < a.c_off + a.c));
}
// a write of `w` ends the life of the tensor in view `v`: another tensor laid out in the same (recycled) buffer, or the same pixel rows with v's channels rewritten
bool view_kills(const View& w, const View& v) {
    if (w.buf != v.buf) return false;
    if (w.nchw || v.nchw || w.pitch != v.pitch || w.n != v.n || w.h != v.h || w.w != v.w) return true;
    return w.c_off <= v.c_off && w.c_off + w.c >= v.c_off + v.c;
}
void step_views(const Step& s, std::vector<const View*>& reads, std::vector<const View*>& writes) {
    reads.push_back(&s.in);
    if (s.has_in2) reads.push_back(&s.in2);
    writes.push_back(&s.out);
    for (const Step& q : s.parts) step_views(q, reads, writes);
}
// a dense 1x1 / stride-1 conv step with nothing but bias and ReLU behind it
const char* plain_1x1(const Step& c) {
    if (c.kind != StepKind::Conv) return "is not a conv";
    if (!c.parts.empty() || IsGroupConv(c.algo) || c.group != 1 || c.algo == ConvAlgo::Stem) return "is a fused or grouped conv step";
    if (c.kh != 1 || c.kw != 1 || c.sh != 1 || c.sw != 1 || c.pt || c.pl || c.pb || c.pr || c.dh != 1 || c.dw != 1) return "is not a 1x1 / stride-1 conv";
    if (c.has_in2) return "has a residual";
    if (c.act.kind != ActKind::None || c.lo != -__builtin_huge_valf() || c.hi != __builtin_huge_valf()) return "has an activation other than ReLU";
    if (c.in.nchw || c.out.nchw || c.in.f16 || c.out.f16 || c.in.f8 || c.out.f8) return "is not fp32 NHWC";
    return nullptr;
}

}  // namespace

std::vector<PairedLaunch> FindPairedLaunches(const Plan& plan) {
    std::vector<PairedLaunch> found;
    if (plan.precision != Precision::F32) return found;
    const std::vector<Step>& st = plan.steps;
    for (size_t i = 0; i + 1 < st.size(); ++i) {
        const Step& pl = st[i];
        const Step& cv = st[i + 1];
        if (pl.kind != StepKind::Pool || cv.kind != StepKind::Conv || cv.in.buf != pl.out.buf) continue;
        PairedLaunch c;
        c.steps = {int(i), int(i + 1)};
        auto miss = [&](const std::string& why) { c.reason = why; found.push_back(c); };
        if (pl.pool_max) { miss("the pool is a max pool"); continue; }
        if (pl.kh != 2 || pl.kw != 2 || pl.sh != 2 || pl.sw != 2) {
            miss("the pool is " + std::to_string(pl.kh) + "x" + std::to_string(pl.kw) + " / stride " + std::to_string(pl.sh) + ", not 2x2 / stride 2");
            continue;
        }
        if (pl.pt || pl.pl || pl.pb || pl.pr) { miss("the pool has padding"); continue; }
        if (pl.in.nchw || pl.out.nchw || pl.in.f16 || pl.out.f16 || pl.in.f8 || pl.out.f8) { miss("the pool is not fp32 NHWC"); continue; }
        if (pl.in.h != 2 * pl.out.h || pl.in.w != 2 * pl.out.w) { miss("the pool's windows do not tile its input"); continue; }
        if (pl.act.kind != ActKind::None || pl.pre_act.kind != ActKind::None) { miss("the pool has an activation other than ReLU"); continue; }
        if (const char* why = plain_1x1(cv)) { miss(std::string("the conv ") + why); continue; }
        if (cv.pre_scale_off >= 0) { miss("the conv has a prologue of its own"); continue; }
        if (!same_view(cv.in, pl.out)) { miss("the conv reads another view than the pool writes"); continue; }
        // nothing else may read the pooled tensor: a later step before the view is written again, or the caller (a graph output)
        bool other = false, dead = false;
        for (size_t j = i + 2; j < st.size() && !other && !dead; ++j) {
            std::vector<const View*> reads, writes;
            step_views(st[j], reads, writes);
            for (const View* r : reads) other = other || views_overlap(*r, pl.out);
            for (const View* w : writes) dead = dead || view_kills(*w, pl.out);
        }
        if (other) { miss("a later step also reads the pooled tensor"); continue; }
        if (!dead) {
            bool is_out = false;
            for (const IoDesc& o : plan.outputs) is_out = is_out || views_overlap(o.view, pl.out);
            if (is_out) { miss("the pooled tensor is a graph output"); continue; }
        }
        // one launch reads the pool's input while other workgroups already store the conv's output: the two may not share a (recycled) buffer
        if (cv.out.buf == pl.in.buf) { miss("the conv's output shares the pool input's buffer"); continue; }
        for (int t = 0; t < kNumConvPooledTiles; ++t)
            if (ConvPooledShapeOk(t, false, cv.in.c, cv.out.c, 0)) c.tiles.push_back(t);
        if (c.tiles.empty()) { miss("no tile takes " + std::to_string(cv.in.c) + " -> " + std::to_string(cv.out.c) + " channels"); continue; }
        c.pairable = true;
        // chain: the step behind the conv is the next block's entry 1x1 on exactly the tensor the conv writes
        if (i + 2 < st.size()) {
            const Step& en = st[i + 2];
            std::string why;
            if (const char* w = plain_1x1(en)) why = std::string("the entry step ") + w;
            else if (en.pre_scale_off < 0) why = "the entry conv has no prologue";
            else if (!same_view(en.in, cv.out)) why = "the entry conv reads another view than the conv writes";
            else if (en.out.c != 128) why = "the entry conv has " + std::to_string(en.out.c) + " output channels, not 128";
            else if (en.out.buf == pl.in.buf || en.out.buf == cv.out.buf) why = "the entry conv's output shares a buffer the launch still reads";
            else {
                for (int t = 0; t < kNumConvPooledTiles; ++t)
                    if (ConvPooledShapeOk(t, true, cv.in.c, cv.out.c, en.out.c)) c.chain_tiles.push_back(t);
                if (c.chain_tiles.empty()) why = "no chain tile holds " + std::to_string(cv.out.c) + " channels";
            }
            if (why.empty()) {
                c.chainable = true;
                c.steps.push_back(int(i + 2));
            } else {
                c.reason = "chain: " + why;
            }
        } else {
            c.reason = "chain: no step behind the conv";
        }
        found.push_back(c);
    }
    return found;
}

std::string PairedLaunchesToJson(const std::vector<PairedLaunch>& v) {
    std::ostringstream o;
    auto list = [&](const std::vector<int>& l) {
        o << "[";
        for (size_t k = 0; k < l.size(); ++k) o << (k ? "," : "") << l[k];
        o << "]";
    };
    o << "[";
    for (size_t i = 0; i < v.size(); ++i) {
        const PairedLaunch& c = v[i];
        o << (i ? "," : "") << "{\"steps\":";
        list(c.steps);
        o << ",\"kind\":" << (!c.pairable ? "null" : (c.chainable ? "\"pool_conv_chain\"" : "\"pool_conv\"")) << ",\"tiles\":";
        list(c.tiles);
        o << ",\"chain_tiles\":";
        list(c.chain_tiles);
        o << ",\"reason\":\"" << c.reason << "\"}";         // (reasons are this file's own text: nothing to escape)
    }
    o << "]";
    return o.str();
}

bool DeviceModel::MakePooledArgs(const PlanInstance& pi, size_t i, int count, bool chain, ConvArgs* a, PooledArgs* p) const {
    const std::vector<Step>& st = pi.plan.steps;
    if (i + size_t(count) > st.size() || count < (chain ? 3 : 2)) return false;
    const float* wb = w_->d_weights;
    auto wp = [&](int64_t off) -> const float* { return off >= 0 ? wb + off : nullptr; };
    const Step& pl = st[i];
    *a = MakeConvArgs(pi, st[i + 1]);
    *p = PooledArgs();
    p->pin = make_arg(pi, pl.in);
    p->pool_scale = wp(pl.pre_scale_off);
    p->pool_shift = wp(pl.pre_shift_off);
    p->pool_relu = pl.pre_relu;
    if (chain) {
        const Step& en = st[i + 2];
        p->out2 = make_arg(pi, en.out);
        p->wfrag2 = w_->d_weights_frag && en.w_off >= 0 ? w_->d_weights_frag + en.w_off : nullptr;
        p->bias2 = wp(en.bias_off);
        p->scale2 = wp(en.pre_scale_off);
        p->shift2 = wp(en.pre_shift_off);
        p->pre_relu2 = en.pre_relu;
        p->relu2 = en.relu;
    }
    return true;
}

int DeviceModel::PairedCount(const PlanInstance& pi, size_t i, size_t last, ConvArgs* a, PooledArgs* p, LaunchRole* role) const {
    if (i >= pi.roles.size()) return 1;
    const LaunchRole& r = pi.roles[i];
    if (r.count <= 1 || i + size_t(r.count) > last) return 1;
    if (!MakePooledArgs(pi, i, r.count, r.chain, a, p) || !ConvPooledEligible(*a, *p, r.tile, r.chain)) return 1;      // the launcher would decline: split launches
    *role = r;
    return r.count;
}

// IE_POOL_CONV=0: nothing.  1 / 2 [":tile"]: every eligible transition pairs (2: chains where it can) without timing; a forced tile that is not
// eligible leaves the steps split.  Unset: one timed choice per signature among the split launches, pool + conv per tile (+ the entry conv on its
// own) and the chain per tile, cached under kPoolConvTuneCode -- and nothing without a search (IE_AUTOTUNE=0, forced kernels, the request path
// on an unseen signature).
void DeviceModel::PairTransitions(TuneContext* ctx, PlanInstance& pi) {
    pi.roles.clear();
    const int mode = pool_conv_mode_;
    if (mode == 0 || precision_ != Precision::F32 || pi.batch_off != 0) return;
    if (mode < 0 && (!autotune_ || ctx == nullptr)) return;
    const std::vector<Step>& st = pi.plan.steps;
    std::vector<LaunchRole> roles(st.size());
    bool any = false;
    for (const PairedLaunch& c : FindPairedLaunches(pi.plan)) {
        if (!c.pairable) continue;
        const size_t i = size_t(c.steps[0]);
        ConvArgs a;
        PooledArgs p;
        auto can = [&](int t, bool chain) {
            return t >= 0 && t < kNumConvPooledTiles && (!chain || c.chainable) && MakePooledArgs(pi, i, chain ? 3 : 2, chain, &a, &p) && ConvPooledEligible(a, p, t, chain);
        };
        int tile = -1;
        bool chain = false;
        if (mode > 0) {
            if (pool_conv_tile_ >= 0) {
                if (mode == 2 && can(pool_conv_tile_, true)) { tile = pool_conv_tile_; chain = true; }
                else if (can(pool_conv_tile_, false)) tile = pool_conv_tile_;
            } else {
                for (int t = 0; mode == 2 && tile < 0 && t < kNumConvPooledTiles; ++t) if (can(t, true)) { tile = t; chain = true; }
                for (int t = 0; tile < 0 && t < kNumConvPooledTiles; ++t) if (can(t, false)) tile = t;
            }
        } else {
            const Step& pl = st[i];
            const Step& cv = st[i + 1];
            const size_t span = c.chainable ? 3 : 2;
            const std::vector<int64_t> key = {cv.out.n * cv.out.h * cv.out.w, cv.out.c, cv.in.c, pl.in.h, pl.in.w, pl.in.pitch, cv.out.pitch, kPoolConvTuneCode,
                                              pl.pre_scale_off >= 0, cv.bias_off >= 0, span == 3 ? st[i + 2].out.pitch : 0};
            std::pair<int, int> hit{-1, 0};
            int code = -1;
            if (ctx->lookup(key, &hit)) {
                if (pool_conv_tune_code(hit.first)) code = hit.first - kPoolConvTuneCode;
            } else if (ctx->allow_search) {
                auto alone = [&](size_t from) { for (size_t j = from; j < i + span; ++j) LaunchStep(pi, st[j], stream_); };
                float best = TimeLaunches(*ctx, [&] { alone(i); });
                code = 0;
                auto consider = [&](int t, bool ch) {
                    if (!can(t, ch)) return;
                    const ConvArgs ta = a;
                    const PooledArgs tp = p;
                    const float ms = TimeLaunches(*ctx, [&] {
                        check(LaunchConvPooled(ta, tp, t, ch, stream_), "conv1x1_pooled");
                        if (!ch) alone(i + 2);
                    });
                    if (ctx->log) std::fprintf(stderr, "[ie-tune] transition at step %zu: pooled tile %d%s %.4f ms (split %.4f ms)\n", i, t, ch ? " chain" : "", ms, best);
                    if (ms < best) { best = ms; code = 1 + (ch ? kNumConvPooledTiles : 0) + t; }
                };
                for (int t = 0; t < kNumConvPooledTiles; ++t) consider(t, false);
                for (int t = 0; t < kNumConvPooledTiles; ++t) consider(t, true);
                ctx->store(key, kPoolConvTuneCode + code, 1);
            }
            if (code >= 1) {
                const bool ch = code > kNumConvPooledTiles;
                const int t = code - 1 - (ch ? kNumConvPooledTiles : 0);
                if (can(t, ch)) { tile = t; chain = ch; }
            }
        }
        if (tile < 0) continue;
        roles[i].count = chain ? 3 : 2;
        roles[i].tile = tile;
        roles[i].chain = chain;
        roles[i + 1].count = 0;
        if (chain) roles[i + 2].count = 0;
        any = true;
    }
    if (any) pi.roles = std::move(roles);
}

}  // namespace ie
