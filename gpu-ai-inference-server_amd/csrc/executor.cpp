#include "executor_internal.h"
#include "env.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <unistd.h>
#include <sstream>
#include <stdexcept>

#include "igemm_tiles.h"
#include "kernels.h"


namespace ie {
namespace {

constexpr size_t kPinnedBytes = size_t(4) << 20;              // pinned staging for results (logits are KBs; larger outputs go direct)
constexpr int64_t kTuneWorkspaceFloats = int64_t(16) << 20;   // 64 MiB of split-K slabs available to the autotuner
constexpr int kMaxChunks = 8;

std::once_flag g_kernels_once;
hipError_t g_kernels_err = hipSuccess;

}  // namespace

int HipDeviceCount() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

std::string HipDeviceInfo(int device_id) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device_id) != hipSuccess) { (void)hipGetLastError(); return "Unknown device"; }
    // Same shape as the reference's string (cuda_utils.cu:51-54); on AMD the "compute capability" pair is the
    // gfx major.minor HIP reports (9.5 for gfx950).
    return "Device " + std::to_string(device_id) + ": " + p.name + " (Compute Capability " + std::to_string(p.major) + "." +
           std::to_string(p.minor) + ")";
}

bool HipMemoryInfo(int device_id, size_t* total, size_t* free_b) {
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipSetDevice(device_id) != hipSuccess) { (void)hipGetLastError(); return false; }
    bool ok = hipMemGetInfo(free_b, total) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    (void)hipSetDevice(prev);
    return ok;
}

DeviceWeights::~DeviceWeights() {
    (void)hipSetDevice(device);
    if (d_weights) (void)hipFree(d_weights);
    if (d_weights16) (void)hipFree(d_weights16);
    if (d_weights16_frag) (void)hipFree(d_weights16_frag);
    if (d_weights_frag) (void)hipFree(d_weights_frag);
    if (d_weights8) (void)hipFree(d_weights8);
    if (d_f8_aux) (void)hipFree(d_f8_aux);
    if (d_weights_wino) (void)hipFree(d_weights_wino);
    if (d_weights_x6) (void)hipFree(d_weights_x6);
    if (d_weights_wino_x6) (void)hipFree(d_weights_wino_x6);
}


DeviceModel::DeviceModel(std::shared_ptr<const OnnxModel> model, int device_id, const DeviceModelOptions& opt)
    : model_(std::move(model)), device_(device_id), precision_(opt.precision) {
    env_ = Env::Read();
    SetLaunchKnobs(env_);
    max_inflight_replays_ = std::max(0, env_.integer("IE_MAX_INFLIGHT_REPLAYS", 0));
    int n = HipDeviceCount();
    if (n <= 0) throw std::runtime_error("No HIP device available: the MI355X engine has no CPU fallback");
    if (device_id < 0 || device_id >= n) throw std::runtime_error("Invalid device id " + std::to_string(device_id));
    check(hipSetDevice(device_), "hipSetDevice");
    std::call_once(g_kernels_once, [] {
        g_kernels_err = InitKernels();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsF16();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsWs();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsWs32();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsWs3();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsStem();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsDirect();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsF8();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsFused();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsWino();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsX6();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsBlock();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsWs8();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsAttn();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsDecode();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsWattn();
        if (g_kernels_err == hipSuccess) g_kernels_err = InitKernelsTrans();
    });
    check(g_kernels_err, "InitKernels");
    fp32_split_ = opt.fp32_split && opt.precision == Precision::F32;
    if (const char* e = env_.get("IE_FP32_SPLIT")) fp32_split_ = std::atoi(e) != 0 && opt.precision == Precision::F32;
    if (opt.share) {
        if (opt.share->device != device_) throw std::runtime_error("internal error: shared weights live on another device");
        w_ = opt.share;
    } else {
        w_ = std::make_shared<DeviceWeights>();
        w_->device = device_;
        w_->uploaded = false;
        owns_weights_ = true;
        // Persistent kernel-choice cache: IE_TUNE_CACHE=<file> (""/"0" = none), else the path the bridge derived from the model directory.
        std::string path = opt.tune_cache_path;
        if (const char* tc = env_.get("IE_TUNE_CACHE")) path = (tc[0] == 0 || (tc[0] == '0' && tc[1] == 0)) ? std::string() : std::string(tc);
        if (fp32_split_ && !path.empty()) path += ".x6";       // choices made with the bf16x6 kernels in the search are their own file
        w_->tune_cache_path = path;
        if (!path.empty()) load_tune_file(path, w_->tune_cache);
    }
    upload_weights_ = opt.upload_weights;
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    check(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking), "hipStreamCreate");
    h2d_events_.resize(kMaxChunks, nullptr);
    for (auto& e : h2d_events_) check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    check(hipEventCreate(&t0_event_), "hipEventCreate");
    check(hipEventCreate(&t1_event_), "hipEventCreate");
    const char* ng = env_.get("IE_DISABLE_GRAPH");
    use_graph_ = !(ng && ng[0] == '1');
    const char* at = env_.get("IE_AUTOTUNE");
    // Measured on MI355X (DenseNet-121 B=32): the in-launch combine (agent-scope release/acquire per tile) costs more than
    // the kernel boundary it removes: 3.63 ms/step vs 3.42 ms/step with the separate reduce kernel.  Two-pass is the default.
    const char* tp = env_.get("IE_SPLITK_IN_LAUNCH");
    two_pass_splitk_ = !(tp && tp[0] == '1');
    autotune_ = !(at && at[0] == '0') && !env_.get("IE_FORCE_TILE") && !env_.get("IE_FORCE_SPLITK") && !env_.get("IE_FORCE_ALGO");
    if (const char* pc = env_.get("IE_POOL_CONV"); pc && pc[0] >= '0' && pc[0] <= '2') {      // "0" | "1[:tile]" | "2[:tile]"
        pool_conv_mode_ = pc[0] - '0';
        if (pc[1] == ':' && pc[2] >= '0' && pc[2] <= '9') pool_conv_tile_ = std::atoi(pc + 2);
    }
    if (const char* od = env_.get("IE_TUNE_ON_DEMAND")) tune_on_demand_ = od[0] == '1';
    if (const char* pc = env_.get("IE_PIPELINE_CHUNKS")) pipeline_chunks_ = std::max(0, std::min(kMaxChunks, std::atoi(pc)));
    if (const char* ph = env_.get("IE_PIPELINE_HEAD")) pipeline_head_ = std::max(0, std::atoi(ph));
    if (const char* mp = env_.get("IE_MAX_PLANS")) max_plans_ = size_t(std::max(1, std::atoi(mp)));
    pinned_bytes_ = kPinnedBytes;
    check(hipHostMalloc(&pinned_, pinned_bytes_, hipHostMallocDefault), "hipHostMalloc");
}

DeviceModel::~DeviceModel() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    for (auto& kv : plans_) FreeInstance(*kv.second);
    for (auto e : h2d_events_) if (e) (void)hipEventDestroy(e);
    if (t0_event_) (void)hipEventDestroy(t0_event_);
    if (t1_event_) (void)hipEventDestroy(t1_event_);
    if (pinned_) (void)hipHostFree(pinned_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void DeviceModel::FreeInstance(PlanInstance& pi) {
    for (auto& ch : pi.chunks) FreeInstance(*ch);
    pi.chunks.clear();
    if (pi.graph_exec) (void)hipGraphExecDestroy(pi.graph_exec);
    if (pi.tail_exec) (void)hipGraphExecDestroy(pi.tail_exec);
    pi.graph_exec = nullptr;
    pi.tail_exec = nullptr;
    for (size_t i = 0; i < pi.buffers.size(); ++i)
        if (pi.buffers[i] && pi.owned[i]) (void)hipFree(pi.buffers[i]);
    pi.buffers.clear();
    if (pi.workspace && pi.owns_workspace) (void)hipFree(pi.workspace);
    if (pi.counters && pi.owns_workspace) (void)hipFree(pi.counters);
    pi.workspace = nullptr;
    pi.counters = nullptr;
    for (void* p : pi.u8_stage) if (p) (void)hipFree(p);
    pi.u8_stage.clear();
}

void DeviceModel::CopySync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* what) {
    if (bytes == 0) return;
    check(hipMemcpyAsync(dst, src, bytes, kind, stream_), what);
    check(hipStreamSynchronize(stream_), what);
}

void DeviceModel::ZeroSync(void* dst, size_t bytes, const char* what) {
    if (bytes == 0) return;
    check(hipMemsetAsync(dst, 0, bytes, stream_), what);
    check(hipStreamSynchronize(stream_), what);
}

// Plan + allocate one instance (and, the first time on this device, put the packed weights into HBM).
namespace {
// the layer i of a cache tensor's graph name, `past_key_values.<i>.key|value` or `present.<i>.key|value` (-1: another name)
int kv_layer_of(const std::string& name) {
    for (const char* prefix : {"past_key_values.", "present."}) {
        const size_t n = std::strlen(prefix);
        if (name.compare(0, n, prefix) != 0) continue;
        const size_t dot = name.find('.', n);
        if (dot == std::string::npos || dot == n || dot - n > 6) return -1;
        for (size_t k = n; k < dot; ++k) if (name[k] < '0' || name[k] > '9') return -1;
        return std::atoi(name.substr(n, dot - n).c_str());
    }
    return -1;
}

// The cache steps of an instance built for a bound lane run in place: the layer is the one named by the step's `past` graph input (a prefill with a
// cache: by its `present` graph output).  A step whose tensors are not of the bound geometry is an error here, before anything is allocated.
void MarkInplace(PlanInstance& pi) {
    const KvBinding& kv = *pi.kv;
    auto layer_of = [&](const View& v, const std::vector<IoDesc>& ios) {
        for (const IoDesc& d : ios) if (d.view.buf == v.buf && d.view.c_off == v.c_off) return kv_layer_of(d.name);
        return -1;
    };
    auto mark = [&](Step& s) {
        if (s.kind != StepKind::KvAppend && !(s.kind == StepKind::Attention && s.past_len > 0)) return;
        const int layer = s.past_k.buf >= 0 ? layer_of(s.past_k, pi.plan.inputs) : layer_of(s.present_k, pi.plan.outputs);
        const int hkv = s.kv_heads > 0 ? s.kv_heads : s.heads;
        const bool fits = layer >= 0 && layer < kv.layers && s.in.n == kv.batch && hkv == kv.kv_heads && s.head_dim == kv.head_dim &&
                          (s.past_len > 0 ? s.past_len == kv.capacity : s.in.w <= kv.capacity);
        if (!fits) throw std::runtime_error("the cache step " + s.name + " does not fit the bound KV cache (layer " + std::to_string(layer) + ")");
        s.inplace = true;
        s.kv_layer = layer;
    };
    for (Step& s : pi.plan.steps) {
        mark(s);
        for (Step& q : s.parts) mark(q);
    }
}
}  // namespace

void DeviceModel::BindKvCache(std::shared_ptr<const KvBinding> kv) {
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamSynchronize(copy_stream_), "hipStreamSynchronize");
    check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    for (auto& p : plans_) FreeInstance(*p.second);
    plans_.clear();
    lru_.clear();
    current_ = nullptr;
    kv_ = std::move(kv);
}

void DeviceModel::UploadKvLens(const int* host) {
    if (!kv_) throw std::runtime_error("internal error: no KV cache is bound");
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipMemcpyAsync(kv_->d_lens, host, size_t(2 * kv_->batch) * sizeof(int), hipMemcpyHostToDevice, stream_), "hipMemcpyAsync(kv lengths)");
}

void DeviceModel::BuildInstance(PlanInstance& pi, const std::vector<std::vector<int64_t>>& shapes) {
    pi.plan = BuildPlan(*model_, shapes, precision_);
    if (kv_) {
        pi.kv = kv_;
        MarkInplace(pi);
    }
    {
        std::lock_guard<std::mutex> g(w_->tune_mu);     // lanes of one device may be built concurrently
        if (!w_->d_weights) {
            w_->weight_floats = pi.plan.weights.size();
            check(hipMalloc(reinterpret_cast<void**>(&w_->d_weights), std::max<size_t>(w_->weight_floats, 4) * sizeof(float)), "hipMalloc(weights)");
            w_->device_bytes += w_->weight_floats * sizeof(float);
            if (upload_weights_) {
                CopySync(w_->d_weights, pi.plan.weights.data(), w_->weight_floats * sizeof(float), hipMemcpyHostToDevice, "hipMemcpy(weights)");
                w_->uploaded = true;
            } else {
                ZeroSync(w_->d_weights, w_->weight_floats * sizeof(float), "hipMemset(weights)");
            }
            if (precision_ == Precision::F16 || precision_ == Precision::F8) {
                check(hipMalloc(&w_->d_weights16, std::max<size_t>(w_->weight_floats, 8) * 2), "hipMalloc(weights16)");
                w_->device_bytes += w_->weight_floats * 2;
                if (precision_ == Precision::F16) {
                    // fragment-major mirror of the dense-layer convs (1x1 -> 128 and 3x3 128 -> 32 channels), whatever step they are part of in
                    // this plan instance: the weights are shared by every plan instance, another batch size may fuse other layers
                    auto add16 = [&](const Step& st) {
                        if (st.kind != StepKind::Conv || IsGroupConv(st.algo) || st.w_off < 0 || st.in.nchw || st.sh != 1 || st.sw != 1) return;
                        const bool one = st.kh == 1 && st.kw == 1 && st.out.c == 128 && st.in.c % 32 == 0;
                        const bool three = st.kh == 3 && st.kw == 3 && st.out.c == 32 && st.in.c == 128;
                        if (one || three) w_->frag16_regions.push_back({st.w_off, int(st.out.c), int(st.kh * st.kw * st.in.c)});
                    };
                    for (const Step& st : pi.plan.steps) {
                        if (st.parts.empty()) add16(st);
                        else for (const Step& q : st.parts) add16(q);
                    }
                    if (!w_->frag16_regions.empty()) {
                        check(hipMalloc(&w_->d_weights16_frag, std::max<size_t>(w_->weight_floats, 8) * 2), "hipMalloc(weights16_frag)");
                        w_->device_bytes += w_->weight_floats * 2;
                    }
                }
                if (precision_ == Precision::F8) {
                    check(hipMalloc(&w_->d_weights8, std::max<size_t>(w_->weight_floats, 16)), "hipMalloc(weights8)");
                    ZeroSync(w_->d_weights8, std::max<size_t>(w_->weight_floats, 16), "hipMemset(weights8)");
                    w_->device_bytes += w_->weight_floats;
                    int64_t aux = 0;
                    auto add8 = [&](const Step& st, int i) {
                        if (st.kind != StepKind::Conv || st.algo != ConvAlgo::IgemmF8) return;
                        w_->f8_convs.push_back({i, st.w_off, int(st.out.c), int(st.kh * st.kw * st.in.c), st.in_src, aux});
                        aux += 2 * ((st.out.c + 3) / 4 * 4);
                    };
                    for (size_t i = 0; i < pi.plan.steps.size(); ++i) {
                        const Step& st = pi.plan.steps[i];
                        if (st.parts.empty()) add8(st, int(i));
                        else for (const Step& q : st.parts) add8(q, int(i));       // a projection-shortcut step: both of its convs
                    }
                    check(hipMalloc(reinterpret_cast<void**>(&w_->d_f8_aux), size_t(std::max<int64_t>(aux, 4)) * sizeof(float)), "hipMalloc(f8 aux)");
                    w_->f8_aux_floats = size_t(aux);
                    w_->device_bytes += size_t(aux) * sizeof(float);
                    w_->act_scale.assign(pi.plan.steps.size(), 0.f);
                }
            } else if (const char* nf = env_.get("IE_NO_FRAG_WEIGHTS"); !(nf && std::atoi(nf) != 0)) {
                auto add_region = [&](const Step& st) {
                    if (st.kind == StepKind::Conv && !IsGroupConv(st.algo) && st.w_off >= 0 && st.out.c % 16 == 0 && st.in.c % 16 == 0 && st.kh * st.kw <= 49)
                        w_->frag_regions.push_back({st.w_off, int(st.out.c), st.kh * st.kw, int(st.in.c)});
                };
                for (const Step& st : pi.plan.steps) {
                    if (st.parts.empty()) add_region(st);
                    else for (const Step& q : st.parts) add_region(q);       // a fused dense-layer step: both of its convs
                }
                if (!w_->frag_regions.empty()) {
                    check(hipMalloc(reinterpret_cast<void**>(&w_->d_weights_frag), w_->weight_floats * sizeof(float)), "hipMalloc(weights_frag)");
                    w_->device_bytes += w_->weight_floats * sizeof(float);
                }
                // Winograd-transformed weights for the 3x3 / s1 / p1 convs with 32 output channels (kernels_wino.hip)
                // (every such conv of the graph, also the ones this first plan instance runs inside a fused dense-layer step: the weights are
                // shared by all plan instances, and another batch size fuses other layers)
                int64_t utot = 0;
                auto add_wino = [&](const Step& st) {
                    if (st.kind == StepKind::Conv && !IsGroupConv(st.algo) && st.w_off >= 0 && st.kh == 3 && st.kw == 3 && st.sh == 1 && st.sw == 1 && st.pt == 1 && st.pl == 1 &&
                        st.out.c == 32 && st.in.c % 32 == 0 && !st.in.nchw) {
                        w_->wino_regions.push_back({st.w_off, utot, 32, int(st.in.c)});
                        utot += int64_t(16) * 32 * st.in.c;
                    }
                };
                for (const Step& st : pi.plan.steps) {
                    if (st.parts.empty()) add_wino(st);
                    else for (const Step& q : st.parts) add_wino(q);
                }
                if (utot > 0) {
                    check(hipMalloc(reinterpret_cast<void**>(&w_->d_weights_wino), size_t(utot) * sizeof(float)), "hipMalloc(weights_wino)");
                    w_->wino_floats = size_t(utot);
                    w_->device_bytes += size_t(utot) * sizeof(float);
                }
                // bf16x6 mirrors (opt-in): the 1x1 convs the split kernel can run, whatever step they are part of in this plan instance
                const bool split = fp32_split_;
                w_->fp32_split = split;
                if (split) {
                    int64_t xtot = 0;
                    auto add_x6 = [&](const Step& st) {
                        if (st.kind == StepKind::Conv && !IsGroupConv(st.algo) && st.w_off >= 0 && st.kh == 1 && st.kw == 1 && st.sh == 1 && st.sw == 1 && st.out.c % 128 == 0 && st.in.c % 32 == 0 &&
                            !st.in.nchw) {
                            w_->x6_regions.push_back({st.w_off, xtot, int(st.out.c), int(st.in.c)});
                            xtot += int64_t(3) * st.out.c * st.in.c * 2;
                        }
                    };
                    for (const Step& st : pi.plan.steps) {
                        if (st.parts.empty()) add_x6(st);
                        else for (const Step& q : st.parts) add_x6(q);
                    }
                    if (xtot > 0) {
                        check(hipMalloc(&w_->d_weights_x6, size_t(xtot)), "hipMalloc(weights_x6)");
                        w_->x6_bytes = size_t(xtot);
                        w_->device_bytes += size_t(xtot);
                    }
                    if (utot > 0) {                     // the split Winograd U: 3 planes x 2 bytes against 4 bytes per element
                        check(hipMalloc(&w_->d_weights_wino_x6, size_t(utot) * 6), "hipMalloc(weights_wino_x6)");
                        w_->device_bytes += size_t(utot) * 6;
                    }
                }
            }
            if (w_->uploaded) WeightsArrived();
        } else if (pi.plan.weights.size() != w_->weight_floats) {
            throw std::runtime_error("internal error: weight blob layout depends on the input shape");
        }
    }
    std::vector<float>().swap(pi.plan.weights);   // the host copy of the blob is only needed for the first upload
    AllocInstance(pi);
}

// Device memory of an instance whose plan is set: activation buffers (element size by buffer type) and split-K scratch.
void DeviceModel::AllocInstance(PlanInstance& pi) {
    pi.buffers.assign(pi.plan.buffer_floats.size(), nullptr);
    pi.owned.assign(pi.plan.buffer_floats.size(), 0);
    for (size_t i = 0; i < pi.plan.buffer_floats.size(); ++i) {
        float* p = nullptr;
        const int dt = pi.plan.buffer_f16[i];
        size_t bytes = size_t(std::max<int64_t>(pi.plan.buffer_floats[i], 16)) * size_t(BufferElemBytes(dt));
        check(hipMalloc(reinterpret_cast<void**>(&p), bytes), "hipMalloc(activations)");
        check(hipMemsetAsync(p, 0, bytes, stream_), "hipMemset(activations)");
        device_bytes_ += bytes;
        pi.buffers[i] = p;
        pi.owned[i] = 1;
    }
    // split-K scratch: slabs + per-tile arrival counters (tile-padded slabs need up to 2x the exact S*M*N)
    pi.workspace_floats = std::max<int64_t>(2 * pi.plan.workspace_floats, kTuneWorkspaceFloats);
    size_t bytes = size_t(pi.workspace_floats) * sizeof(float);
    check(hipMalloc(reinterpret_cast<void**>(&pi.workspace), bytes), "hipMalloc(workspace)");
    pi.owns_workspace = true;
    device_bytes_ += bytes;
    if (!two_pass_splitk_) {
        check(hipMalloc(reinterpret_cast<void**>(&pi.counters), kNumCounters * sizeof(int)), "hipMalloc(counters)");
        check(hipMemsetAsync(pi.counters, 0, kNumCounters * sizeof(int), stream_), "hipMemset(counters)");
    }
}

// Capture steps [first, last) of `pi` into an executable graph.
void DeviceModel::Capture(PlanInstance& pi, size_t first, size_t last, hipGraphExec_t* exec) {
    hipGraph_t graph = nullptr;
    check(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    try {
        RunSteps(pi, first, last, nullptr);
    } catch (...) {
        (void)hipStreamEndCapture(stream_, &graph);
        if (graph) (void)hipGraphDestroy(graph);
        throw;
    }
    check(hipStreamEndCapture(stream_, &graph), "hipStreamEndCapture");
    hipError_t e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    check(e, "hipGraphInstantiate");
}

PlanInstance& DeviceModel::Prepare(const std::vector<std::vector<int64_t>>& shapes, bool allow_tune) {
    std::vector<int64_t> key;
    for (auto& s : shapes) { key.push_back(int64_t(s.size())); key.insert(key.end(), s.begin(), s.end()); }
    auto touch = [&](const std::vector<int64_t>& k) {
        for (size_t i = 0; i < lru_.size(); ++i) if (lru_[i] == k) { lru_.erase(lru_.begin() + long(i)); break; }
        lru_.push_back(k);
    };
    check(hipSetDevice(device_), "hipSetDevice");
    auto it = plans_.find(key);
    if (it != plans_.end()) {
        touch(key);
        current_ = it->second.get();
        if (allow_tune) EnsurePipeline(*current_, true);
        return *current_;
    }
    while (plans_.size() >= max_plans_ && !lru_.empty()) {        // make room: drop the least recently used instance
        check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        auto old = plans_.find(lru_.front());
        if (old != plans_.end()) {
            if (current_ == old->second.get()) current_ = nullptr;
            FreeInstance(*old->second);
            plans_.erase(old);
        }
        lru_.erase(lru_.begin());
    }

    auto pi = std::make_unique<PlanInstance>();
    try {
        BuildInstance(*pi, shapes);
        check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        if (autotune_) Autotune(*pi, pi->plan.steps.size(), allow_tune || tune_on_demand_);
        else PairTransitions(nullptr, *pi);              // (only an explicit IE_POOL_CONV pairs without a search)
        // fp8 mode bakes the activation scales into the launches: nothing is captured before they exist (a replica that owns a
        // never-uploaded blob is built before the weight broadcast); RefreshGraphs captures on first use
        if (use_graph_ && !(precision_ == Precision::F8 && !w_->f8_ready)) {
            pi->captured_gen = w_->f8_gen.load();
            Capture(*pi, 0, pi->plan.steps.size(), &pi->graph_exec);
            pi->graph_ready = true;
        }
        if (allow_tune) EnsurePipeline(*pi, true);
    } catch (...) {
        FreeInstance(*pi);
        throw;
    }
    current_ = pi.get();
    plans_[key] = std::move(pi);
    touch(key);
    return *current_;
}

// Rebuilds what is derived from the fp32 weight blob: the half mirror (fp16 mode) or the fragment-major conv weights (fp32 mode).
void DeviceModel::WeightsArrived(const std::vector<float>* adopt_act_scales) {
    check(hipSetDevice(device_), "hipSetDevice");
    w_->uploaded = true;
    if (w_->d_weights_x6)
        for (const auto& xr : w_->x6_regions)
            check(LaunchSplitWeightsX6(w_->d_weights + xr.w_off, static_cast<char*>(w_->d_weights_x6) + xr.byte_off, xr.cout, xr.k, stream_), "split_weights_x6");
    if (w_->d_weights_wino) {
        check(hipSetDevice(device_), "hipSetDevice");
        for (const auto& wr : w_->wino_regions) {
            check(LaunchWinogradWeights(w_->d_weights + wr.w_off, w_->d_weights_wino + wr.u_off, wr.cout, wr.cin, stream_), "winograd_weights");
            if (w_->d_weights_wino_x6)
                check(LaunchWinogradWeightsX6(w_->d_weights + wr.w_off, static_cast<char*>(w_->d_weights_wino_x6) + wr.u_off * 6, wr.cout, wr.cin, stream_), "winograd_weights_x6");
        }
        check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    }
    if (!w_->d_weights16 && !w_->d_weights_frag) return;      // (the fp16 fragment-major mirror only exists beside the half mirror)
    check(hipSetDevice(device_), "hipSetDevice");
    w_->f8_ready = false;
    if (w_->d_weights16) check(LaunchConvertF32ToF16(w_->d_weights, w_->d_weights16, int64_t(w_->weight_floats), stream_), "convert_f32_f16");
    if (w_->d_weights16_frag)
        for (const auto& fr : w_->frag16_regions)
            check(LaunchPermuteWeightsFrag16(static_cast<const char*>(w_->d_weights16) + fr.w_off * 2, static_cast<char*>(w_->d_weights16_frag) + fr.w_off * 2, fr.rows, fr.k,
                                             stream_), "permute_weights_frag16");
    if (w_->d_weights_frag)
        for (const DeviceWeights::FragRegion& fr : w_->frag_regions)
            check(LaunchPermuteWeightsFrag(w_->d_weights + fr.w_off, w_->d_weights_frag + fr.w_off, fr.cout, fr.kk, fr.cin, stream_), "permute_weights_frag");
    check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    if (precision_ == Precision::F8) PrepareF8(adopt_act_scales);
}

std::vector<std::pair<std::string, uint64_t>> DeviceModel::MirrorChecksums() {
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    const DeviceWeights& W = *w_;
    std::vector<std::pair<std::string, uint64_t>> out;
    std::vector<char> host;
    auto fnv = [](uint64_t h, const char* p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= uint8_t(p[i]); h *= 0x100000001B3ull; } return h; };
    auto pull = [&](const void* dev, size_t bytes) {
        host.resize(bytes);
        if (bytes) CopySync(host.data(), dev, bytes, hipMemcpyDeviceToHost, "hipMemcpy(mirror)");
    };
    constexpr uint64_t kBasis = 0xCBF29CE484222325ull;
    if (W.d_weights16) { pull(W.d_weights16, W.weight_floats * 2); out.push_back({"half", fnv(kBasis, host.data(), host.size())}); }
    if (W.d_weights16_frag) {
        uint64_t h = kBasis;
        for (const auto& fr : W.frag16_regions) { pull(static_cast<const char*>(W.d_weights16_frag) + fr.w_off * 2, size_t(fr.rows) * size_t(fr.k) * 2); h = fnv(h, host.data(), host.size()); }
        out.push_back({"half_fragment_major", h});
    }
    if (W.d_weights_frag) {        // only the conv regions of the fragment-major blob are ever written
        uint64_t h = kBasis;
        for (const auto& fr : W.frag_regions) {
            pull(W.d_weights_frag + fr.w_off, size_t(fr.cout) * size_t(fr.kk) * size_t(fr.cin) * sizeof(float));
            h = fnv(h, host.data(), host.size());
        }
        out.push_back({"fragment_major", h});
    }
    if (W.d_weights_wino) { pull(W.d_weights_wino, W.wino_floats * sizeof(float)); out.push_back({"winograd_u", fnv(kBasis, host.data(), host.size())}); }
    if (W.d_weights_x6) { pull(W.d_weights_x6, W.x6_bytes); out.push_back({"bf16x6", fnv(kBasis, host.data(), host.size())}); }
    if (W.d_weights8) {
        uint64_t h = kBasis;
        for (const auto& fc : W.f8_convs) { pull(static_cast<const char*>(W.d_weights8) + fc.w_off, size_t(fc.cout) * size_t(fc.k)); h = fnv(h, host.data(), host.size()); }
        out.push_back({"e4m3", h});
        pull(W.d_f8_aux, W.f8_aux_floats * sizeof(float));
        out.push_back({"e4m3_scales", fnv(kBasis, host.data(), host.size())});
        out.push_back({"act_scales", fnv(kBasis, reinterpret_cast<const char*>(W.act_scale.data()), W.act_scale.size() * sizeof(float))});
    }
    return out;
}

namespace {

// The counter-based generator of modelgen/rng.py, so the calibration images have the distribution of
// modelgen.models.synthetic_input: 0.6 x a coarse per-image grid of random levels (nearest-upsampled) + 0.4 x U[0,1) noise.
uint64_t rng_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
uint64_t rng_key(uint64_t seed, const std::string& stream) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (unsigned char b : stream) { h ^= b; h *= 0x100000001B3ull; }
    return rng_mix(seed * 0x9E3779B97F4A7C15ull + h);
}
float rng_uniform(uint64_t key, uint64_t i) {
    return float(double(rng_mix(key + (i + 1) * 0x9E3779B97F4A7C15ull) >> 40) * (1.0 / 16777216.0));
}
std::vector<float> synthetic_images(int64_t b, int64_t c, int64_t h, int64_t w, const std::string& stream) {
    std::vector<float> x(size_t(b * c * h * w));
    const uint64_t kf = rng_key(20250704, stream), kc = rng_key(20250704, stream + "/coarse");
    if (h < 8 || w < 8) {
        for (size_t i = 0; i < x.size(); ++i) x[i] = rng_uniform(kf, i);
        return x;
    }
    const int64_t cell = std::max<int64_t>(h / 7, 1), gh = (h + cell - 1) / cell, gw = (w + cell - 1) / cell;
    for (int64_t n = 0; n < b; ++n)
        for (int64_t ch = 0; ch < c; ++ch)
            for (int64_t y = 0; y < h; ++y)
                for (int64_t xx = 0; xx < w; ++xx) {
                    const uint64_t i = uint64_t(((n * c + ch) * h + y) * w + xx);
                    const uint64_t j = uint64_t(((n * c + ch) * gh + y / cell) * gw + xx / cell);
                    x[i] = 0.6f * rng_uniform(kc, j) + 0.4f * rng_uniform(kf, i);
                }
    return x;
}

}  // namespace

// fp8 mode, once per DeviceWeights (and again after the blob was rewritten):
//   1. every fp8 conv's weight rows -> e4m3 with a per-row scale (max |w| / 448);
//   2. calibration: the SAME graph planned in fp16 mode runs eagerly on IE_F8_CALIB_BATCH (default 8) synthetic images and the
//      max |x| of every step's output is taken; a tensor's scale is margin x max / 448 (margin 2: inputs of another
//      draw saturate only beyond twice the calibrated range; e4m3 precision is relative, the headroom costs no mantissa bits);
//      max pools keep their input's scale (their output IS one of their inputs);
//   3. epilogue multipliers escale[o] = (input tensor scale) x (weight row scale).
void DeviceModel::PrepareF8(const std::vector<float>* adopt) {
    DeviceWeights& W = *w_;
    if (W.f8_ready || !W.uploaded) return;
    if (adopt && adopt->size() != W.act_scale.size()) adopt = nullptr;
    check(hipSetDevice(device_), "hipSetDevice");
    for (const auto& fc : W.f8_convs)
        check(LaunchQuantizeRowsE4m3(W.d_weights + fc.w_off, static_cast<char*>(W.d_weights8) + fc.w_off, W.d_f8_aux + fc.aux_off, fc.cout, fc.k, stream_),
              "quantize_rows_e4m3");
    // ---- calibration pass in fp16 (skipped when the scales of the weight owner that already calibrated are adopted) ----
    if (adopt) W.act_scale = *adopt;
    else {
    int64_t nc = 8;
    if (const char* e = env_.get("IE_F8_CALIB_BATCH")) nc = std::max(1, std::min(64, std::atoi(e)));
    float margin = 2.0f;
    if (const char* e = env_.get("IE_F8_MARGIN")) margin = std::max(1.0f, float(std::atof(e)));
    std::vector<std::vector<int64_t>> shapes;
    for (const auto& vi : model_->inputs) {
        std::vector<int64_t> sh = vi.dims;
        for (size_t k = 0; k < sh.size(); ++k) if (sh[k] <= 0) sh[k] = (k == 0 ? nc : 1);
        shapes.push_back(sh);
    }
    PlanInstance cal;
    cal.plan = BuildPlan(*model_, shapes, Precision::F16, true);       // the fp8 plan's step fusions, so the step lists line up
    if (cal.plan.steps.size() != W.act_scale.size()) throw std::runtime_error("fp8 calibration: the fp16 plan of the graph has a different step list");
    std::vector<float>().swap(cal.plan.weights);
    float* d_amax = nullptr;
    try {
        AllocInstance(cal);
        check(hipMalloc(reinterpret_cast<void**>(&d_amax), cal.plan.steps.size() * sizeof(float)), "hipMalloc(amax)");
        check(hipMemsetAsync(d_amax, 0, cal.plan.steps.size() * sizeof(float), stream_), "hipMemset(amax)");
        for (size_t i = 0; i < cal.plan.inputs.size(); ++i) {
            const View& v = cal.plan.inputs[i].view;
            const std::vector<float> x = synthetic_images(v.n, v.c, v.h, v.w, "calibration/" + cal.plan.inputs[i].name);
            check(hipMemcpyAsync(cal.buffers[size_t(v.buf)], x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice, stream_), "hipMemcpy(calibration input)");
            check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        }
        for (size_t i = 0; i < cal.plan.steps.size(); ++i) {
            LaunchStep(cal, cal.plan.steps[i], stream_);
            check(LaunchAbsMax(make_arg(cal, cal.plan.steps[i].out), d_amax + i, stream_), "absmax");
        }
        std::vector<float> amax(cal.plan.steps.size());
        check(hipMemcpyAsync(amax.data(), d_amax, amax.size() * sizeof(float), hipMemcpyDeviceToHost, stream_), "hipMemcpy(amax)");
        check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        for (size_t i = 0; i < amax.size(); ++i) {
            const Step& st = cal.plan.steps[i];
            float sc = (amax[i] > 0.f ? amax[i] : 1.f) * margin / 448.0f;
            if (st.kind == StepKind::Pool && st.pool_max && st.in_src >= 0 && W.act_scale[size_t(st.in_src)] > 0.f) sc = W.act_scale[size_t(st.in_src)];
            W.act_scale[i] = sc;
        }
    } catch (...) {
        if (d_amax) (void)hipFree(d_amax);
        FreeInstance(cal);
        throw;
    }
    (void)hipFree(d_amax);
    FreeInstance(cal);
    }
    for (const auto& fc : W.f8_convs) {
        if (fc.in_src < 0) throw std::runtime_error("fp8 precision: a conv reads a tensor whose producer is unknown");
        const int64_t half = (fc.cout + 3) / 4 * 4;
        check(LaunchScaleVector(W.d_f8_aux + fc.aux_off, W.d_f8_aux + fc.aux_off + half, W.act_scale[size_t(fc.in_src)], fc.cout, stream_), "scale_vector");
    }
    check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    W.f8_gen.fetch_add(1);
    W.f8_ready = true;
}

// ---- pipelined host path --------------------------------------------------------------------------------------------------
// Cut the batch of `pi` into image ranges and decide how many leading steps run per range (PlanInstance::chunks / head_steps).
// The range plans come from the planner for the range's batch size (so they carry their own kernel choices); they are accepted
// only when they are the parent's plan with a smaller n: same steps, same views, same weight offsets.
void DeviceModel::EnsurePipeline(PlanInstance& pi, bool allow_tune) {
    if (pi.pipeline_tried) return;
    pi.pipeline_tried = true;
    if (pi.kv) return;       // a bound instance: the cache's length arrays are indexed by the image of the whole batch
    if (pipeline_chunks_ < 2 || pi.plan.inputs.empty() || pi.plan.steps.size() < 4) return;
    const int64_t B = pi.plan.inputs[0].dims.empty() ? 0 : pi.plan.inputs[0].dims[0];
    for (auto& d : pi.plan.inputs) if (d.dims.empty() || d.dims[0] != B || d.view.n != B) return;
    for (auto& d : pi.plan.outputs) if (d.dims.empty() || d.dims[0] != B) return;
    int C = pipeline_chunks_;
    while (C > 1 && (B % C != 0 || B / C < 4)) C /= 2;
    if (C < 2) return;
    const int64_t Bc = B / C;
    std::vector<std::vector<int64_t>> sub_shapes;
    for (auto& d : pi.plan.inputs) { sub_shapes.push_back(d.dims); sub_shapes.back()[0] = Bc; }
    Plan sub;
    try {
        sub = BuildPlan(*model_, sub_shapes, precision_);
    } catch (const std::exception&) {
        return;          // e.g. the model fixes its batch dimension
    }
    const Plan& full = pi.plan;
    if (sub.steps.size() != full.steps.size() || sub.weights.size() != w_->weight_floats || 2 * sub.workspace_floats > pi.workspace_floats) return;
    auto same_view = [&](const View& a, const View& b) {
        return a.buf == b.buf && a.c == b.c && a.h == b.h && a.w == b.w && a.c_off == b.c_off && a.pitch == b.pitch && a.nchw == b.nchw && a.f16 == b.f16 &&
               a.n * C == b.n;
    };
    auto image_stride = [](const View& v) { return v.nchw ? v.c * v.h * v.w : v.h * v.w * v.pitch; };
    // ---- how many steps per range: enough modelled compute to cover the upload of the remaining ranges ----
    size_t head = 0;
    {
        double in_bytes = 0;
        for (auto& d : full.inputs) in_bytes += double(d.view.numel()) * double(d.view.esize());
        const double t_h2d = in_bytes * double(C - 1) / double(C) / 40e9;                // pageable H2D: ~40 GB/s measured
        const double peak = precision_ == Precision::F32 ? 0.45 * 157.3e12 : 0.3 * 2.5e15;
        double total = 0;
        std::vector<double> est(full.steps.size());
        for (size_t i = 0; i < full.steps.size(); ++i) { est[i] = std::max(full.steps[i].flops / peak, full.steps[i].bytes / 2.5e12) + 4e-6; total += est[i]; }
        const double want = std::min(t_h2d, 0.6 * total);
        double acc = 0;
        while (head < full.steps.size() - 1 && acc < want) acc += est[head++];
        if (pipeline_head_ >= 0) head = std::min<size_t>(size_t(pipeline_head_), full.steps.size() - 1);
    }
    // ---- validity: range plan == parent plan with n / C, and no buffer that is read by the tail holds tensors of two different
    //      image strides during the head (a later range would overwrite an earlier range's live rows) ----
    auto valid = [&](size_t h) {
        for (size_t i = 0; i < h; ++i) {
            const Step &a = sub.steps[i], &b = full.steps[i];
            if (b.kind == StepKind::KvAppend || b.past_len > 0) return false;      // (cache views are not compared below: such a step stays in the tail)
            if (a.kind != b.kind ||!same_view(a.in, b.in) || !same_view(a.out, b.out) || a.has_in2 != b.has_in2 || (a.has_in2 && !same_view(a.in2, b.in2)) ||
                a.w_off != b.w_off || a.bias_off != b.bias_off || a.pre_scale_off != b.pre_scale_off || a.pre_shift_off != b.pre_shift_off ||
                a.parts.size() != b.parts.size())
                return false;
            for (size_t q = 0; q < a.parts.size(); ++q)
                if (!same_view(a.parts[q].in, b.parts[q].in) || !same_view(a.parts[q].out, b.parts[q].out) || a.parts[q].w_off != b.parts[q].w_off) return false;
        }
        // Tensors that cross from the head into the tail: a tail step reads a view that no earlier TAIL step has written.  Range c+1
        // runs its head after range c finished its own, so inside the head a range may overwrite rows of earlier ranges only in
        // buffers whose content is dead at the boundary.  Rows of different ranges are disjoint when every tensor the head puts into
        // a buffer has the same image stride; so: every buffer holding a crossing tensor must see ONE image stride during the head.
        std::map<int, int64_t> head_stride;       // buffer -> image stride of the head's tensors in it (-1 = mixed)
        auto note = [&](const View& v) {
            auto f = head_stride.find(v.buf);
            if (f == head_stride.end()) head_stride[v.buf] = image_stride(v);
            else if (f->second != image_stride(v)) f->second = -1;
        };
        for (size_t i = 0; i < h; ++i) {
            note(full.steps[i].in); note(full.steps[i].out);
            if (full.steps[i].has_in2) note(full.steps[i].in2);
            for (const Step& q : full.steps[i].parts) { note(q.in); note(q.out); }
        }
        std::vector<const View*> tail_written;
        auto covered = [&](const View& v) {      // the union of the tail's earlier writes (concat slices) spans the view's channels
            int64_t pos = v.c_off;
            const int64_t end = v.c_off + v.c;
            bool progress = true;
            while (pos < end && progress) {
                progress = false;
                for (const View* w : tail_written)
                    if (w->buf == v.buf && w->nchw == v.nchw && image_stride(*w) == image_stride(v) && w->c_off <= pos && w->c_off + w->c > pos) {
                        pos = w->c_off + w->c;
                        progress = true;
                    }
            }
            return pos >= end;
        };
        for (size_t i = h; i < full.steps.size(); ++i) {
            for (const View* v : {&full.steps[i].in, full.steps[i].has_in2 ? &full.steps[i].in2 : nullptr}) {
                if (!v || covered(*v)) continue;
                auto f = head_stride.find(v->buf);
                if (f != head_stride.end() && (f->second == -1 || f->second != image_stride(*v))) return false;
            }
            for (const Step& q : full.steps[i].parts) {      // a fused step also reads its 3x3's input and writes its 3x3's slice
                if (!covered(q.in)) {
                    auto f = head_stride.find(q.in.buf);
                    if (f != head_stride.end() && (f->second == -1 || f->second != image_stride(q.in))) return false;
                }
                tail_written.push_back(&q.out);
            }
            tail_written.push_back(&full.steps[i].out);
        }
        return true;
    };
    while (head > 0 && !valid(head)) --head;
    if (head == 0) return;
    std::vector<float>().swap(sub.weights);
    for (int c = 0; c < C; ++c) {
        auto ch = std::make_unique<PlanInstance>();
        ch->plan = sub;
        ch->buffers = pi.buffers;
        ch->owned.assign(pi.buffers.size(), 0);
        ch->workspace = pi.workspace;
        ch->workspace_floats = pi.workspace_floats;
        ch->counters = pi.counters;
        ch->batch_off = int64_t(c) * Bc;
        pi.chunks.push_back(std::move(ch));
    }
    try {
        if (autotune_) {
            Autotune(*pi.chunks[0], head, allow_tune || tune_on_demand_);
            for (int c = 1; c < C; ++c)
                for (size_t i = 0; i < head; ++i) {
                    Step& d = pi.chunks[size_t(c)]->plan.steps[i];
                    const Step& s0 = pi.chunks[0]->plan.steps[i];
                    d.algo = s0.algo; d.tile = s0.tile; d.splitk = s0.splitk;
                }
        }
        if (use_graph_ && !(precision_ == Precision::F8 && !w_->f8_ready) && pi.graph_ready) {
            for (auto& ch : pi.chunks) { Capture(*ch, 0, head, &ch->graph_exec); ch->graph_ready = true; }
            Capture(pi, head, pi.plan.steps.size(), &pi.tail_exec);
        }
    } catch (...) {
        for (auto& ch : pi.chunks) FreeInstance(*ch);
        pi.chunks.clear();
        if (pi.tail_exec) { (void)hipGraphExecDestroy(pi.tail_exec); pi.tail_exec = nullptr; }
        throw;
    }
    pi.head_steps = int(head);
}

void DeviceModel::RunSteps(PlanInstance& pi, size_t first, size_t last, std::vector<hipEvent_t>* events) {
    size_t k = 0;
    if (events) check(hipEventRecord((*events)[k++], stream_), "hipEventRecord");
    ConvArgs pa;
    PooledArgs pp;
    LaunchRole role;
    for (size_t i = first; i < last && i < pi.plan.steps.size(); ++i) {
        // a paired launch covers its steps at once (one event behind it); when its launcher declines, or the range cuts it, the steps launch alone
        if (const int n = PairedCount(pi, i, std::min(last, pi.plan.steps.size()), &pa, &pp, &role); n > 1) {
            check(LaunchConvPooled(pa, pp, role.tile, role.chain, stream_), "conv1x1_pooled");
            i += size_t(n - 1);
        } else {
            LaunchStep(pi, pi.plan.steps[i], stream_);
        }
        if (events) check(hipEventRecord((*events)[k++], stream_), "hipEventRecord");
    }
}

// Graphs hold the fp8 activation scales as by-value kernel arguments: an instance captured before the scales existed (deferred) or
// under scales that have since been recalibrated (EngineWeightsUpdated, the weight broadcast) is captured again here, on the lane
// that owns it, before its next launch.
void DeviceModel::RefreshGraphs(PlanInstance& pi) {
    if (!use_graph_) return;
    if (precision_ == Precision::F8 && !w_->f8_ready) throw std::runtime_error("fp8 precision: scales are not calibrated yet");
    const uint64_t gen = w_->f8_gen.load();
    if (pi.graph_ready && pi.captured_gen == gen) return;
    check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    auto drop = [](hipGraphExec_t& g) { if (g) (void)hipGraphExecDestroy(g); g = nullptr; };
    drop(pi.graph_exec);
    pi.graph_ready = false;
    Capture(pi, 0, pi.plan.steps.size(), &pi.graph_exec);
    pi.graph_ready = true;
    if (!pi.chunks.empty() && pi.head_steps > 0) {
        for (auto& ch : pi.chunks) {
            drop(ch->graph_exec);
            ch->graph_ready = false;
            Capture(*ch, 0, size_t(pi.head_steps), &ch->graph_exec);
            ch->graph_ready = true;
        }
        drop(pi.tail_exec);
        Capture(pi, size_t(pi.head_steps), pi.plan.steps.size(), &pi.tail_exec);
    }
    pi.captured_gen = gen;
}

void DeviceModel::Enqueue(PlanInstance& pi) {
    check(hipSetDevice(device_), "hipSetDevice");
    RefreshGraphs(pi);
    if (pi.graph_ready) check(hipGraphLaunch(pi.graph_exec, stream_), "hipGraphLaunch");
    else RunSteps(pi, 0, pi.plan.steps.size(), nullptr);
}

void DeviceModel::Synchronize() {
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
}

std::vector<StepTiming> DeviceModel::Profile(PlanInstance& pi, int iters) {
    check(hipSetDevice(device_), "hipSetDevice");
    const size_t ns = pi.plan.steps.size();
    std::vector<hipEvent_t> ev(ns + 1);
    for (auto& e : ev) check(hipEventCreate(&e), "hipEventCreate");
    std::vector<StepTiming> out(ns);
    // one entry per plan step; a launch that covers k steps is one timed group: its k entries carry the launched kernel's label and share its time
    // in proportion to each step's own lower bound max(bytes / 8 TB/s, flops / 157.3 TFLOP/s)
    std::vector<std::pair<size_t, int>> groups;
    for (size_t i = 0; i < ns;) {
        ConvArgs pa;
        PooledArgs pp;
        LaunchRole role;
        const int n = PairedCount(pi, i, ns, &pa, &pp, &role);
        groups.emplace_back(i, n);
        for (size_t j = i; j < i + size_t(n); ++j) {
            out[j].name = pi.plan.steps[j].name;
            Step handed;
            out[j].kernel = n > 1 ? "conv1x1_pooled_kernel<f32,t" + std::to_string(role.tile) + (role.chain ? ",chain>" : ">")
                                  : kernel_label(LaunchedStep(pi, pi.plan.steps[j], handed));
            out[j].flops = pi.plan.steps[j].flops;
            out[j].bytes = pi.plan.steps[j].bytes;
        }
        i += size_t(n);
    }
    try {
        RunSteps(pi, 0, ns, nullptr);   // warm
        check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        // per step the MEDIAN over the passes: one disturbed pass (clock ramp, a neighbour's burst) must not colour a family's figure
        const size_t ng = groups.size();
        std::vector<std::vector<float>> samples(ng);
        for (int it = 0; it < iters; ++it) {
            RunSteps(pi, 0, ns, &ev);
            check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
            for (size_t i = 0; i < ng; ++i) {
                float ms = 0;
                check(hipEventElapsedTime(&ms, ev[i], ev[i + 1]), "hipEventElapsedTime");
                samples[i].push_back(ms);
            }
        }
        for (size_t g = 0; g < ng; ++g) {
            std::sort(samples[g].begin(), samples[g].end());
            const size_t n = samples[g].size();
            const double ms = n == 0 ? 0.0 : (n % 2 ? samples[g][n / 2] : 0.5 * (samples[g][n / 2 - 1] + samples[g][n / 2]));
            auto bound = [&](size_t j) { return std::max({out[j].bytes / 8e12, out[j].flops / 157.3e12, 1e-12}); };
            double sum = 0;
            for (size_t j = groups[g].first; j < groups[g].first + size_t(groups[g].second); ++j) sum += bound(j);
            for (size_t j = groups[g].first; j < groups[g].first + size_t(groups[g].second); ++j) out[j].ms = ms * bound(j) / sum;
        }
    } catch (...) {
        for (auto& e : ev) (void)hipEventDestroy(e);
        throw;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return out;
}

void DeviceModel::InferHost(PlanInstance& pi, const std::vector<const void*>& inputs, const std::vector<size_t>& in_bytes,
                            const std::vector<void*>& outputs, const std::vector<size_t>& out_bytes, const std::vector<char>& in_u8) {
    std::vector<std::vector<InSeg>> in(pi.plan.inputs.size());
    for (size_t i = 0; i < pi.plan.inputs.size(); ++i) {
        const bool u8 = i < in_u8.size() && in_u8[i];
        const size_t need = size_t(pi.plan.inputs[i].view.numel()) * (u8 ? 1 : size_t(pi.plan.inputs[i].view.esize()));
        in[i].push_back({inputs[i], inputs[i] ? std::min(in_bytes[i], need) : 0, need, 0, u8});
    }
    std::vector<std::vector<OutSeg>> out(pi.plan.outputs.size());
    for (size_t i = 0; i < outputs.size() && i < pi.plan.outputs.size(); ++i) {
        if (!outputs[i] || out_bytes[i] == 0) continue;
        out[i].push_back({outputs[i], out_bytes[i], size_t(pi.plan.outputs[i].view.numel()) * sizeof(float), 0});
    }
    InferHostSegments(pi, in, out);
}

// The ModelInfer data path: caller memory -> HBM, forward, HBM -> caller memory.  This replaces the five host copies each way of
// the reference (inference_bridge.cpp:738-749, 806-812 and model.cpp:1229-1238, 1290-1311) with ONE DMA per direction straight
// from / to the caller's buffers (hipMemcpyAsync takes pageable memory at ~40-55 GB/s on this platform, measured by
// scripts/probes/h2d_probe.cpp; a caller that hands over pinned memory gets a fully asynchronous copy), and overlaps the upload
// with compute: the batch is cut into image ranges, range c's upload is followed by the head steps of range c on the compute
// stream while range c+1 uploads on the copy stream; the remaining steps run once on the whole batch.
void DeviceModel::InferHostSegments(PlanInstance& pi, const std::vector<std::vector<InSeg>>& in, const std::vector<std::vector<OutSeg>>& out) {
    check(hipSetDevice(device_), "hipSetDevice");
    EnsurePipeline(pi, false);
    RefreshGraphs(pi);
    const int C = pi.chunks.empty() ? 1 : int(pi.chunks.size());
    struct Job { int chunk; char* dst; const char* src; size_t copy, zero; };      // copy `copy` bytes src -> dst, then zero `zero` bytes behind them
    std::vector<Job> jobs;
    struct U8 { size_t input; };
    std::vector<char> is_u8(pi.plan.inputs.size(), 0);
    try {
        for (size_t i = 0; i < pi.plan.inputs.size() && i < in.size(); ++i) {
            const View& v = pi.plan.inputs[i].view;
            char* base = reinterpret_cast<char*>(pi.buffers[size_t(v.buf)]);
            const bool u8 = !in[i].empty() && in[i][0].u8;
            is_u8[i] = u8 ? 1 : 0;
            if (u8) {       // bytes go to a device staging buffer; a kernel per range converts them into the fp32 input buffer
                if (pi.u8_stage.size() < pi.plan.inputs.size()) pi.u8_stage.resize(pi.plan.inputs.size(), nullptr);
                if (!pi.u8_stage[i]) {
                    check(hipMalloc(&pi.u8_stage[i], std::max<size_t>(size_t(v.numel()), 16)), "hipMalloc(u8 staging)");
                    device_bytes_ += size_t(v.numel());
                }
                base = static_cast<char*>(pi.u8_stage[i]);
            }
            if (u8 && v.i64) throw std::runtime_error("internal error: UINT8 payload for an INT64 input");
            const size_t total = size_t(v.numel()) * (u8 ? 1 : size_t(v.esize()));      // (fp32 or int64: the input buffer's own element size)
            const size_t per_chunk = total / size_t(C);          // C divides the batch, so ranges are whole images
            for (const InSeg& sg : in[i]) {
                if (sg.u8 != u8) throw std::runtime_error("internal error: mixed UINT8 / FLOAT32 segments for one input");
                if (sg.dev_off + sg.need > total) throw std::runtime_error("internal error: input segment exceeds the planned tensor");
                const size_t have = sg.host ? std::min(sg.have, sg.need) : 0;
                size_t off = 0;
                while (off < sg.need) {                          // split at range boundaries
                    const size_t dev = sg.dev_off + off;
                    const int c = int(std::min<size_t>(dev / per_chunk, size_t(C - 1)));
                    const size_t end = std::min(sg.need, (size_t(c) + 1) * per_chunk - sg.dev_off);
                    const size_t nb = end - off;
                    const size_t cp = off < have ? std::min(nb, have - off) : 0;
                    jobs.push_back({c, base + dev, cp ? static_cast<const char*>(sg.host) + off : nullptr, cp, nb - cp});
                    off = end;
                }
            }
        }
        // ---- upload + head, range by range ----
        for (int c = 0; c < C; ++c) {
            for (const Job& j : jobs) {
                if (j.chunk != c) continue;
                if (j.copy) check(hipMemcpyAsync(j.dst, j.src, j.copy, hipMemcpyHostToDevice, copy_stream_), "hipMemcpyAsync(H2D)");
                if (j.zero) check(hipMemsetAsync(j.dst + j.copy, 0, j.zero, copy_stream_), "hipMemsetAsync");
            }
            for (size_t i = 0; i < pi.plan.inputs.size(); ++i) {
                if (!is_u8[i]) continue;
                const View& v = pi.plan.inputs[i].view;
                const int64_t n = v.numel() / C;
                check(LaunchConvertU8ToF32(static_cast<char*>(pi.u8_stage[i]) + int64_t(c) * n, pi.buffers[size_t(v.buf)] + int64_t(c) * n, n, u8_scale_, u8_bias_,
                                           copy_stream_), "convert_u8_f32");
            }
            check(hipEventRecord(h2d_events_[size_t(c)], copy_stream_), "hipEventRecord");
            check(hipStreamWaitEvent(stream_, h2d_events_[size_t(c)], 0), "hipStreamWaitEvent");
            if (c == 0) check(hipEventRecord(t0_event_, stream_), "hipEventRecord");
            if (C > 1) {
                PlanInstance& ch = *pi.chunks[size_t(c)];
                if (ch.graph_ready) check(hipGraphLaunch(ch.graph_exec, stream_), "hipGraphLaunch(head)");
                else RunSteps(ch, 0, size_t(pi.head_steps), nullptr);
            }
        }
        if (C > 1) {
            if (pi.tail_exec) check(hipGraphLaunch(pi.tail_exec, stream_), "hipGraphLaunch(tail)");
            else RunSteps(pi, size_t(pi.head_steps), pi.plan.steps.size(), nullptr);
            ++pipelined_calls_;
        } else {
            Enqueue(pi);
        }
        check(hipEventRecord(t1_event_, stream_), "hipEventRecord");
        last_chunks_ = C;
        last_head_steps_ = C > 1 ? pi.head_steps : 0;
        // ---- D2H: results are small (logits): one transfer per output into pinned staging, ONE synchronisation, then the
        //      per-caller scatter on the host; an output too large for the staging goes straight to the caller's memory ----
        struct Scatter { size_t j, lo, stage_off; };
        std::vector<Scatter> staged;
        size_t stage_used = 0;
        for (size_t j = 0; j < pi.plan.outputs.size() && j < out.size(); ++j) {
            if (out[j].empty()) continue;
            const View& v = pi.plan.outputs[j].view;
            const char* src = reinterpret_cast<const char*>(pi.buffers[size_t(v.buf)]);
            const size_t total = size_t(v.numel()) * sizeof(float);
            size_t lo = SIZE_MAX, hi = 0;
            for (const OutSeg& sg : out[j]) {
                const size_t nb = std::min(sg.cap, sg.need);
                if (!nb) continue;
                if (sg.dev_off + nb > total) throw std::runtime_error("internal error: output segment exceeds the planned tensor");
                lo = std::min(lo, sg.dev_off);
                hi = std::max(hi, sg.dev_off + nb);
            }
            if (hi <= lo) continue;
            if (stage_used + (hi - lo) <= pinned_bytes_) {
                check(hipMemcpyAsync(static_cast<char*>(pinned_) + stage_used, src + lo, hi - lo, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
                staged.push_back({j, lo, stage_used});
                stage_used += (hi - lo + 63) & ~size_t(63);
            } else {
                for (const OutSeg& sg : out[j]) {
                    const size_t nb = std::min(sg.cap, sg.need);
                    if (nb) check(hipMemcpyAsync(sg.host, src + sg.dev_off, nb, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
                }
            }
        }
        check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
        {
            float ms = 0;
            last_forward_ms_ = hipEventElapsedTime(&ms, t0_event_, t1_event_) == hipSuccess ? double(ms) : 0.0;
        }
        for (const Scatter& sc : staged)
            for (const OutSeg& sg : out[sc.j]) {
                const size_t nb = std::min(sg.cap, sg.need);
                if (nb) std::memcpy(sg.host, static_cast<char*>(pinned_) + sc.stage_off + (sg.dev_off - sc.lo), nb);
            }
        for (size_t j = 0; j < out.size(); ++j)
            for (const OutSeg& sg : out[j]) {
                const size_t nb = std::min(sg.cap, sg.need);
                if (sg.cap > nb) std::memset(static_cast<char*>(sg.host) + nb, 0, sg.cap - nb);
            }
    } catch (...) {
        (void)hipStreamSynchronize(copy_stream_);
        (void)hipStreamSynchronize(stream_);
        throw;
    }
}

}  // namespace ie
