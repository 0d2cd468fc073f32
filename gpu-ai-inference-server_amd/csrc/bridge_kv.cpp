// The resident KV cache behind the C ABI (include/inference_engine_ext.h EngineKvCache*): the object and its calls, the binding of a loaded
// model, and ModelInfer's path on a bound model.  The cache lives in HBM and is appended in place by the in-place kernels (kernels_decode.hip); the
// per-image valid lengths live here, on the host, and reach the kernels through a small device array uploaded in front of every forward, so the
// captured hipGraph of a bound plan instance replays unchanged from call to call.
#include "bridge_internal.h"

namespace ie_bridge {
namespace {

void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) { (void)hipGetLastError(); throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e)); }
}

size_t tensor_floats(const ie::KvBinding& g) { return size_t(g.batch) * size_t(g.kv_heads) * size_t(g.capacity) * size_t(g.head_dim); }

// the layer of `past_key_values.<i>.key|value` / `present.<i>.key|value` and whether it is the value (-1: not such a name)
int cache_layer(const std::string& name, size_t prefix, bool* value) {
    const size_t dot = name.find('.', prefix);
    if (dot == std::string::npos || dot == prefix || dot - prefix > 6) return -1;
    for (size_t k = prefix; k < dot; ++k) if (name[k] < '0' || name[k] > '9') return -1;
    const std::string tail = name.substr(dot + 1);
    if (tail != "key" && tail != "value") return -1;
    *value = tail == "value";
    return std::atoi(name.substr(prefix, dot - prefix).c_str());
}

// What a graph's cache tensors say: layers, and the dims every one of them shares.  "" or the reason the graph cannot bind
struct GraphCache { int layers = 0; int64_t batch = 0, kv_heads = 0, past = 0, present = 0, head_dim = 0; };
std::string graph_cache(const ie::ModelInfo& info, GraphCache* out) {
    GraphCache g;
    std::vector<int> seen_past, seen_present;      // per layer: bit 0 key, bit 1 value
    auto take = [&](const ie::OnnxValueInfo& vi, size_t prefix, std::vector<int>& seen, int64_t* rows) -> std::string {
        bool value = false;
        const int layer = cache_layer(vi.name, prefix, &value);
        if (layer < 0) return "the cache tensor " + vi.name + " is not named <prefix>.<layer>.key or .value";
        if (vi.dims.size() != 4) return "the cache tensor " + vi.name + " is not of rank 4";
        if (size_t(layer) >= seen.size()) seen.resize(size_t(layer) + 1, 0);
        seen[size_t(layer)] |= value ? 2 : 1;
        const int64_t d[4] = {vi.dims[0], vi.dims[1], vi.dims[2], vi.dims[3]};
        int64_t* mine[4] = {&g.batch, &g.kv_heads, rows, &g.head_dim};
        for (int k = 0; k < 4; ++k) {
            if (d[k] <= 0 && k > 0) return "the cache tensor " + vi.name + " has a symbolic dimension";
            if (*mine[k] == 0) *mine[k] = d[k];
            else if (*mine[k] != d[k] && !(k == 0 && d[k] <= 0)) return "the cache tensors of the graph differ in their dimensions (" + vi.name + ")";
        }
        return "";
    };
    for (const auto& vi : info.inputs)
        if (kv_past_name(vi.name)) if (const std::string e = take(vi, 16, seen_past, &g.past); !e.empty()) return e;
    for (const auto& vi : info.outputs)
        if (kv_present_name(vi.name)) if (const std::string e = take(vi, 8, seen_present, &g.present); !e.empty()) return e;
    if (seen_present.empty()) return seen_past.empty() ? "the model has no cache: neither past_key_values.* inputs nor present.* outputs" : "the model has past_key_values.* inputs but no present.* outputs";
    for (int s : seen_present) if (s != 3) return "a layer of the model lacks its present key or value output";
    if (!seen_past.empty()) {
        if (seen_past.size() != seen_present.size()) return "the model has past_key_values.* inputs for " + std::to_string(seen_past.size()) + " layers and present.* outputs for " + std::to_string(seen_present.size());
        for (int s : seen_past) if (s != 3) return "a layer of the model lacks its past key or value input";
        if (g.present <= g.past) return "the present.* outputs do not have more rows than the past_key_values.* inputs";
    }
    g.layers = int(seen_present.size());
    *out = g;
    return "";
}

// lane 0 of a loaded model, the model's lifetime held by the caller
struct LaneHold {
    ModelObj& M;
    explicit LaneHold(ModelObj& m) : M(m) { M.pool.AcquireOne(0); }
    ~LaneHold() { M.pool.Release(0, 1); }
};

void forget_locked(EngineKvCache& C, const ModelObj* m) {
    for (auto it = C.bound.begin(); it != C.bound.end();) {
        const auto sp = it->lock();
        if (!sp || sp.get() == m) it = C.bound.erase(it);
        else ++it;
    }
}

// M.life held exclusively: no request of M is in flight
void unbind(ModelObj& M) {
    EngineKvCache* C = M.kv;
    if (!C) return;
    { std::lock_guard<std::mutex> g(C->mu); forget_locked(*C, &M); }
    M.kv = nullptr;
    M.kv_lq = M.kv_past = 0;
    if (!M.lanes.empty()) M.lanes[0]->BindKvCache(nullptr);
}

void standing(EngineKvCache& C) {      // C.mu held: lengths as they stand, and as many new tokens as still fit (the kernels cut them at the step's own count)
    const int n = C.dev->batch;
    C.upload.assign(size_t(2 * n), 0);
    for (int i = 0; i < n; ++i) { C.upload[size_t(i)] = int(C.lens[size_t(i)]); C.upload[size_t(n + i)] = C.dev->capacity - int(C.lens[size_t(i)]); }
}

}  // namespace

void KvForget(ModelObj& M) {
    if (!M.kv) return;
    { std::lock_guard<std::mutex> g(M.kv->mu); forget_locked(*M.kv, &M); }
    M.kv = nullptr;
    M.kv_lq = M.kv_past = 0;
}

void UploadStandingLens(ModelObj& M, ie::DeviceModel& D) {
    EngineKvCache* C = M.kv;
    if (!C) return;
    std::lock_guard<std::mutex> g(C->mu);
    standing(*C);
    D.UploadKvLens(C->upload.data());
    D.Synchronize();
}

std::string KvCacheJson(ModelObj& M) {
    EngineKvCache* C = M.kv;
    if (!C) return "";
    std::lock_guard<std::mutex> g(C->mu);
    std::ostringstream o;
    const ie::KvBinding& d = *C->dev;
    o << "{\"device\":" << C->device_id << ",\"layers\":" << d.layers << ",\"batch\":" << d.batch << ",\"kv_heads\":" << d.kv_heads << ",\"capacity\":" << d.capacity
      << ",\"head_dim\":" << d.head_dim << ",\"bytes\":" << C->bytes << ",\"lengths\":[";
    for (size_t i = 0; i < C->lens.size(); ++i) o << (i ? "," : "") << C->lens[i];
    size_t models = 0;
    for (const auto& w : C->bound) if (!w.expired()) ++models;
    o << "],\"models_bound\":" << models << ",\"new_tokens_per_call\":" << M.kv_lq << "}";
    return o.str();
}

void RunBound(ModelObj& M, ModelObj::Pending& r) {
    std::shared_lock<std::shared_mutex> life(M.life);
    auto fail = [&](const std::string& msg) { r.ok = false; r.err = msg; };
    if (!M.loaded.load() || M.lanes.empty()) return fail("Model not loaded");
    EngineKvCache* C = M.kv;
    if (!C) return fail("The KV cache was unbound while the request was waiting");
    try {
        LaneHold lane(M);                                // (lock order everywhere: the model's life, its lane, the cache)
        std::lock_guard<std::mutex> cache(C->mu);
        const ie::KvBinding& g = *C->dev;
        const int N = g.batch, P = M.kv_past, Lq = M.kv_lq;
        const auto& gin = M.info.inputs;
        // the shapes of the whole graph: the cache inputs are the cache's own
        for (size_t k = 0; k < gin.size(); ++k) {
            if (kv_past_name(gin[k].name)) r.shapes[k] = {N, g.kv_heads, g.capacity, g.head_dim};
            else if (r.shapes[k].empty() || r.shapes[k][0] != N)
                return fail("Input " + gin[k].name + " of a model bound to a KV cache needs the cache's batch " + std::to_string(N) + " as its leading dimension");
        }
        // ---- the mask, before anything is enqueued: ones below the image's length only, then a prefix of ones over the new tokens that still fits ----
        std::vector<int> c(size_t(N), Lq);
        for (size_t k = 0; k < gin.size(); ++k) {
            if (gin[k].elem_type != ie::ONNX_INT64 || k >= M.id_rows.size() || M.id_rows[k] >= 0) continue;      // (id_rows -1: a key mask)
            const std::vector<int64_t>& sh = r.shapes[k];
            if (sh.size() != 2 || sh[1] != int64_t(P) + Lq) return fail("Input " + gin[k].name + " of a model bound to a KV cache must be [" + std::to_string(N) + ", " + std::to_string(P + Lq) + "]");
            const char* p = static_cast<const char*>(r.in_ptr[k]);
            auto at = [&](int n, int j) { int64_t v; std::memcpy(&v, p + (size_t(n) * size_t(P + Lq) + size_t(j)) * sizeof(int64_t), sizeof(v)); return v; };
            for (int n = 0; n < N; ++n) {
                const int64_t len = C->lens[size_t(n)];
                for (int j = int(len); j < P; ++j)
                    if (at(n, j) != 0)
                        return fail("Input " + gin[k].name + ": image " + std::to_string(n) + " has a one in cache column " + std::to_string(j) + ", at or beyond its cached length " + std::to_string(len) +
                                    " (a resident cache is right-padded)");
                int cn = 0;
                while (cn < Lq && at(n, P + cn) != 0) ++cn;
                for (int j = cn; j < Lq; ++j)
                    if (at(n, P + j) != 0)
                        return fail("Input " + gin[k].name + ": image " + std::to_string(n) + " has a one in new-token column " + std::to_string(P + j) + " behind a zero in column " + std::to_string(P + cn) +
                                    " (the ones of the new tokens must form a prefix)");
                c[size_t(n)] = cn;
            }
        }
        for (int n = 0; n < N; ++n) {
            const int64_t len = C->lens[size_t(n)];
            if (P == 0 && len != 0) return fail("A prefill graph bound to a KV cache needs an empty cache: image " + std::to_string(n) + " holds " + std::to_string(len) + " rows");
            if (len + c[size_t(n)] > g.capacity)
                return fail("The KV cache is full: image " + std::to_string(n) + " holds " + std::to_string(len) + " of " + std::to_string(g.capacity) + " rows and the request appends " +
                            std::to_string(c[size_t(n)]) + " (new-token columns " + std::to_string(P) + " .. " + std::to_string(P + c[size_t(n)] - 1) + ")");
        }
        // ---- outputs by index in graph order, as ModelInfer gives them; a `present` one cannot be had ----
        const auto& gout = M.info.outputs;
        for (int i = 0; i < r.num_outputs; ++i) {
            const std::string asked = r.outputs[i].name ? r.outputs[i].name : "";
            const std::string mine = size_t(i) < gout.size() ? gout[size_t(i)].name : "";
            const bool wanted = r.outputs[i].data && r.outputs[i].data_size > 0;
            if (kv_present_name(asked) || (wanted && kv_present_name(mine)))
                return fail("Output " + (kv_present_name(asked) ? asked : mine) + " is not available from a model bound to a KV cache: the rows are in the cache (EngineKvCacheRead)");
        }
        ie::DeviceModel& D = *M.lanes[0];
        ie::PlanInstance& pi = D.Prepare(r.shapes, false);
        std::vector<std::vector<ie::DeviceModel::InSeg>> in(pi.plan.inputs.size());
        for (size_t k = 0; k < pi.plan.inputs.size() && k < gin.size(); ++k) {
            if (kv_past_name(gin[k].name)) continue;       // nothing is uploaded: the steps read the cache
            const bool u8 = r.in_u8[k] != 0;
            const size_t need = size_t(pi.plan.inputs[k].view.numel()) * (u8 ? 1 : size_t(pi.plan.inputs[k].view.esize()));
            in[k].push_back({r.in_ptr[k], r.in_ptr[k] ? std::min(r.in_bytes[k], need) : 0, need, 0, u8});
        }
        std::vector<std::vector<ie::DeviceModel::OutSeg>> out(pi.plan.outputs.size());
        for (int i = 0; i < r.num_outputs && size_t(i) < pi.plan.outputs.size(); ++i) {
            const TensorData& o = r.outputs[i];
            if (o.data_type != DATATYPE_FLOAT32 || !o.data || o.data_size == 0) continue;
            out[size_t(i)].push_back({o.data, o.data_size, size_t(pi.plan.outputs[size_t(i)].view.numel()) * sizeof(float), 0});
        }
        C->upload.assign(size_t(2 * N), 0);
        for (int n = 0; n < N; ++n) { C->upload[size_t(n)] = int(C->lens[size_t(n)]); C->upload[size_t(N + n)] = c[size_t(n)]; }
        D.UploadKvLens(C->upload.data());
        D.InferHostSegments(pi, in, out);                // (waits for the forward: the lengths below are those of a finished call)
        M.Account(D, pi);
        write_out_dims(r.outputs, r.num_outputs, pi.plan.outputs, 0);
        for (int n = 0; n < N; ++n) C->lens[size_t(n)] += c[size_t(n)];
        r.ok = true;
    } catch (const std::exception& e) {
        fail(std::string("ONNX inference error: ") + e.what());
    }
}

}  // namespace ie_bridge

using ie_bridge::set_error;

extern "C" {

EngineKvCacheHandle EngineKvCacheCreate(int device_id, int layers, int batch, int kv_heads, int capacity, int head_dim, ErrorMessage* error) {
    if (layers < 1 || batch < 1 || kv_heads < 1 || capacity < 1 || head_dim < 1 || layers > 4096 || batch > 65535 || kv_heads > 65535) {
        set_error(error, "EngineKvCacheCreate: layers, batch, kv_heads, capacity and head_dim must be positive (layers <= 4096, batch and kv_heads <= 65535)");
        return nullptr;
    }
    if (device_id < 0 || device_id >= ie::HipDeviceCount()) { set_error(error, "EngineKvCacheCreate: no HIP device " + std::to_string(device_id)); return nullptr; }
    auto C = std::make_unique<EngineKvCache>();
    auto dev = std::make_shared<ie::KvBinding>();
    try {
        dev->layers = layers; dev->batch = batch; dev->kv_heads = kv_heads; dev->capacity = capacity; dev->head_dim = head_dim;
        const size_t bytes = ie_bridge::tensor_floats(*dev) * sizeof(float);
        ie_bridge::hip_ok(hipSetDevice(device_id), "hipSetDevice");
        ie_bridge::hip_ok(hipStreamCreateWithFlags(&C->stream, hipStreamNonBlocking), "hipStreamCreate");
        for (int l = 0; l < 2 * layers; ++l) {
            float* p = nullptr;
            ie_bridge::hip_ok(hipMalloc(reinterpret_cast<void**>(&p), bytes), "hipMalloc(kv cache)");
            (l % 2 ? dev->v : dev->k).push_back(p);
            ie_bridge::hip_ok(hipMemsetAsync(p, 0, bytes, C->stream), "hipMemsetAsync(kv cache)");
        }
        ie_bridge::hip_ok(hipMalloc(reinterpret_cast<void**>(&dev->d_lens), size_t(2 * batch) * sizeof(int)), "hipMalloc(kv lengths)");
        ie_bridge::hip_ok(hipMemsetAsync(dev->d_lens, 0, size_t(2 * batch) * sizeof(int), C->stream), "hipMemsetAsync(kv lengths)");
        ie_bridge::hip_ok(hipStreamSynchronize(C->stream), "hipStreamSynchronize");
        C->bytes = bytes * size_t(2 * layers);
    } catch (const std::exception& e) {
        for (float* p : dev->k) (void)hipFree(p);
        for (float* p : dev->v) (void)hipFree(p);
        if (dev->d_lens) (void)hipFree(dev->d_lens);
        if (C->stream) (void)hipStreamDestroy(C->stream);
        set_error(error, e.what());
        return nullptr;
    }
    C->dev = std::move(dev);
    C->device_id = device_id;
    C->lens.assign(size_t(batch), 0);
    return C.release();
}

void EngineKvCacheDestroy(EngineKvCacheHandle cache) {
    if (!cache) return;
    // the bound models first, one by one, each with no request in flight
    for (;;) {
        std::shared_ptr<ie_bridge::ModelObj> m;
        {
            std::lock_guard<std::mutex> g(cache->mu);
            while (!cache->bound.empty() && !(m = cache->bound.back().lock())) cache->bound.pop_back();
        }
        if (!m) break;
        std::unique_lock<std::shared_mutex> life(m->life);
        try {
            if (m->kv == cache) ie_bridge::unbind(*m);
            else { std::lock_guard<std::mutex> g(cache->mu); ie_bridge::forget_locked(*cache, m.get()); }
        } catch (...) {
            std::lock_guard<std::mutex> g(cache->mu);
            ie_bridge::forget_locked(*cache, m.get());
            m->kv = nullptr;
        }
    }
    (void)hipSetDevice(cache->device_id);
    if (cache->stream) { (void)hipStreamSynchronize(cache->stream); (void)hipStreamDestroy(cache->stream); }
    for (float* p : cache->dev->k) (void)hipFree(p);
    for (float* p : cache->dev->v) (void)hipFree(p);
    if (cache->dev->d_lens) (void)hipFree(cache->dev->d_lens);
    delete cache;
}

bool EngineKvCacheBind(ModelHandle handle, EngineKvCacheHandle cache, ErrorMessage* error) {
    if (!handle) { set_error(error, "Invalid model handle"); return false; }
    try {
        ie_bridge::ModelObj& M = *handle->model;
        std::unique_lock<std::shared_mutex> life(M.life);      // waits for every request of the model in flight
        if (!M.loaded.load() || M.lanes.empty()) { set_error(error, "Model not loaded"); return false; }
        if (!cache) { ie_bridge::unbind(M); return true; }
        auto refuse = [&](const std::string& why) { set_error(error, "EngineKvCacheBind: " + why); return false; };
        const ie::KvBinding& g = *cache->dev;
        if (M.lanes[0]->precision() == ie::Precision::F8) return refuse("fp8 precision has no cache steps; a resident cache binds to fp32 and fp16 models");
        if (M.num_shards > 1) return refuse("the model has " + std::to_string(M.num_shards) + " shard replicas; a resident cache binds to a model of one lane");
        if (M.lanes.size() > 1) return refuse("the model has " + std::to_string(M.lanes.size()) + " execution lanes (instance_count); a resident cache binds to a model of one lane");
        if (M.batchable && M.max_batch > 1) return refuse("the model uses the dynamic batcher; a resident cache binds to a model without it");
        if (M.lanes[0]->device() != cache->device_id) return refuse("the model is on device " + std::to_string(M.lanes[0]->device()) + ", the cache on device " + std::to_string(cache->device_id));
        ie_bridge::GraphCache gc;
        if (const std::string e = ie_bridge::graph_cache(M.info, &gc); !e.empty()) return refuse(e);
        auto differs = [&](const char* what, int64_t graph, int64_t mine) { return refuse(std::string("geometry mismatch in ") + what + ": the model has " + std::to_string(graph) + ", the cache " + std::to_string(mine)); };
        if (gc.layers != g.layers) return differs("layers", gc.layers, g.layers);
        if (gc.batch > 0 && gc.batch != g.batch) return differs("batch", gc.batch, g.batch);
        if (gc.kv_heads != g.kv_heads) return differs("kv_heads", gc.kv_heads, g.kv_heads);
        if (gc.head_dim != g.head_dim) return differs("head_dim", gc.head_dim, g.head_dim);
        if (gc.past > 0 && gc.past != g.capacity) return differs("capacity (the rows of past_key_values.*)", gc.past, g.capacity);
        if (gc.past == 0 && gc.present > g.capacity) return differs("capacity (the rows a prefill writes)", gc.present, g.capacity);
        if (M.kv) ie_bridge::unbind(M);
        M.lanes[0]->BindKvCache(cache->dev);
        M.kv = cache;
        M.kv_past = int(gc.past);
        M.kv_lq = int(gc.present - gc.past);
        std::lock_guard<std::mutex> cm(cache->mu);
        cache->bound.push_back(handle->model);
        return true;
    } catch (const std::exception& e) { set_error(error, e.what()); return false; }
    catch (...) { set_error(error, "unknown error"); return false; }
}

bool EngineKvCacheGetLengths(EngineKvCacheHandle cache, int64_t* lens, ErrorMessage* error) {
    if (!cache) { set_error(error, "Invalid KV cache handle"); return false; }
    if (!lens) { set_error(error, "Invalid parameters"); return false; }
    std::lock_guard<std::mutex> g(cache->mu);
    std::copy(cache->lens.begin(), cache->lens.end(), lens);
    return true;
}

bool EngineKvCacheSetLengths(EngineKvCacheHandle cache, const int64_t* lens, ErrorMessage* error) {
    if (!cache) { set_error(error, "Invalid KV cache handle"); return false; }
    if (!lens) { set_error(error, "Invalid parameters"); return false; }
    std::lock_guard<std::mutex> g(cache->mu);
    for (size_t i = 0; i < cache->lens.size(); ++i)
        if (lens[i] < 0 || lens[i] > cache->dev->capacity) {
            set_error(error, "EngineKvCacheSetLengths: length " + std::to_string(lens[i]) + " of image " + std::to_string(i) + " is outside 0 .. " + std::to_string(cache->dev->capacity));
            return false;
        }
    std::copy(lens, lens + cache->lens.size(), cache->lens.begin());
    return true;
}

namespace {
// one layer's whole K or V tensor to or from the host, with every bound model's lane drained first (an EngineRunPrepared without sync may be in flight)
bool cache_copy(EngineKvCacheHandle cache, int layer, int which, void* dst, const void* src, size_t bytes, bool to_host, ErrorMessage* error) {
    if (!cache) { set_error(error, "Invalid KV cache handle"); return false; }
    if (!(to_host ? dst : const_cast<void*>(src))) { set_error(error, "Invalid parameters"); return false; }
    try {
        std::lock_guard<std::mutex> g(cache->mu);
        const ie::KvBinding& d = *cache->dev;
        if (layer < 0 || layer >= d.layers || (which != 0 && which != 1)) { set_error(error, "EngineKvCache: no layer " + std::to_string(layer) + " / tensor " + std::to_string(which) + " (0 key, 1 value)"); return false; }
        const size_t have = ie_bridge::tensor_floats(d) * sizeof(float);
        if (bytes != have) { set_error(error, "EngineKvCache: a layer's tensor is " + std::to_string(have) + " bytes, not " + std::to_string(bytes)); return false; }
        for (const auto& w : cache->bound)
            if (const auto m = w.lock()) {
                std::shared_lock<std::shared_mutex> life(m->life, std::try_to_lock);      // (a model being loaded or unloaded has nothing in flight)
                if (life.owns_lock() && m->loaded.load() && !m->lanes.empty()) m->lanes[0]->Synchronize();
            }
        float* p = (which ? d.v : d.k)[size_t(layer)];
        ie_bridge::hip_ok(hipSetDevice(cache->device_id), "hipSetDevice");
        ie_bridge::hip_ok(to_host ? hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, cache->stream) : hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, cache->stream), "hipMemcpyAsync(kv cache)");
        ie_bridge::hip_ok(hipStreamSynchronize(cache->stream), "hipStreamSynchronize");
        return true;
    } catch (const std::exception& e) { set_error(error, e.what()); return false; }
    catch (...) { set_error(error, "unknown error"); return false; }
}
}  // namespace

bool EngineKvCacheRead(EngineKvCacheHandle cache, int layer, int which, float* dst, size_t bytes, ErrorMessage* error) {
    return cache_copy(cache, layer, which, dst, nullptr, bytes, true, error);
}

bool EngineKvCacheWrite(EngineKvCacheHandle cache, int layer, int which, const float* src, size_t bytes, ErrorMessage* error) {
    return cache_copy(cache, layer, which, nullptr, src, bytes, false, error);
}

}  // extern "C"
