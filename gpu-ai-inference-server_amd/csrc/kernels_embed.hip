// Token embedding lookup fused with the LayerNormalization behind it (BERT-class graphs) on gfx950.
//
//   x[r, :]   = word[ids[r]] + type[tids[r]] + pos[r mod L]                       for every token row r = (n, l); type / pos optional
//   out[r, c] = (x[r, c] - mean_r) * rsqrt(var_r + eps) * gamma[c] + beta[c]
//
// Bandwidth-bound: two or three fp32 table rows read and one row written per token, ~8 flops per element; the sum never exists in memory.  The
// tables, gamma and beta are fp32 in every precision, the statistics fp32; the variance is that of the CENTRED values (mean first, then
// sum((x - mean)^2)), as in kernels_ln.hip -- embedding tables with a large common offset lose every digit to E[x^2] - mean^2.
//
// Indices are int64 as the graph input holds them.  A negative index counts from the end (ONNX Gather); the wrapped index is then clamped into
// [0, rows - 1], so no index a caller can put into the buffer reads outside a table (ModelInfer refuses out-of-range ids before it enqueues
// anything; the clamp covers the device-resident entry points).
//
//   embed_ln_kernel<T, LANES, NV>    the fast path: a group of LANES (8 / 16 / 32 / 64) lanes owns one token row, lane l the 16-byte output vectors
//                                    l, l + LANES, ... (at most NV: 4 floats / 8 halfs each).  The row is built once in registers from 16-byte
//                                    table loads; both reductions are cross-lane shuffles inside the group (no LDS, no barrier).
//   embed_ln_generic_kernel          one wave per token row, any D, pitch and offset, float or half output; the row is rebuilt from the tables for
//                                    each of its three passes (the same fp32 sums every time).
//
//   embed_sum_kernel<T, LANES>       gamma null: the sum itself is the result (a pre-LN model, GPT-2: the sum is read by a LayerNormalization and by the
//   embed_sum_generic_kernel         residual Add, so it has to exist).  The same lane groups, the same row assembly from 16-byte table loads, no
//                                    statistics and no shuffles; the sum is fp32, the store in out's element type.  The generic form is one wave per row.
//
// All only enqueue work on the given stream: they are graph-capturable, and a replay is bit-identical to the eager run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kEmbBlock = 256;

// ONNX Gather index -> table row: negative wraps once, then the clamp
__device__ __forceinline__ int64_t table_row(int64_t id, int rows) {
    if (id < 0) id += rows;
    return id < 0 ? 0 : (id >= rows ? int64_t(rows) - 1 : id);
}

template <int V>
__device__ __forceinline__ void add_row(const float* p, float* d) {
#pragma unroll
    for (int k = 0; k < V; k += 4) {
        const float4 x = *reinterpret_cast<const float4*>(p + k);
        d[k] += x.x; d[k + 1] += x.y; d[k + 2] += x.z; d[k + 3] += x.w;
    }
}
template <int V>
__device__ __forceinline__ void load_row(const float* p, float* d) {
#pragma unroll
    for (int k = 0; k < V; k += 4) {
        const float4 x = *reinterpret_cast<const float4*>(p + k);
        d[k] = x.x; d[k + 1] = x.y; d[k + 2] = x.z; d[k + 3] = x.w;
    }
}

// output vector cv of a token row: word + type + pos (the fp32 sum every embed kernel starts from)
template <int V>
__device__ __forceinline__ void sum_vec(const float* wrow, const float* trow, const float* prow, int cv, float* x) {
    load_row<V>(wrow + cv * V, x);
    if (trow) add_row<V>(trow + cv * V, x);
    if (prow) add_row<V>(prow + cv * V, x);
}

// rows = N * L token rows; cvn = D / V output vectors per row (<= LANES * NV); row r is written at r * a.out.sw
template <typename T, int LANES, int NV>
__global__ __launch_bounds__(kEmbBlock) void embed_ln_kernel(const EmbedArgs a, const int64_t rows, const int cvn) {
    constexpr int V = 16 / int(sizeof(T));
    const int lane = int(threadIdx.x) % LANES;
    const int64_t row = (int64_t(blockIdx.x) * kEmbBlock + threadIdx.x) / LANES;
    const bool live = row < rows;                  // the same for every lane of a group; a dead group still runs the shuffles
    const int64_t r = live ? row : 0;
    const int D = a.out.c;
    const float* wrow = a.word + table_row(a.ids[r], a.vocab) * D;
    const float* trow = a.type ? a.type + table_row(a.tids[r], a.types) * D : nullptr;
    const float* prow = a.pos ? a.pos + (r % a.out.w) * D : nullptr;

    float x[NV][V];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int cv = j * LANES + lane;
        if (live && cv < cvn) sum_vec<V>(wrow, trow, prow, cv, x[j]);
        else {
#pragma unroll
            for (int v = 0; v < V; ++v) x[j][v] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) s += x[j][v];
    }
    const float inv_d = 1.f / float(D);
    const float mean = group_sum<LANES>(s) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const bool has = j * LANES + lane < cvn;   // (the zero filling of an absent vector must not count as -mean)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            x[j][v] = has ? x[j][v] - mean : 0.f;
            q = fmaf(x[j][v], x[j][v], q);
        }
    }
    const float rstd = 1.f / sqrtf(group_sum<LANES>(q) * inv_d + a.eps);
    T* out = reinterpret_cast<T*>(a.out.p) + r * a.out.sw;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int cv = j * LANES + lane;
        if (!live || cv >= cvn) continue;
        float g[V], b[V], o[V];
        load_row<V>(a.gamma + cv * V, g);
        if (a.beta) load_row<V>(a.beta + cv * V, b);
        else {
#pragma unroll
            for (int v = 0; v < V; ++v) b[v] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = fmaf(x[j][v] * rstd, g[v], b[v]);
        store16(out + cv * V, o);
    }
}

// one wave per token row (kEmbBlock / 64 rows per workgroup)
__global__ __launch_bounds__(kEmbBlock) void embed_ln_generic_kernel(const EmbedArgs a, const int64_t rows) {
    const int lane = int(threadIdx.x) % 64;
    const int64_t row = int64_t(blockIdx.x) * (kEmbBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int D = a.out.c;
    const float* wrow = a.word + table_row(a.ids[row], a.vocab) * D;
    const float* trow = a.type ? a.type + table_row(a.tids[row], a.types) * D : nullptr;
    const float* prow = a.pos ? a.pos + (row % a.out.w) * D : nullptr;
    auto at = [&](int c) {
        float v = wrow[c];
        if (trow) v += trow[c];
        if (prow) v += prow[c];
        return v;
    };
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += at(c);
    const float mean = group_sum<64>(s) / float(D);
    float q = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float d = at(c) - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(group_sum<64>(q) / float(D) + a.eps);
    const int64_t ob = (row / a.out.w) * a.out.sn + (row % a.out.w) * a.out.sw;
    for (int c = lane; c < D; c += 64) {
        const float o = fmaf((at(c) - mean) * rstd, a.gamma[c], a.beta ? a.beta[c] : 0.f);
        const int64_t oi = ob + int64_t(c) * a.out.sc;
        if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
        else a.out.p[oi] = o;
    }
}

// rows = N * L token rows; cvn = D / V output vectors per row, lane l of a group writes the vectors l, l + LANES, ...; row r is written at r * a.out.sw
template <typename T, int LANES>
__global__ __launch_bounds__(kEmbBlock) void embed_sum_kernel(const EmbedArgs a, const int64_t rows, const int cvn) {
    constexpr int V = 16 / int(sizeof(T));
    const int lane = int(threadIdx.x) % LANES;
    const int64_t r = (int64_t(blockIdx.x) * kEmbBlock + threadIdx.x) / LANES;
    if (r >= rows) return;                         // (no shuffle and no barrier below)
    const int D = a.out.c;
    const float* wrow = a.word + table_row(a.ids[r], a.vocab) * D;
    const float* trow = a.type ? a.type + table_row(a.tids[r], a.types) * D : nullptr;
    const float* prow = a.pos ? a.pos + (r % a.out.w) * D : nullptr;
    T* out = reinterpret_cast<T*>(a.out.p) + r * a.out.sw;
    for (int cv = lane; cv < cvn; cv += LANES) {
        float x[V];
        sum_vec<V>(wrow, trow, prow, cv, x);
        store16(out + cv * V, x);
    }
}

// one wave per token row (kEmbBlock / 64 rows per workgroup)
__global__ __launch_bounds__(kEmbBlock) void embed_sum_generic_kernel(const EmbedArgs a, const int64_t rows) {
    const int lane = int(threadIdx.x) % 64;
    const int64_t row = int64_t(blockIdx.x) * (kEmbBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int D = a.out.c;
    const float* wrow = a.word + table_row(a.ids[row], a.vocab) * D;
    const float* trow = a.type ? a.type + table_row(a.tids[row], a.types) * D : nullptr;
    const float* prow = a.pos ? a.pos + (row % a.out.w) * D : nullptr;
    const int64_t ob = (row / a.out.w) * a.out.sn + (row % a.out.w) * a.out.sw;
    for (int c = lane; c < D; c += 64) {
        float o = wrow[c];
        if (trow) o += trow[c];
        if (prow) o += prow[c];
        const int64_t oi = ob + int64_t(c) * a.out.sc;
        if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
        else a.out.p[oi] = o;
    }
}

template <typename T, int LANES, int NV>
hipError_t launch_nv(const EmbedArgs& a, int64_t rows, int cvn, hipStream_t stream) {
    const int64_t blocks = (rows * LANES + kEmbBlock - 1) / kEmbBlock;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    embed_ln_kernel<T, LANES, NV><<<dim3(unsigned(blocks)), dim3(kEmbBlock), 0, stream>>>(a, rows, cvn);
    return hipGetLastError();
}

template <typename T, int LANES>
hipError_t launch_lanes(const EmbedArgs& a, int64_t rows, int cvn, hipStream_t stream) {
    if (!a.gamma) {
        const int64_t blocks = (rows * LANES + kEmbBlock - 1) / kEmbBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        embed_sum_kernel<T, LANES><<<dim3(unsigned(blocks)), dim3(kEmbBlock), 0, stream>>>(a, rows, cvn);
        return hipGetLastError();
    }
    const int nv = (cvn + LANES - 1) / LANES;
    if (nv <= 1) return launch_nv<T, LANES, 1>(a, rows, cvn, stream);
    if (nv <= 2) return launch_nv<T, LANES, 2>(a, rows, cvn, stream);
    if (nv <= 3) return launch_nv<T, LANES, 3>(a, rows, cvn, stream);
    if (nv <= 4) return launch_nv<T, LANES, 4>(a, rows, cvn, stream);
    return launch_nv<T, LANES, kLnMaxVectors>(a, rows, cvn, stream);
}

template <typename T>
hipError_t launch_fast(const EmbedArgs& a, int tile, int64_t rows, hipStream_t stream) {
    const int cvn = a.out.c / (16 / int(sizeof(T)));
    switch (kLnLanes[tile]) {
        case 8: return launch_lanes<T, 8>(a, rows, cvn, stream);
        case 16: return launch_lanes<T, 16>(a, rows, cvn, stream);
        case 32: return launch_lanes<T, 32>(a, rows, cvn, stream);
        default: return launch_lanes<T, 64>(a, rows, cvn, stream);
    }
}

}  // namespace

bool EmbedEligible(const EmbedArgs& a, int tile) {
    if (tile < 0 || tile >= kNumEmbedTiles || !a.ids || !a.word || (!a.gamma && a.beta) || !a.out.p || a.vocab < 1) return false;
    if ((a.type != nullptr) != (a.tids != nullptr) || (a.type && a.types < 1)) return false;
    if (a.out.f8 || a.out.c < 1 || a.out.h != 1 || a.out.w < 1 || a.out.n < 0 || a.out.sn != int64_t(a.out.w) * a.out.sw) return false;
    if (tile == 0) return true;
    // (the offset is in the base pointer: its alignment stands for the offset condition)
    return a.out.sc == 1 && EmbedTileFits(a.out.c, a.out.f16 != 0, a.out.sw, 0, tile) && Aligned16(a.out.p) && Aligned16(a.word) && (!a.type || Aligned16(a.type)) &&
           (!a.pos || Aligned16(a.pos)) && (!a.gamma || Aligned16(a.gamma)) && (!a.beta || Aligned16(a.beta));
}

hipError_t LaunchEmbed(const EmbedArgs& a, int tile, hipStream_t stream) {
    if (!EmbedEligible(a, tile)) return hipErrorInvalidValue;
    const int64_t rows = int64_t(a.out.n) * a.out.w;
    if (rows == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t blocks = (rows + kEmbBlock / 64 - 1) / (kEmbBlock / 64);
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.gamma) hipLaunchKernelGGL(embed_ln_generic_kernel, dim3(unsigned(blocks)), dim3(kEmbBlock), 0, stream, a, rows);
        else hipLaunchKernelGGL(embed_sum_generic_kernel, dim3(unsigned(blocks)), dim3(kEmbBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    return a.out.f16 ? launch_fast<_Float16>(a, tile, rows, stream) : launch_fast<float>(a, tile, rows, stream);
}

}  // namespace ie
