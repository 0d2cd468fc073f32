// LayerNormalization over the channel axis of an NHWC view (ConvNeXt-class graphs) on gfx950.
//
//   out[p, c] = (x[p, c] - mean_p) * rsqrt(var_p + eps) * gamma[c] + beta[c]      for every pixel row p = (n, y, x)
//
// Bandwidth-bound: one read and one write of the tensor, ~8 flops per element.  fp32 accumulation in both element types.  The variance is
// that of the CENTRED values -- the mean first, then sum((x - mean)^2) -- never E[x^2] - mean^2, which loses every digit when |mean| >> std.
//
//   layernorm_kernel<T, LANES, NV>   the fast path: a group of LANES (8 / 16 / 32 / 64) lanes owns one pixel row, a wave 64 / LANES rows.  Lane l
//                                    holds the 16-byte channel vectors l, l + LANES, ... (at most NV of them: 4 floats / 8 halfs each) of its
//                                    row in registers from the one load to the store; both reductions run inside the group with cross-lane
//                                    shuffles (no LDS, no barrier).  gamma / beta are read as 16-byte vectors.
//   layernorm_generic_kernel         one wave per pixel row, any C, channel stride, pitch and channel offset, mixed element types; the row is
//                                    re-read for each of its three passes.
//
// RMSNorm (Llama-class graphs) is the compile-time variant RMS of both bodies, launched under its own kernel names:
//
//   out[p, c] = x[p, c] * rsqrt(mean_c(x[p, :]^2) + eps) * gamma[c]
//
//   rmsnorm_kernel<T, LANES, NV>     the fast body without the mean pass, the centring and beta: one reduction (the sum of squares) and the store
//   rmsnorm_generic_kernel           the generic body with two passes over the row instead of three
//
// The same tiles, eligibility and default tile as the layer norm (LnTileFits, LnDefaultTile); a row of zeros gives zeros (rsqrt(eps) is finite).
//
// Both are correct when out aliases in (the planner recycles buffers): a group / wave reads all of its row before it writes any of it, and no
// other group touches that row.  Rows past the end are masked (the row count need not be a multiple of the rows per workgroup).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kLnBlock = 256;

// rows: pixel rows of the view; cvn = C / V channel vectors per row (<= LANES * NV); row p starts at p * a.in.sw / p * a.out.sw
template <typename T, int LANES, int NV, bool RMS>
__device__ __forceinline__ void ln_rows(const LnArgs& a, const int64_t rows, const int cvn) {
    constexpr int V = 16 / int(sizeof(T));
    const int lane = int(threadIdx.x) % LANES;
    const int64_t row = (int64_t(blockIdx.x) * kLnBlock + threadIdx.x) / LANES;
    const bool live = row < rows;                  // the same for every lane of a group; a dead group still runs the shuffles
    const T* in = reinterpret_cast<const T*>(a.in.p) + (live ? row : 0) * a.in.sw;
    T* out = reinterpret_cast<T*>(a.out.p) + (live ? row : 0) * a.out.sw;

    float x[NV][V];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int cv = j * LANES + lane;
        if (live && cv < cvn) load16<T>(in + cv * V, x[j]);
        else {
#pragma unroll
            for (int v = 0; v < V; ++v) x[j][v] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if constexpr (RMS) s = fmaf(x[j][v], x[j][v], s);      // (the zero filling of an absent vector adds nothing)
            else s += x[j][v];
        }
    }
    const float inv_c = 1.f / float(a.in.c);
    float q = 0.f;
    if constexpr (RMS) q = s;
    else {
        const float mean = group_sum<LANES>(s) * inv_c;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const bool has = j * LANES + lane < cvn;   // (the zero filling of an absent vector must not count as -mean)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                x[j][v] = has ? x[j][v] - mean : 0.f;
                q = fmaf(x[j][v], x[j][v], q);
            }
        }
    }
    const float rstd = 1.f / sqrtf(group_sum<LANES>(q) * inv_c + a.eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int cv = j * LANES + lane;
        if (!live || cv >= cvn) continue;
        float g[V], b[V];
        load16<float>(a.gamma + cv * V, g);
        if constexpr (V == 8) load16<float>(a.gamma + cv * V + 4, g + 4);
        if constexpr (RMS) {
            float o[V];
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = x[j][v] * rstd * g[v];
            store16<T>(out + cv * V, o);
            continue;
        }
        if (a.beta) {
            load16<float>(a.beta + cv * V, b);
            if constexpr (V == 8) load16<float>(a.beta + cv * V + 4, b + 4);
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) b[v] = 0.f;
        }
        float o[V];
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = fmaf(x[j][v] * rstd, g[v], b[v]);
        store16<T>(out + cv * V, o);
    }
}

template <typename T, int LANES, int NV>
__global__ __launch_bounds__(kLnBlock) void layernorm_kernel(const LnArgs a, const int64_t rows, const int cvn) {
    ln_rows<T, LANES, NV, false>(a, rows, cvn);
}

template <typename T, int LANES, int NV>
__global__ __launch_bounds__(kLnBlock) void rmsnorm_kernel(const LnArgs a, const int64_t rows, const int cvn) {
    ln_rows<T, LANES, NV, true>(a, rows, cvn);
}

// one wave per pixel row (kLnBlock / 64 rows per workgroup)
template <bool RMS>
__device__ __forceinline__ void ln_row_generic(const LnArgs& a, const int64_t rows) {
    const int lane = int(threadIdx.x) % 64;
    const int64_t row = int64_t(blockIdx.x) * (kLnBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int C = a.in.c;
    const int px = int(row % a.in.w);
    const int64_t r = row / a.in.w;
    const int py = int(r % a.in.h);
    const int64_t pn = r / a.in.h;
    const int64_t ib = pn * a.in.sn + int64_t(py) * a.in.sh + int64_t(px) * a.in.sw;
    const int64_t ob = pn * a.out.sn + int64_t(py) * a.out.sh + int64_t(px) * a.out.sw;
    if constexpr (RMS) {
        float q = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = ld_any(a.in.p, a.in.f16, ib + int64_t(c) * a.in.sc);
            q = fmaf(d, d, q);
        }
        const float rstd = 1.f / sqrtf(group_sum<64>(q) / float(C) + a.eps);  // (the shuffles order every lane's reads before any lane's writes)
        for (int c = lane; c < C; c += 64) {
            const float o = ld_any(a.in.p, a.in.f16, ib + int64_t(c) * a.in.sc) * rstd * a.gamma[c];
            const int64_t oi = ob + int64_t(c) * a.out.sc;
            if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
            else a.out.p[oi] = o;
        }
        return;
    }
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += ld_any(a.in.p, a.in.f16, ib + int64_t(c) * a.in.sc);
    const float mean = group_sum<64>(s) / float(C);
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = ld_any(a.in.p, a.in.f16, ib + int64_t(c) * a.in.sc) - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(group_sum<64>(q) / float(C) + a.eps);      // (the shuffles order every lane's reads before any lane's writes)
    for (int c = lane; c < C; c += 64) {
        const float d = ld_any(a.in.p, a.in.f16, ib + int64_t(c) * a.in.sc) - mean;
        const float o = fmaf(d * rstd, a.gamma[c], a.beta ? a.beta[c] : 0.f);
        const int64_t oi = ob + int64_t(c) * a.out.sc;
        if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
        else a.out.p[oi] = o;
    }
}

__global__ __launch_bounds__(kLnBlock) void layernorm_generic_kernel(const LnArgs a, const int64_t rows) { ln_row_generic<false>(a, rows); }
__global__ __launch_bounds__(kLnBlock) void rmsnorm_generic_kernel(const LnArgs a, const int64_t rows) { ln_row_generic<true>(a, rows); }

template <typename T, int LANES, int NV>
hipError_t launch_nv(const LnArgs& a, int64_t rows, int cvn, hipStream_t stream) {
    const int64_t blocks = (rows * LANES + kLnBlock - 1) / kLnBlock;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (a.rms) rmsnorm_kernel<T, LANES, NV><<<dim3(unsigned(blocks)), dim3(kLnBlock), 0, stream>>>(a, rows, cvn);
    else layernorm_kernel<T, LANES, NV><<<dim3(unsigned(blocks)), dim3(kLnBlock), 0, stream>>>(a, rows, cvn);
    return hipGetLastError();
}

template <typename T, int LANES>
hipError_t launch_lanes(const LnArgs& a, int64_t rows, int cvn, hipStream_t stream) {
    const int nv = (cvn + LANES - 1) / LANES;
    if (nv <= 1) return launch_nv<T, LANES, 1>(a, rows, cvn, stream);
    if (nv <= 2) return launch_nv<T, LANES, 2>(a, rows, cvn, stream);
    if (nv <= 3) return launch_nv<T, LANES, 3>(a, rows, cvn, stream);
    if (nv <= 4) return launch_nv<T, LANES, 4>(a, rows, cvn, stream);
    return launch_nv<T, LANES, kLnMaxVectors>(a, rows, cvn, stream);
}

template <typename T>
hipError_t launch_fast(const LnArgs& a, int tile, int64_t rows, hipStream_t stream) {
    const int cvn = a.in.c / (16 / int(sizeof(T)));
    switch (kLnLanes[tile]) {
        case 8: return launch_lanes<T, 8>(a, rows, cvn, stream);
        case 16: return launch_lanes<T, 16>(a, rows, cvn, stream);
        case 32: return launch_lanes<T, 32>(a, rows, cvn, stream);
        default: return launch_lanes<T, 64>(a, rows, cvn, stream);
    }
}

}  // namespace

bool LayerNormEligible(const LnArgs& a, int tile) {
    if (tile < 0 || tile >= kNumLnTiles || !a.in.p || !a.out.p || !a.gamma || (a.rms && a.beta)) return false;
    if (a.in.f8 || a.out.f8 || a.in.c < 1 || a.in.c != a.out.c || a.in.n != a.out.n || a.in.h != a.out.h || a.in.w != a.out.w) return false;
    if (tile == 0) return true;
    const int V = a.out.f16 ? 8 : 4;
    // stricter than VecViewOk alone: the fast kernel walks n * h * w pixel rows one pitch apart (RowsDense)
    return LnTileFits(a.in.c, a.out.f16 != 0, tile) && a.in.f16 == a.out.f16 && VecViewOk(a.in, V) && RowsDense(a.in) &&
           VecViewOk(a.out, V) && RowsDense(a.out) && Aligned16(a.gamma) && (!a.beta || Aligned16(a.beta));
}

hipError_t LaunchLayerNorm(const LnArgs& a, int tile, hipStream_t stream) {
    if (!LayerNormEligible(a, tile)) return hipErrorInvalidValue;
    const int64_t rows = int64_t(a.in.n) * a.in.h * a.in.w;
    if (rows == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t blocks = (rows + kLnBlock / 64 - 1) / (kLnBlock / 64);
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.rms) hipLaunchKernelGGL(rmsnorm_generic_kernel, dim3(unsigned(blocks)), dim3(kLnBlock), 0, stream, a, rows);
        else hipLaunchKernelGGL(layernorm_generic_kernel, dim3(unsigned(blocks)), dim3(kLnBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    return a.out.f16 ? launch_fast<_Float16>(a, tile, rows, stream) : launch_fast<float>(a, tile, rows, stream);
}

}  // namespace ie
