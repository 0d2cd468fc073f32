// Class token and position embedding of a Vision Transformer on gfx950: the Concat(axis 1) of the class-token constant with the patch tokens and
// the Add of the position embedding behind it, as one pointwise pass.
//
//   out[n, 0, :] = cls + pos[0]        out[n, 1 + p, :] = in[n, p, :] + pos[1 + p]        (pos absent: nothing is added)
//
// token_assemble_kernel<T, VEC>: one thread per 16-byte vector of the output (VEC: 4 floats / 8 halfs) or per element (any D, pitch, offset).
// cls and pos are fp32 in every precision; the sum is formed in fp32.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kTokBlock = 256;

// per: V-element groups per output row (D / V); total = N * (L0 + 1) * per
template <typename T, int V>
__global__ __launch_bounds__(kTokBlock) void token_assemble_kernel(const TokenAssembleArgs a, const int per, const int64_t total) {
    const int64_t g = int64_t(blockIdx.x) * kTokBlock + threadIdx.x;
    if (g >= total) return;
    const int d = int(g % per) * V;
    const int64_t r = g / per;
    const int row = int(r % a.out.w);
    const int64_t n = r / a.out.w;
    float x[V];
    if (row == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] = a.cls[d + v];
    } else {
        const T* src = reinterpret_cast<const T*>(a.in.p) + n * a.in.sn + int64_t(row - 1) * a.in.sw + d;
        if constexpr (V > 1) {
            T tmp[V];
            *reinterpret_cast<uint4*>(tmp) = *reinterpret_cast<const uint4*>(src);
#pragma unroll
            for (int v = 0; v < V; ++v) x[v] = float(tmp[v]);
        } else x[0] = float(src[0]);
    }
    if (a.pos) {
        const float* ps = a.pos + int64_t(row) * a.out.c + d;
#pragma unroll
        for (int v = 0; v < V; ++v) x[v] += ps[v];
    }
    T* dst = reinterpret_cast<T*>(a.out.p) + n * a.out.sn + int64_t(row) * a.out.sw + d;
    if constexpr (V > 1) {
        T tmp[V];
#pragma unroll
        for (int v = 0; v < V; ++v) tmp[v] = T(x[v]);
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(tmp);
    } else dst[0] = T(x[0]);
}

bool args_ok(const TokenAssembleArgs& a) {
    return a.in.p && a.out.p && a.cls && !a.in.f8 && !a.out.f8 && a.in.f16 == a.out.f16 && a.in.sc == 1 && a.out.sc == 1 && a.in.h == 1 && a.out.h == 1 &&
           a.in.c == a.out.c && a.in.n == a.out.n && a.out.w == a.in.w + 1 && a.in.c >= 1;
}

template <typename T, int V>
hipError_t launch(const TokenAssembleArgs& a, hipStream_t stream) {
    const int per = a.out.c / V;
    const int64_t total = int64_t(a.out.n) * a.out.w * per;
    const int64_t blocks = (total + kTokBlock - 1) / kTokBlock;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    token_assemble_kernel<T, V><<<dim3(unsigned(blocks)), dim3(kTokBlock), 0, stream>>>(a, per, total);
    return hipGetLastError();
}

}  // namespace

bool TokenAssembleVectorised(const TokenAssembleArgs& a) {
    const int V = a.out.f16 ? 8 : 4;
    auto ok = [&](const TensorArg& t) { return t.c % V == 0 && t.sw % V == 0 && t.sn % V == 0 && Aligned16(t.p); };
    return args_ok(a) && ok(a.in) && ok(a.out);
}

hipError_t LaunchTokenAssemble(const TokenAssembleArgs& a, hipStream_t stream) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    if (TokenAssembleVectorised(a)) return a.out.f16 ? launch<_Float16, 8>(a, stream) : launch<float, 4>(a, stream);
    return a.out.f16 ? launch<_Float16, 1>(a, stream) : launch<float, 1>(a, stream);
}

}  // namespace ie
