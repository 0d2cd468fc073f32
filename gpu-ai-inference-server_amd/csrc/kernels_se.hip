// Squeeze-and-excitation blocks (MobileNetV3 / EfficientNet) on gfx950.
//
// out[n, y, x, c] = in[n, y, x, c] * gate[n, c],  gate = act(b2 + W2 * act1(b1 + W1 * mean_yx(in[n]))).  Bandwidth-bound: the block reads its
// input twice (squeeze, apply) and writes it once; the two FCs are a few MFLOP.  Three phases, four launches, all deterministic (every sum runs
// in a fixed order, no atomics):
//
//   se_squeeze_kernel<T, V>   grid (pixel chunk, image, group of 64 channel vectors).  Lanes own one 16-byte channel vector (4 floats / 8 halfs;
//                             V = 1: one channel, for channel counts or pitches the vectors do not tile) and walk the chunk's pixels in rows
//                             of lanes; the rows are summed through LDS in row order.  Writes fp32 partial sums [chunk][N][C] to the workspace.  A single (C/64, N)
//                             grid leaves most of the part idle on the large early maps (EfficientNet's first SE: 112x112x32 at batch 32
//                             is 32 workgroups); SeSqueezeChunks splits those maps into up to 64 chunks of >= 64 pixels.
//   se_fc1_kernel             one wave per hidden unit and group of 16 images: means (partials summed in chunk order, / HW), dot product
//                             with the unit's weight row (lanes stride the channels, butterfly reduction), + bias, act1.  A weight row is
//                             read once per 16 images, not once per image.
//   se_fc2_kernel             one lane per output channel and group of 8 images: the group's hidden values are staged in LDS, W2 is packed
//                             transposed ([mid][C]) so the lanes of a wave read consecutive floats; + bias, the gate's activation.  Writes the fp32 gate [N][C].
//   se_apply_kernel<T, V>     y = x * gate[n, c] on 16-byte NHWC vectors (V = 1: scalar), fp32 math, output in the input's element type.
//
// Workspace: partials [chunks][N][C] | hidden [N][mid] | gate [N][C], offsets rounded to 8 floats (SeWorkspaceFloats sizes it).  The executor
// captures a forward pass on one stream, so steps reuse the workspace one after the other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kSeBlock = 256;
constexpr int kSeVecs = 64;           // channel vectors per squeeze workgroup
constexpr int kFc1Images = 16;       // images per fc1 wave
constexpr int kFc2Images = 8;        // images per fc2 lane
constexpr int kFc2Tile = 256;        // hidden units staged in LDS per pass

// V consecutive elements <-> floats (V = 16 bytes' worth, or 1)
template <typename T, int V>
__device__ __forceinline__ void ldv(const T* p, float* d) {
    if constexpr (V == 1) d[0] = float(*p);
    else load16<T>(p, d);
}
template <typename T, int V>
__device__ __forceinline__ void stv(T* p, const float* v) {
    if constexpr (V == 1) *p = T(v[0]);
    else store16<T>(p, v);
}

struct SeWs {
    float* part;
    float* hid;
    float* gate;
};
__host__ __device__ inline int64_t round8(int64_t x) { return (x + 7) & ~int64_t(7); }
SeWs se_ws(const SeArgs& a) {
    const int64_t nc = int64_t(a.in.n) * a.in.c;
    const int64_t hid = round8(int64_t(a.chunks) * nc);
    const int64_t gate = round8(hid + int64_t(a.in.n) * a.mid);
    return {a.workspace, a.workspace + hid, a.workspace + gate};
}

template <typename T, int V>
__global__ __launch_bounds__(kSeBlock) void se_squeeze_kernel(const TensorArg in, float* __restrict__ part, const int ppc) {
    __shared__ float red[kSeBlock * V];
    const int k = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int C = in.c, HW = in.h * in.w;
    const int cv0 = blockIdx.z * kSeVecs;                  // this workgroup's channel vectors: [cv0, cv0 + cvb)
    const int cvb = min(kSeVecs, C / V - cv0);
    const int rows = kSeBlock / cvb;                       // >= 4 rows of lanes walk the chunk's pixels
    const int p0 = k * ppc, p1 = min(HW, p0 + ppc);
    const T* __restrict__ base = reinterpret_cast<const T*>(in.p) + int64_t(n) * in.sn;
    float* __restrict__ dst = part + (int64_t(k) * in.n + n) * C + cv0 * V;
    const int r = tid / cvb, cl = tid - r * cvb;
    if (r < rows) {
        float acc[V], x[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.f;
        for (int p = p0 + r; p < p1; p += rows) {
            const int y = p / in.w, xx = p - y * in.w;
            ldv<T, V>(base + int64_t(y) * in.sh + int64_t(xx) * in.sw + (cv0 + cl) * V, x);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += x[v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) red[(r * cvb + cl) * V + v] = acc[v];
    }
    __syncthreads();
    for (int i = tid; i < cvb * V; i += kSeBlock) {
        const int ci = i / V, vi = i - ci * V;
        float s = 0.f;
        for (int rr = 0; rr < rows; ++rr) s += red[(rr * cvb + ci) * V + vi];
        dst[i] = s;
    }
}

__global__ __launch_bounds__(kSeBlock) void se_fc1_kernel(const float* __restrict__ part, const float* __restrict__ w1, const float* __restrict__ b1,
                                                           float* __restrict__ hid, const int N, const int C, const int mid, const int chunks,
                                                           const float inv_hw, const int act1, const float aa, const float ab) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (kSeBlock / 64) + (threadIdx.x >> 6);
    const int n0 = blockIdx.y * kFc1Images;
    if (j >= mid) return;             // (no block-wide synchronisation below)
    const float* __restrict__ wr = w1 + int64_t(j) * C;
    const int64_t NC = int64_t(N) * C;
    float acc[kFc1Images];
#pragma unroll
    for (int i = 0; i < kFc1Images; ++i) acc[i] = 0.f;
#pragma unroll 2
    for (int c = lane; c < C; c += 64) {
        const float w = wr[c];
#pragma unroll
        for (int i = 0; i < kFc1Images; ++i) {
            if (n0 + i < N) {
                const float* pp = part + int64_t(n0 + i) * C + c;
                float s = 0.f;
                for (int k = 0; k < chunks; ++k) s += pp[k * NC];
                acc[i] = fmaf(w, s * inv_hw, acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kFc1Images; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_xor(acc[i], off);
    const float bias = b1 ? b1[j] : 0.f;
#pragma unroll
    for (int i = 0; i < kFc1Images; ++i)
        if (lane == i && n0 + i < N) hid[int64_t(n0 + i) * mid + j] = ApplyAct(act1, aa, ab, acc[i] + bias);
}

__global__ __launch_bounds__(64) void se_fc2_kernel(const float* __restrict__ hid, const float* __restrict__ w2t, const float* __restrict__ b2,
                                                     float* __restrict__ gate, const int N, const int C, const int mid, const int act, const float aa,
                                                     const float ab) {
    __shared__ float hs[kFc2Images][kFc2Tile];         // the group's hidden values, one tile of units at a time (LDS broadcast reads)
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int n0 = blockIdx.y * kFc2Images;
    const bool live = c < C;
    float acc[kFc2Images];
#pragma unroll
    for (int i = 0; i < kFc2Images; ++i) acc[i] = 0.f;
    for (int j0 = 0; j0 < mid; j0 += kFc2Tile) {
        const int jn = min(kFc2Tile, mid - j0);
        __syncthreads();
        for (int q = threadIdx.x; q < kFc2Images * kFc2Tile; q += 64) {
            const int i = q / kFc2Tile, j = q - i * kFc2Tile;
            hs[i][j] = n0 + i < N && j < jn ? hid[int64_t(n0 + i) * mid + j0 + j] : 0.f;
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int j = 0; j < jn; ++j) {
                const float w = w2t[int64_t(j0 + j) * C + c];
#pragma unroll
                for (int i = 0; i < kFc2Images; ++i) acc[i] = fmaf(w, hs[i][j], acc[i]);
            }
        }
    }
    if (!live) return;
    const float bias = b2 ? b2[c] : 0.f;
#pragma unroll
    for (int i = 0; i < kFc2Images; ++i)
        if (n0 + i < N) gate[int64_t(n0 + i) * C + c] = ApplyAct(act, aa, ab, acc[i] + bias);
}

template <typename T, int V>
__global__ __launch_bounds__(kSeBlock) void se_apply_kernel(const TensorArg in, const TensorArg out, const float* __restrict__ gate, const int64_t total,
                                                             const int cvn) {
    const int64_t idx = int64_t(blockIdx.x) * kSeBlock + threadIdx.x;
    if (idx >= total) return;
    const int cv = int(idx % cvn);
    int64_t m = idx / cvn;
    const int x = int(m % in.w);
    m /= in.w;
    const int y = int(m % in.h);
    const int n = int(m / in.h);
    const int c = cv * V;
    float v[V], g[V];
    ldv<T, V>(reinterpret_cast<const T*>(in.p) + int64_t(n) * in.sn + int64_t(y) * in.sh + int64_t(x) * in.sw + c, v);
    const float* gp = gate + int64_t(n) * in.c + c;
    if constexpr (V == 1) g[0] = gp[0];
    else {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(gp)[q];
            g[4 * q] = t.x; g[4 * q + 1] = t.y; g[4 * q + 2] = t.z; g[4 * q + 3] = t.w;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] *= g[i];
    stv<T, V>(reinterpret_cast<T*>(out.p) + int64_t(n) * out.sn + int64_t(y) * out.sh + int64_t(x) * out.sw + c, v);
}

template <typename T, int V>
hipError_t launch_phase(const SeArgs& a, int phase, hipStream_t stream) {
    const SeWs ws = se_ws(a);
    const int N = a.in.n, C = a.in.c, HW = a.in.h * a.in.w;
    if (phase == 0) {
        const int ppc = (HW + a.chunks - 1) / a.chunks;
        const int groups = (C / V + kSeVecs - 1) / kSeVecs;
        se_squeeze_kernel<T, V><<<dim3(unsigned(a.chunks), unsigned(N), unsigned(groups)), dim3(kSeBlock), 0, stream>>>(a.in, ws.part, ppc);
    } else if (phase == 1) {
        const dim3 grid(unsigned((a.mid + kSeBlock / 64 - 1) / (kSeBlock / 64)), unsigned((N + kFc1Images - 1) / kFc1Images));
        se_fc1_kernel<<<grid, dim3(kSeBlock), 0, stream>>>(ws.part, a.w1, a.b1, ws.hid, N, C, a.mid, a.chunks, 1.f / float(HW), a.act1, a.act1_a, a.act1_b);
    } else if (phase == 2) {
        const dim3 grid(unsigned((C + 63) / 64), unsigned((N + kFc2Images - 1) / kFc2Images));
        se_fc2_kernel<<<grid, dim3(64), 0, stream>>>(ws.hid, a.w2t, a.b2, ws.gate, N, C, a.mid, a.act, a.act_a, a.act_b);
    } else {
        const int cvn = C / V;
        const int64_t total = int64_t(N) * HW * cvn;
        const int64_t blocks = (total + kSeBlock - 1) / kSeBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        se_apply_kernel<T, V><<<dim3(unsigned(blocks)), dim3(kSeBlock), 0, stream>>>(a.in, a.out, ws.gate, total, cvn);
    }
    return hipGetLastError();
}

}  // namespace

bool SqueezeExciteEligible(const SeArgs& a) {
    if (!a.in.p || !a.out.p || !a.w1 || !a.w2t || !a.workspace || a.mid < 1) return false;
    if (a.in.f8 || a.out.f8 || a.in.f16 != a.out.f16 || a.in.sc != 1 || a.out.sc != 1) return false;
    if (a.in.n != a.out.n || a.in.c != a.out.c || a.in.h != a.out.h || a.in.w != a.out.w || a.in.n < 1 || a.in.c < 1 || a.in.h * a.in.w < 1) return false;
    if (a.chunks < 1 || a.chunks > a.in.h * a.in.w || a.in.n > 65535 || a.chunks > 65535 || a.in.c > 65535 * kSeVecs) return false;
    return a.workspace_floats >= SeWorkspaceFloats(a.in.n, a.in.c, a.mid, a.chunks);
}

hipError_t LaunchSqueezeExcitePhase(const SeArgs& a, int phase, hipStream_t stream) {
    if (!SqueezeExciteEligible(a) || phase < 0 || phase > 3) return hipErrorInvalidValue;
    const int V = a.in.f16 ? 8 : 4;
    const bool vec = VecViewOk(a.in, V) && VecViewOk(a.out, V);
    if (a.in.f16) return vec ? launch_phase<_Float16, 8>(a, phase, stream) : launch_phase<_Float16, 1>(a, phase, stream);
    return vec ? launch_phase<float, 4>(a, phase, stream) : launch_phase<float, 1>(a, phase, stream);
}

hipError_t LaunchSqueezeExcite(const SeArgs& a, hipStream_t stream) {
    for (int phase = 0; phase < 4; ++phase) {
        const hipError_t e = LaunchSqueezeExcitePhase(a, phase, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace ie
