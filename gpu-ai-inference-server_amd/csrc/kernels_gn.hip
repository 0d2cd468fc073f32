// GroupNormalization of an NHWC view (GroupNorm ResNets, the diffusion VAE decoder) on gfx950.
//
//   out[n, p, c] = act((x[n, p, c] - mean_ng) * rsqrt(var_ng + eps) * gamma[c] + beta[c])      g = c / (C / groups), p every pixel of image n
//
// The statistics run over a group's channels AND the whole map of one image, so no wave can compute them from one pixel row.  Bandwidth-bound:
// ~8 flops per element.  fp32 statistics in both element types.  The variance is that of the CENTRED values: Welford partials combined with
// Chan's formula (tile 1), or the mean first and then the squares (tile 0); never E[x^2] - mean^2.  No atomics: every combine runs in a fixed
// order, so two runs, and eager against graph replay, give the same bits.
// The result is computed as (x - mean) * (gamma * rstd) + beta, not as a * x + (beta - mean * a): with a constant group (variance 0, rstd =
// 1 / sqrt(eps) = 316) the second form leaves the rounding of mean * a, ~|mean| * 316 * 2^-24, on an output that should be beta exactly.
//
//   groupnorm_generic_kernel        tile 0: one workgroup per (image, group), three passes over its data (sum, centred squares, apply).  Any
//                                   C / groups, channel stride, pitch, channel offset, mixed element types.  The fallback and the cross-check.
//   groupnorm_stats_kernel<T, CPV>  tile 1, first launch: grid (slab of pixels, image).  Thread t keeps channel vector t % (C / V) (16 bytes: V = 4
//                                   floats / 8 halfs) and walks the slab's pixels t / (C / V), + R, ...; its partial therefore belongs to fixed
//                                   groups.  CPV = min(C / groups, V) channels of a vector share a group: a vector is NG = V / CPV whole groups
//                                   (C / groups < V) or lies inside one (C / groups a multiple of V).  Per vector and group: the CPV values' own
//                                   mean and centred squares, merged into the running (mean, M2) by Chan's formula.  The partials meet in LDS:
//                                   first the threads of one vector column in row order, then the columns of one group in channel order.  One
//                                   (count, mean, M2) record per (image, slab, group) goes to the workspace.
//   groupnorm_apply_kernel<T, ACT>  tile 1, second launch, the same grid: every workgroup combines its image's records in slab order (mean and
//                                   rstd per group into LDS; up to 16 threads share a group's slabs, each a contiguous run), every thread
//                                   takes mean, gamma * rstd and beta of its channel vector into registers and streams its pixels with
//                                   16-byte loads and stores.
//
// out may alias in: in tile 0 a workgroup has read all of its (image, group) before its first store and nobody else touches those elements; in tile
// 1 every element is read and written by the same lane of the apply launch, after the statistics launch has finished (stream order).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

// Chan's combine of (n, mean, m2) with (nb, mb, m2b); n + nb > 0
__device__ __forceinline__ void chan(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
    const float tot = n + nb, d = mb - mean, f = nb / tot;
    mean = fmaf(d, f, mean);
    m2 += m2b + d * d * n * f;
    n = tot;
}

// the sum of v over the workgroup, the same value in every thread: shuffles inside a wave, then the kGnBlock / 64 wave sums in wave order
__device__ __forceinline__ float block_sum(float v, float* s_w) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();                               // (the previous sum's readers are done with s_w)
    if (threadIdx.x % 64 == 0) s_w[threadIdx.x / 64] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kGnBlock / 64; ++w) s += s_w[w];
    return s;
}

// grid.x = image * groups + group
__global__ __launch_bounds__(kGnBlock) void groupnorm_generic_kernel(const GnArgs a) {
    __shared__ float s_w[kGnBlock / 64];
    const int G = a.groups, cpg = a.in.c / G;
    const int g = int(blockIdx.x) % G;
    const int64_t img = int64_t(blockIdx.x) / G;
    const int64_t elems = int64_t(a.in.h) * a.in.w * cpg;
    const int64_t ib = img * a.in.sn + int64_t(g) * cpg * a.in.sc, ob = img * a.out.sn + int64_t(g) * cpg * a.out.sc;
    auto in_at = [&](int64_t e) {
        const int64_t pix = e / cpg;
        return ib + (pix / a.in.w) * a.in.sh + (pix % a.in.w) * a.in.sw + (e % cpg) * a.in.sc;
    };
    float s = 0.f;
    for (int64_t e = threadIdx.x; e < elems; e += kGnBlock) s += ld_any(a.in.p, a.in.f16, in_at(e));
    const float mean = block_sum(s, s_w) / float(elems);
    float q = 0.f;
    for (int64_t e = threadIdx.x; e < elems; e += kGnBlock) {
        const float d = ld_any(a.in.p, a.in.f16, in_at(e)) - mean;
        q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(block_sum(q, s_w) / float(elems) + a.eps);      // (its barriers order every thread's reads before any thread's writes)
    for (int64_t e = threadIdx.x; e < elems; e += kGnBlock) {
        const int c = g * cpg + int(e % cpg);
        const float d = ld_any(a.in.p, a.in.f16, in_at(e)) - mean;
        const float o = ApplyAct(a.act, a.act_a, a.act_b, fmaf(d, a.gamma[c] * rstd, a.beta ? a.beta[c] : 0.f));
        const int64_t pix = e / cpg;
        const int64_t oi = ob + (pix / a.out.w) * a.out.sh + (pix % a.out.w) * a.out.sw + (e % cpg) * a.out.sc;
        if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
        else a.out.p[oi] = o;
    }
}

// pixels of [p0, p1) that row r of R walks: p0 + r, p0 + r + R, ...
__device__ __forceinline__ int rows_of(int npx, int r, int R) { return npx > r ? (npx - r + R - 1) / R : 0; }

// grid (slabs, images); slab_px pixels per slab; cvn = C / V channel vectors per pixel (<= kGnBlock)
template <typename T, int CPV>
__global__ __launch_bounds__(kGnBlock) void groupnorm_stats_kernel(const GnArgs a, const int slab_px, const int cvn) {
    constexpr int V = 16 / int(sizeof(T)), NG = V / CPV;
    __shared__ float s_mean[kGnBlock * NG], s_m2[kGnBlock * NG];
    const int t = int(threadIdx.x), R = kGnBlock / cvn;
    const int cvi = t % cvn, r = t / cvn;          // r >= R: an idle thread (kGnBlock is no multiple of cvn)
    const int hw = a.in.h * a.in.w;
    const int p0 = int(blockIdx.x) * slab_px, p1 = min(p0 + slab_px, hw), npx = p1 - p0;
    const T* in = reinterpret_cast<const T*>(a.in.p) + int64_t(blockIdx.y) * a.in.sn + cvi * V;

    float mean[NG], m2[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) mean[j] = m2[j] = 0.f;
    float seen = 0.f;                              // vectors merged so far: seen * CPV values per group
    if (r < R)
        for (int p = p0 + r; p < p1; p += R) {
            float x[V];
            load16<T>(in + int64_t(p) * a.in.sw, x);
            const float f = 1.f / (seen + 1.f);    // Chan with nb = CPV, n = seen * CPV: nb / (n + nb)
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                float cm = 0.f, cq = 0.f;
#pragma unroll
                for (int i = 0; i < CPV; ++i) cm += x[j * CPV + i];
                cm *= 1.f / float(CPV);
#pragma unroll
                for (int i = 0; i < CPV; ++i) { const float d = x[j * CPV + i] - cm; cq = fmaf(d, d, cq); }
                const float d = cm - mean[j];
                mean[j] = fmaf(d, f, mean[j]);
                m2[j] += cq + d * d * (seen * float(CPV)) * f;
            }
            seen += 1.f;
        }
#pragma unroll
    for (int j = 0; j < NG; ++j) { s_mean[t * NG + j] = mean[j]; s_m2[t * NG + j] = m2[j]; }
    __syncthreads();
    // the R threads of one (vector, sub-group) column, in row order; the result replaces row 0's partial (slot col, which no other column reads)
    const int cols = cvn * NG;
    for (int col = t; col < cols; col += kGnBlock) {
        const int ccv = col / NG, j = col % NG;
        float n = 0.f, mu = 0.f, q = 0.f;
        for (int rr = 0; rr < R; ++rr) {
            const int cnt = rows_of(npx, rr, R);
            if (cnt == 0) break;
            const int k = (rr * cvn + ccv) * NG + j;
            chan(n, mu, q, float(cnt * CPV), s_mean[k], s_m2[k]);
        }
        s_mean[col] = mu;
        s_m2[col] = q;
    }
    __syncthreads();
    // the columns of one group, in channel order: C / groups / V of them where a group is several vectors, else the column is the group
    const int G = a.groups, cpg = a.in.c / G, vpg = cpg > V ? cpg / V : 1;
    float* rec = a.workspace + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * G * 3;
    for (int g = t; g < G; g += kGnBlock) {
        float n = 0.f, mu = 0.f, q = 0.f;
        for (int k = 0; k < vpg; ++k) chan(n, mu, q, float(npx * CPV), s_mean[g * vpg + k], s_m2[g * vpg + k]);
        rec[g * 3 + 0] = n;
        rec[g * 3 + 1] = mu;
        rec[g * 3 + 2] = q;
    }
}

// the same grid and thread layout as the statistics launch
template <typename T, int ACT>
__global__ __launch_bounds__(kGnBlock) void groupnorm_apply_kernel(const GnArgs a, const int slab_px, const int cvn) {
    constexpr int V = 16 / int(sizeof(T));
    __shared__ float s_mean[kGnMaxVectors * 8], s_rstd[kGnMaxVectors * 8];      // per group (groups <= C <= kGnMaxVectors * V)
    __shared__ float s_pn[kGnBlock], s_pm[kGnBlock], s_pq[kGnBlock];
    const int t = int(threadIdx.x), R = kGnBlock / cvn;
    const int cvi = t % cvn, r = t / cvn;
    const int G = a.groups, cpg = a.in.c / G, slabs = int(gridDim.x);
    const float* rec = a.workspace + int64_t(blockIdx.y) * slabs * G * 3;
    // P threads per group (a power of two), each over a contiguous run of slabs in slab order, then the P partials in order: the same order in
    // every workgroup of the image, so all of them get the same bits
    int P = 1;
    while (P < 16 && 2 * P * G <= kGnBlock) P *= 2;
    const int run = (slabs + P - 1) / P, part = t % P;
    for (int g0 = 0; g0 < G; g0 += kGnBlock / P) {       // (uniform bounds: every thread meets the barriers)
        const int g = g0 + t / P;
        float n = 0.f, mu = 0.f, q = 0.f;
        if (g < G)
            for (int s = part * run; s < min(slabs, (part + 1) * run); ++s) {
                const float* rs = rec + (int64_t(s) * G + g) * 3;
                chan(n, mu, q, rs[0], rs[1], rs[2]);
            }
        s_pn[t] = n; s_pm[t] = mu; s_pq[t] = q;
        __syncthreads();
        if (g < G && part == 0) {
            n = mu = q = 0.f;
            for (int k = 0; k < P; ++k)
                if (s_pn[t + k] > 0.f) chan(n, mu, q, s_pn[t + k], s_pm[t + k], s_pq[t + k]);
            s_mean[g] = mu;
            s_rstd[g] = 1.f / sqrtf(q / n + a.eps);
        }
        __syncthreads();
    }
    if (r >= R) return;
    float mu[V], av[V], bv[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = cvi * V + i, g = c / cpg;
        mu[i] = s_mean[g];
        av[i] = a.gamma[c] * s_rstd[g];
        bv[i] = a.beta ? a.beta[c] : 0.f;
    }
    const int hw = a.in.h * a.in.w;
    const int p0 = int(blockIdx.x) * slab_px, p1 = min(p0 + slab_px, hw);
    const T* in = reinterpret_cast<const T*>(a.in.p) + int64_t(blockIdx.y) * a.in.sn + cvi * V;
    T* out = reinterpret_cast<T*>(a.out.p) + int64_t(blockIdx.y) * a.out.sn + cvi * V;
    for (int p = p0 + r; p < p1; p += R) {
        float x[V];
        load16<T>(in + int64_t(p) * a.in.sw, x);
#pragma unroll
        for (int i = 0; i < V; ++i) x[i] = ApplyAct(ACT, 0.f, 0.f, fmaf(x[i] - mu[i], av[i], bv[i]));
        store16<T>(out + int64_t(p) * a.out.sw, x);
    }
}

// stricter than VecViewOk: tile 1 walks the h * w pixels of an image one pitch apart, so no gap between the rows of an image
bool image_dense(const TensorArg& t) { return t.sh == int64_t(t.w) * t.sw; }

template <typename T, int CPV>
void launch_stats_cpv(const GnArgs& a, dim3 grid, int slab_px, int cvn, hipStream_t stream) {
    groupnorm_stats_kernel<T, CPV><<<grid, dim3(kGnBlock), 0, stream>>>(a, slab_px, cvn);
}

template <typename T>
hipError_t launch_stats(const GnArgs& a, dim3 grid, int slab_px, int cvn, hipStream_t stream) {
    constexpr int V = 16 / int(sizeof(T));
    const int cpg = a.in.c / a.groups, cpv = cpg < V ? cpg : V;
    if (cpv == 1) launch_stats_cpv<T, 1>(a, grid, slab_px, cvn, stream);
    else if (cpv == 2) launch_stats_cpv<T, 2>(a, grid, slab_px, cvn, stream);
    else if (cpv == 4) launch_stats_cpv<T, 4>(a, grid, slab_px, cvn, stream);
    else if (cpv == V) launch_stats_cpv<T, V>(a, grid, slab_px, cvn, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T>
hipError_t launch_apply(const GnArgs& a, dim3 grid, int slab_px, int cvn, hipStream_t stream) {
    switch (a.act) {
        case 0: groupnorm_apply_kernel<T, 0><<<grid, dim3(kGnBlock), 0, stream>>>(a, slab_px, cvn); break;
        case 1: groupnorm_apply_kernel<T, 1><<<grid, dim3(kGnBlock), 0, stream>>>(a, slab_px, cvn); break;
        case 3: groupnorm_apply_kernel<T, 3><<<grid, dim3(kGnBlock), 0, stream>>>(a, slab_px, cvn); break;
        case 5: groupnorm_apply_kernel<T, 5><<<grid, dim3(kGnBlock), 0, stream>>>(a, slab_px, cvn); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

bool GroupNormEligible(const GnArgs& a, int tile) {
    if (tile < 0 || tile >= kNumGnTiles || !a.in.p || !a.out.p || !a.gamma) return false;
    if (a.in.f8 || a.out.f8 || a.in.c < 1 || a.groups < 1 || a.in.c % a.groups || a.in.c != a.out.c || a.in.n != a.out.n || a.in.h != a.out.h || a.in.w != a.out.w) return false;
    if (int64_t(a.in.n) * a.groups >= (int64_t(1) << 31)) return false;
    if (tile == 0) return true;
    const int V = a.out.f16 ? 8 : 4;
    const int64_t hw = int64_t(a.in.h) * a.in.w;
    return GnTileFits(a.in.c, a.groups, a.out.f16 != 0, a.in.sw, 0, a.out.sw, 0, a.act, tile) && a.in.f16 == a.out.f16 && VecViewOk(a.in, V) && image_dense(a.in) &&
           VecViewOk(a.out, V) && image_dense(a.out) && hw < (int64_t(1) << 31) && a.in.n <= 65535 && a.workspace &&
           a.workspace_floats >= GnWorkspaceFloats(a.in.n, hw, a.in.c, a.groups, a.out.f16 != 0);
}

hipError_t LaunchGroupNormPhase(const GnArgs& a, int phase, hipStream_t stream) {
    if (!GroupNormEligible(a, 1) || phase < 0 || phase > 1) return hipErrorInvalidValue;
    const int64_t hw = int64_t(a.in.h) * a.in.w;
    if (hw == 0 || a.in.n == 0) return hipSuccess;
    const bool f16 = a.out.f16 != 0;
    const int cvn = a.in.c / (f16 ? 8 : 4), slab_px = int(GnSlabPixels(a.in.n, hw, a.in.c, f16));
    const dim3 grid(unsigned(GnSlabs(a.in.n, hw, a.in.c, f16)), unsigned(a.in.n));
    if (phase == 0) return f16 ? launch_stats<_Float16>(a, grid, slab_px, cvn, stream) : launch_stats<float>(a, grid, slab_px, cvn, stream);
    return f16 ? launch_apply<_Float16>(a, grid, slab_px, cvn, stream) : launch_apply<float>(a, grid, slab_px, cvn, stream);
}

hipError_t LaunchGroupNorm(const GnArgs& a, int tile, hipStream_t stream) {
    if (!GroupNormEligible(a, tile)) return hipErrorInvalidValue;
    if (int64_t(a.in.n) * a.in.h * a.in.w == 0) return hipSuccess;
    if (tile == 0) {
        hipLaunchKernelGGL(groupnorm_generic_kernel, dim3(unsigned(a.in.n * a.groups)), dim3(kGnBlock), 0, stream, a);
        return hipGetLastError();
    }
    if (const hipError_t e = LaunchGroupNormPhase(a, 0, stream); e != hipSuccess) return e;
    return LaunchGroupNormPhase(a, 1, stream);
}

}  // namespace ie
