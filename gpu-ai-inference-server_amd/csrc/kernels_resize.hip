// Resize / Upsample (ONNX) on gfx950: the segmentation heads' upsampling and the ASPP pooling branch's broadcast.
//
// out(n, c, y, x) = interpolation of in(n, c, ., .) at the source coordinate of (y, x), separately per axis.  Memory-bound: a few FLOPs per
// element against 2-4 bytes read (mostly from L2: an upsampled map re-reads each source pixel many times) and 2-4 bytes written.  fp32
// interpolation math for both element types; the source coordinate is computed once per output row / column in double from the ONNX formulas
// (the kernels are nowhere near the FP64 rate), so nearest-pixel ties break exactly as in the specification's reference.  Deterministic: every
// output element is written once by one lane, no atomics, no LDS, no scratch.
//
//   resize_vec_kernel<T>     NHWC -> NHWC, one lane per 16-byte channel vector (4 floats / 8 halfs), lanes of a wave along C then W:
//                            loads and stores coalesced along C.  Needs C, both pitches and channel offsets multiples of the vector width.
//   resize_nchw_kernel<T>    NHWC -> the dense NCHW fp32 graph output: one lane per output pixel, looping over the channels, so for each
//                            channel the lanes of a wave store consecutive x (coalesced along W).  Any C (21 classes is the common case).
//   resize_generic_kernel    one thread per output element in the output's own order; anything the two above decline.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kResizeBlock = 256;

// Source coordinate of output index `o` along an axis of `in_len` -> `out_len` (ResizeCoord), ONNX Resize-13/19
__device__ inline double src_coord(int coord, int o, int in_len, int out_len, double scale) {
    switch (coord) {
        case 1: return out_len > 1 ? (double(o) + 0.5) / scale - 0.5 : 0.0;                       // pytorch_half_pixel
        case 2: return out_len > 1 ? double(o) * double(in_len - 1) / double(out_len - 1) : 0.0;  // align_corners
        case 3: return double(o) / scale;                                                            // asymmetric
        default: return (double(o) + 0.5) / scale - 0.5;                                            // half_pixel
    }
}

// One axis of one output index: nearest -> (i0, i0, w = 0); linear -> (i0, i1, w) with value = (1 - w) * in[i0] + w * in[i1]
struct Tap { int i0, i1; float w; };
__device__ inline Tap axis_tap(const ResizeArgs& a, int o, int in_len, int out_len, double scale) {
    const double x = src_coord(a.coord, o, in_len, out_len, scale);
    Tap t;
    if (a.mode == 0) {
        double r;
        switch (a.nearest) {
            case 1: r = (x == floor(x) + 0.5) ? ceil(x) : rint(x); break;      // round_prefer_ceil
            case 2: r = floor(x); break;
            case 3: r = ceil(x); break;
            default: r = (x == floor(x) + 0.5) ? floor(x) : rint(x); break;    // round_prefer_floor
        }
        const int i = int(fmin(fmax(r, 0.0), double(in_len - 1)));
        t.i0 = t.i1 = i;
        t.w = 0.f;
    } else {
        const double f = floor(x);
        const int i = int(f);
        t.w = float(x - f);
        t.i0 = min(max(i, 0), in_len - 1);
        t.i1 = min(max(i + 1, 0), in_len - 1);
    }
    return t;
}

__device__ inline float ld1(const float* p, int f16, int64_t i) { return f16 ? float(reinterpret_cast<const _Float16*>(p)[i]) : p[i]; }
__device__ inline void st1(float* p, int f16, int64_t i, float v) {
    if (f16) reinterpret_cast<_Float16*>(p)[i] = _Float16(v);
    else p[i] = v;
}

__global__ __launch_bounds__(kResizeBlock) void resize_generic_kernel(const ResizeArgs a, const int out_nchw, const int64_t total) {
    const int64_t idx = int64_t(blockIdx.x) * kResizeBlock + threadIdx.x;
    if (idx >= total) return;
    const int C = a.out.c, OH = a.out.h, OW = a.out.w;
    int n, c, y, x;
    int64_t m = idx;
    if (out_nchw) { x = int(m % OW); m /= OW; y = int(m % OH); m /= OH; c = int(m % C); n = int(m / C); }
    else { c = int(m % C); m /= C; x = int(m % OW); m /= OW; y = int(m % OH); n = int(m / OH); }
    const Tap ty = axis_tap(a, y, a.in.h, OH, a.scale_h), tx = axis_tap(a, x, a.in.w, OW, a.scale_w);
    const int64_t base = int64_t(n) * a.in.sn + int64_t(c) * a.in.sc;
    const float v00 = ld1(a.in.p, a.in.f16, base + ty.i0 * a.in.sh + tx.i0 * a.in.sw);
    float v = v00;
    if (a.mode != 0) {
        const float v01 = ld1(a.in.p, a.in.f16, base + ty.i0 * a.in.sh + tx.i1 * a.in.sw);
        const float v10 = ld1(a.in.p, a.in.f16, base + ty.i1 * a.in.sh + tx.i0 * a.in.sw);
        const float v11 = ld1(a.in.p, a.in.f16, base + ty.i1 * a.in.sh + tx.i1 * a.in.sw);
        const float top = v00 + tx.w * (v01 - v00), bot = v10 + tx.w * (v11 - v10);
        v = top + ty.w * (bot - top);
    }
    st1(a.out.p, a.out.f16, int64_t(n) * a.out.sn + int64_t(y) * a.out.sh + int64_t(x) * a.out.sw + int64_t(c) * a.out.sc, v);
}

// 16 bytes of T as 4 floats (fp32) or 8 floats (half)
template <typename T> struct Vec;
template <> struct Vec<float> {
    static constexpr int V = 4;
    typedef f32x4 v_t;
};
template <> struct Vec<_Float16> {
    static constexpr int V = 8;
    typedef h8 v_t;
};

template <typename T>
__global__ __launch_bounds__(kResizeBlock) void resize_vec_kernel(const ResizeArgs a, const int64_t total) {
    constexpr int V = Vec<T>::V;
    typedef typename Vec<T>::v_t v_t;
    typedef float f_t __attribute__((ext_vector_type(V)));
    const int64_t idx = int64_t(blockIdx.x) * kResizeBlock + threadIdx.x;
    if (idx >= total) return;
    const int CV = a.out.c / V, OH = a.out.h, OW = a.out.w;
    int64_t m = idx;
    const int cv = int(m % CV); m /= CV;
    const int x = int(m % OW); m /= OW;
    const int y = int(m % OH);
    const int n = int(m / OH);
    const Tap ty = axis_tap(a, y, a.in.h, OH, a.scale_h), tx = axis_tap(a, x, a.in.w, OW, a.scale_w);
    const T* in = reinterpret_cast<const T*>(a.in.p) + int64_t(n) * a.in.sn + cv * V;
    f_t v = __builtin_convertvector(*reinterpret_cast<const v_t*>(in + ty.i0 * a.in.sh + tx.i0 * a.in.sw), f_t);
    if (a.mode != 0) {
        const f_t v01 = __builtin_convertvector(*reinterpret_cast<const v_t*>(in + ty.i0 * a.in.sh + tx.i1 * a.in.sw), f_t);
        const f_t v10 = __builtin_convertvector(*reinterpret_cast<const v_t*>(in + ty.i1 * a.in.sh + tx.i0 * a.in.sw), f_t);
        const f_t v11 = __builtin_convertvector(*reinterpret_cast<const v_t*>(in + ty.i1 * a.in.sh + tx.i1 * a.in.sw), f_t);
        const f_t top = v + tx.w * (v01 - v), bot = v10 + tx.w * (v11 - v10);
        v = top + ty.w * (bot - top);
    }
    T* out = reinterpret_cast<T*>(a.out.p) + int64_t(n) * a.out.sn + int64_t(y) * a.out.sh + int64_t(x) * a.out.sw + cv * V;
    *reinterpret_cast<v_t*>(out) = __builtin_convertvector(v, v_t);
}

template <typename T>
__global__ __launch_bounds__(kResizeBlock) void resize_nchw_kernel(const ResizeArgs a, const int64_t total) {
    const int64_t idx = int64_t(blockIdx.x) * kResizeBlock + threadIdx.x;
    if (idx >= total) return;
    const int C = a.out.c, OH = a.out.h, OW = a.out.w;
    int64_t m = idx;
    const int x = int(m % OW); m /= OW;
    const int y = int(m % OH);
    const int n = int(m / OH);
    const Tap ty = axis_tap(a, y, a.in.h, OH, a.scale_h), tx = axis_tap(a, x, a.in.w, OW, a.scale_w);
    const T* in = reinterpret_cast<const T*>(a.in.p) + int64_t(n) * a.in.sn;
    const int64_t o00 = ty.i0 * a.in.sh + tx.i0 * a.in.sw, o01 = ty.i0 * a.in.sh + tx.i1 * a.in.sw;
    const int64_t o10 = ty.i1 * a.in.sh + tx.i0 * a.in.sw, o11 = ty.i1 * a.in.sh + tx.i1 * a.in.sw;
    float* out = a.out.p + int64_t(n) * a.out.sn + int64_t(y) * a.out.sh + x;
    if (a.mode == 0) {
        for (int c = 0; c < C; ++c) out[int64_t(c) * a.out.sc] = float(in[o00 + c]);
    } else {
        for (int c = 0; c < C; ++c) {
            const float v00 = float(in[o00 + c]), v01 = float(in[o01 + c]), v10 = float(in[o10 + c]), v11 = float(in[o11 + c]);
            const float top = v00 + tx.w * (v01 - v00), bot = v10 + tx.w * (v11 - v10);
            out[int64_t(c) * a.out.sc] = top + ty.w * (bot - top);
        }
    }
}

}  // namespace

int ResizePath(const ResizeArgs& a) {
    if (a.in.sc != 1 || a.in.f8 || a.out.f8) return 0;
    if (a.out.sc != 1) return !a.out.f16 && a.out.sw == 1 && a.out.sh == a.out.w && a.out.sc == int64_t(a.out.h) * a.out.w ? 2 : 0;   // dense NCHW
    if (a.in.f16 != a.out.f16) return 0;
    const int V = a.in.f16 ? 8 : 4;
    const bool ok = a.in.c % V == 0 && a.in.sw % V == 0 && a.in.sh % V == 0 && a.in.sn % V == 0 && a.out.sw % V == 0 && a.out.sh % V == 0 &&
                    a.out.sn % V == 0 && Aligned16(a.in.p) && Aligned16(a.out.p);
    return ok ? 1 : 0;
}

hipError_t LaunchResize(const ResizeArgs& a, int path, hipStream_t stream) {
    if (a.in.n != a.out.n || a.in.c != a.out.c || a.in.h < 1 || a.in.w < 1 || a.in.f8 || a.out.f8) return hipErrorInvalidValue;
    if (!(a.scale_h > 0.0) || !(a.scale_w > 0.0)) return hipErrorInvalidValue;
    const int64_t pixels = int64_t(a.out.n) * a.out.h * a.out.w;
    if (pixels == 0 || a.out.c == 0) return hipSuccess;
    if (path == 1) {
        if (ResizePath(a) != 1) return hipErrorInvalidValue;
        const int V = a.in.f16 ? 8 : 4;
        const int64_t total = pixels * (a.out.c / V);
        const int64_t blocks = (total + kResizeBlock - 1) / kResizeBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.in.f16) resize_vec_kernel<_Float16><<<dim3(unsigned(blocks)), dim3(kResizeBlock), 0, stream>>>(a, total);
        else resize_vec_kernel<float><<<dim3(unsigned(blocks)), dim3(kResizeBlock), 0, stream>>>(a, total);
        return hipGetLastError();
    }
    if (path == 2) {
        if (ResizePath(a) != 2) return hipErrorInvalidValue;
        const int64_t blocks = (pixels + kResizeBlock - 1) / kResizeBlock;
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.in.f16) resize_nchw_kernel<_Float16><<<dim3(unsigned(blocks)), dim3(kResizeBlock), 0, stream>>>(a, pixels);
        else resize_nchw_kernel<float><<<dim3(unsigned(blocks)), dim3(kResizeBlock), 0, stream>>>(a, pixels);
        return hipGetLastError();
    }
    if (path != 0) return hipErrorInvalidValue;
    const int64_t total = pixels * a.out.c;
    const int64_t blocks = (total + kResizeBlock - 1) / kResizeBlock;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const int out_nchw = a.out.sc != 1;
    resize_generic_kernel<<<dim3(unsigned(blocks)), dim3(kResizeBlock), 0, stream>>>(a, out_nchw, total);
    return hipGetLastError();
}

}  // namespace ie
