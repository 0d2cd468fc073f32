// What the MFMA attention kernels share (included by kernels_attn.hip, kernels_wattn.hip and kernels_decode.hip only): the constants of the masked
// softmax, the rotary embedding of a 16-byte vector, and AttnWave, the state and the steps of one wave of 32 queries over key tiles of 32.
//
// Operand orientation.  The scores are computed swapped, S^T = K . Q^T: the MFMA's A operand is the K tile (row = key), its B operand
// Q^T (column = query), so in the 32x32 result (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) a lane owns ONE query column and
// 16 of its 32 keys; the other 16 sit in lane ^ 32.  Row maximum and sum are 15 in-lane operations and one exchange with lane ^ 32.  The second
// product is O^T += V^T . P^T, which sums over P^T's row index: the probabilities feed it as the B operand from the registers they are in.
// The reduction index of a product may be walked in any order as long as both operands agree:
//   QK^T   lane half hf supplies the head-dim elements hf * HD/2 ... of its Q row and of its K row: whole 16-byte vectors on both sides
//   PV     fp32 (32x32x2): register r is one k-step: keys (r & 3) + 8 (r >> 2) in lane half 0 and that + 4 in lane half 1, and the A operand is V at
//          that key.  fp16 (32x32x16): registers 8 s ... 8 s + 7 as halfs are k-step s; element j of lane half hf is key
//          16 s + 8 (j >> 2) + 4 hf + (j & 3), and the V fragment is gathered in the same order (scripts/probes/attn_pv_order.hip checks both maps
//          with exact integers).
#pragma once
#include "device_util.h"

namespace ie {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kFltMax = 3.402823466e+38f;
constexpr float kMaskShiftMax = 16777216.f;      // 2^24: the largest key bias that is taken out of every score of an image (kernels_attn.hip MASK)

// One 16-byte vector of a q / k row after the rotary embedding: x = the vector (elements e0 ...), xp = its partner vector (elements e0 +/- HD/2 ...),
// c / s = the cos / sin entries e0 ... of the token position's table row, sg = -1 for a vector of the first half of the head, +1 for one of the second.
// fp32 arithmetic; halfs are rounded once, here.  rope_rot: the table entries are in registers already, c / s = the V / 4 float4s of the vector's
// cos / sin entries (tile 2 loads them a tile ahead); rope_vec loads them from the table row
template <typename T>
__device__ __forceinline__ uint4 rope_rot(uint4 x, uint4 xp, const float4* c, const float4* s, float sg) {
    const float4 c0 = c[0], s0 = s[0];
    if constexpr (sizeof(T) == 2) {
        const float4 c1 = c[1], s1 = s[1];
        const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const h8 a = __builtin_bit_cast(h8, x), b = __builtin_bit_cast(h8, xp);
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = _Float16(fmaf(float(a[j]), cc[j], sg * float(b[j]) * ss[j]));
        return __builtin_bit_cast(uint4, o);
    } else {
        const float4 a = __builtin_bit_cast(float4, x), b = __builtin_bit_cast(float4, xp);
        return __builtin_bit_cast(uint4, make_float4(fmaf(a.x, c0.x, sg * b.x * s0.x), fmaf(a.y, c0.y, sg * b.y * s0.y), fmaf(a.z, c0.z, sg * b.z * s0.z),
                                                     fmaf(a.w, c0.w, sg * b.w * s0.w)));
    }
}

template <typename T>
__device__ __forceinline__ uint4 rope_vec(uint4 x, uint4 xp, const float* c, const float* s, float sg) {
    float4 cv[2], sv[2];
    cv[0] = *reinterpret_cast<const float4*>(c);
    sv[0] = *reinterpret_cast<const float4*>(s);
    if constexpr (sizeof(T) == 2) {
        cv[1] = *reinterpret_cast<const float4*>(c + 4);
        sv[1] = *reinterpret_cast<const float4*>(s + 4);
    }
    return rope_rot<T>(x, xp, cv, sv, sg);
}

// What a wave carries through its key tiles: its lane's half of its Q row, the O^T accumulators (o1: HD == 64 only) and the softmax statistics of its
// query.  col = lane & 31 is the lane's query column (and its K row in QK^T, its V column in PV), hf = lane >> 5 its lane half; Kt / Vt are the LDS
// rows of a tile's first key, RS their stride in elements
template <typename T, int HD>
struct AttnWave {
    static constexpr bool F16 = sizeof(T) == 2;
    static constexpr int HH = HD / 2;              // head-dim elements one lane half supplies to QK^T
    float4 q4[F16 ? 1 : HH / 4];
    h8 q8[F16 ? HH / 8 : 1];
    f32x16 o0, o1;
    float m, lsum;

    // m0: -inf where every tile a wave visits holds a visible key for each of its queries (key_tile), -FLT_MAX where a tile may hold none
    __device__ __forceinline__ void reset(float m0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
        m = m0;
        lsum = 0.f;
    }

    // qrow = this lane's half of its Q row
    __device__ __forceinline__ void init(const T* qrow, float m0) {
        if constexpr (F16) {
#pragma unroll
            for (int k = 0; k < HH / 8; ++k) q8[k] = *reinterpret_cast<const h8*>(qrow + 8 * k);
        } else {
#pragma unroll
            for (int k = 0; k < HH / 4; ++k) q4[k] = *reinterpret_cast<const float4*>(qrow + 4 * k);
        }
        reset(m0);
    }

    // init with the rotary embedding: qhead = element 0 of the head's Q row, cr / sr = the cos / sin table rows of its token position.  The lane halves
    // are exactly the two rope halves: lane half hf rotates its half with the other half as the partner
    __device__ __forceinline__ void init_rope(const T* qhead, int hf, const float* cr, const float* sr, float m0) {
        constexpr int V = 16 / int(sizeof(T));
        const T* mine = qhead + hf * HH;
        const T* other = qhead + (1 - hf) * HH;
        const float sg = hf ? 1.f : -1.f;
#pragma unroll
        for (int k = 0; k < HH / V; ++k) {
            const uint4 r = rope_vec<T>(*reinterpret_cast<const uint4*>(mine + V * k), *reinterpret_cast<const uint4*>(other + V * k), cr + hf * HH + V * k,
                                        sr + hf * HH + V * k, sg);
            if constexpr (F16) q8[k] = __builtin_bit_cast(h8, r);
            else q4[k] = __builtin_bit_cast(float4, r);
        }
        reset(m0);
    }

    // S^T of one tile of 32 keys: register r of the result is the raw score of key (r & 3) + 8 (r >> 2) + 4 hf of the tile
    template <int RS>
    __device__ __forceinline__ f32x16 qk_tile(const T* Kt, int col, int hf) const {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const T* krow = Kt + col * RS + hf * HH;
        if constexpr (F16) {
#pragma unroll
            for (int k = 0; k < HH; k += 8)
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const h8*>(krow + k), q8[k / 8], s, 0, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < HH; k += 4) {
                const float4 kf = *reinterpret_cast<const float4*>(krow + k);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, q4[k / 4].x, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, q4[k / 4].y, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, q4[k / 4].z, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, q4[k / 4].w, s, 0, 0, 0);
            }
        }
        return s;
    }

    // The online softmax on a tile's 16 scores of this lane (units of log2, hidden keys at -inf): m and lsum move on, O is rescaled by exp2(m - m')
    // and the probabilities are left in s.  The new maximum must be finite, or exp2(-inf - -inf) is NaN: the caller either starts m at -FLT_MAX or
    // shows every query a key in every tile
    __device__ __forceinline__ void softmax_update(f32x16& s) {
        float mx = -__builtin_huge_valf();
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = fast_exp2(m - mn);     // 0 on the first tile of a wave that started at m = -inf
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = fast_exp2(s[r] - mn);
            ps += s[r];
            o0[r] *= alpha;
            if constexpr (HD == 64) o1[r] *= alpha;
        }
        lsum = fmaf(lsum, alpha, ps);              // this lane half's share of the row sum
    }

    // O^T += V^T . P^T of one tile, p = the probabilities in the registers the scores came in
    template <int RS>
    __device__ __forceinline__ void pv_tile(const T* Vt, const f32x16& p, int col, int hf) {
        if constexpr (F16) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                h8 pb, va0, va1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kt = 16 * st + 8 * (j >> 2) + 4 * hf + (j & 3);
                    pb[j] = _Float16(p[8 * st + j]);
                    va0[j] = Vt[kt * RS + col];
                    if constexpr (HD == 64) va1[j] = Vt[kt * RS + 32 + col];
                }
                o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va0, pb, o0, 0, 0, 0);
                if constexpr (HD == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va1, pb, o1, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kt = (r & 3) + 8 * (r >> 2) + 4 * hf;
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(float(Vt[kt * RS + col]), p[r], o0, 0, 0, 0);
                if constexpr (HD == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(float(Vt[kt * RS + 32 + col]), p[r], o1, 0, 0, 0);
            }
        }
    }

    // One tile of 32 keys.  rule(kt, raw) is the caller's score of the tile's key kt for this lane's query, in units of log2: the scaled raw score
    // with whatever bias the kernel has, -inf for a key the query does not see
    template <int RS, typename Rule>
    __device__ __forceinline__ void key_tile(const T* Kt, const T* Vt, int col, int hf, Rule rule) {
        f32x16 s = qk_tile<RS>(Kt, col, hf);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = rule((r & 3) + 8 * (r >> 2) + 4 * hf, s[r]);
        softmax_update(s);
        pv_tile<RS>(Vt, s, col, hf);
    }

    // O / l of this lane's query into its output row (columns h HD ...): registers 4 g ... 4 g + 3 of o0 (o1: + 32) are the output columns
    // 8 g + 4 hf ... of the query.  lsum holds the whole row sum by now (the caller has added the two lane halves)
    __device__ __forceinline__ void store(T* orow, int hf) const {
        const float inv = 1.f / lsum;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int e0 = 8 * g + 4 * hf;
            if constexpr (F16) {
                h4 x, y;
#pragma unroll
                for (int t = 0; t < 4; ++t) { x[t] = _Float16(o0[4 * g + t] * inv); y[t] = _Float16(o1[4 * g + t] * inv); }
                *reinterpret_cast<h4*>(orow + e0) = x;
                if constexpr (HD == 64) *reinterpret_cast<h4*>(orow + 32 + e0) = y;
            } else {
                *reinterpret_cast<float4*>(orow + e0) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
                if constexpr (HD == 64)
                    *reinterpret_cast<float4*>(orow + 32 + e0) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
            }
        }
    }
};

}  // namespace ie
