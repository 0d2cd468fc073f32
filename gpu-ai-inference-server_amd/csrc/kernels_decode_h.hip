// The half-precision resident KV cache on gfx950: the kernels that exist only for a cache whose K and V are IEEE half, dense
// [N][Hkv][cache_rows][hd] like the fp32 one (kernels.h DecodeArgs::cache_f16; the typed pointers of DecodeArgs then address halfs).  Such a cache is
// resident (in place) and serves half activations only, so every kernel here is the in-place form for T = half.  Tile 0 and tile 5 over a
// half cache are forms of kernels_decode.hip's own kernels (the wave and the MFMA tile do not change, only what they read), and the combine launch
// behind tile 4 is that file's too.
//
//   kv_convert_kernel<TO_HALF>           EngineKvCacheWrite / Read on a half cache: fp32 staging -> half (round to nearest even, NaN stays NaN) and back (exact).
//   kv_append_rows_h_kernel<V>           one lane per V consecutive halfs of the step's new rows (V = 8: 16 bytes; 4: a head dim that is no multiple of 8;
//                                        1: none of 4).  v is copied as the half it is; k is rotated in fp32 (kv_append_kernel's arithmetic) and rounded once.
//   attention_decode_h_kernel<HD, G>     tile 4.  The workgroup is tile 4's: (image, K / V head, key split s of S), four waves.  A key row is HD / 8 lanes of
//                                        16 bytes, so a wave takes 512 / HD keys and the workgroup 2048 / HD contiguous keys per iteration: twice tile
//                                        4's key tile from the same number of bytes in flight.  The lane's slice of the g <= G query rows is four packed
//                                        half2 registers per head, rounded after the fp32 rotation as tile 5 rounds its q, and q.k is four v_dot2 with an
//                                        fp32 accumulator, reduced over the HD / 8 lanes of the key; the scale is applied to the fp32 score.  The online
//                                        softmax is fp32 per key slot and head; o is eight fp32 per head, updated by fma(p, float(v_e), o al) straight
//                                        from the packed V register.  The prologue runs once per workgroup: one thread per element rotates the g query
//                                        rows (and, in the owning split, the new k row) and ROUNDS them to half into LDS, from which every lane takes its
//                                        16-byte slices; the owning split stores the rounded new row at row len and attends to it as stored: the step
//                                        sees what every later step will read.  A split without keys writes its records and leaves before the prologue.
//                                        Merge: tile 4 keeps a record per key slot in LDS, which with 64 slots (hd 32) and G = 8 would be 64 KiB.  Here the
//                                        512 / HD slots of a wave meet first, in registers, by a butterfly over the lane bits above the key's lanes (fixed
//                                        order: bit-identical from run to run), and four wave records go to LDS: 16 KiB at hd 128, G = 8, whatever the slots.
// The rules of tile 4 hold unchanged: the next iteration's K / V vectors are requested before this iteration's arithmetic; no workgroup reads a row at or
// beyond len; a split without keys writes (-FLT_MAX, 0, 0); S == 1 writes the token row, S > 1 the records attention_decode_combine_kernel adds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_mfma.h"
#include "decode_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

template <bool TO_HALF>
__global__ __launch_bounds__(kDecodeBlock) void kv_convert_kernel(const void* src, void* dst, const int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * kDecodeBlock + threadIdx.x;
    if (i >= n) return;
    if constexpr (TO_HALF) static_cast<_Float16*>(dst)[i] = _Float16(static_cast<const float*>(src)[i]);
    else static_cast<float*>(dst)[i] = float(static_cast<const _Float16*>(src)[i]);
}

template <int V>
__global__ __launch_bounds__(kDecodeBlock) void kv_append_rows_h_kernel(const DecodeArgs a, const int64_t total) {
    const int64_t i = int64_t(blockIdx.x) * kDecodeBlock + threadIdx.x;      // ((n Hkv + kvh) new_len + l) hd / V + ev
    if (i >= total) return;
    const int hd = a.head_dim, vpr = hd / V;
    const int ev = int(i % vpr);
    const int l = int((i / vpr) % a.new_len);
    const int64_t nh = i / (int64_t(vpr) * a.new_len);      // n Hkv + kvh
    const int kvh = int(nh % a.kv_heads);
    const int64_t n = nh / a.kv_heads;
    const Resident rs = resident(a, n);
    if (l >= rs.c) return;
    const int64_t o = (nh * a.cache_rows + rs.len + l) * hd + int64_t(ev) * V;
    const bool rope = a.rope_cos != nullptr;
    const int64_t r = rope ? rope_row(a, n, l) : 0;
    const int64_t kb = qkv_base(a, n, l, 1, kvh), vb = qkv_base(a, n, l, 2, kvh);
    typedef _Float16 hv __attribute__((ext_vector_type(V)));
    hv k, v;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        k[j] = _Float16(rotated<_Float16>(a, kb, r, ev * V + j, rope));
        v[j] = reinterpret_cast<const _Float16*>(a.in.p)[vb + int64_t(ev * V + j) * a.in.sc];
    }
    *reinterpret_cast<hv*>(reinterpret_cast<_Float16*>(a.present_k) + o) = k;
    *reinterpret_cast<hv*>(reinterpret_cast<_Float16*>(a.present_v) + o) = v;
}

struct H2x4 { h2 v[4]; };

// eight products of a lane's q slice and a K vector: four v_dot2_f32_f16 on one fp32 accumulator
__device__ __forceinline__ float dot8(const h2 (&q)[4], const h8 k) {
    const H2x4 kk = __builtin_bit_cast(H2x4, k);
    float s = __builtin_amdgcn_fdot2(q[0], kk.v[0], 0.f, false);
    s = __builtin_amdgcn_fdot2(q[1], kk.v[1], s, false);
    s = __builtin_amdgcn_fdot2(q[2], kk.v[2], s, false);
    return __builtin_amdgcn_fdot2(q[3], kk.v[3], s, false);
}

// grid = (splits, Hkv, N), as tile 4's in-place form (kernels_decode.hip attention_decode_kernel): the S splits share the image's len cached keys in whole
// key tiles of KT at run time
template <int HD, int G>
__global__ __launch_bounds__(kDecodeBlock) void attention_decode_h_kernel(const DecodeArgs a) {
    constexpr int LPK = HD / 8;                    // lanes of one key row
    constexpr int KPW = 64 / LPK;                  // key slots of a wave
    constexpr int KT = 4 * KPW;                    // keys of the workgroup per iteration (kernels.h DecodeKeyTileHalf)
    static_assert(KT == DecodeKeyTileHalf(HD), "kernels.h DecodeKeyTileHalf");
    __shared__ float s_ml[4][G][2];
    __shared__ float s_o[4][G][HD];
    __shared__ __attribute__((aligned(16))) _Float16 s_q[G + 2][HD];      // the g rotated query rows; rows G, G + 1: the new k and v row (owning split)
    const int S = int(gridDim.x), sp = int(blockIdx.x), kvh = int(blockIdx.y);
    const int64_t n = blockIdx.z;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    const int sub = lane / LPK, el = lane % LPK, slot = wave * KPW + sub;
    const int g = a.heads / a.kv_heads;
    const Resident rs = resident(a, n);
    const int P = rs.len;                          // the cached keys alone, the new one comes from registers below
    const int tiles = (P + KT - 1) / KT, per = (tiles + S - 1) / S;
    const int k0 = sp * per * KT, k1 = min(P, (sp + 1) * per * KT);      // this split's keys (none where per * S overshoots)
    const int owner = tiles > 0 ? (tiles - 1) / per : S - 1;      // the split that holds the last cached key (none cached: the last split) owns the new row
    if (k0 >= k1 && sp != owner) {                 // workgroup-uniform: a split without keys (S > 1) leaves its records before any prologue
        for (int idx = int(threadIdx.x); idx < g * HD; idx += kDecodeBlock) {
            float* rec = a.workspace + ((n * a.heads + kvh * g + idx / HD) * S + sp) * int64_t(HD + 2);
            if (idx % HD == 0) { rec[0] = -kFltMax; rec[1] = 0.f; }
            rec[2 + idx % HD] = 0.f;
        }
        return;
    }
    const int64_t nh = n * a.kv_heads + kvh;
    const _Float16* pk = reinterpret_cast<const _Float16*>(a.past_k) + nh * a.cache_rows * HD;
    const _Float16* pv = reinterpret_cast<const _Float16*>(a.past_v) + nh * a.cache_rows * HD;
    _Float16* ok = reinterpret_cast<_Float16*>(a.present_k) + nh * a.cache_rows * HD;
    _Float16* ov = reinterpret_cast<_Float16*>(a.present_v) + nh * a.cache_rows * HD;
    // the K / V vectors of a cached row; the next iteration's are requested before this iteration's arithmetic, so their latency lies under it, and
    // the first iteration's before the prologue
    auto load_row = [&](int j, h8& kx, h8& vx) {
        kx = *reinterpret_cast<const h8*>(pk + int64_t(j) * HD + el * 8);
        vx = *reinterpret_cast<const h8*>(pv + int64_t(j) * HD + el * 8);
    };
    h8 kn, vn;
#pragma unroll
    for (int e = 0; e < 8; ++e) { kn[e] = _Float16(0.f); vn[e] = _Float16(0.f); }
    if (k0 + slot < k1) load_row(k0 + slot, kn, vn);
    // Prologue, once per workgroup through LDS: one thread per element rotates the g query rows in fp32 and rounds them once (unscaled); the owning
    // split adds the new row the same way, k rotated and rounded, v as the half it is.  Every lane then takes its 16-byte slices.  (Rotating in every
    // lane, as tile 4 over an fp32 cache does, is 32 g scalar loads per lane here: the listing and the times of both forms are in DESIGN 3.36)
    {
        const bool rope = a.rope_cos != nullptr;
        const int64_t r = rope ? rope_row(a, n, 0) : 0;
        const int rows = sp == owner ? g + 2 : g;
        for (int idx = int(threadIdx.x); idx < rows * HD; idx += kDecodeBlock) {
            const int row = idx / HD, e = idx % HD;
            if (row < g) s_q[row][e] = _Float16(rotated<_Float16>(a, qkv_base(a, n, 0, 0, kvh * g + row), r, e, rope));
            else if (row == g) s_q[G][e] = _Float16(rotated<_Float16>(a, qkv_base(a, n, 0, 1, kvh), r, e, rope));
            else s_q[G + 1][e] = reinterpret_cast<const _Float16*>(a.in.p)[qkv_base(a, n, 0, 2, kvh) + int64_t(e) * a.in.sc];
        }
    }
    __syncthreads();
    H2x4 q[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) q[gi] = __builtin_bit_cast(H2x4, *reinterpret_cast<const h8*>(&s_q[gi < g ? gi : 0][el * 8]));
    float m[G], l[G], o[G][8];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        m[gi] = -kFltMax;
        l[gi] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[gi][e] = 0.f;
    }
    // one key's softmax step for every head of the group: the score from the packed q and K, the accumulation straight from the packed V
    auto attend = [&](const h8 kx, const h8 vx, bool take, float bias) {
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            float s = group_sum<LPK>(dot8(q[gi].v, kx)) * a.scale;
            if (take && gi < g) {
                if (a.mask) s = fmaxf(s + bias, -kFltMax);
                const float mn = fmaxf(m[gi], s), al = __expf(m[gi] - mn), p = __expf(s - mn);
                l[gi] = l[gi] * al + p;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[gi][e] = fmaf(p, float(vx[e]), o[gi][e] * al);
                m[gi] = mn;
            }
        }
    };
    for (int jb = k0; jb < k1; jb += KT) {         // workgroup-uniform
        const int j = jb + slot;
        const bool valid = j < k1;
        const h8 kx = kn, vx = vn;                 // (a slot past the split's end keeps stale finite values: its scores are never used)
        if (j + KT < k1) load_row(j + KT, kn, vn);
        attend(kx, vx, valid, valid && a.mask ? key_bias(a, n, j) : 0.f);
    }
    // the owning split takes the new row, rounded to half, from the prologue's LDS rows: slot 0 stores it at row len and attends to it as stored.
    // c == 0 (a padded token, or a full cache): nothing is stored, the key is not visible
    if (sp == owner) {                             // workgroup-uniform
        const h8 kx = *reinterpret_cast<const h8*>(&s_q[G][el * 8]), vx = *reinterpret_cast<const h8*>(&s_q[G + 1][el * 8]);
        const bool mine = slot == 0 && rs.c > 0;
        if (mine) {
            *reinterpret_cast<h8*>(ok + int64_t(P) * HD + el * 8) = kx;
            *reinterpret_cast<h8*>(ov + int64_t(P) * HD + el * 8) = vx;
        }
        attend(kx, vx, mine, 0.f);
        // nothing visible at all (no cached key, no new one): the weight 1 on a zero row keeps the token's output finite, and next to a real maximum
        // the record's weight is exactly 0
        if (slot == 0 && P == 0 && rs.c == 0) {
#pragma unroll
            for (int gi = 0; gi < G; ++gi) l[gi] = 1.f;
        }
    }
    // merge, first inside the wave: the KPW key slots of a head meet by a butterfly over the lane bits above the key's own lanes, in a fixed order
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        if (gi >= g) continue;                     // workgroup-uniform
        float M = m[gi];
#pragma unroll
        for (int x = LPK; x < 64; x <<= 1) M = fmaxf(M, __shfl_xor(M, x, 64));
        const float w = __expf(m[gi] - M);
        float L = l[gi] * w;
#pragma unroll
        for (int x = LPK; x < 64; x <<= 1) L += __shfl_xor(L, x, 64);
        float O[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            O[e] = o[gi][e] * w;
#pragma unroll
            for (int x = LPK; x < 64; x <<= 1) O[e] += __shfl_xor(O[e], x, 64);
        }
        if (sub == 0) {
            if (el == 0) { s_ml[wave][gi][0] = M; s_ml[wave][gi][1] = L; }
            *reinterpret_cast<float4*>(&s_o[wave][gi][el * 8]) = make_float4(O[0], O[1], O[2], O[3]);
            *reinterpret_cast<float4*>(&s_o[wave][gi][el * 8 + 4]) = make_float4(O[4], O[5], O[6], O[7]);
        }
    }
    __syncthreads();
    // then the four wave records, one thread per (query head, element)
    for (int idx = int(threadIdx.x); idx < g * HD; idx += kDecodeBlock) {
        const int gi = idx / HD, e = idx % HD;
        float M = -kFltMax;
#pragma unroll
        for (int t = 0; t < 4; ++t) M = fmaxf(M, s_ml[t][gi][0]);
        float Lsum = 0.f, O = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float w = __expf(s_ml[t][gi][0] - M);
            Lsum = fmaf(s_ml[t][gi][1], w, Lsum);
            O = fmaf(s_o[t][gi][e], w, O);
        }
        const int h = kvh * g + gi;
        if (S == 1) {
            reinterpret_cast<_Float16*>(a.out.p)[n * a.out.sn + (int64_t(h) * HD + e) * a.out.sc] = _Float16(O / Lsum);
        } else {                                   // record (n, h, split): m, l, o[HD]
            float* rec = a.workspace + ((n * a.heads + h) * S + sp) * int64_t(HD + 2);
            if (e == 0) { rec[0] = M; rec[1] = Lsum; }
            rec[2 + e] = O;
        }
    }
}

template <int HD>
hipError_t launch_decode_h(const DecodeArgs& a, hipStream_t stream) {
    const dim3 grid(unsigned(a.splits), unsigned(a.kv_heads), unsigned(a.in.n));
    const int g = a.heads / a.kv_heads;
    if (g == 1) hipLaunchKernelGGL((attention_decode_h_kernel<HD, 1>), grid, dim3(kDecodeBlock), 0, stream, a);
    else if (g == 2) hipLaunchKernelGGL((attention_decode_h_kernel<HD, 2>), grid, dim3(kDecodeBlock), 0, stream, a);
    else if (g <= 4) hipLaunchKernelGGL((attention_decode_h_kernel<HD, 4>), grid, dim3(kDecodeBlock), 0, stream, a);
    else hipLaunchKernelGGL((attention_decode_h_kernel<HD, 8>), grid, dim3(kDecodeBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t LaunchKvConvert(const void* src, void* dst, int64_t n, bool to_half, hipStream_t stream) {
    if (!src || !dst || n < 0 || (n + kDecodeBlock - 1) / kDecodeBlock >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const dim3 grid(unsigned((n + kDecodeBlock - 1) / kDecodeBlock));
    if (to_half) hipLaunchKernelGGL((kv_convert_kernel<true>), grid, dim3(kDecodeBlock), 0, stream, src, dst, n);
    else hipLaunchKernelGGL((kv_convert_kernel<false>), grid, dim3(kDecodeBlock), 0, stream, src, dst, n);
    return hipGetLastError();
}

// the new rows alone; the caller (LaunchKvAppend) has checked the operands: in place, half activations
hipError_t LaunchKvAppendRowsHalf(const DecodeArgs& a, hipStream_t stream) {
    if (!a.cache_f16 || a.cache_rows <= 0 || !a.in.f16) return hipErrorInvalidValue;
    const int64_t halfs = int64_t(a.in.n) * a.kv_heads * a.new_len * a.head_dim;
    const bool aligned = Aligned16(a.present_k) && Aligned16(a.present_v);
    const int V = aligned && a.head_dim % 8 == 0 ? 8 : (aligned && a.head_dim % 4 == 0 ? 4 : 1);
    const int64_t total = halfs / V;
    if (total / kDecodeBlock >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 grid(unsigned((total + kDecodeBlock - 1) / kDecodeBlock));
    if (V == 8) hipLaunchKernelGGL((kv_append_rows_h_kernel<8>), grid, dim3(kDecodeBlock), 0, stream, a, total);
    else if (V == 4) hipLaunchKernelGGL((kv_append_rows_h_kernel<4>), grid, dim3(kDecodeBlock), 0, stream, a, total);
    else hipLaunchKernelGGL((kv_append_rows_h_kernel<1>), grid, dim3(kDecodeBlock), 0, stream, a, total);
    return hipGetLastError();
}

// tile 4 alone; the caller (LaunchAttentionDecode) has checked the operands and launches the combine where splits > 1
hipError_t LaunchDecodeHalf(const DecodeArgs& a, hipStream_t stream) {
    if (!a.cache_f16 || a.cache_rows <= 0 || !a.in.f16 || !a.out.f16) return hipErrorInvalidValue;
    return a.head_dim == 32 ? launch_decode_h<32>(a, stream) : (a.head_dim == 64 ? launch_decode_h<64>(a, stream) : launch_decode_h<128>(a, stream));
}

}  // namespace ie
