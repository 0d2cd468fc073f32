// Multi-head attention over a token view (ViT-class graphs) on gfx950.
//
//   out[n, i, h * hd + e] = sum_j softmax_j(scale * q[n, h, i, :] . k[n, h, j, :]) * v[n, h, j, e]
//
// The operand is the qkv buffer the qkv Linear wrote: row (n, j) holds q | k | v, each D = heads * hd wide, head h at columns h * hd.  The result
// goes straight into the token buffer the projection Linear reads.  Scores, softmax statistics and accumulation are fp32 in both element types; the
// softmax subtracts the row maximum; no score is ever written to memory.
//
//   attention_generic_kernel        tile 0: one wave per (image, head, query row).  Any L, hd, pitch, offset, float or half.  Pass 1: the row
//                                   maximum (lane l takes the keys l, l + 64, ...).  Pass 2: per block of 64 keys each lane computes one
//                                   probability, the wave then walks the block with a shuffle broadcast while lane l accumulates output column l
//                                   (columns beyond 64 in further sweeps).  The fallback and the cross-check.
//   attention_mfma_kernel<T, HD>    tile 1: a workgroup = (image, head, 128 queries) = 4 waves x 32 queries.  The head's K and V rows are staged
//                                   once into LDS as 16-byte vectors, L padded with zero rows to whole 32-key tiles, every row padded by one
//                                   vector (the row stride is then 4 banks mod 64 in fp32 and 36 in fp16: the 16 lanes of a ds_read_b128 group hit
//                                   16 different bank quads).  Each wave keeps its 32 Q rows in registers and walks the keys in tiles of 32 with
//                                   an online softmax (running maximum m and sum l per query; O rescaled by exp(m - m') whenever m grows).
//   attention_stream_kernel<T, HD>  tile 2: one wide head (HD 128 / 256 / 512, no mask).  A workgroup = (image, head, 32 queries); its 4 waves split the
//                                   head dim; K and V are streamed in tiles of 32 keys, LDS does not depend on L (described at the kernel).
//                                   <T, HD, CAUSAL> and <T, HD, CAUSAL, ROPE> (HD 128 / 256) are its causal and rotary forms.
//
// Tile 1 computes the scores swapped, S^T = K . Q^T, and feeds P^T to the second product from the registers it is in: attn_mfma.h describes the
// orientation and the operand orders, and holds the wave (AttnWave) that tiles 1 and 3 and the window kernel share.
// Padded keys (j >= L) get -inf before the maximum; padded queries are computed from the last row and never stored.
//
//   attention_chunk_kernel<T, HD>   tile 3: tile 1's workgroup, orientation, online softmax and epilogue, for any L: K and V pass through LDS in chunks of
//                                   kAttnChunkKeys keys (stage, barrier, the chunk's key tiles, barrier), so LDS is a constant (described at the kernel).
//
// CAUSAL (every tile; never with MASK): query i attends to the keys j <= i.  The keys above the diagonal are left out, not computed and discarded:
// tile 0 ends its key loops at i + 1; a workgroup of tile 1 / 3 stages only the key rows below 128 (qb + 1), a wave's key-tile loop ends with the tile
// that holds its last query (key0 <= q0 + 31), and only the tile with key0 == q0 tests its elements (key > query -> -inf, before the maximum).  A
// workgroup of tile 2 (32 queries) walks the key tiles 0 ... qb and tests the last one.
//
// Grouped K / V heads (every tile; Llama-class graphs): a token row is q (D) | k (Dkv) | v (Dkv) with Dkv = kv_heads * hd, and query head h reads
// K / V head h / (heads / kv_heads).  Only the K / V base offsets change: every (image, head, query block) workgroup still stages (tile 2: streams) its
// K / V head itself.
//
// ROPE (tile 0 at run time; tiles 1, 2 and 3 as a template parameter of their CAUSAL form): the rotary position embedding of q and k inside the loads the
// kernels already do.  x'[e] = x[e] cos[i][e] + s(e) x[p(e)] sin[i][e] at token position i, p(e) = e +/- hd/2, s = -1 in the first half of the head and
// +1 in the second, with full-width fp32 tables [L][hd] (the two halves of a table row need not be equal).  The staging thread of K vector (row, cv)
// also loads the partner vector (cv + VPR/2) % VPR of the row and the cos / sin vectors of the row's GLOBAL key position (tile 3: chunk base + row)
// and writes the rotated vector to LDS; AttnWave::init_rope loads a lane's own half and the partner half of its Q row (the lane halves of the QK^T
// reduction are exactly the two rope halves) and rotates at its query's position.  fp32 arithmetic; a half operand is rounded once, where it enters
// LDS (k) or the MFMA fragment (q).  V is staged as it is.  No extra pass over the qkv buffer, no extra LDS.  Tile 2 has no K in LDS: it rotates the K
// fragments in registers (described at the kernel), a half operand rounded once, where it becomes the MFMA fragment.
//
// MASK (tiles 0 and 1): the key mask of a BERT-class graph.  Key j of image n gets the bias (1 - float(mask[n, j])) * c on its scaled score, computed in
// fp32 as the graph computes it.  Tile 1 stages the image's L biases in LDS behind K / V, already in units of log2 and clamped at -FLT_MAX
// (c = finfo.min times log2 e would overflow to -inf, and a fully masked row would be exp2(-inf - -inf) = NaN), padded keys at -inf; the bias is
// added to the fp32 scaled score before the running maximum.  -FLT_MAX + s rounds to -FLT_MAX for every real score, so a fully masked row with
// c = min is the uniform average of V, as the graph's own fp32 (and fp64) sum gives; with c = -10000 it is the unmasked softmax.
// A softmax does not change when one number is taken from every score of a row, and the biases of an image are the same for all of its queries: where
// the image's largest bias is no larger in magnitude than 2^24 (kMaskShiftMax: up to there an fp32 sum keeps something of a score of order 1) it is
// subtracted from every bias first -- exactly, for 0 / 1 masks -- so the fully masked image of c = -10000 computes its softmax on the bare scores
// instead of on scores rounded to the 1e-3 spacing of floats near 10^4.  Beyond 2^24 (c = min) nothing is subtracted and the sum absorbs the scores,
// as the graph's does.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_mfma.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kAttnBlock = 256;

// rows = N * heads * L query rows, one wave each
template <bool MASK, bool CAUSAL>
__global__ __launch_bounds__(kAttnBlock) void attention_generic_kernel(const AttnArgs a, const int64_t rows) {
    const int lane = int(threadIdx.x) % 64;
    const int64_t row = int64_t(blockIdx.x) * (kAttnBlock / 64) + threadIdx.x / 64;
    if (row >= rows) return;                       // wave-uniform
    const int L = a.in.w, hd = a.head_dim, D = a.heads * hd;
    const int i = int(row % L);
    const int h = int((row / L) % a.heads);
    const int64_t n = row / (int64_t(L) * a.heads);
    const int64_t qb = n * a.in.sn + int64_t(i) * a.in.sw + int64_t(h) * hd * a.in.sc;       // q row; key row j: kb + j * sw
    const int Hkv = a.kv_heads > 0 ? a.kv_heads : a.heads, kvh = Hkv == a.heads ? h : h / (a.heads / Hkv);      // grouped K / V heads: head h reads K / V head h / group
    const int64_t kb = n * a.in.sn + int64_t(D + kvh * hd) * a.in.sc, vb = kb + int64_t(Hkv) * hd * a.in.sc;
    const int64_t ob = n * a.out.sn + int64_t(i) * a.out.sw + int64_t(h) * hd * a.out.sc;
    const int Lk = CAUSAL ? i + 1 : L;             // the keys of this query: j < Lk
    [[maybe_unused]] float shift = 0.f;            // MASK: the image's largest bias, where it is small enough to be taken out exactly
    if constexpr (MASK) {
        float bm = -kFltMax;
        for (int j = lane; j < L; j += 64) bm = fmaxf(bm, (1.f - float(a.mask[n * a.mask_sn + j])) * a.mask_value);
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) bm = fmaxf(bm, __shfl_xor(bm, x, 64));
        shift = fabsf(bm) <= kMaskShiftMax ? bm : 0.f;
    }
    // element e of the row at `rb` (token position pos) after the rotary embedding: x[e] cos[pos][e] -/+ x[e +/- hd/2] sin[pos][e]
    auto rotated = [&](int64_t rb, int pos, int e) {
        const int hh = hd / 2, p = e < hh ? e + hh : e - hh;
        const float x = ld_any(a.in.p, a.in.f16, rb + int64_t(e) * a.in.sc), xp = ld_any(a.in.p, a.in.f16, rb + int64_t(p) * a.in.sc);
        const int64_t t = int64_t(pos) * hd + e;
        return fmaf(x, a.rope_cos[t], (e < hh ? -xp : xp) * a.rope_sin[t]);
    };
    auto score = [&](int j) {
        float s = 0.f;
        if (a.rope_cos) {                          // (a runtime flag: this kernel is the fallback and the cross-check)
            for (int e = 0; e < hd; ++e) s = fmaf(rotated(qb, i, e), rotated(kb + int64_t(j) * a.in.sw, j, e), s);
        } else {
            for (int e = 0; e < hd; ++e) s = fmaf(ld_any(a.in.p, a.in.f16, qb + int64_t(e) * a.in.sc), ld_any(a.in.p, a.in.f16, kb + int64_t(j) * a.in.sw + int64_t(e) * a.in.sc), s);
        }
        if constexpr (MASK) return fmaxf(s * a.scale + ((1.f - float(a.mask[n * a.mask_sn + j])) * a.mask_value - shift), -kFltMax);
        else return s * a.scale;
    };
    float m = -__builtin_huge_valf();
    for (int j = lane; j < Lk; j += 64) m = fmaxf(m, score(j));
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, 64));
    for (int e0 = 0; e0 < hd; e0 += 64) {
        const int e = e0 + lane;
        float l = 0.f, acc = 0.f;
        for (int j0 = 0; j0 < Lk; j0 += 64) {
            const int j = j0 + lane;
            const float p = j < Lk ? expf(score(j) - m) : 0.f;
            l += p;
            const int cnt = Lk - j0 < 64 ? Lk - j0 : 64;
            for (int t = 0; t < cnt; ++t) {
                const float pj = __shfl(p, t, 64);
                if (e < hd) acc = fmaf(pj, ld_any(a.in.p, a.in.f16, vb + int64_t(j0 + t) * a.in.sw + int64_t(e) * a.in.sc), acc);
            }
        }
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) l += __shfl_xor(l, x, 64);
        if (e < hd) {
            const float o = acc / l;
            const int64_t oi = ob + int64_t(e) * a.out.sc;
            if (a.out.f16) reinterpret_cast<_Float16*>(a.out.p)[oi] = _Float16(o);
            else a.out.p[oi] = o;
        }
    }
}

// One tile of 32 keys of a wave of tile 1 / 3: Kt / Vt = the LDS rows of key key0, Bt = the biases from key0 on (MASK).  query = q0 + col (CAUSAL); diag:
// this is the tile with key0 == q0, the only one of a causal wave whose elements are tested.
// Every tile a wave visits holds at least one visible key for each of its queries, which keeps the running maximum finite although it starts at -inf: a
// tile holds a real key (key0 < L); causal, a tile below the diagonal holds only keys < q0 <= every query of the wave, and the diagonal tile's first key
// q0 is <= every query of the wave and real (q0 < L; the padded queries q0 + col >= L are only ever compared as q0 + col, which admits more keys, not fewer).
template <int RS, bool MASK, bool CAUSAL, typename T, int HD>
__device__ __forceinline__ void key_tile(AttnWave<T, HD>& w, const T* Kt, const T* Vt, const float* Bt, int key0, int L, int query, bool diag, float sl2, float shift, int col, int hf) {
    const bool tail = key0 + 32 > L;               // the last tile holds padded keys
    if constexpr (MASK) {
        w.template key_tile<RS>(Kt, Vt, col, hf, [=](int kt, float s) {
            const float b = Bt[kt];                // -inf on a padded key, else finite: the biased score of a real key stays finite
            return b < -kFltMax ? b : fmaxf(fmaf(s, sl2, b - shift), -kFltMax);
        });
    } else if constexpr (CAUSAL) {
        w.template key_tile<RS>(Kt, Vt, col, hf, [=](int kt, float s) { return (tail && key0 + kt >= L) || (diag && key0 + kt > query) ? -__builtin_huge_valf() : s * sl2; });
    } else {
        w.template key_tile<RS>(Kt, Vt, col, hf, [=](int kt, float s) { return tail && key0 + kt >= L ? -__builtin_huge_valf() : s * sl2; });
    }
}

// grid = N * heads * qblocks workgroups (qblocks = ceil(L / 128)); dynamic LDS = AttnLdsBytes(L, HD, half) (by L, causal or not)
// ROPE (CAUSAL only): the staging thread of K vector (row, cv) also loads the partner vector (cv + VPR / 2) % VPR of the row and the cos / sin vectors of
// the row's key position and writes the rotated vector to LDS; AttnWave::init_rope rotates the wave's Q rows; V is staged as it is
template <typename T, int HD, bool MASK, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(kAttnBlock) void attention_mfma_kernel(const AttnArgs a, const int qblocks) {
    static_assert(!(MASK && CAUSAL), "a key mask together with a causal mask is not built");
    static_assert(!ROPE || CAUSAL, "the rotary form is built for causal steps only");
    constexpr int V = 16 / int(sizeof(T));         // elements per 16-byte vector
    constexpr int RS = HD + V;                     // LDS row stride in elements
    constexpr int HH = HD / 2;
    constexpr int VPR = HD / V;                    // vectors per K / V row
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
    const int L = a.in.w, Lp = (L + 31) / 32 * 32, D = a.heads * HD;
    T* Ks = reinterpret_cast<T*>(attn_smem);
    T* Vs = Ks + size_t(Lp) * RS;
    const int qb = int(blockIdx.x) % qblocks;
    const int hn = int(blockIdx.x) / qblocks;
    const int h = hn % a.heads, n = hn / a.heads;
    const T* base = reinterpret_cast<const T*>(a.in.p) + int64_t(n) * a.in.sn + h * HD;      // the head's q: token row j at + j * sw
    // the head's k and v from `base`: + D and + 2 D, or with grouped K / V heads (head h reads K / V head h / group) + D + (kvh - h) HD and that + Dkv
    // (no division on the path every other model takes: one K / V head per query head)
    const int kvn = a.kv_heads > 0 ? a.kv_heads : a.heads, ko = kvn == a.heads ? D : D + (h / (a.heads / kvn) - h) * HD, vo = ko + kvn * HD;
    const int Ls = CAUSAL && 128 * (qb + 1) < Lp ? 128 * (qb + 1) : Lp;                    // CAUSAL: no query of this workgroup sees a key beyond its last query

    for (int idx = int(threadIdx.x); idx < Ls * VPR; idx += kAttnBlock) {
        const int row = idx / VPR, cv = idx % VPR;
        uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;                                   // rows past L: zeros (a zero probability times them stays zero)
        if (row < L) {
            const T* r = base + int64_t(row) * a.in.sw + cv * V;
            kv = *reinterpret_cast<const uint4*>(r + ko);
            vv = *reinterpret_cast<const uint4*>(r + vo);
            if constexpr (ROPE) {
                constexpr int HV = VPR / 2;            // vectors per rope half
                const int64_t t = int64_t(row) * HD + cv * V;
                kv = rope_vec<T>(kv, *reinterpret_cast<const uint4*>(r + ko + (cv < HV ? HV : -HV) * V), a.rope_cos + t, a.rope_sin + t, cv < HV ? -1.f : 1.f);
            }
        }
        *reinterpret_cast<uint4*>(Ks + row * RS + cv * V) = kv;
        *reinterpret_cast<uint4*>(Vs + row * RS + cv * V) = vv;
    }
    [[maybe_unused]] float* Bs = reinterpret_cast<float*>(Vs + size_t(Lp) * RS);      // MASK: the image's key biases in units of log2 (16-byte aligned: RS * sizeof(T) is)
    if constexpr (MASK) {
        for (int j = int(threadIdx.x); j < Lp; j += kAttnBlock)
            Bs[j] = j < L ? fmaxf((1.f - float(a.mask[int64_t(n) * a.mask_sn + j])) * a.mask_value * kLog2e, -kFltMax) : -__builtin_huge_valf();
    }
    __syncthreads();

    const int wave = int(threadIdx.x) / 64, lane = int(threadIdx.x) % 64, col = lane & 31, hf = lane >> 5;
    const int q0 = qb * 128 + wave * 32;
    if (q0 >= L) return;                           // wave-uniform, behind the kernel's only barrier
    const int qi = q0 + col < L ? q0 + col : L - 1;
    AttnWave<T, HD> w;                             // this lane's half of its Q row in registers for the whole kernel
    if constexpr (ROPE) w.init_rope(base + int64_t(qi) * a.in.sw, hf, a.rope_cos + int64_t(qi) * HD, a.rope_sin + int64_t(qi) * HD, -__builtin_huge_valf());
    else w.init(base + int64_t(qi) * a.in.sw + hf * HH, -__builtin_huge_valf());
    const float sl2 = a.scale * kLog2e;            // scores in units of log2: exp(x) = exp2(x * log2 e)
    [[maybe_unused]] float shift = 0.f;            // MASK: the image's largest bias (every wave finds it for itself), where it is small enough to be taken out exactly
    if constexpr (MASK) {
        float bm = -kFltMax;
        for (int j = lane; j < L; j += 64) bm = fmaxf(bm, Bs[j]);
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) bm = fmaxf(bm, __shfl_xor(bm, x, 64));
        shift = fabsf(bm) <= kMaskShiftMax * kLog2e ? bm : 0.f;
    }

    const int kend = CAUSAL ? q0 + 32 : Lp;        // CAUSAL: the wave's last tile is the one that holds its queries (q0 + 32 <= Ls)
    for (int key0 = 0; key0 < kend; key0 += 32)
        key_tile<RS, MASK, CAUSAL>(w, Ks + key0 * RS, Vs + key0 * RS, Bs + key0, key0, L, q0 + col, key0 == q0, sl2, shift, col, hf);

    w.lsum += __shfl_xor(w.lsum, 32, 64);
    if (q0 + col >= L) return;
    w.store(reinterpret_cast<T*>(a.out.p) + int64_t(n) * a.out.sn + int64_t(q0 + col) * a.out.sw + h * HD, hf);
}

// Tile 3.  grid = N * heads * qblocks workgroups (qblocks = ceil(L / 128)); dynamic LDS = AttnChunkLdsBytes(HD, half), whatever L.
// Tile 1 with K and V staged chunk by chunk: per chunk of kAttnChunkKeys keys the workgroup stages the rows, meets at a barrier, every wave walks the
// chunk's key tiles (tile 1's key_tile, so scores, statistics and accumulation are tile 1's to the bit), and a second barrier lets the next chunk
// overwrite the rows (single-buffered: one workgroup per CU at fp32 hd 64 either way).
// EVERY wave takes part in EVERY barrier: a wave whose queries lie beyond L, and a causal wave that is already past its diagonal, keep staging and
// waiting and only skip the key tiles; there is no return in front of the last barrier (tile 1 may leave behind its only barrier; here that would hang
// the workgroup).  CAUSAL: the workgroup's chunk loop ends with the chunk that holds key 128 qb + 127.
// The late query blocks of a causal step do the most work: block ids are dealt out reversed, the last query block of every (image, head) first, so the
// grid's tail is made of the light workgroups.
template <typename T, int HD, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(kAttnBlock) void attention_chunk_kernel(const AttnArgs a, const int qblocks) {
    constexpr int V = 16 / int(sizeof(T));         // elements per 16-byte vector
    constexpr int RS = HD + V;                     // LDS row stride in elements
    constexpr int HH = HD / 2;
    constexpr int VPR = HD / V;                    // vectors per K / V row
    constexpr int KC = kAttnChunkKeys;
    static_assert(KC % 32 == 0, "whole key tiles per chunk");
    static_assert(!ROPE || CAUSAL, "the rotary form is built for causal steps only");
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
    const int L = a.in.w, Lp = (L + 31) / 32 * 32, D = a.heads * HD;
    T* Ks = reinterpret_cast<T*>(attn_smem);
    T* Vs = Ks + size_t(KC) * RS;
    const int nh = int(gridDim.x) / qblocks;       // images x heads
    const int qb = qblocks - 1 - int(blockIdx.x) / nh;
    const int hn = int(blockIdx.x) % nh;
    const int h = hn % a.heads, n = hn / a.heads;
    const T* base = reinterpret_cast<const T*>(a.in.p) + int64_t(n) * a.in.sn + h * HD;      // the head's q: token row j at + j * sw
    // the head's k and v from `base`: + D and + 2 D, or with grouped K / V heads (head h reads K / V head h / group) + D + (kvh - h) HD and that + Dkv
    // (no division on the path every other model takes: one K / V head per query head)
    const int kvn = a.kv_heads > 0 ? a.kv_heads : a.heads, ko = kvn == a.heads ? D : D + (h / (a.heads / kvn) - h) * HD, vo = ko + kvn * HD;
    const int wave = int(threadIdx.x) / 64, lane = int(threadIdx.x) % 64, col = lane & 31, hf = lane >> 5;
    const int q0 = qb * 128 + wave * 32;
    const bool live = q0 < L;                      // wave-uniform
    const int qi = q0 + col < L ? q0 + col : L - 1;
    AttnWave<T, HD> w;
    if constexpr (ROPE) w.init_rope(base + int64_t(qi) * a.in.sw, hf, a.rope_cos + int64_t(qi) * HD, a.rope_sin + int64_t(qi) * HD, -__builtin_huge_valf());
    else w.init(base + int64_t(qi) * a.in.sw + hf * HH, -__builtin_huge_valf());
    const float sl2 = a.scale * kLog2e;
    const int Ls = CAUSAL && 128 * (qb + 1) < Lp ? 128 * (qb + 1) : Lp;      // the workgroup's keys: whole tiles, the same for its four waves
    const int kend = !live ? 0 : (CAUSAL ? q0 + 32 : Lp);                 // this wave's keys (live: q0 + 32 <= Ls)

    for (int c0 = 0; c0 < Ls; c0 += KC) {          // (the bounds are the workgroup's: every wave runs every iteration)
        const int rows = Ls - c0 < KC ? Ls - c0 : KC;
        for (int idx = int(threadIdx.x); idx < rows * VPR; idx += kAttnBlock) {
            const int lr = idx / VPR, cv = idx % VPR, row = c0 + lr;
            uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;                               // rows past L: zeros
            if (row < L) {
                const T* r = base + int64_t(row) * a.in.sw + cv * V;
                kv = *reinterpret_cast<const uint4*>(r + ko);
                vv = *reinterpret_cast<const uint4*>(r + vo);
                if constexpr (ROPE) {                  // (row = the key's global position, not its row inside the chunk)
                    constexpr int HV = VPR / 2;
                    const int64_t t = int64_t(row) * HD + cv * V;
                    kv = rope_vec<T>(kv, *reinterpret_cast<const uint4*>(r + ko + (cv < HV ? HV : -HV) * V), a.rope_cos + t, a.rope_sin + t, cv < HV ? -1.f : 1.f);
                }
            }
            *reinterpret_cast<uint4*>(Ks + lr * RS + cv * V) = kv;
            *reinterpret_cast<uint4*>(Vs + lr * RS + cv * V) = vv;
        }
        __syncthreads();
        const int cend = c0 + rows < kend ? c0 + rows : kend;
        for (int key0 = c0; key0 < cend; key0 += 32)
            key_tile<RS, false, CAUSAL>(w, Ks + (key0 - c0) * RS, Vs + (key0 - c0) * RS, nullptr, key0, L, q0 + col, key0 == q0, sl2, 0.f, col, hf);
        __syncthreads();                           // the next chunk overwrites the rows
    }

    w.lsum += __shfl_xor(w.lsum, 32, 64);
    if (q0 + col < L) w.store(reinterpret_cast<T*>(a.out.p) + int64_t(n) * a.out.sn + int64_t(q0 + col) * a.out.sw + h * HD, hf);
}

// Tile 2: one wide head.  grid = N * heads * qblocks workgroups (qblocks = ceil(L / 32)); dynamic LDS = AttnStreamLdsBytes(HD, half).
// A workgroup is (image, head, 32 queries); wave w owns the head-dim slice [w SL, (w + 1) SL), SL = HD / 4, of Q, K, V and O.  Per tile of 32 keys:
//   1. the wave's PARTIAL S^T = K_slice . Q_slice^T (tile 1's orientation) from its Q registers and K fragments read straight from global memory
//   2. the four partial tiles meet in LDS and every wave adds them in the same order ((p0 + p1) + p2) + p3: all four hold bit-identical scores,
//      hence bit-identical m, l, alpha and P (a wave that summed in another order would rescale its O slice by another factor than its neighbours)
//   3. tile 1's online softmax on the summed tile, in every wave
//   4. O_slice^T += V_slice^T . P^T with SL / 32 accumulator blocks, P from the registers it is in, V through LDS (the A operand reads V by column)
// The K fragments and the V vectors of tile t + 1 are loaded into registers before tile t's softmax and second product (one wave per SIMD at hd 512
// fp32: nobody else hides the loads).  V tiles and partial tiles are double-buffered by tile parity, so one barrier per tile is enough: what tile t + 1
// overwrites was last read in tile t - 1, and every wave has passed tile t's barrier behind those reads.
// QK^T reduction order: lane half hf supplies the 16-byte vectors 2 k + hf (k = 0 ...) of the slice of its Q row and of its K row, not one contiguous
// half as in tile 1: the two halves of a K row's 32 bytes then come from one cache line, and a fragment load touches 32 lines instead of 64.
// Grouped K / V heads (every form, a run-time property): the K / V offsets of head h are those of K / V head h / (heads / kv_heads); with one K / V
// head per query head they are D and 2 D.  The query heads of a group are consecutive (image, head)s, so the id dealing below leaves them on one L2
// (a group is cut only where an L2's run of ids ends): the group's K / V head is read from HBM once.
// CAUSAL: the workgroup of query block qb walks the key tiles 0 ... qb; its last tile is the diagonal one (key0 == q0), where key key0 + r is
// replaced by -inf for the query q0 + col when key > query.  The loads of the tile behind the diagonal one read real rows (or the last row) and are
// never used.  The late query blocks do the most work: within an (image, head) the ids are dealt out with qb reversed, the longest workgroup first.
// ROPE (CAUSAL only, HD 128 / 256): q and k enter the scores rotated (kernels.h AttnArgs), the qkv buffer stays as it is.  The partner of element e
// is e +/- HD/2, which in the contiguous slicing belongs to wave w ^ 2: for QK^T (only) wave w therefore owns the two half-slices
// [w SL/2, (w + 1) SL/2) and HD/2 + the same, so a lane holds both partners itself, vectors k and k + NQ/2 of its registers.  The partial scores
// are sums over the wave's elements, whatever they are, and are still added ((p0 + p1) + p2) + p3 by every wave; V and O keep the contiguous
// slices.  Q is rotated once, at its query's position qi; a K fragment is rotated where it is used, at its key's global position, with the cos / sin
// vectors that were loaded a tile ahead together with it (the added traffic: NQ * V / 4 float4s of each table per lane and tile, L2-resident).
// Waves per SIMD the register allocation of a tile-2 form must leave room for: what the LDS of the plain form lets run (workgroups per CU =
// budget / AttnStreamLdsBytes, one wave per SIMD each), so the table registers of a rotary form cost no occupancy (fp16: 3 at hd 128, 2 at hd 256).
// The other forms state a minimum of 1, which is what a 256-thread kernel has without the attribute (one wave per SIMD): their code does not change
template <typename T, int HD, bool ROPE>
constexpr int kStreamWaves = ROPE ? int(kAttnLdsBudget / AttnStreamLdsBytes(HD, sizeof(T) == 2)) : 1;

template <typename T, int HD, bool CAUSAL = false, bool ROPE = false>
__global__ __launch_bounds__(kAttnBlock) __attribute__((amdgpu_waves_per_eu(kStreamWaves<T, HD, ROPE>))) void attention_stream_kernel(const AttnArgs a, const int qblocks) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int V = 16 / int(sizeof(T));         // elements per 16-byte vector
    constexpr int SL = HD / 4;                     // head-dim slice of one wave
    constexpr int NQ = SL / (2 * V);               // 16-byte vectors of its Q row (and of one K row) a lane holds
    constexpr int NB = SL / 32;                    // accumulator blocks of 32 output columns per wave
    constexpr int VPR = HD / V;                    // vectors per V row
    constexpr int NV = 32 * VPR / kAttnBlock;      // vectors of a V tile one thread stages
    constexpr int VT = 32 * HD;                    // elements of a V tile
    constexpr int TV = V / 4;                      // ROPE: float4s of a table row per 16-byte operand vector
    static_assert(NQ >= 1 && NB >= 1 && NV >= 1 && 32 * VPR % kAttnBlock == 0, "head dim");
    static_assert(!ROPE || (CAUSAL && NQ % 2 == 0 && HD <= 256), "the rotary form is built for causal steps of head dim 128 / 256 only");
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
    T* Vs = reinterpret_cast<T*>(attn_smem);                                               // [2][32 keys][HD]
    float4* Ps = reinterpret_cast<float4*>(attn_smem + 2 * VT * sizeof(T));                // [2][4 waves][4 register groups][64 lanes]
    const int L = a.in.w, D = a.heads * HD;
    // Workgroups are handed to the 8 XCDs in turn (blockIdx % 8 labels the ones that share an L2).  Every workgroup of an (image, head) streams the
    // same K and V, so the ids are dealt out anew: the workgroups of one L2 get one run of consecutive (image, head, query block)s
    const int xg = int(blockIdx.x) % 8, xq = int(gridDim.x) / 8, xr = int(gridDim.x) % 8;
    const int bid = (xg < xr ? xg * (xq + 1) : xr * (xq + 1) + (xg - xr) * xq) + int(blockIdx.x) / 8;
    const int qb = CAUSAL ? qblocks - 1 - bid % qblocks : bid % qblocks;
    const int hn = bid / qblocks;
    const int h = hn % a.heads, n = hn / a.heads;
    const int tid = int(threadIdx.x), wave = tid / 64, lane = tid % 64, col = lane & 31, hf = lane >> 5;
    const T* base = reinterpret_cast<const T*>(a.in.p) + int64_t(n) * a.in.sn + h * HD;      // token row j: + j * sw; q at + 0, k at + ko, v at + vo
    // the head's k and v from `base`: + D and + 2 D, or with grouped K / V heads (head h reads K / V head h / group) + D + (kvh - h) HD and that + Dkv
    const int kvn = a.kv_heads > 0 ? a.kv_heads : a.heads, ko = kvn == a.heads ? D : D + (h / (a.heads / kvn) - h) * HD, vo = ko + kvn * HD;
    const int q0 = qb * 32;                        // < L: qblocks = ceil(L / 32)
    const int qi = q0 + col < L ? q0 + col : L - 1;
    const int ntiles = CAUSAL ? qb + 1 : (L + 31) / 32;      // CAUSAL: the last tile is the diagonal one, key0 == q0

    // element (inside the head) of vector k of this lane's share of a Q / K row
    auto voff = [&](int k) {
        if constexpr (ROPE) return (k < NQ / 2 ? 0 : HD / 2) + wave * (SL / 2) + (2 * (k % (NQ / 2)) + hf) * V;
        else return wave * SL + (2 * k + hf) * V;
    };
    uint4 qv[NQ], kv[NQ], vv[NV];                  // Q for the whole kernel; K fragments and V vectors of the tile to come
    [[maybe_unused]] float4 ct[ROPE ? NQ * TV : 1], st[ROPE ? NQ * TV : 1];      // ROPE: the cos / sin entries of the lane's vectors at the position of `kv`'s row
    [[maybe_unused]] auto load_tables = [&](int pos) {          // pos < L: the tables are [L][HD]
        const float* cr = a.rope_cos + int64_t(pos) * HD;
        const float* sr = a.rope_sin + int64_t(pos) * HD;
#pragma unroll
        for (int k = 0; k < NQ; ++k)
#pragma unroll
            for (int j = 0; j < TV; ++j) {
                ct[k * TV + j] = *reinterpret_cast<const float4*>(cr + voff(k) + 4 * j);
                st[k * TV + j] = *reinterpret_cast<const float4*>(sr + voff(k) + 4 * j);
            }
    };
    [[maybe_unused]] auto rotate = [&](uint4 (&x)[NQ]) {        // by the tables in ct / st; vectors k and k + NQ / 2 are partners
#pragma unroll
        for (int k = 0; k < NQ / 2; ++k) {
            const uint4 lo = x[k], hi = x[k + NQ / 2];
            x[k] = rope_rot<T>(lo, hi, ct + k * TV, st + k * TV, -1.f);
            x[k + NQ / 2] = rope_rot<T>(hi, lo, ct + (k + NQ / 2) * TV, st + (k + NQ / 2) * TV, 1.f);
        }
    };
    {
        const T* qrow = base + int64_t(qi) * a.in.sw;
#pragma unroll
        for (int k = 0; k < NQ; ++k) qv[k] = *reinterpret_cast<const uint4*>(qrow + voff(k));
        if constexpr (ROPE) {
            load_tables(qi);
            rotate(qv);
        }
    }
    // Every load is unconditional, its row clamped to the last one: a load under a lane condition becomes a branch of its own, and the copies behind
    // it made the compiler wait for all loads in flight right behind the barrier.  A K row past L gives scores that are replaced by -inf below; a V
    // row past L is zeroed where it is written to LDS; the loads behind the last tile read the last row again and are never used.
    auto load_k = [&](int key0) {
        const int row = key0 + col < L ? key0 + col : L - 1;
        const T* krow = base + int64_t(row) * a.in.sw + ko;
#pragma unroll
        for (int k = 0; k < NQ; ++k) kv[k] = *reinterpret_cast<const uint4*>(krow + voff(k));
        if constexpr (ROPE) load_tables(row);      // (the clamped row: a position of the table)
    };
    auto load_v = [&](int key0) {
#pragma unroll
        for (int it = 0; it < NV; ++it) {
            const int id = it * kAttnBlock + tid, cv = id % VPR, row = key0 + id / VPR < L ? key0 + id / VPR : L - 1;
            vv[it] = *reinterpret_cast<const uint4*>(base + int64_t(row) * a.in.sw + vo + cv * V);
        }
    };
    load_k(0);
    load_v(0);

    f32x16 o[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
    float m = -__builtin_huge_valf(), lsum = 0.f;
    const float sl2 = a.scale * kLog2e;            // scores in units of log2: exp(x) = exp2(x * log2 e)

    // (one copy of the body: left alone the compiler peels the diagonal tile off a causal loop, a second body whose live ranges add 20 - 50 registers)
#pragma clang loop unroll(disable)
    for (int t = 0; t < ntiles; ++t) {
        const int key0 = 32 * t, buf = t & 1;
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        if constexpr (ROPE) rotate(kv);            // at the key's global position: ct / st came with this tile's fragments
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            if constexpr (F16) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, kv[k]), __builtin_bit_cast(h8, qv[k]), s, 0, 0, 0);
            } else {
                const float4 kf = __builtin_bit_cast(float4, kv[k]), qf = __builtin_bit_cast(float4, qv[k]);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf.x, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf.y, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf.z, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf.w, s, 0, 0, 0);
            }
        }
        load_k(key0 + 32);
        float4* pw = Ps + ((buf * 4 + wave) * 4) * 64 + lane;
#pragma unroll
        for (int g = 0; g < 4; ++g) pw[g * 64] = make_float4(s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
        T* vs = Vs + buf * VT;
#pragma unroll
        for (int it = 0; it < NV; ++it) {          // rows past L: zeros (a zero probability times them stays zero); row * HD + cv * V = id * V
            const int id = it * kAttnBlock + tid;
            *reinterpret_cast<uint4*>(vs + id * V) = key0 + id / VPR < L ? vv[it] : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        load_v(key0 + 32);
        const float4* pr = Ps + (buf * 16) * 64 + lane;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 p0 = pr[g * 64], p1 = pr[(4 + g) * 64], p2 = pr[(8 + g) * 64], p3 = pr[(12 + g) * 64];
            s[4 * g] = ((p0.x + p1.x) + p2.x) + p3.x;
            s[4 * g + 1] = ((p0.y + p1.y) + p2.y) + p3.y;
            s[4 * g + 2] = ((p0.z + p1.z) + p2.z) + p3.z;
            s[4 * g + 3] = ((p0.w + p1.w) + p2.w) + p3.w;
        }
        const bool tail = key0 + 32 > L;           // the last tile holds padded keys
        [[maybe_unused]] const bool diag = t == ntiles - 1;      // CAUSAL: key0 == q0, the only tile whose elements are tested
        float mx = -__builtin_huge_valf();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
            // (the query's unclamped index: a padded query q0 + col >= L then sees every real key of the tile, not fewer than its row L - 1)
            if constexpr (CAUSAL) s[r] = (tail && key >= L) || (diag && key > q0 + col) ? -__builtin_huge_valf() : s[r] * sl2;
            else s[r] = tail && key >= L ? -__builtin_huge_valf() : s[r] * sl2;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // finite: every tile has at least one real key (key0 < L) that each query sees.  CAUSAL: a tile below the diagonal holds only keys
        // < q0 <= every query of the workgroup, all real since q0 < L; the diagonal tile's first key q0 is real and <= every query q0 + col
        const float mn = fmaxf(m, mx);
        const float alpha = fast_exp2(m - mn);     // 0 on the first tile (m = -inf)
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = fast_exp2(s[r] - mn);
            ps += s[r];
        }
        lsum = fmaf(lsum, alpha, ps);              // this lane half's share of the row sum
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {      // no maximum of the wave's 32 queries grew: O stays as it is (a product with 1 is exact)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
        }
        const T* vc = vs + wave * SL + col;        // this lane's column of the wave's V slice: key row j at + j * HD, block b at + 32 b
        if constexpr (F16) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                h8 pb;
#pragma unroll
                for (int j = 0; j < 8; ++j) pb[j] = _Float16(s[8 * st + j]);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    h8 va;
#pragma unroll
                    for (int j = 0; j < 8; ++j) va[j] = vc[(16 * st + 8 * (j >> 2) + 4 * hf + (j & 3)) * HD + 32 * b];
                    o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb, o[b], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = (r & 3) + 8 * (r >> 2) + 4 * hf;
#pragma unroll
                for (int b = 0; b < NB; ++b) o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(float(vc[key * HD + 32 * b]), s[r], o[b], 0, 0, 0);
            }
        }
    }

    lsum += __shfl_xor(lsum, 32, 64);
    const bool live = q0 + col < L;                // padded queries were computed from the last row and are not stored
    const float inv = 1.f / lsum;
    T* orow = reinterpret_cast<T*>(a.out.p) + int64_t(n) * a.out.sn + int64_t(q0 + col) * a.out.sw + h * HD + wave * SL;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if constexpr (F16) {
            // registers 4 g ... 4 g + 3 are the columns 8 g + 4 hf ... + 3: the lane halves trade so that half 0 holds the eight columns of the even
            // groups and half 1 those of the odd groups, one 16-byte vector each
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                uint2 mine[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    h4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = _Float16(o[b][4 * (2 * p + x) + e] * inv);
                    mine[x] = __builtin_bit_cast(uint2, y);
                }
                const uint2 give = hf ? mine[0] : mine[1], keep = hf ? mine[1] : mine[0];
                uint2 got;
                got.x = unsigned(__shfl_xor(int(give.x), 32, 64));
                got.y = unsigned(__shfl_xor(int(give.y), 32, 64));
                const uint4 w = hf ? make_uint4(got.x, got.y, keep.x, keep.y) : make_uint4(keep.x, keep.y, got.x, got.y);
                if (live) *reinterpret_cast<uint4*>(orow + 32 * b + 8 * (2 * p + hf)) = w;
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (live) *reinterpret_cast<float4*>(orow + 32 * b + 8 * g + 4 * hf) = make_float4(o[b][4 * g] * inv, o[b][4 * g + 1] * inv, o[b][4 * g + 2] * inv, o[b][4 * g + 3] * inv);
        }
    }
}

// the MFMA kernels' view: a token view (one row per image), token rows one pitch apart through the whole tensor.  Differs from VecViewOk twice: the
// images must be dense (stricter), and the row stride of the single row addresses nothing, so it carries no condition (laxer: checked as 0)
bool token_view_ok(const TensorArg& t, int V) {
    TensorArg row = t;
    row.sh = 0;
    return t.h == 1 && t.sn == int64_t(t.w) * t.sw && VecViewOk(row, V);
}

template <typename T, int HD, bool MASK, bool CAUSAL, bool ROPE>
hipError_t launch_mfma(const AttnArgs& a, hipStream_t stream) {
    const int qblocks = (a.in.w + 127) / 128;
    const int64_t blocks = int64_t(a.in.n) * a.heads * qblocks;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const size_t lds = size_t(AttnLdsBytes(a.in.w, HD, sizeof(T) == 2, MASK));
    attention_mfma_kernel<T, HD, MASK, CAUSAL, ROPE><<<dim3(unsigned(blocks)), dim3(kAttnBlock), lds, stream>>>(a, qblocks);
    return hipGetLastError();
}

template <typename T, int HD, bool CAUSAL, bool ROPE>
hipError_t launch_chunk(const AttnArgs& a, hipStream_t stream) {
    const int qblocks = (a.in.w + 127) / 128;
    const int64_t blocks = int64_t(a.in.n) * a.heads * qblocks;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    attention_chunk_kernel<T, HD, CAUSAL, ROPE><<<dim3(unsigned(blocks)), dim3(kAttnBlock), size_t(AttnChunkLdsBytes(HD, sizeof(T) == 2)), stream>>>(a, qblocks);
    return hipGetLastError();
}

// tiles 1 and 3 by head dim (32 / 64: the eligibility admitted nothing else)
template <typename T, bool MASK, bool CAUSAL, bool ROPE = false>
hipError_t launch_mfma_hd(const AttnArgs& a, hipStream_t stream) {
    return a.head_dim == 64 ? launch_mfma<T, 64, MASK, CAUSAL, ROPE>(a, stream) : launch_mfma<T, 32, MASK, CAUSAL, ROPE>(a, stream);
}
template <typename T, bool CAUSAL, bool ROPE = false>
hipError_t launch_chunk_hd(const AttnArgs& a, hipStream_t stream) {
    return a.head_dim == 64 ? launch_chunk<T, 64, CAUSAL, ROPE>(a, stream) : launch_chunk<T, 32, CAUSAL, ROPE>(a, stream);
}

template <typename T, int HD, bool CAUSAL, bool ROPE>
hipError_t launch_stream(const AttnArgs& a, hipStream_t stream) {
    const int qblocks = (a.in.w + 31) / 32;
    const int64_t blocks = int64_t(a.in.n) * a.heads * qblocks;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    attention_stream_kernel<T, HD, CAUSAL, ROPE><<<dim3(unsigned(blocks)), dim3(kAttnBlock), size_t(AttnStreamLdsBytes(HD, sizeof(T) == 2)), stream>>>(a, qblocks);
    return hipGetLastError();
}

// tile 2 by head dim (128 / 256 / 512, a rotary step 128 / 256: the eligibility admitted nothing else)
template <typename T, bool CAUSAL = false, bool ROPE = false>
hipError_t launch_stream_hd(const AttnArgs& a, hipStream_t stream) {
    if (a.head_dim == 128) return launch_stream<T, 128, CAUSAL, ROPE>(a, stream);
    if (a.head_dim == 256) return launch_stream<T, 256, CAUSAL, ROPE>(a, stream);
    if constexpr (!ROPE) {
        if (a.head_dim == 512) return launch_stream<T, 512, CAUSAL, ROPE>(a, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

bool AttentionEligible(const AttnArgs& a, int tile) {
    if (tile < 0 || tile >= kNumAttnTiles || !a.in.p || !a.out.p || a.heads < 1 || a.head_dim < 1) return false;
    const int64_t D = int64_t(a.heads) * a.head_dim;
    const int kvn = a.kv_heads > 0 ? a.kv_heads : a.heads;
    if (kvn > a.heads || a.heads % kvn) return false;          // whole groups of query heads per K / V head
    if (a.in.f8 || a.out.f8 || a.in.c != D + 2 * int64_t(kvn) * a.head_dim || a.out.c != D || a.in.n != a.out.n || a.in.h != 1 || a.out.h != 1 || a.in.w != a.out.w || a.in.w < 1)
        return false;
    if (a.mask && a.mask_sn < a.in.w) return false;
    if (a.causal && a.mask) return false;                     // no kernel has both masks
    const bool rope = a.rope_cos || a.rope_sin;
    if (rope && (!a.rope_cos || !a.rope_sin || a.mask || a.head_dim % 2)) return false;      // both tables; no kernel rotates under a key mask
    if (tile == 0) return true;
    if (rope && (!a.causal || !Aligned16(a.rope_cos) || !Aligned16(a.rope_sin))) return false;      // tiles 1, 2 and 3 rotate in their causal form only
    if (tile == 2 && rope && a.head_dim != 128 && a.head_dim != 256) return false;                  // (no rotary form at hd 512)
    const int V = a.out.f16 ? 8 : 4;
    // (the offsets are in the base pointers: their alignment stands for the offset condition)
    if (a.in.f16 != a.out.f16 || !token_view_ok(a.in, V) || !token_view_ok(a.out, V)) return false;
    if (tile == 3) return AttnChunkFits(a.in.w, a.head_dim, a.out.f16 != 0, a.in.c, a.in.sw, 0, a.out.c, a.out.sw, 0, a.mask != nullptr);
    return tile == 1 ? AttnMfmaFits(a.in.w, a.head_dim, a.out.f16 != 0, a.in.c, a.in.sw, 0, a.out.c, a.out.sw, 0, a.mask != nullptr)
                     : AttnStreamFits(a.in.w, a.head_dim, a.out.f16 != 0, a.in.c, a.in.sw, 0, a.out.c, a.out.sw, 0, a.mask != nullptr);
}

hipError_t LaunchAttention(const AttnArgs& a, int tile, hipStream_t stream) {
    if (!AttentionEligible(a, tile)) return hipErrorInvalidValue;
    if (a.in.n == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t rows = int64_t(a.in.n) * a.heads * a.in.w;
        const int64_t blocks = (rows + kAttnBlock / 64 - 1) / (kAttnBlock / 64);
        if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
        if (a.mask) hipLaunchKernelGGL((attention_generic_kernel<true, false>), dim3(unsigned(blocks)), dim3(kAttnBlock), 0, stream, a, rows);
        else if (a.causal) hipLaunchKernelGGL((attention_generic_kernel<false, true>), dim3(unsigned(blocks)), dim3(kAttnBlock), 0, stream, a, rows);
        else hipLaunchKernelGGL((attention_generic_kernel<false, false>), dim3(unsigned(blocks)), dim3(kAttnBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    if (tile == 2) {
        if (a.rope_cos) return a.out.f16 ? launch_stream_hd<_Float16, true, true>(a, stream) : launch_stream_hd<float, true, true>(a, stream);
        if (a.causal) return a.out.f16 ? launch_stream_hd<_Float16, true>(a, stream) : launch_stream_hd<float, true>(a, stream);
        return a.out.f16 ? launch_stream_hd<_Float16>(a, stream) : launch_stream_hd<float>(a, stream);
    }
    if (tile == 3) {
        if (a.rope_cos) return a.out.f16 ? launch_chunk_hd<_Float16, true, true>(a, stream) : launch_chunk_hd<float, true, true>(a, stream);
        if (a.causal) return a.out.f16 ? launch_chunk_hd<_Float16, true>(a, stream) : launch_chunk_hd<float, true>(a, stream);
        return a.out.f16 ? launch_chunk_hd<_Float16, false>(a, stream) : launch_chunk_hd<float, false>(a, stream);
    }
    if (a.mask) return a.out.f16 ? launch_mfma_hd<_Float16, true, false>(a, stream) : launch_mfma_hd<float, true, false>(a, stream);
    if (a.rope_cos) return a.out.f16 ? launch_mfma_hd<_Float16, false, true, true>(a, stream) : launch_mfma_hd<float, false, true, true>(a, stream);
    if (a.causal) return a.out.f16 ? launch_mfma_hd<_Float16, false, true>(a, stream) : launch_mfma_hd<float, false, true>(a, stream);
    return a.out.f16 ? launch_mfma_hd<_Float16, false, false>(a, stream) : launch_mfma_hd<float, false, false>(a, stream);
}

hipError_t InitKernelsAttn() {
    const void* const kernels[] = {
        reinterpret_cast<const void*>(&attention_mfma_kernel<float, 32, false, false, false>), reinterpret_cast<const void*>(&attention_mfma_kernel<float, 64, false, false, false>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 32, false, false, false>), reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 64, false, false, false>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<float, 32, true, false, false>), reinterpret_cast<const void*>(&attention_mfma_kernel<float, 64, true, false, false>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 32, true, false, false>), reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 64, true, false, false>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<float, 32, false, true, false>), reinterpret_cast<const void*>(&attention_mfma_kernel<float, 64, false, true, false>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 32, false, true, false>), reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 64, false, true, false>),
        reinterpret_cast<const void*>(&attention_chunk_kernel<float, 32, false, false>), reinterpret_cast<const void*>(&attention_chunk_kernel<float, 64, false, false>),
        reinterpret_cast<const void*>(&attention_chunk_kernel<_Float16, 32, false, false>), reinterpret_cast<const void*>(&attention_chunk_kernel<_Float16, 64, false, false>),
        reinterpret_cast<const void*>(&attention_chunk_kernel<float, 32, true, false>), reinterpret_cast<const void*>(&attention_chunk_kernel<float, 64, true, false>),
        reinterpret_cast<const void*>(&attention_chunk_kernel<_Float16, 32, true, false>), reinterpret_cast<const void*>(&attention_chunk_kernel<_Float16, 64, true, false>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<float, 32, false, true, true>), reinterpret_cast<const void*>(&attention_mfma_kernel<float, 64, false, true, true>),
        reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 32, false, true, true>), reinterpret_cast<const void*>(&attention_mfma_kernel<_Float16, 64, false, true, true>),
        reinterpret_cast<const void*>(&attention_chunk_kernel<float, 32, true, true>), reinterpret_cast<const void*>(&attention_chunk_kernel<float, 64, true, true>),
        reinterpret_cast<const void*>(&attention_chunk_kernel<_Float16, 32, true, true>), reinterpret_cast<const void*>(&attention_chunk_kernel<_Float16, 64, true, true>),
        reinterpret_cast<const void*>(&attention_stream_kernel<float, 128>), reinterpret_cast<const void*>(&attention_stream_kernel<float, 256>),
        reinterpret_cast<const void*>(&attention_stream_kernel<float, 512>), reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 128>),
        reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 256>), reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 512>),
        reinterpret_cast<const void*>(&attention_stream_kernel<float, 128, true>), reinterpret_cast<const void*>(&attention_stream_kernel<float, 256, true>),
        reinterpret_cast<const void*>(&attention_stream_kernel<float, 512, true>), reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 128, true>),
        reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 256, true>), reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 512, true>),
        reinterpret_cast<const void*>(&attention_stream_kernel<float, 128, true, true>), reinterpret_cast<const void*>(&attention_stream_kernel<float, 256, true, true>),
        reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 128, true, true>), reinterpret_cast<const void*>(&attention_stream_kernel<_Float16, 256, true, true>)};
    for (const void* k : kernels)
        if (const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, int(kAttnLdsBudget)); e != hipSuccess) return e;
    return hipSuccess;
}

}  // namespace ie
