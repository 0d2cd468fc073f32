// Mixture-of-experts MLP (com.microsoft MoE) on gfx950: the MLP of a Mixtral-class decoder, a router's choice of top_k of E expert MLPs per token.
//
//   p = softmax(router[t, :]),  sel = the top_k largest p (on equal values the lower expert),  g_j = p[sel_j] (/ sum_j g_j)
//   y[t] = r[t] + sum_j g_j * ((act(x[t] W1[sel_j] + b1) * (x[t] W3[sel_j] + b3)) W2[sel_j] + b2)
//
// A slot is one (token, choice) pair, slot = t * top_k + j.  Five launches, every grid fixed by rows, top_k, E, D and I alone; nothing is read back:
//
//   moe_route_kernel     a wave per token, a lane per expert: the softmax in fp32 (half logits are widened), top_k rounds of a wave-wide arg-max that
//                        takes the larger value and on equal values the lower index, the optional renormalisation; writes sel[slot] and gate[slot].
//   moe_group_kernel     one workgroup: counts per expert, their exclusive scan, the slots sorted by expert and by slot index inside one (ballots over
//                        the slots in order: no atomics, the order is the slot order), and the table of (expert, first sorted row, rows) per row block.
//                        A table entry past the last block holds expert -1.
//   moe_up_kernel<ACT, GATED, MT>   tile 1.  A workgroup of 4 waves owns one table entry -- one expert, up to MT tiles of 16 sorted rows -- and 16 columns
//                        of I.  An entry of expert -1 leaves before its first weight load: only the experts that tokens chose are read.
//   moe_down_kernel<MT>  tile 1, the same split over (table entry, 16 columns of D): A is h, contiguous in sorted order, B is W2[e]; the epilogue adds b2,
//                        multiplies by the slot's gate and stores fp32 part[slot][D].
//   moe_combine_kernel   y[t] = r[t] + part[t k] + ... + part[t k + k - 1] in that order, rounded once.
//   moe_generic_kernel<DOWN>   tile 0: a wave per (sorted row, column), the lanes split the reduction, fp32 weights and FMAs, a shuffle tree; any view, float or
//                        half activations.  The fp32-precision route, the fallback for D or I that are no multiple of 32, and the cross-check.
//
// Tile 1, per wave and K-chunk of 128 (the waves take the chunks round-robin: split K inside the workgroup), after qlinear_mfma_kernel's lane layout:
//   * weights are [E][N][K] halfs, K contiguous.  Lane (c = lane % 16, g = lane / 16) reads four 16-byte vectors of column n0 + c, the 32 consecutive k
//     from chunk + 32 g on, straight into the B fragments of four v_mfma_f32_16x16x32_f16: no LDS trip.  MFMA j takes vector j of every lane group, so
//     its 32-deep K is {chunk + 32 g + 8 j + i}: a permuted walk of K, the same on both operands.  The next chunk's vectors are in flight under the MFMAs.
//   * the A fragment of row tile t is eight consecutive halfs of the row of slot list[r0 + 16 t + c] -- x[slot / top_k] through the slot list in the up
//     kernel, h[r0 + 16 t + c] in the down kernel -- one 16-byte load, shared by the gate and the up product.  Rows past the entry's count and k past
//     K load nothing and enter as zeros (K % 32 == 0: a lane's 32 k are all inside or all outside).
//   * the four waves' accumulators meet in LDS and are added in wave order; the up epilogue forms act(u1 + b1) * (u3 + b3) in fp32 and rounds once.
// Every sum has one fixed order, and the order of the rows inside an expert's list is the slot order: two runs are bit-equal.
//
//   moe_gemm_up_kernel<ACT, GATED> / moe_gemm_down_kernel   tile 2 (prefill row counts): a grouped GEMM over the table entries, which the
//                        group kernel then cuts at 128 rows.  A workgroup of 4 waves owns one entry and one column tile; wave (wm, wn) a 64 x 64 quarter in
//                        2 x 2 accumulators of v_mfma_f32_32x32x16_f16, after qlinear_gemm_kernel's skeleton.
// Tile 2, per K-step of 64:
//   * both operands are staged alike: thread t reads four 16-byte vectors, k0 + 8 (t % 8) .. of image rows t / 8 + 32 i, of the weights (rows of W[e],
//     K contiguous) and of the gathered activations (the row of slot list[r0 + row] in the up kernel, h[r0 + row] in the down kernel; the row pointers are
//     resolved once).  Rows past the entry's count, 32-column groups past N and k past K read nothing and enter as zeros.
//   * gated up product: the 128 weight rows are 64 columns of h; wave wn's 64 rows are 32 columns of W1[e], then the same 32 columns of W3[e], so its two
//     column accumulators are u1 and u3 of the same h columns in the same lanes and act(u1 + b1) * (u3 + b3) needs no exchange.  The activation rows are
//     staged once for both products.
//   * both LDS images have rows of 64 + 8 halfs (36 words); two stages: the loads of step s + 1 are issued before the MFMAs of step s and written into the
//     other stage after them; ONE barrier closes the step.  LDS: 2 x 256 x 72 x 2 = 73 728 bytes, two workgroups per CU.
// D = W x A^T (the weights are the MFMA's first operand): a lane owns one row and quads of consecutive columns; v_permlane32_swap leaves it with eight
// consecutive columns for 16-byte stores.  No K split and no atomics: every output is one fixed-order sum.  The grid runs the entries fastest.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kMoeBlock = 256;         // 4 waves
constexpr int kMoeWaves = kMoeBlock / 64;
constexpr int kMoeChunk = 128;         // tile 1: k per wave and step (4 lane groups x 32)
constexpr int kMoeExpertsPerWave = kMoeMaxExperts / kMoeWaves;

// the parts of the workspace (kernels.h MoeLayout) as pointers
struct MoeWs {
    int* sel;
    float* gate;
    int* offs;
    int* list;
    int4* tab;
    float* part;
    float* h;
};

// element offset of pixel row m of a view
__device__ __forceinline__ int64_t moe_row(const TensorArg& t, int64_t m) {
    const int px = int(m % t.w);
    const int64_t q = m / t.w;
    return (q / t.h) * t.sn + (q % t.h) * t.sh + int64_t(px) * t.sw;
}

__global__ __launch_bounds__(kMoeBlock) void moe_route_kernel(const MoeArgs a, const MoeWs ws, const int rows) {
    const int lane = int(threadIdx.x) % 64;
    const int t = int(blockIdx.x) * kMoeWaves + int(threadIdx.x) / 64;
    if (t >= rows) return;                         // wave-uniform
    const int E = a.experts, k = a.top_k;
    const float v = lane < E ? ld_any(a.router.p, a.router.f16, moe_row(a.router, t) + int64_t(lane) * a.router.sc) : -__builtin_huge_valf();
    float mx = v;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    float p = lane < E ? expf(v - mx) : 0.f;
    const float sum = group_sum<64>(p);
    p = lane < E ? p / sum : -1.f;                 // (a taken expert and a lane past E hold -1: below every probability)
    float my_g = 0.f, total = 0.f;
    int my_e = 0;
    for (int j = 0; j < k; ++j) {
        float bv = p;
        int bi = lane;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == bi) p = -1.f;
        if (lane == j) { my_g = bv; my_e = bi; }
        total += bv;                               // selection order, the same in every lane
    }
    if (lane < k) {
        ws.sel[int64_t(t) * k + lane] = my_e;
        ws.gate[int64_t(t) * k + lane] = a.normalize ? my_g / total : my_g;
    }
}

__global__ __launch_bounds__(kMoeBlock) void moe_group_kernel(const MoeWs ws, const int slots, const int E, const int block_rows, const int max_blocks) {
    __shared__ int cnt[kMoeMaxExperts], off[kMoeMaxExperts];
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    // wave w counts the experts w, w + 4, ..: one read of sel per 64 slots, a ballot per expert
    int c[kMoeExpertsPerWave];
#pragma unroll
    for (int j = 0; j < kMoeExpertsPerWave; ++j) c[j] = 0;
    for (int base = 0; base < slots; base += 64) {
        const int s = base + lane;
        const int v = s < slots ? ws.sel[s] : -1;
#pragma unroll
        for (int j = 0; j < kMoeExpertsPerWave; ++j) c[j] += __popcll(__ballot(v == wave + kMoeWaves * j));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kMoeExpertsPerWave; ++j) cnt[wave + kMoeWaves * j] = c[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0, b = 0;
        for (int e = 0; e < E; ++e) {
            off[e] = o;
            ws.offs[e] = o;
            for (int r = 0; r < cnt[e] && b < max_blocks; r += block_rows, ++b) ws.tab[b] = make_int4(e, o + r, min(block_rows, cnt[e] - r), 0);
            o += cnt[e];
        }
        ws.offs[E] = o;
        for (; b < max_blocks; ++b) ws.tab[b] = make_int4(-1, 0, 0, 0);
    }
    __syncthreads();
    // the same walk again: a slot's place is its expert's offset plus the count of earlier slots of that expert
#pragma unroll
    for (int j = 0; j < kMoeExpertsPerWave; ++j) c[j] = wave + kMoeWaves * j < E ? off[wave + kMoeWaves * j] : 0;
    for (int base = 0; base < slots; base += 64) {
        const int s = base + lane;
        const int v = s < slots ? ws.sel[s] : -1;
#pragma unroll
        for (int j = 0; j < kMoeExpertsPerWave; ++j) {
            const unsigned long long m = __ballot(v == wave + kMoeWaves * j);
            if (v == wave + kMoeWaves * j) ws.list[c[j] + __popcll(m & ((1ull << lane) - 1ull))] = s;
            c[j] += __popcll(m);
        }
    }
}

// what a lane holds of one chunk of one weight matrix: 32 consecutive k of its column
struct MoeFrag {
    h8 v[4];
};

__device__ __forceinline__ MoeFrag moe_load(const _Float16* wrow, int k, int K) {
    MoeFrag f;
#pragma unroll
    for (int j = 0; j < 4; ++j) f.v[j] = h8{0, 0, 0, 0, 0, 0, 0, 0};
    if (k < K) {                                   // (K % 32 == 0: the lane's 32 k are all inside or all outside)
#pragma unroll
        for (int j = 0; j < 4; ++j) f.v[j] = *reinterpret_cast<const h8*>(wrow + k + 8 * j);
    }
    return f;
}

// The K loop of tile 1 for one table entry: acc1[t] (and acc3[t]) += A rows of row tile t x the 16 columns at w1row (w3row); arow[t] = the row lane c
// loads for tile t, live[t] = it exists
template <bool GATED, int MT>
__device__ __forceinline__ void moe_mfma_loop(const _Float16* const* arow, const bool* live, const _Float16* w1row, const _Float16* w3row, int K, int wave, int g,
                                              f32x4* acc1, f32x4* acc3) {
    const int nchunks = (K + kMoeChunk - 1) / kMoeChunk;
    int k = wave * kMoeChunk + 32 * g;
    MoeFrag cur1 = moe_load(w1row, k, K), cur3;
    if constexpr (GATED) cur3 = moe_load(w3row, k, K);
    for (int ch = wave; ch < nchunks; ch += kMoeWaves) {
        const int kn = k + kMoeWaves * kMoeChunk;
        const bool more = ch + kMoeWaves < nchunks;
        const MoeFrag nxt1 = moe_load(w1row, more ? kn : K, K);
        MoeFrag nxt3;
        if constexpr (GATED) nxt3 = moe_load(w3row, more ? kn : K, K);
        const bool in_k = k < K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                h8 xa = h8{0, 0, 0, 0, 0, 0, 0, 0};
                if (live[t] && in_k) xa = *reinterpret_cast<const h8*>(arow[t] + k + 8 * j);
                acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa, cur1.v[j], acc1[t], 0, 0, 0);
                if constexpr (GATED) acc3[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa, cur3.v[j], acc3[t], 0, 0, 0);
            }
        }
        cur1 = nxt1;
        if constexpr (GATED) cur3 = nxt3;
        k = kn;
    }
}

// the four waves' sums of eight columns of one row, in wave order (accumulator element v of lane (c, g) is row 4 g + v, column c of the 16 x 16 tile)
template <int MT>
__device__ __forceinline__ void moe_reduce8(const float (*red)[MT][64][4], int t, int r, int c0, float* v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int src = (r / 4) * 16 + c0 + i;
        float s = red[0][t][src][r % 4];
#pragma unroll
        for (int w = 1; w < kMoeWaves; ++w) s += red[w][t][src][r % 4];
        v[i] = s;
    }
}

template <int ACT, bool GATED, int MT>
__global__ __launch_bounds__(kMoeBlock) void moe_up_kernel(const MoeArgs a, const MoeWs ws) {
    __shared__ float red[GATED ? 2 : 1][kMoeWaves][MT][64][4];
    const int4 tb = ws.tab[blockIdx.y];
    const int e = tb.x, r0 = tb.y, nr = tb.z;
    if (e < 0) return;                             // no such (expert, row block) in this run: nothing is loaded
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    const int c = lane % 16, g = lane / 16;
    const int D = a.in.c, I = a.inter;
    const int n0 = int(blockIdx.x) * 16;
    const _Float16* w1row = reinterpret_cast<const _Float16*>(a.w1h) + (int64_t(e) * I + n0 + c) * D;
    const _Float16* w3row = GATED ? reinterpret_cast<const _Float16*>(a.w3h) + (int64_t(e) * I + n0 + c) * D : nullptr;
    const _Float16* x = reinterpret_cast<const _Float16*>(a.in.p);
    const _Float16* arow[MT];
    bool live[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        live[t] = 16 * t + c < nr;
        const int slot = live[t] ? ws.list[r0 + 16 * t + c] : 0;
        arow[t] = x + int64_t(slot / a.top_k) * a.in.sw;
    }
    f32x4 acc1[MT], acc3[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc1[t] = acc3[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    moe_mfma_loop<GATED, MT>(arow, live, w1row, w3row, D, wave, g, acc1, acc3);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        *reinterpret_cast<f32x4*>(&red[0][wave][t][lane][0]) = acc1[t];
        if constexpr (GATED) *reinterpret_cast<f32x4*>(&red[1][wave][t][lane][0]) = acc3[t];
    }
    __syncthreads();
    // one lane per (row tile, row, 8 columns): the sums in wave order, the biases, act(u1) * u3 in fp32, one rounding, a 16-byte store
    _Float16* h = reinterpret_cast<_Float16*>(ws.h);
    for (int idx = int(threadIdx.x); idx < MT * 32; idx += kMoeBlock) {
        const int t = idx / 32, r = (idx % 32) / 2, c0 = (idx % 2) * 8;
        if (16 * t + r >= nr) continue;
        const int64_t bo = int64_t(e) * I + n0 + c0;
        float v[8], u[8];
        moe_reduce8<MT>(red[0], t, r, c0, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ApplyAct(ACT, 0.f, 0.f, v[i] + (a.b1 ? a.b1[bo + i] : 0.f));
        if constexpr (GATED) {
            moe_reduce8<MT>(red[GATED ? 1 : 0], t, r, c0, u);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] *= u[i] + (a.b3 ? a.b3[bo + i] : 0.f);
        }
        store16<_Float16>(h + int64_t(r0 + 16 * t + r) * I + n0 + c0, v);
    }
}

template <int MT>
__global__ __launch_bounds__(kMoeBlock) void moe_down_kernel(const MoeArgs a, const MoeWs ws) {
    __shared__ float red[kMoeWaves][MT][64][4];
    const int4 tb = ws.tab[blockIdx.y];
    const int e = tb.x, r0 = tb.y, nr = tb.z;
    if (e < 0) return;
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    const int c = lane % 16, g = lane / 16;
    const int D = a.in.c, I = a.inter;
    const int n0 = int(blockIdx.x) * 16;
    const _Float16* w2row = reinterpret_cast<const _Float16*>(a.w2h) + (int64_t(e) * D + n0 + c) * I;
    const _Float16* h = reinterpret_cast<const _Float16*>(ws.h);
    const _Float16* arow[MT];
    bool live[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        live[t] = 16 * t + c < nr;
        arow[t] = h + int64_t(r0 + (live[t] ? 16 * t + c : 0)) * I;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    moe_mfma_loop<false, MT>(arow, live, w2row, nullptr, I, wave, g, acc, nullptr);
#pragma unroll
    for (int t = 0; t < MT; ++t) *reinterpret_cast<f32x4*>(&red[wave][t][lane][0]) = acc[t];
    __syncthreads();
    for (int idx = int(threadIdx.x); idx < MT * 32; idx += kMoeBlock) {
        const int t = idx / 32, r = (idx % 32) / 2, c0 = (idx % 2) * 8;
        if (16 * t + r >= nr) continue;
        const int slot = ws.list[r0 + 16 * t + r];
        const float gate = ws.gate[slot];
        float v[8];
        moe_reduce8<MT>(red, t, r, c0, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (v[i] + (a.b2 ? a.b2[int64_t(e) * D + n0 + c0 + i] : 0.f)) * gate;
        float* o = ws.part + int64_t(slot) * D + n0 + c0;
        store16<float>(o, v);
        store16<float>(o + 4, v + 4);
    }
}

// tile 0: blockIdx.x = the sorted row, a wave per column
template <bool DOWN>
__global__ __launch_bounds__(kMoeBlock) void moe_generic_kernel(const MoeArgs a, const MoeWs ws) {
    const int lane = int(threadIdx.x) % 64;
    const int D = a.in.c, I = a.inter;
    const int n = int(blockIdx.y) * kMoeWaves + int(threadIdx.x) / 64;
    if (n >= (DOWN ? D : I)) return;               // wave-uniform
    const int64_t row = blockIdx.x;
    const int slot = ws.list[row];
    const int e = ws.sel[slot];
    if constexpr (DOWN) {
        const float* hrow = ws.h + row * I;
        const float* w = a.w2 + (int64_t(e) * D + n) * I;
        float acc = 0.f;
        for (int k = lane; k < I; k += 64) acc = fmaf(hrow[k], w[k], acc);
        acc = group_sum<64>(acc);
        if (lane == 0) ws.part[int64_t(slot) * D + n] = (acc + (a.b2 ? a.b2[int64_t(e) * D + n] : 0.f)) * ws.gate[slot];
    } else {
        const int64_t xb = moe_row(a.in, slot / a.top_k);
        const float* w1 = a.w1 + (int64_t(e) * I + n) * D;
        const float* w3 = a.w3 ? a.w3 + (int64_t(e) * I + n) * D : nullptr;
        float u1 = 0.f, u3 = 0.f;
        for (int k = lane; k < D; k += 64) {
            const float xv = ld_any(a.in.p, a.in.f16, xb + int64_t(k) * a.in.sc);
            u1 = fmaf(xv, w1[k], u1);
            if (w3) u3 = fmaf(xv, w3[k], u3);
        }
        u1 = group_sum<64>(u1);
        u3 = group_sum<64>(u3);
        if (lane != 0) return;
        float v = ApplyAct(a.act, 0.f, 0.f, u1 + (a.b1 ? a.b1[int64_t(e) * I + n] : 0.f));
        if (w3) v *= u3 + (a.b3 ? a.b3[int64_t(e) * I + n] : 0.f);
        ws.h[row * I + n] = v;
    }
}

// VEC: half result (and residual), rows one pitch apart, eight columns per lane; else one element per lane of any view
template <bool VEC>
__global__ __launch_bounds__(kMoeBlock) void moe_combine_kernel(const MoeArgs a, const MoeWs ws, const int64_t rows) {
    const int D = a.in.c, k = a.top_k;
    const int per = VEC ? D / 8 : D;
    const int64_t idx = int64_t(blockIdx.x) * kMoeBlock + threadIdx.x;
    if (idx >= rows * per) return;
    const int64_t t = idx / per;
    const int d = int(idx % per) * (VEC ? 8 : 1);
    if constexpr (VEC) {
        float v[8], q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
        if (a.res.p) load16<_Float16>(reinterpret_cast<const _Float16*>(a.res.p) + t * a.res.sw + d, v);
        for (int j = 0; j < k; ++j) {
            const float* p = ws.part + (t * k + j) * D + d;
            load16<float>(p, q);
            load16<float>(p + 4, q + 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += q[i];
        }
        store16<_Float16>(reinterpret_cast<_Float16*>(a.out.p) + t * a.out.sw + d, v);
    } else {
        float v = a.res.p ? ld_any(a.res.p, a.res.f16, moe_row(a.res, t) + int64_t(d) * a.res.sc) : 0.f;
        for (int j = 0; j < k; ++j) v += ws.part[(t * k + j) * D + d];
        st_any(a.out.p, a.out.f16, moe_row(a.out, t) + int64_t(d) * a.out.sc, v);
    }
}

// ---- tile 2 ------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kMgTile = 128;                       // sorted rows of a table entry, and weight rows of a workgroup's LDS image
constexpr int kMgStep = 64;                        // k per step
constexpr int kMgPitch = kMgStep + 8;              // halfs per LDS row: 36 words
constexpr int kMgStage = 2 * kMgTile * kMgPitch;   // halfs per stage: the weight image [128][72], then the activation image [128][72]
constexpr int kMgLdsBytes = 2 * kMgStage * 2;      // 73 728

// what a thread holds of the next K-step while this one's MFMAs run: the 8 k from 8 (tid % 8) on of the image rows tid / 8 + 32 i of either side
struct MgFetch {
    h8 w[4], x[4];
};

// The K loop of tile 2: acc[jn][jm] += W rows (wn * 64 + jn * 32 ..) x A rows (wm * 64 + jm * 32 ..) over K, both sides staged through the two LDS stages.
// wrow[i] / xrow[i] = where image row tid / 8 + 32 i starts in global memory (at k = 8 (tid % 8)), wlive[i] / xlive[i] = it exists (else zeros, nothing is
// read); skip (wave-uniform) = the wave's 64 A rows are all past the entry's count: it stages and meets the barriers, and leaves its accumulators zero
__device__ __forceinline__ void moe_gemm_loop(const _Float16* const* wrow, const bool* wlive, const _Float16* const* xrow, const bool* xlive, int K, bool skip,
                                              _Float16* smem, f32x16 (*acc)[2]) {
    const int tid = int(threadIdx.x), lane = tid % 64, wave = tid / 64;
    const int r = lane % 32, hh = lane / 32, wm = wave / 2, wn = wave % 2;
    const int sr = tid / 8, sk = 8 * (tid % 8);
    auto fetch = [&](int k0) {
        MgFetch f;
        const bool in_k = k0 + sk < K;             // (K % 32 == 0: the 8 k are all inside or all outside)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f.w[i] = f.x[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
            if (wlive[i] && in_k) f.w[i] = *reinterpret_cast<const h8*>(wrow[i] + k0);
            if (xlive[i] && in_k) f.x[i] = *reinterpret_cast<const h8*>(xrow[i] + k0);
        }
        return f;
    };
    auto stage = [&](const MgFetch& f, _Float16* st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<h8*>(st + (sr + 32 * i) * kMgPitch + sk) = f.w[i];
            *reinterpret_cast<h8*>(st + (kMgTile + sr + 32 * i) * kMgPitch + sk) = f.x[i];
        }
    };
    const int nsteps = (K + kMgStep - 1) / kMgStep;
    stage(fetch(0), smem);
    __syncthreads();
    const int woff = (wn * 64 + r) * kMgPitch + 8 * hh, xoff = (kMgTile + wm * 64 + r) * kMgPitch + 8 * hh;
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;          // workgroup-uniform
        MgFetch nxt;
        if (more) nxt = fetch((s + 1) * kMgStep);
        const _Float16* st = smem + (s & 1) * kMgStage;
        if (!skip) {
#pragma unroll
            for (int ks = 0; ks < kMgStep / 16; ++ks) {
                h8 wf[2], xf[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    wf[j] = *reinterpret_cast<const h8*>(st + woff + j * 32 * kMgPitch + 16 * ks);
                    xf[j] = *reinterpret_cast<const h8*>(st + xoff + j * 32 * kMgPitch + 16 * ks);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i / 2][i % 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i / 2], xf[i % 2], acc[i / 2][i % 2], 0, 0, 0);
            }
        }
        if (more) stage(nxt, smem + ((s + 1) & 1) * kMgStage);     // the stage step s - 1 read: every wave is past the barrier that closed it
        __syncthreads();
    }
}

// accumulator element 4 g + q of lane (r, hh) is weight row 8 g + 4 hh + q, A row r of the 32 x 32 tile.  Swapping the quads of groups 2 gp and 2 gp + 1
// between the half-waves leaves lane (r, hh) with the eight weight rows 8 (2 gp + hh) .. of A row r (every lane takes part: no branch around the swaps)
__device__ __forceinline__ void moe_gemm_eight(const f32x16& acc, int gp, float* v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float lo = acc[8 * gp + q], hi = acc[8 * gp + 4 + q];
        const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi), false, false);
        const unsigned s0 = sw[0], s1 = sw[1];
        v[q] = __builtin_bit_cast(float, s0);
        v[4 + q] = __builtin_bit_cast(float, s1);
    }
}

__device__ __forceinline__ void moe_gemm_zero(f32x16 (*acc)[2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i / 2][i % 2][e] = 0.f;
}

// Tile 2, the up product: blockIdx.x = the table entry (fastest: the workgroups resident together share an expert's column strip), blockIdx.y = the column
// tile.  GATED: 64 columns of h; wave wn's 64 weight rows are the 32 columns n0 + 32 wn .. of W1[e], then the same 32 columns of W3[e], so its two column
// accumulators are u1 and u3 of the same h columns in the same lanes.  Plain: 128 columns of W1[e]
template <int ACT, bool GATED>
__global__ __launch_bounds__(kMoeBlock) void moe_gemm_up_kernel(const MoeArgs a, const MoeWs ws) {
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_mg[];
    const int4 tb = ws.tab[blockIdx.x];
    const int e = tb.x, r0 = tb.y, nr = tb.z;
    if (e < 0) return;                             // no such (expert, row block) in this run: nothing is loaded
    const int tid = int(threadIdx.x), lane = tid % 64, wave = tid / 64;
    const int r = lane % 32, hh = lane / 32, wm = wave / 2, wn = wave % 2;
    const int D = a.in.c, I = a.inter;
    const int n0 = int(blockIdx.y) * (GATED ? 64 : kMgTile);
    const int sr = tid / 8, sk = 8 * (tid % 8);
    const _Float16* x = reinterpret_cast<const _Float16*>(a.in.p);
    const _Float16* wrow[4];
    const _Float16* xrow[4];
    bool wlive[4], xlive[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // image row sr + 32 i: gated = (wave column i / 2, W1 or W3 by i % 2); a 32-column group past I reads nothing (I % 32 == 0)
        const int col = n0 + (GATED ? 32 * (i / 2) : 32 * i) + sr;
        wlive[i] = col < I;
        const void* w = GATED && (i % 2) ? a.w3h : a.w1h;
        wrow[i] = reinterpret_cast<const _Float16*>(w) + (int64_t(e) * I + (wlive[i] ? col : 0)) * D + sk;
        xlive[i] = sr + 32 * i < nr;
        const int slot = xlive[i] ? ws.list[r0 + sr + 32 * i] : 0;
        xrow[i] = x + int64_t(slot / a.top_k) * a.in.sw + sk;
    }
    f32x16 acc[2][2];                              // [32 weight rows jn][32 A rows jm] of the wave's quarter
    moe_gemm_zero(acc);
    moe_gemm_loop(wrow, wlive, xrow, xlive, D, wm * 64 >= nr, smem_mg, acc);
    _Float16* h = reinterpret_cast<_Float16*>(ws.h);
#pragma unroll
    for (int jm = 0; jm < 2; ++jm) {
        const int row = wm * 64 + jm * 32 + r;
#pragma unroll
        for (int jn = 0; jn < (GATED ? 1 : 2); ++jn) {
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float v[8], u[8];
                moe_gemm_eight(acc[jn][jm], gp, v);
                if constexpr (GATED) moe_gemm_eight(acc[1][jm], gp, u);
                const int n = n0 + (GATED ? wn * 32 : wn * 64 + jn * 32) + 8 * (2 * gp + hh);
                if (row >= nr || n >= I) continue;                 // (I % 32 == 0: the eight columns are all inside or all outside)
                const int64_t bo = int64_t(e) * I + n;
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = ApplyAct(ACT, 0.f, 0.f, v[i] + (a.b1 ? a.b1[bo + i] : 0.f));
                if constexpr (GATED) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= u[i] + (a.b3 ? a.b3[bo + i] : 0.f);
                }
                store16<_Float16>(h + int64_t(r0 + row) * I + n, v);
            }
        }
    }
}

// Tile 2, the down product: A = h, contiguous in sorted order, B = 128 columns of W2[e]; (sum + b2) * gate[slot] as fp32 into part[slot]
__global__ __launch_bounds__(kMoeBlock) void moe_gemm_down_kernel(const MoeArgs a, const MoeWs ws) {
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_mg[];
    const int4 tb = ws.tab[blockIdx.x];
    const int e = tb.x, r0 = tb.y, nr = tb.z;
    if (e < 0) return;
    const int tid = int(threadIdx.x), lane = tid % 64, wave = tid / 64;
    const int r = lane % 32, hh = lane / 32, wm = wave / 2, wn = wave % 2;
    const int D = a.in.c, I = a.inter;
    const int n0 = int(blockIdx.y) * kMgTile;
    const int sr = tid / 8, sk = 8 * (tid % 8);
    const _Float16* h = reinterpret_cast<const _Float16*>(ws.h);
    const _Float16* wrow[4];
    const _Float16* xrow[4];
    bool wlive[4], xlive[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = n0 + 32 * i + sr;          // (D % 32 == 0: a 32-column group is all inside or all outside)
        wlive[i] = col < D;
        wrow[i] = reinterpret_cast<const _Float16*>(a.w2h) + (int64_t(e) * D + (wlive[i] ? col : 0)) * I + sk;
        xlive[i] = sr + 32 * i < nr;
        xrow[i] = h + int64_t(r0 + (xlive[i] ? sr + 32 * i : 0)) * I + sk;
    }
    f32x16 acc[2][2];
    moe_gemm_zero(acc);
    moe_gemm_loop(wrow, wlive, xrow, xlive, I, wm * 64 >= nr, smem_mg, acc);
#pragma unroll
    for (int jm = 0; jm < 2; ++jm) {
        const int row = wm * 64 + jm * 32 + r;
        const int slot = row < nr ? ws.list[r0 + row] : 0;
        const float gate = row < nr ? ws.gate[slot] : 0.f;
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) {
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float v[8];
                moe_gemm_eight(acc[jn][jm], gp, v);
                const int n = n0 + wn * 64 + jn * 32 + 8 * (2 * gp + hh);
                if (row >= nr || n >= D) continue;
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (v[i] + (a.b2 ? a.b2[int64_t(e) * D + n + i] : 0.f)) * gate;
                float* o = ws.part + int64_t(slot) * D + n;
                store16<float>(o, v);
                store16<float>(o + 4, v + 4);
            }
        }
    }
}

template <int ACT>
void launch_gemm_up(const MoeArgs& a, const MoeWs& ws, unsigned blocks, hipStream_t stream) {
    // the table entries run fastest: the workgroups resident together share an expert's column strip
    if (a.w3h) moe_gemm_up_kernel<ACT, true><<<dim3(blocks, unsigned((a.inter + 63) / 64)), dim3(kMoeBlock), kMgLdsBytes, stream>>>(a, ws);
    else moe_gemm_up_kernel<ACT, false><<<dim3(blocks, unsigned((a.inter + kMgTile - 1) / kMgTile)), dim3(kMoeBlock), kMgLdsBytes, stream>>>(a, ws);
}

template <int ACT, bool GATED>
void launch_up(const MoeArgs& a, const MoeWs& ws, int mt, dim3 grid, hipStream_t stream) {
    if (mt == 1) moe_up_kernel<ACT, GATED, 1><<<grid, dim3(kMoeBlock), 0, stream>>>(a, ws);
    else if (mt == 2) moe_up_kernel<ACT, GATED, 2><<<grid, dim3(kMoeBlock), 0, stream>>>(a, ws);
    else moe_up_kernel<ACT, GATED, 4><<<grid, dim3(kMoeBlock), 0, stream>>>(a, ws);
}

template <int ACT>
void launch_up_gated(const MoeArgs& a, const MoeWs& ws, int mt, dim3 grid, hipStream_t stream) {
    if (a.w3h) launch_up<ACT, true>(a, ws, mt, grid, stream);
    else launch_up<ACT, false>(a, ws, mt, grid, stream);
}

bool same_rows(const TensorArg& x, const TensorArg& y) { return x.n == y.n && x.h == y.h && x.w == y.w; }

}  // namespace

hipError_t InitKernelsMoe() {
    const void* const kernels[] = {
        reinterpret_cast<const void*>(&moe_gemm_up_kernel<0, true>), reinterpret_cast<const void*>(&moe_gemm_up_kernel<0, false>),
        reinterpret_cast<const void*>(&moe_gemm_up_kernel<3, true>), reinterpret_cast<const void*>(&moe_gemm_up_kernel<3, false>),
        reinterpret_cast<const void*>(&moe_gemm_up_kernel<5, true>), reinterpret_cast<const void*>(&moe_gemm_up_kernel<5, false>),
        reinterpret_cast<const void*>(&moe_gemm_up_kernel<6, true>), reinterpret_cast<const void*>(&moe_gemm_up_kernel<6, false>),
        reinterpret_cast<const void*>(&moe_gemm_down_kernel)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kMgLdsBytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool MoeEligible(const MoeArgs& a, int tile) {
    if (tile < 0 || tile >= kNumMoeTiles || !a.in.p || !a.router.p || !a.out.p || !a.w1 || !a.w2 || !a.workspace) return false;
    if (a.in.f8 || a.router.f8 || a.out.f8 || a.res.f8 || a.in.c < 1 || a.inter < 1 || a.out.c != a.in.c) return false;
    if (a.experts < 1 || a.experts > kMoeMaxExperts || a.top_k < 1 || a.top_k > kMoeMaxTopK || a.top_k > a.experts || a.router.c != a.experts) return false;
    if (a.act != 0 && a.act != 3 && a.act != 5 && a.act != 6) return false;
    if (!same_rows(a.in, a.out) || !same_rows(a.in, a.router) || (a.res.p && (!same_rows(a.res, a.out) || a.res.c != a.out.c))) return false;
    const int64_t rows = int64_t(a.in.n) * a.in.h * a.in.w, slots = rows * a.top_k;
    // 32-bit slot and row arithmetic; the workspace holds every part
    if (slots >= (int64_t(1) << 22) || MoeLayout(slots, a.experts, a.in.c, a.inter).total > a.workspace_floats) return false;
    if (tile == 0) return (int64_t(a.in.c > a.inter ? a.in.c : a.inter) + kMoeWaves - 1) / kMoeWaves <= 65535;
    // half operands, rows one pitch apart (a 16-byte vector per lane on every side), whole 32-deep K steps on both products
    if (!a.in.f16 || !a.out.f16 || a.in.c % 32 || a.inter % 32 || !a.w1h || !a.w2h || (a.w3 && !a.w3h)) return false;
    if (!VecViewOk(a.in, 8) || !RowsDense(a.in) || !VecViewOk(a.out, 8) || !RowsDense(a.out)) return false;
    if (a.res.p && (!a.res.f16 || !VecViewOk(a.res, 8) || !RowsDense(a.res))) return false;
    if (!Aligned16(a.w1h) || !Aligned16(a.w2h) || !Aligned16(a.w3h) || !Aligned16(a.workspace)) return false;
    if (tile == 1) return MoeMaxBlocks(slots, a.experts, 16 * MoeRowTiles(slots)) <= 65535;
    // tile 2: the table entries within 65 535 (they would fit the grid's x axis far beyond; the bound keeps either axis order open), the column tiles on y
    return MoeMaxBlocks(slots, a.experts, kMgTile) <= 65535 && (int64_t(a.inter) + 63) / 64 <= 65535 && (int64_t(a.in.c) + kMgTile - 1) / kMgTile <= 65535;
}

hipError_t LaunchMoe(const MoeArgs& a, int tile, hipStream_t stream) {
    if (!MoeEligible(a, tile)) return hipErrorInvalidValue;
    const int64_t rows = int64_t(a.in.n) * a.in.h * a.in.w, slots = rows * a.top_k;
    if (rows == 0) return hipSuccess;
    const int D = a.in.c, I = a.inter;
    const MoeLayout lay(slots, a.experts, D, I);
    float* const w = a.workspace;
    const MoeWs ws{reinterpret_cast<int*>(w + lay.sel), w + lay.gate, reinterpret_cast<int*>(w + lay.offs), reinterpret_cast<int*>(w + lay.list),
                   reinterpret_cast<int4*>(w + lay.tab), w + lay.part, w + lay.h};
    const int mt = MoeRowTiles(slots);
    const int block_rows = tile == 2 ? kMgTile : 16 * mt;
    const int blocks = int(MoeMaxBlocks(slots, a.experts, block_rows));
    const dim3 block(kMoeBlock);
    moe_route_kernel<<<dim3(unsigned((rows + kMoeWaves - 1) / kMoeWaves)), block, 0, stream>>>(a, ws, int(rows));
    moe_group_kernel<<<dim3(1), block, 0, stream>>>(ws, int(slots), a.experts, block_rows, blocks);
    if (tile == 0) {
        moe_generic_kernel<false><<<dim3(unsigned(slots), unsigned((I + kMoeWaves - 1) / kMoeWaves)), block, 0, stream>>>(a, ws);
        moe_generic_kernel<true><<<dim3(unsigned(slots), unsigned((D + kMoeWaves - 1) / kMoeWaves)), block, 0, stream>>>(a, ws);
        moe_combine_kernel<false><<<dim3(unsigned((rows * D + kMoeBlock - 1) / kMoeBlock)), block, 0, stream>>>(a, ws, rows);
        return hipGetLastError();
    }
    if (tile == 2) {
        switch (a.act) {
            case 3: launch_gemm_up<3>(a, ws, unsigned(blocks), stream); break;
            case 5: launch_gemm_up<5>(a, ws, unsigned(blocks), stream); break;
            case 6: launch_gemm_up<6>(a, ws, unsigned(blocks), stream); break;
            default: launch_gemm_up<0>(a, ws, unsigned(blocks), stream); break;
        }
        moe_gemm_down_kernel<<<dim3(unsigned(blocks), unsigned((D + kMgTile - 1) / kMgTile)), block, kMgLdsBytes, stream>>>(a, ws);
        moe_combine_kernel<true><<<dim3(unsigned((rows * (D / 8) + kMoeBlock - 1) / kMoeBlock)), block, 0, stream>>>(a, ws, rows);
        return hipGetLastError();
    }
    const dim3 up(unsigned(I / 16), unsigned(blocks)), down(unsigned(D / 16), unsigned(blocks));
    switch (a.act) {
        case 3: launch_up_gated<3>(a, ws, mt, up, stream); break;
        case 5: launch_up_gated<5>(a, ws, mt, up, stream); break;
        case 6: launch_up_gated<6>(a, ws, mt, up, stream); break;
        default: launch_up_gated<0>(a, ws, mt, up, stream); break;
    }
    if (mt == 1) moe_down_kernel<1><<<down, block, 0, stream>>>(a, ws);
    else if (mt == 2) moe_down_kernel<2><<<down, block, 0, stream>>>(a, ws);
    else moe_down_kernel<4><<<down, block, 0, stream>>>(a, ws);
    moe_combine_kernel<true><<<dim3(unsigned((rows * (D / 8) + kMoeBlock - 1) / kMoeBlock)), block, 0, stream>>>(a, ws, rows);
    return hipGetLastError();
}

}  // namespace ie
