// 4-bit weight-only Linear (com.microsoft MatMulNBits) on gfx950: the Linears of an int4 Llama, which at decode batch sizes are a pure weight stream.
//
//   out[m, n] = sum_k x[m, k] * (q[n, k] - z[n, k / BS]) * s[n, k / BS] + bias[n] + res[m, n]
//
// The operands stay as the ONNX file packs them: codes [N][K / 2] bytes (element 2i of a row in the low nibble of byte i), fp32 scales [N][K / BS],
// zero points [N][ceil(K / BS / 2)] bytes packed the same way (absent: 8).  Nothing is repacked at load and nothing is mirrored.
//
//   qlinear_generic_kernel          tile 0: one wave per output column and block of 8 pixel rows; the lanes split the row's K / 2 bytes (coalesced), every
//                                   weight is (q - z) * s formed in fp32 and met by fp32 FMAs, the 64 partial sums meet in a shuffle tree.  Any view, float
//                                   or half activations: the fallback, the cross-check and the fp32-precision route.
//   qlinear_mfma_kernel<BS, ZP, MT> tile 1 (half activations and result): a workgroup of 4 waves owns 16 output columns and MT <= 4 tiles of 16 pixel
//                                   rows; larger M is a second grid axis of 64-row blocks that re-streams the strip from L2.
//
// Tile 1, per wave and K-chunk of 128 (the waves take the chunks round-robin: split K inside the workgroup):
//   * lane (c = lane % 16, g = lane / 16) reads ONE 16-byte vector of column n0 + c: the 32 consecutive k from chunk + 32 g on.  That is one scale and
//     one zero point at every block size (32 divides BS), read straight into registers: the weights never pass through LDS and are read exactly once
//     per 64 rows.  The next chunk's vector, scale and zero point are in flight while this one is expanded.
//   * the four dwords of the vector feed four consecutive v_mfma_f32_16x16x32_f16: MFMA j takes dword j, eight k of every one of the four lane groups,
//     so its 32-deep K is {chunk + 32 g + 8 j + i}: a permuted walk of K, which a sum may take in any order as long as both operands agree.
//   * a dword expands two nibbles per step: ((d >> 4 p) & 0x000F000F) | 0x64006400 is the half pair (1024 + q[p], 1024 + q[p + 4]); one packed half
//     subtract of (1024 + z) leaves the exact integers q - z, and float(q - z) * s rounds ONCE into the half the MFMA reads (v_fma_mix).  So the B
//     fragment holds k in the order 0 4 1 5 2 6 3 7, and the activation fragment -- eight consecutive halfs of row m, one 16-byte load from the
//     L2-resident activations -- is shuffled into the same order in registers.  Rows past M load nothing and enter as zeros.
//   * K need only be a multiple of 32: a lane group whose 32 k lie past K feeds zeros on both sides.
// Then the four waves' accumulators meet in LDS and are summed in wave order (fixed: two runs are bit-equal), and the epilogue -- bias, residual, the
// conversion to half -- leaves in 16-byte stores, eight columns of one row per lane.  LDS: 4 x MT x 1 KiB, only for that reduction.
//
//   qlinear_gemm_kernel<BS, ZP>     tile 2 (half activations and result; prefill row counts): a workgroup of 4 waves owns 128 rows x 128
//                                   columns, wave (wm, wn) a 64 x 64 quarter in 2 x 2 accumulators of v_mfma_f32_32x32x16_f16 (64 registers).
//
// Tile 2, per K-step of 64:
//   * weights: thread t reads ONE 16-byte vector, the 32 codes k0 + 32 (t % 2) .. of column n0 + t / 2, with their one scale and zero point (tile 1's
//     ql_load), expands them with tile 1's ql_expand -- the same halfs, bit for bit -- puts each group of eight back into the order 0 .. 7 (a register
//     renaming: the two halfs of a pair land in other dwords) and writes four 16-byte vectors into the LDS image W[column][k].  Every packed byte of
//     the strip is read and expanded once per workgroup and K-step: once per 128 rows where tile 1 does it once per 64, and by 256 lanes at once.
//   * activations: thread t reads four 16-byte vectors, k0 + 8 (t % 8) .. of rows t / 8 + 32 i, and writes them to the LDS image X[row][k] as they are.
//     Rows past M, columns past N and k past K enter as zeros (nothing is read for them).
//   * both images have rows of 64 + 8 halfs: a pitch of 36 words, so the 16 lanes of a ds_read_b128 group fall on 16 different bank quads (the
//     layout of the attention K / V images).  A fragment of either side is lane (r = lane % 32, hh = lane / 32) reading the eight halfs
//     k = 16 ks + 8 hh .. of row r: per 16 k a wave reads two weight and two activation fragments for four MFMAs.
//   * two LDS stages: the loads of step s + 1 are issued before the MFMAs of step s, expanded and written into the other stage after them, and ONE
//     barrier closes the step.  LDS: 2 x 256 x 72 x 2 = 73 728 bytes, two workgroups per CU.
// D = W x X^T (the weights are the MFMA's first operand): a lane owns one row m and quads of consecutive columns; v_permlane32_swap trades quads between
// the half-waves so that each lane holds eight consecutive columns, and bias, residual and the one rounding to half leave as in tile 1, in 16-byte
// stores.  No K split and no atomics: every output is one fixed-order sum.  The grid runs the row blocks fastest, so that the workgroups resident
// together share column strips of the weights.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {
namespace {

constexpr int kQlBlock = 256;          // 4 waves
constexpr int kQlWaves = kQlBlock / 64;
constexpr int kQlRows = 8;             // generic kernel: pixel rows per wave
constexpr int kQlChunk = 128;          // MFMA kernel: k per wave and step (4 lane groups x 32)

// the zero point of block `blk` of a row whose packed zero points start at zrow (null: 8)
__device__ __forceinline__ int ql_zero_point(const uint8_t* zrow, int blk) {
    return zrow ? (zrow[blk >> 1] >> (4 * (blk & 1))) & 15 : 8;
}

__global__ __launch_bounds__(kQlBlock) void qlinear_generic_kernel(const QLinearArgs a, const int64_t rows) {
    const int lane = int(threadIdx.x) % 64;
    const int n = int(blockIdx.x) * kQlWaves + int(threadIdx.x) / 64;
    if (n >= a.out.c) return;                      // wave-uniform
    const int K = a.in.c, nblk = K / a.block;
    const int64_t m0 = int64_t(blockIdx.y) * kQlRows;
    const uint8_t* qrow = a.codes + int64_t(n) * (K / 2);
    const float* srow = a.scales + int64_t(n) * nblk;
    const uint8_t* zrow = a.zps ? a.zps + int64_t(n) * ((nblk + 1) / 2) : nullptr;
    int64_t ib[kQlRows], ob[kQlRows], rb[kQlRows];
#pragma unroll
    for (int r = 0; r < kQlRows; ++r) {
        const int64_t m = m0 + r < rows ? m0 + r : rows - 1;       // (a row past the end repeats the last one and is not stored)
        const int px = int(m % a.in.w);
        const int64_t t = m / a.in.w;
        const int py = int(t % a.in.h);
        const int64_t pn = t / a.in.h;
        ib[r] = pn * a.in.sn + int64_t(py) * a.in.sh + int64_t(px) * a.in.sw;
        ob[r] = pn * a.out.sn + int64_t(py) * a.out.sh + int64_t(px) * a.out.sw;
        rb[r] = a.res.p ? pn * a.res.sn + int64_t(py) * a.res.sh + int64_t(px) * a.res.sw : 0;
    }
    float acc[kQlRows];
#pragma unroll
    for (int r = 0; r < kQlRows; ++r) acc[r] = 0.f;
    for (int b = lane; b < K / 2; b += 64) {
        const int k = 2 * b, blk = k / a.block;
        const unsigned q = qrow[b];
        const float s = srow[blk], z = float(ql_zero_point(zrow, blk));
        const float w0 = (float(q & 15u) - z) * s, w1 = (float(q >> 4) - z) * s;
#pragma unroll
        for (int r = 0; r < kQlRows; ++r) {
            acc[r] = fmaf(ld_any(a.in.p, a.in.f16, ib[r] + int64_t(k) * a.in.sc), w0, acc[r]);
            acc[r] = fmaf(ld_any(a.in.p, a.in.f16, ib[r] + int64_t(k + 1) * a.in.sc), w1, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kQlRows; ++r) acc[r] = group_sum<64>(acc[r]);
    if (lane != 0) return;
    const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < kQlRows; ++r) {
        if (m0 + r >= rows) break;
        float v = acc[r] + bias;
        if (a.res.p) v += ld_any(a.res.p, a.res.f16, rb[r] + int64_t(n) * a.res.sc);
        st_any(a.out.p, a.out.f16, ob[r] + int64_t(n) * a.out.sc, v);
    }
}

// what a lane holds of one chunk: the 32 codes, their scale, and 1024 + zero point as a half pair
struct QlWeights {
    u32x4 q;
    float s;
    h2 zs;
};

template <int BS, bool ZP>
__device__ __forceinline__ QlWeights ql_load(const uint8_t* qrow, const float* srow, const uint8_t* zrow, int k, int K) {
    QlWeights w;
    w.q = u32x4{0u, 0u, 0u, 0u};
    w.s = 0.f;
    w.zs = h2{_Float16(1032.f), _Float16(1032.f)};
    if (k < K) {                                   // (K % 32 == 0: the lane's 32 k are all inside or all outside)
        w.q = *reinterpret_cast<const u32x4*>(qrow + k / 2);
        const int blk = k / BS;
        w.s = srow[blk];
        if constexpr (ZP) {
            const _Float16 z = _Float16(float(1024 + ql_zero_point(zrow, blk)));
            w.zs = h2{z, z};
        }
    }
    return w;
}

// dword j of the codes -> the B fragment of MFMA j: the halfs of k = 0 4 1 5 2 6 3 7 of its eight, each float(q - z) * s rounded once
__device__ __forceinline__ h8 ql_expand(unsigned d, const QlWeights& w) {
    h8 b;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned t = ((d >> (4 * p)) & 0x000F000Fu) | 0x64006400u;
        const h2 dq = __builtin_bit_cast(h2, t) - w.zs;        // exact: integers below 2048
        b[2 * p] = _Float16(float(dq[0]) * w.s);
        b[2 * p + 1] = _Float16(float(dq[1]) * w.s);
    }
    return b;
}

template <int BS, bool ZP, int MT>
__global__ __launch_bounds__(kQlBlock) void qlinear_mfma_kernel(const QLinearArgs a, const int rows) {
    __shared__ float red[kQlWaves][MT][64][4];
    const int lane = int(threadIdx.x) % 64, wave = int(threadIdx.x) / 64;
    const int c = lane % 16, g = lane / 16;
    const int K = a.in.c, N = a.out.c;
    const int n0 = int(blockIdx.x) * 16, m0 = int(blockIdx.y) * (16 * MT);
    const int nblk = K / BS;
    const uint8_t* qrow = a.codes + int64_t(n0 + c) * (K / 2);
    const float* srow = a.scales + int64_t(n0 + c) * nblk;
    const uint8_t* zrow = ZP ? a.zps + int64_t(n0 + c) * ((nblk + 1) / 2) : nullptr;
    const _Float16* x = reinterpret_cast<const _Float16*>(a.in.p);
    // the activation rows this lane loads for the MT row tiles (row tile t: m0 + 16 t + c); a row past M loads nothing
    const _Float16* xrow[MT];
    bool live[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = m0 + 16 * t + c;
        live[t] = m < rows;
        xrow[t] = x + int64_t(live[t] ? m : 0) * a.in.sw;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunks = (K + kQlChunk - 1) / kQlChunk;
    int k = wave * kQlChunk + 32 * g;
    QlWeights cur = ql_load<BS, ZP>(qrow, srow, zrow, k, K);
    for (int ch = wave; ch < nchunks; ch += kQlWaves) {
        const int kn = k + kQlWaves * kQlChunk;
        const QlWeights nxt = ql_load<BS, ZP>(qrow, srow, zrow, ch + kQlWaves < nchunks ? kn : K, K);
        const bool in_k = k < K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const h8 b = ql_expand(cur.q[j], cur);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                h8 xa = h8{0, 0, 0, 0, 0, 0, 0, 0};
                if (live[t] && in_k) xa = *reinterpret_cast<const h8*>(xrow[t] + k + 8 * j);
                const h8 af = __builtin_shufflevector(xa, xa, 0, 4, 1, 5, 2, 6, 3, 7);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, b, acc[t], 0, 0, 0);
            }
        }
        cur = nxt;
        k = kn;
    }
    // accumulator element v of lane (c, g) is row 4 g + v, column c of the 16 x 16 tile
#pragma unroll
    for (int t = 0; t < MT; ++t)
        *reinterpret_cast<f32x4*>(&red[wave][t][lane][0]) = acc[t];
    __syncthreads();
    // one lane per (row tile, row, 8 columns): the four waves' sums in wave order, the epilogue, a 16-byte store
    for (int idx = int(threadIdx.x); idx < MT * 32; idx += kQlBlock) {
        const int t = idx / 32, r = (idx % 32) / 2, c0 = (idx % 2) * 8;
        const int m = m0 + 16 * t + r;
        if (m >= rows) continue;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int src = (r / 4) * 16 + c0 + i;
            float s = red[0][t][src][r % 4];
#pragma unroll
            for (int w = 1; w < kQlWaves; ++w) s += red[w][t][src][r % 4];
            v[i] = s;
        }
        if (a.bias) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += a.bias[n0 + c0 + i];
        }
        if (a.res.p) {
            float rv[8];
            load16<_Float16>(reinterpret_cast<const _Float16*>(a.res.p) + int64_t(m) * a.res.sw + n0 + c0, rv);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += rv[i];
        }
        store16<_Float16>(reinterpret_cast<_Float16*>(a.out.p) + int64_t(m) * a.out.sw + n0 + c0, v);
    }
    (void)N;
}

template <int BS, bool ZP>
hipError_t launch_mfma(const QLinearArgs& a, int rows, hipStream_t stream) {
    const dim3 block(kQlBlock);
    const unsigned cols = unsigned(a.out.c / 16);
    if (rows <= 16) qlinear_mfma_kernel<BS, ZP, 1><<<dim3(cols, 1), block, 0, stream>>>(a, rows);
    else if (rows <= 32) qlinear_mfma_kernel<BS, ZP, 2><<<dim3(cols, 1), block, 0, stream>>>(a, rows);
    else if (rows <= 48) qlinear_mfma_kernel<BS, ZP, 3><<<dim3(cols, 1), block, 0, stream>>>(a, rows);
    else qlinear_mfma_kernel<BS, ZP, 4><<<dim3(cols, unsigned((rows + 63) / 64)), block, 0, stream>>>(a, rows);
    return hipGetLastError();
}

template <int BS>
hipError_t launch_mfma_zp(const QLinearArgs& a, int rows, hipStream_t stream) {
    return a.zps ? launch_mfma<BS, true>(a, rows, stream) : launch_mfma<BS, false>(a, rows, stream);
}

// ---- tile 2 ------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kQgTile = 128;                       // rows and columns of a workgroup's output tile
constexpr int kQgStep = 64;                        // k per step
constexpr int kQgPitch = kQgStep + 8;              // halfs per LDS row: 36 words
constexpr int kQgStage = 2 * kQgTile * kQgPitch;   // halfs per stage: the weight image [128][72], then the activation image [128][72]
constexpr int kQgLdsBytes = 2 * kQgStage * 2;      // 73 728

// what a thread holds of the next K-step while this one's MFMAs run
struct QgFetch {
    QlWeights w;
    h8 x[4];
};

template <int BS, bool ZP>
__global__ __launch_bounds__(kQlBlock) void qlinear_gemm_kernel(const QLinearArgs a, const int rows) {
    extern __shared__ __attribute__((aligned(16))) _Float16 smem_qg[];
    const int tid = int(threadIdx.x), lane = tid % 64, wave = tid / 64;
    const int r = lane % 32, hh = lane / 32, wm = wave / 2, wn = wave % 2;
    const int K = a.in.c, N = a.out.c;
    const int m0 = int(blockIdx.x) * kQgTile, n0 = int(blockIdx.y) * kQgTile;
    const int nblk = K / BS;
    // staging roles.  Weights: column wc, the 32 k from 32 wk on; a column past N reads nothing (its k is K: ql_load's zeros)
    const int wc = tid / 2, wk = 32 * (tid % 2);
    const bool wlive = n0 + wc < N;
    const int wcol = wlive ? n0 + wc : n0;
    const uint8_t* qrow = a.codes + int64_t(wcol) * (K / 2);
    const float* srow = a.scales + int64_t(wcol) * nblk;
    const uint8_t* zrow = ZP ? a.zps + int64_t(wcol) * ((nblk + 1) / 2) : nullptr;
    // activations: rows xr + 32 i, the 8 k from xk on; a row past M reads nothing
    const int xr = tid / 8, xk = 8 * (tid % 8);
    const _Float16* xrow[4];
    bool xlive[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + xr + 32 * i;
        xlive[i] = m < rows;
        xrow[i] = reinterpret_cast<const _Float16*>(a.in.p) + int64_t(xlive[i] ? m : 0) * a.in.sw + xk;
    }
    auto fetch = [&](int k0) {
        QgFetch f;
        f.w = ql_load<BS, ZP>(qrow, srow, zrow, wlive ? k0 + wk : K, K);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f.x[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
            if (xlive[i] && k0 + xk < K) f.x[i] = *reinterpret_cast<const h8*>(xrow[i] + k0);      // (K % 32 == 0: the 8 k are all inside or all outside)
        }
        return f;
    };
    auto stage = [&](const QgFetch& f, _Float16* st) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const h8 b = ql_expand(f.w.q[j], f.w);                 // k in the order 0 4 1 5 2 6 3 7
            *reinterpret_cast<h8*>(st + wc * kQgPitch + wk + 8 * j) = __builtin_shufflevector(b, b, 0, 2, 4, 6, 1, 3, 5, 7);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<h8*>(st + (kQgTile + xr + 32 * i) * kQgPitch + xk) = f.x[i];
    };

    f32x16 acc[2][2];                                  // [32 columns jn][32 rows jm] of the wave's quarter
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i / 2][i % 2][e] = 0.f;

    const int nsteps = (K + kQgStep - 1) / kQgStep;
    stage(fetch(0), smem_qg);
    __syncthreads();
    const int woff = (wn * 64 + r) * kQgPitch + 8 * hh, xoff = (kQgTile + wm * 64 + r) * kQgPitch + 8 * hh;
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;                          // workgroup-uniform
        QgFetch nxt;
        if (more) nxt = fetch((s + 1) * kQgStep);
        const _Float16* st = smem_qg + (s & 1) * kQgStage;
#pragma unroll
        for (int ks = 0; ks < kQgStep / 16; ++ks) {
            h8 wf[2], xf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                wf[j] = *reinterpret_cast<const h8*>(st + woff + j * 32 * kQgPitch + 16 * ks);
                xf[j] = *reinterpret_cast<const h8*>(st + xoff + j * 32 * kQgPitch + 16 * ks);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i / 2][i % 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i / 2], xf[i % 2], acc[i / 2][i % 2], 0, 0, 0);
        }
        if (more) stage(nxt, smem_qg + ((s + 1) & 1) * kQgStage);  // the stage step s - 1 read: every wave is past the barrier that closed it
        __syncthreads();
    }
    // accumulator element 4 g + q of lane (r, hh) is column 8 g + 4 hh + q, row r of the 32 x 32 tile.  Swapping the quads of groups 2 gp and 2 gp + 1
    // between the half-waves leaves lane (r, hh) with the eight columns 8 (2 gp + hh) .. of row r (every lane takes part: no branch around the swaps)
#pragma unroll
    for (int jm = 0; jm < 2; ++jm) {
        const int m = m0 + wm * 64 + jm * 32 + r;
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) {
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float lo = acc[jn][jm][8 * gp + q], hi = acc[jn][jm][8 * gp + 4 + q];      // (values: a bit cast of a vector element reads element 0)
                    const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi), false, false);
                    const unsigned s0 = sw[0], s1 = sw[1];
                    v[q] = __builtin_bit_cast(float, s0);
                    v[4 + q] = __builtin_bit_cast(float, s1);
                }
                const int n = n0 + wn * 64 + jn * 32 + 8 * (2 * gp + hh);
                if (m >= rows || n >= N) continue;                 // (N % 16 == 0: the eight columns are all inside or all outside)
                if (a.bias) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] += a.bias[n + i];
                }
                if (a.res.p) {
                    float rv[8];
                    load16<_Float16>(reinterpret_cast<const _Float16*>(a.res.p) + int64_t(m) * a.res.sw + n, rv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] += rv[i];
                }
                store16<_Float16>(reinterpret_cast<_Float16*>(a.out.p) + int64_t(m) * a.out.sw + n, v);
            }
        }
    }
}

template <int BS>
hipError_t launch_gemm(const QLinearArgs& a, int rows, hipStream_t stream) {
    // the row blocks run fastest: the workgroups resident together share column strips of the weights
    const dim3 grid(unsigned((rows + kQgTile - 1) / kQgTile), unsigned((a.out.c + kQgTile - 1) / kQgTile));
    if (a.zps) qlinear_gemm_kernel<BS, true><<<grid, dim3(kQlBlock), kQgLdsBytes, stream>>>(a, rows);
    else qlinear_gemm_kernel<BS, false><<<grid, dim3(kQlBlock), kQgLdsBytes, stream>>>(a, rows);
    return hipGetLastError();
}

bool same_shape(const TensorArg& x, const TensorArg& y) { return x.n == y.n && x.h == y.h && x.w == y.w; }

}  // namespace

hipError_t InitKernelsQLinear() {
    const void* const kernels[] = {
        reinterpret_cast<const void*>(&qlinear_gemm_kernel<32, true>), reinterpret_cast<const void*>(&qlinear_gemm_kernel<32, false>),
        reinterpret_cast<const void*>(&qlinear_gemm_kernel<64, true>), reinterpret_cast<const void*>(&qlinear_gemm_kernel<64, false>),
        reinterpret_cast<const void*>(&qlinear_gemm_kernel<128, true>), reinterpret_cast<const void*>(&qlinear_gemm_kernel<128, false>)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kQgLdsBytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool QLinearEligible(const QLinearArgs& a, int tile) {
    if (tile < 0 || tile >= kNumQLinearTiles || !a.in.p || !a.out.p || !a.codes || !a.scales) return false;
    if (a.in.f8 || a.out.f8 || a.res.f8 || a.in.c < 2 || a.out.c < 1 || !same_shape(a.in, a.out)) return false;
    if ((a.block != 32 && a.block != 64 && a.block != 128) || a.in.c % a.block) return false;
    if (a.res.p && (!same_shape(a.res, a.out) || a.res.c != a.out.c)) return false;
    if (tile == 0) return true;
    const int64_t rows = int64_t(a.in.n) * a.in.h * a.in.w;
    // half operands, rows one pitch apart (a 16-byte vector per lane on every side), whole 16-column tiles, and 32-bit row arithmetic
    if (!a.in.f16 || !a.out.f16 || a.out.c % 16 || rows >= (int64_t(1) << 22) || rows > 65535 * 64) return false;
    if (!VecViewOk(a.in, 8) || !RowsDense(a.in) || !VecViewOk(a.out, 8) || !RowsDense(a.out)) return false;
    if (a.res.p && (!a.res.f16 || !VecViewOk(a.res, 8) || !RowsDense(a.res))) return false;
    if (!Aligned16(a.codes) || a.out.c / 16 > 0x7fffffff) return false;
    // tile 2: the row blocks within 65 535 (they would fit the grid's x axis far beyond; the bound keeps either axis order open), the column tiles on y
    return tile == 1 || ((rows + kQgTile - 1) / kQgTile <= 65535 && (a.out.c + kQgTile - 1) / kQgTile <= 65535);
}

hipError_t LaunchQLinear(const QLinearArgs& a, int tile, hipStream_t stream) {
    if (!QLinearEligible(a, tile)) return hipErrorInvalidValue;
    const int64_t rows = int64_t(a.in.n) * a.in.h * a.in.w;
    if (rows == 0) return hipSuccess;
    if (tile == 0) {
        const int64_t gy = (rows + kQlRows - 1) / kQlRows;
        if (gy > 65535) return hipErrorInvalidValue;
        hipLaunchKernelGGL(qlinear_generic_kernel, dim3(unsigned((a.out.c + kQlWaves - 1) / kQlWaves), unsigned(gy)), dim3(kQlBlock), 0, stream, a, rows);
        return hipGetLastError();
    }
    if (tile == 2) {
        switch (a.block) {
            case 32: return launch_gemm<32>(a, int(rows), stream);
            case 64: return launch_gemm<64>(a, int(rows), stream);
            default: return launch_gemm<128>(a, int(rows), stream);
        }
    }
    switch (a.block) {
        case 32: return launch_mfma_zp<32>(a, int(rows), stream);
        case 64: return launch_mfma_zp<64>(a, int(rows), stream);
        default: return launch_mfma_zp<128>(a, int(rows), stream);
    }
}

}  // namespace ie
