// DenseNet transition in one launch (fp32): BN -> ReLU -> 2x2 / stride 2 average pool -> 1x1 conv, and optionally the entry 1x1 conv of the
// next dense block behind it.
//
// The planner runs a transition as pool_kernel (BN + ReLU prologue, pooled tensor to memory), then conv1x1_as_kernel on the pooled tensor, then
// conv1x1_as_kernel again for the next block's entry conv on the channels the transition conv has just written.  conv1x1_pooled_kernel is
// conv1x1_as_kernel (kernels_direct.hip: activations-stationary, fragment-major weight ring, v_mfma_f32_16x16x4_f32, one accumulator walked
// in chunk order, quad stores) with two additions:
//   (a) pooled staging: LDS row m = (b, oy, ox) is built from the four input pixels (2 oy + ky, 2 ox + kx) exactly as pool_kernel<4> builds
//       the pooled tensor -- fma(x, scale, shift) (the compiler contracts pool_kernel's multiply-add to v_fma_f32), max(., 0) if the prologue has
//       a ReLU, summed in (ky, kx) order into an accumulator that starts at +0, times 0.25f -- so the staged row is bit-equal to the tensor the
//       pool step would have written, and the GEMM behind it is the as-kernel's, chunk for chunk.  The pooled tensor is never written.
//   (b) CHAIN: the workgroup's tile holds every output channel of the transition conv (grid.y == 1).  After the usual stores each lane also
//       writes fma(v, scale2, shift2) (then the ReLU) of its quads into LDS rows [pixel][Cout + pad] -- the value the entry conv's staging
//       would have formed from the stored tensor -- and every wave runs the as-kernel's loop again over those rows for 16 of the entry conv's
//       128 output channels.  Same operands, same chunk order, same accumulator: bit-equal to conv1x1_as_kernel on the stored tensor.
// m -> (b, oy, ox): the tile's first pixel is split on the scalar unit (host-passed 2^32 reciprocals, one correction step); a lane's row adds
// at most 31 pixels to it, resolved with 24-bit multiplies by host-passed 2^20 reciprocals (kernels.h FusedConsts): no division, no
// quarter-rate multiply.  Rows from M on map to image index >= N: their byte offset lies behind the buffer descriptor's range and reads zeros.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "device_util.h"
#include "env.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {

namespace {

// v * s for factors below 2^24 on the full-rate 24-bit multiplier, s wave-uniform (a kernel argument or derived from one).  Written as the
// instruction itself: the optimiser rewrites __umul24 into a 32-bit multiply -- quarter rate -- wherever it learns the range of one operand, and the
// instruction selector finds the 24-bit form again only when it can prove both ranges inside one basic block, which a factor hoisted out of the
// staging loop never allows
__device__ __forceinline__ unsigned mul24(unsigned v, unsigned s) {
    unsigned r;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "s"(s), "v"(v));
    return r;
}

// conv1x1_as_kernel's K loop: this wave's 16 * TNW output channels (16-channel blocks nb ..) over CH chunks of 16 input channels, activations
// from LDS rows of pitch P floats, weights from the fragment-major mirror through a D-deep register ring with static slots.
template <int TNW, int PB, int D>
struct AsLoop {
    u32x4 ring[D][TNW];
    int c_l = 0;
    __device__ __forceinline__ void issue(const __amdgpu_buffer_rsrc_t rs_w, unsigned wlane, int nb, int CH, int slot) {
        const int c = c_l < CH ? c_l : CH - 1;             // past the last chunk the last chunk is loaded again (in range, never consumed)
#pragma unroll
        for (int j = 0; j < TNW; ++j) ring[slot][j] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, wlane, ((nb + j) * CH + c) * 1024, 0);
        ++c_l;
    }
    // every ring slot holds its chunk; acc must be zero on entry
    __device__ __forceinline__ void run(const __amdgpu_buffer_rsrc_t rs_w, unsigned wlane, int nb, int CH, const float* sA, int P, int r, int gk, f32x4 (&acc)[PB][TNW]) {
        const float* abase[PB];                            // this lane's fragment address in each pixel block, at the current ring trip
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) abase[pb] = sA + (mul24(r, P) + pb * 16 * P + gk * 4);
        // activation fragments are read one chunk ahead of the MFMAs that consume them; the read ahead of the last chunk runs 16 floats past K:
        // the row's pad and the head of the next row (the launcher allocates 64 bytes behind the last row)
        f32x4 avn[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) avn[pb] = *reinterpret_cast<const f32x4*>(abase[pb]);
        auto compute = [&](int slot) {
            f32x4 av[PB];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) av[pb] = avn[pb];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) avn[pb] = *reinterpret_cast<const f32x4*>(abase[pb] + (slot + 1) * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < TNW; ++j)
#pragma unroll
                    for (int pb = 0; pb < PB; ++pb)
                        acc[pb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, ring[slot][j])[e], av[pb][e], acc[pb][j], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, PB, 0);                 // next chunk's fragment reads first ...
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * PB * TNW, 0);       // ... then this chunk's MFMAs
        };
        const int full = CH / D, rem = CH - full * D;
        for (int it = 0; it < full; ++it) {
#pragma unroll
            for (int s = 0; s < D; ++s) {
                compute(s);
                issue(rs_w, wlane, nb, CH, s);
            }
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) abase[pb] += D * 16;
        }
#pragma unroll
        for (int s = 0; s < D; ++s)
            if (s < rem) compute(s);                       // wave-uniform: the last CH % D chunks are already in their slots
    }
};

}  // namespace

// a.in: the POOLED view (shape only: the tensor is never read or written); a.debug: LDS row pad << 8 | log2(staging columns) << 16 (launcher).
// CHAIN: blockIdx.y == 0 only, Cout == 16 * TNW * WAVES, the second conv has 16 * WAVES output channels.
template <int WAVES, int TNW, int PB, bool PRE, bool CHAIN>
__global__ __launch_bounds__(64 * WAVES) void conv1x1_pooled_kernel(const ConvArgs a, const PooledArgs p) {
    constexpr int NT = 64 * WAVES, D = PB == 1 ? 16 : 8, BNW = 16 * TNW, BN = BNW * WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_trans[];
    float* const sA = reinterpret_cast<float*>(smem_trans);                        // [16 * PB][P]

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pad = (a.debug >> 8) & 0xff;
    const int K = a.in.c, P = K + pad, CH = K >> 4, Cout = a.out.c;
    const int M = a.out.n * a.out.h * a.out.w;
    const int m0 = blockIdx.x * (16 * PB), n0 = blockIdx.y * BN + wave * BNW;
    const int ipitch = int(p.pin.sw), opitch = int(a.out.sw);

    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wfrag), 0, Cout * K * 4, kBufferRsrcFlags);
    const int nb = n0 >> 4;
    AsLoop<TNW, PB, D> loop;
    unsigned wlane = unsigned(tid & 63) * 16u;
    // the last quarter of the ring is primed behind the staging loop (its slots are first consumed 3/4 of a ring trip after the barrier)
    constexpr int DLATE = D / 4;
#pragma unroll
    for (int s = 0; s < D - DLATE; ++s) loop.issue(rs_w, wlane, nb, CH, s);

    // ---- this workgroup's 16 * PB POOLED pixel rows -> LDS ----
    // As in conv1x1_as_kernel a thread keeps one 4-channel column (of CT = 1 << cs) and walks rows; K > 4 * CT is walked in column blocks with the
    // prologue constants loaded once per block.  A row is one output pixel: its window's first input pixel is found from (b, oy, ox), the four
    // window pixels are the scalar offsets 0, one pixel, one image row, both.
    {
        constexpr int R = 16 * PB;
        static_assert(R * 64 >= NT, "the widest column block (64 columns) must not span more rows than the tile has");      // (the launcher picks cs so that NT >> cs <= R)
        const int cs = a.debug >> 16, CT = 1 << cs;
        const int rstep = NT >> cs, npass = R / rstep;                            // wave-uniform (R, NT and CT are powers of two)
        const int col = tid & (CT - 1), row0 = tid >> cs;
        const unsigned IH = unsigned(p.pin.h), IW = unsigned(p.pin.w), OH = unsigned(a.out.h), OW = unsigned(a.out.w);
        const int in_px = p.pin.n * p.pin.h * p.pin.w;
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(p.pin.p, 0, ((in_px - 1) * ipitch + K) * 4, kBufferRsrcFlags);
        const __amdgpu_buffer_rsrc_t rs_sc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pool_scale), 0, PRE ? K * 4 : 0, kBufferRsrcFlags);
        const __amdgpu_buffer_rsrc_t rs_sf = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.pool_shift), 0, PRE ? K * 4 : 0, kBufferRsrcFlags);
        // the tile's first pixel, on the scalar unit
        const unsigned ohw = OH * OW;
        const unsigned b0 = udiv_uniform(unsigned(m0), ohw, p.k.mg32_ohw), rem0 = unsigned(m0) - b0 * ohw;
        const unsigned oy0 = udiv_uniform(rem0, OW, p.k.mg32_ow), ox0 = rem0 - oy0 * OW;
        const unsigned pitch4 = unsigned(ipitch) * 4u;
        const int tap_x = int(pitch4), tap_y = int(IW * pitch4);                   // byte offsets of the window's other pixels (scalar)
        const unsigned c16 = unsigned(col) * 16u;                                  // byte offset of the lane's column within a block
        // byte offset of the window of tile row `row` (< 32): ox0 + row < OW + 31 and oy0 + q < OH + 31, so the 2^20 reciprocals are exact
        // (launcher: OW, OH <= 512) and every product fits 24 x 24 -> 32 bits (launcher: input pixels and byte pitch below 2^24)
        auto window = [&](unsigned row) {
            const unsigned n = ox0 + row;
            const unsigned q = mul24(n, p.k.mg20_ow) >> 20;
            const unsigned ox = n - mul24(q, OW);
            const unsigned y = oy0 + q;
            const unsigned q2 = mul24(y, p.k.mg20_oh) >> 20;
            const unsigned oy = y - mul24(q2, OH);
            const unsigned ipx = mul24(mul24(b0 + q2, IH) + 2u * oy, IW) + 2u * ox;
            return mul24(ipx, pitch4);
        };
        unsigned row = unsigned(row0);
        unsigned cb = c16;                                                         // + the column block's byte offset
        unsigned char* l = smem_trans + (mul24(row0, P) * 4u + c16);             // the LDS address itself
        const int lstep = rstep * P * 4, lnext = CT * 16 - npass * lstep;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        auto stage = [&](auto relu_) {                                             // the prologue's ReLU is decided once, not per element
            constexpr bool RELU = decltype(relu_)::value;
            for (int left = K * 4; left > 0; left -= CT * 16) {                    // bytes of a row from this column block on
                if (c16 < unsigned(left)) {
                    f32x4 sc = zero, sf = zero;
                    if constexpr (PRE) {
                        sc = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_sc, c16, K * 4 - left, 0));
                        sf = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_sf, c16, K * 4 - left, 0));
                    }
                    auto group = [&](auto n_) {                                    // N rows: their 4 N loads in flight, then prologue + pool + LDS write
                        constexpr int N = decltype(n_)::value;
                        asm volatile("; ie-mark pooled-stage n=%0 relu=%1" ::"n"(N), "n"(int(RELU)));   // names the variant's blocks for scripts/isa_mix.py
                        u32x4 v[N][4];
#pragma unroll
                        for (int u = 0; u < N; ++u) {
                            const unsigned g = window(row) + cb;
                            v[u][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, g, 0, 0);
                            v[u][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, g, tap_x, 0);
                            v[u][2] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, g, tap_y, 0);
                            v[u][3] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, g, tap_y + tap_x, 0);
                            row += unsigned(rstep);
                        }
#pragma unroll
                        for (int u = 0; u < N; ++u) {
                            f32x4 acc = zero;                                      // pool_kernel<4>: +0, then the window in (ky, kx) order
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                f32x4 x = __builtin_bit_cast(f32x4, v[u][t]);
                                if constexpr (PRE) x = __builtin_elementwise_fma(x, sc, sf);       // one rounding per element, as v_fma_f32
                                if constexpr (PRE && RELU) x = __builtin_elementwise_max(x, zero);
                                acc = acc + x;
                            }
                            *reinterpret_cast<f32x4*>(l) = acc * 0.25f;
                            l += lstep;
                        }
                        asm volatile("; ie-mark pooled-stage-end n=%0 relu=%1" ::"n"(N), "n"(int(RELU)));
                    };
                    if (npass >= 2) {                                              // npass is a power of two
                        for (int p0 = 0; p0 < npass; p0 += 2) group(std::integral_constant<int, 2>{});
                    } else {
                        group(std::integral_constant<int, 1>{});
                    }
                    row = unsigned(row0);
                    cb += unsigned(CT) * 16u;
                    l += lnext;
                }
            }
        };
        if (PRE && __builtin_amdgcn_readfirstlane(p.pool_relu) != 0) stage(std::true_type{});
        else stage(std::false_type{});
    }
#pragma unroll
    for (int s = D - DLATE; s < D; ++s) loop.issue(rs_w, wlane, nb, CH, s);
    __syncthreads();

    int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(lane));
    const int r = lane & 15, gk = lane >> 4;
    wlane = unsigned(lane) * 16u;
    f32x4 acc[PB][TNW];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int j = 0; j < TNW; ++j) acc[pb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    loop.run(rs_w, wlane, nb, CH, sA, P, r, gk, acc);

    // Epilogue: as conv1x1_as_kernel.  Rows past M lie behind the descriptor's range: their stores are dropped without a predicate.
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    {
        const __amdgpu_buffer_rsrc_t rs_out =
            __builtin_amdgcn_make_buffer_rsrc(a.out.p, 0, int((int64_t(M - 1) * opitch + Cout) * 4), kBufferRsrcFlags);
        const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias != nullptr ? Cout * 4 : 0, kBufferRsrcFlags);
        const unsigned o0 = (unsigned(m0) * unsigned(opitch) + mul24(r, opitch) + 4 * gk) * 4u;
        const unsigned ostep = unsigned(opitch) * 64u;
        auto finish = [&](auto relu_, auto bias_) {            // bias and ReLU are decided once, not per element
            constexpr bool RELU = decltype(relu_)::value, BIAS = decltype(bias_)::value;
            asm volatile("; ie-mark pooled-finish relu=%0 bias=%1" ::"n"(int(RELU)), "n"(int(BIAS)));
#pragma unroll
            for (int j = 0; j < TNW; ++j) {
                f32x4 bq = zero;
                if constexpr (BIAS) bq = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_b, unsigned(gk) * 16u, (n0 + j * 16) * 4, 0));
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    f32x4 v = acc[pb][j];
                    if constexpr (BIAS) v += bq;
                    if constexpr (RELU) v = __builtin_elementwise_max(v, zero);
                    acc[pb][j] = v;                            // (the chain reads the stored value)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_out, o0 + pb * ostep, (n0 + j * 16) * 4, 0);
                }
            }
        };
        switch (__builtin_amdgcn_readfirstlane((a.relu ? 1 : 0) | (a.bias != nullptr ? 2 : 0))) {
            case 0: finish(std::false_type{}, std::false_type{}); break;
            case 1: finish(std::true_type{}, std::false_type{}); break;
            case 2: finish(std::false_type{}, std::true_type{}); break;
            default: finish(std::true_type{}, std::true_type{}); break;
        }
    }

    if constexpr (CHAIN) {
        // ---- the entry 1x1 of the next block on the tile just stored: K2 = Cout, 16 output channels per wave ----
        const int K2 = Cout, P2 = K2 + pad, CH2 = K2 >> 4, Cout2 = p.out2.c;
        const __amdgpu_buffer_rsrc_t rs_w2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wfrag2), 0, Cout2 * K2 * 4, kBufferRsrcFlags);
        AsLoop<1, PB, D> loop2;
#pragma unroll
        for (int s = 0; s < D; ++s) loop2.issue(rs_w2, wlane, wave, CH2, s);       // in flight across the two barriers
        __syncthreads();                                                           // every wave has left the first loop: the staging area is free
        {
            const __amdgpu_buffer_rsrc_t rs_s2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.scale2), 0, K2 * 4, kBufferRsrcFlags);
            const __amdgpu_buffer_rsrc_t rs_t2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.shift2), 0, K2 * 4, kBufferRsrcFlags);
            const bool relu2 = __builtin_amdgcn_readfirstlane(p.pre_relu2) != 0;
#pragma unroll
            for (int j = 0; j < TNW; ++j) {
                const f32x4 s2 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_s2, unsigned(gk) * 16u, (n0 + j * 16) * 4, 0));
                const f32x4 t2 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_t2, unsigned(gk) * 16u, (n0 + j * 16) * 4, 0));
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    f32x4 x = __builtin_elementwise_fma(acc[pb][j], s2, t2);       // the entry conv's prologue on the value it would have read back
                    if (relu2) x = __builtin_elementwise_max(x, zero);
                    *reinterpret_cast<f32x4*>(sA + (mul24(r, P2) + pb * 16 * P2 + n0 + j * 16 + 4 * gk)) = x;
                }
            }
        }
        __syncthreads();
        f32x4 acc2[PB][1];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) acc2[pb][0] = zero;
        loop2.run(rs_w2, wlane, wave, CH2, sA, P2, r, gk, acc2);
        const int opitch2 = int(p.out2.sw);
        const __amdgpu_buffer_rsrc_t rs_out2 =
            __builtin_amdgcn_make_buffer_rsrc(p.out2.p, 0, int((int64_t(M - 1) * opitch2 + Cout2) * 4), kBufferRsrcFlags);
        const __amdgpu_buffer_rsrc_t rs_b2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias2), 0, p.bias2 != nullptr ? Cout2 * 4 : 0, kBufferRsrcFlags);
        const unsigned o2 = (unsigned(m0) * unsigned(opitch2) + mul24(r, opitch2) + 4 * gk) * 4u;
        f32x4 bq = zero;
        if (p.bias2 != nullptr) bq = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_b2, unsigned(gk) * 16u, wave * 64, 0));
        const bool relu_out2 = __builtin_amdgcn_readfirstlane(p.relu2) != 0;
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            f32x4 v = acc2[pb][0];
            if (p.bias2 != nullptr) v += bq;
            if (relu_out2) v = __builtin_elementwise_max(v, zero);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_out2, o2 + pb * unsigned(opitch2) * 64u, wave * 64, 0);
        }
    }
}

namespace {

struct TransTile { int waves, tnw, pb; bool chain; };
// conv1x1_as_kernel's shapes; the two 8-wave / 32-pixel shapes (128 and 256 channels per workgroup) can chain.  Tile 5 is one wave with 16 channels:
// it takes the channel counts that are no multiple of 64 (a 352 -> 176 transition), restaging the rows once per 16-channel block.  Tiles 6 and 7 are
// the chain shapes on 16-pixel blocks: twice the workgroups, so that a grid of about one workgroup round (784 32-pixel tiles on 768 resident slots at
// batch 32) no longer runs its load phase and its MFMA phase one after the other across the whole chip
constexpr TransTile kTransTiles[kNumConvPooledTiles] = {{8, 1, 2, true}, {4, 1, 2, false}, {8, 2, 2, true}, {4, 1, 1, false}, {2, 2, 1, false}, {1, 1, 2, false},
                                                        {8, 1, 1, true}, {8, 2, 1, true}};

unsigned mg20(unsigned d) { return ((1u << 20) + d - 1) / d; }
unsigned mg32(unsigned d) { return d == 1 ? 0xffffffffu : unsigned((uint64_t(1) << 32) / d); }

// log2 of the staging loop's column count, as launch_as_t picks it: fewest row groups first, then fewest load slots, then the widest block
int col_shift(int K, int threads, int rows) {
    const int c4n = K / 4;
    int best = 6;
    long best_key = -1;
    for (int s = 6; s >= 4 && (threads >> s) <= rows; --s) {      // a row pass never spans more rows than the tile has
        const int ct = 1 << s, blocks = (c4n + ct - 1) / ct, npass = rows * ct / threads;
        const long key = (long(blocks * ((npass + 1) / 2)) << 24) + blocks * npass;
        if (best_key < 0 || key < best_key) best = s, best_key = key;
    }
    return best;
}

size_t lds_bytes(const ConvArgs& a, const TransTile& t, bool chain, int pad) {
    const size_t rows = size_t(16 * t.pb);
    const size_t first = rows * (a.in.c + pad) * 4 + 64, second = chain ? rows * (a.out.c + pad) * 4 + 64 : 0;
    return std::max(first, second);
}

template <int T>
hipError_t launch_t(const ConvArgs& a_in, const PooledArgs& p_in, bool chain, hipStream_t stream) {
    constexpr TransTile t = kTransTiles[T];
    ConvArgs a = a_in;
    PooledArgs p = p_in;
    const int pad = Knobs().as_pad;
    a.debug = (pad << 8) | (col_shift(a.in.c, 64 * t.waves, 16 * t.pb) << 16);
    p.k.mg20_ow = mg20(unsigned(a.out.w));
    p.k.mg20_oh = mg20(unsigned(a.out.h));
    p.k.mg32_ohw = mg32(unsigned(a.out.h) * unsigned(a.out.w));
    p.k.mg32_ow = mg32(unsigned(a.out.w));
    const int64_t M = int64_t(a.out.n) * a.out.h * a.out.w;
    const dim3 grid(unsigned((M + 16 * t.pb - 1) / (16 * t.pb)), unsigned(a.out.c / (16 * t.tnw * t.waves)));
    const size_t lds = lds_bytes(a, t, chain, pad);
    if (lds > size_t(160) * 1024) return hipErrorInvalidValue;
    const bool pre = p.pool_scale != nullptr;
    if constexpr (t.chain) {
        if (chain) {
            if (pre) conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, true, true><<<grid, dim3(64 * t.waves), lds, stream>>>(a, p);
            else conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, false, true><<<grid, dim3(64 * t.waves), lds, stream>>>(a, p);
            return hipGetLastError();
        }
    }
    if (chain) return hipErrorInvalidValue;
    if (pre) conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, true, false><<<grid, dim3(64 * t.waves), lds, stream>>>(a, p);
    else conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, false, false><<<grid, dim3(64 * t.waves), lds, stream>>>(a, p);
    return hipGetLastError();
}

template <int T>
hipError_t init_t() {
    constexpr TransTile t = kTransTiles[T];
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if constexpr (t.chain) {
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_pooled_kernel<t.waves, t.tnw, t.pb, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    return e;
}

}  // namespace

bool ConvPooledShapeOk(int tile, bool chain, int64_t k, int64_t cout, int64_t cout2) {
    if (tile < 0 || tile >= kNumConvPooledTiles) return false;
    const TransTile t = kTransTiles[tile];
    const int64_t bn = 16 * t.tnw * t.waves;
    if (k <= 0 || (k % 16) || cout <= 0 || (cout % bn)) return false;
    if (size_t(16 * t.pb) * (k + 8) * 4 + 64 > size_t(160) * 1024) return false;
    if (!chain) return true;
    return t.chain && cout == bn && cout2 == 16 * t.waves;
}

bool ConvPooledEligible(const ConvArgs& a, const PooledArgs& p, int tile, bool chain) {
    if (!ConvPooledShapeOk(tile, chain, a.in.c, a.out.c, chain ? p.out2.c : 0)) return false;
    const TransTile t = kTransTiles[tile];
    // the conv: what conv1x1_as_kernel asks of its operands, without a prologue of its own
    if (a.in.f16 || a.out.f16 || a.in.f8 || a.out.f8 || a.wfrag == nullptr || a.res.p != nullptr || a.pre_scale != nullptr) return false;
    if (a.kh != 1 || a.kw != 1 || a.sh != 1 || a.sw != 1 || a.pt != 0 || a.pl != 0) return false;
    if (a.out.h != a.in.h || a.out.w != a.in.w || a.out.n != a.in.n) return false;
    if (a.out.sc != 1 || (a.out.sw % 4) || a.out.sh != a.out.w * a.out.sw || a.out.sn != a.out.h * a.out.sh || !Aligned16(a.out.p)) return false;
    if (!Aligned16(a.wfrag) || (a.bias && !Aligned16(a.bias))) return false;
    // the pool's input: an NHWC channel slice at twice the resolution, pixels at a constant pitch
    const TensorArg& x = p.pin;
    if (x.p == nullptr || x.f16 || x.f8 || x.sc != 1 || x.c != a.in.c || x.n != a.in.n || x.h != 2 * a.in.h || x.w != 2 * a.in.w) return false;
    if ((x.sw % 4) || x.sw < x.c || x.sh != x.w * x.sw || x.sn != x.h * x.sh || !Aligned16(x.p)) return false;
    if ((p.pool_scale == nullptr) != (p.pool_shift == nullptr)) return false;
    if (p.pool_scale && (!Aligned16(p.pool_scale) || !Aligned16(p.pool_shift))) return false;
    const int64_t M = int64_t(a.out.n) * a.out.h * a.out.w;
    if (M <= 0 || M > (int64_t(1) << 22) || a.out.h > 512 || a.out.w > 512) return false;       // 2^20 reciprocals: (extent + 31) * extent < 2^20
    // rows past M map up to 32 images past the last one: their pixel index and byte offset must not wrap (24-bit factors, 32-bit offsets)
    const int64_t px_span = (int64_t(x.n) + 33) * x.h * x.w;
    if (px_span >= (int64_t(1) << 24) || x.sw * 4 >= (int64_t(1) << 24) || px_span * x.sw * 4 >= (int64_t(1) << 32)) return false;
    if (int64_t(x.n) * x.h * x.w * x.sw * 4 >= (int64_t(1) << 31)) return false;
    if (a.out.sw >= (int64_t(1) << 22) || (M + 32) * a.out.sw * 4 >= (int64_t(1) << 31) || int64_t(a.out.c) * a.in.c * 4 >= (int64_t(1) << 31)) return false;
    if (lds_bytes(a, t, chain, Knobs().as_pad) > size_t(160) * 1024) return false;
    if (!chain) return true;
    // the entry conv: reads exactly the tile just stored, 16 output channels per wave
    const TensorArg& o2 = p.out2;
    if (p.wfrag2 == nullptr || !Aligned16(p.wfrag2) || p.scale2 == nullptr || p.shift2 == nullptr || !Aligned16(p.scale2) || !Aligned16(p.shift2)) return false;
    if (p.bias2 && !Aligned16(p.bias2)) return false;
    if (o2.p == nullptr || o2.f16 || o2.f8 || o2.sc != 1 || o2.n != a.out.n || o2.h != a.out.h || o2.w != a.out.w) return false;
    if ((o2.sw % 4) || o2.sh != o2.w * o2.sw || o2.sn != o2.h * o2.sh || !Aligned16(o2.p)) return false;
    if (o2.sw >= (int64_t(1) << 22) || (M + 32) * o2.sw * 4 >= (int64_t(1) << 31)) return false;
    return true;
}

hipError_t LaunchConvPooled(const ConvArgs& a, const PooledArgs& p, int tile, bool chain, hipStream_t stream) {
    if (!ConvPooledEligible(a, p, tile, chain)) return hipErrorInvalidValue;
    switch (tile) {
        case 0: return launch_t<0>(a, p, chain, stream);
        case 1: return launch_t<1>(a, p, chain, stream);
        case 2: return launch_t<2>(a, p, chain, stream);
        case 3: return launch_t<3>(a, p, chain, stream);
        case 4: return launch_t<4>(a, p, chain, stream);
        case 5: return launch_t<5>(a, p, chain, stream);
        case 6: return launch_t<6>(a, p, chain, stream);
        case 7: return launch_t<7>(a, p, chain, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t InitKernelsTrans() {
    hipError_t e;
    if ((e = init_t<0>()) != hipSuccess) return e;
    if ((e = init_t<1>()) != hipSuccess) return e;
    if ((e = init_t<2>()) != hipSuccess) return e;
    if ((e = init_t<3>()) != hipSuccess) return e;
    if ((e = init_t<4>()) != hipSuccess) return e;
    if ((e = init_t<5>()) != hipSuccess) return e;
    if ((e = init_t<6>()) != hipSuccess) return e;
    return init_t<7>();
}

}  // namespace ie
