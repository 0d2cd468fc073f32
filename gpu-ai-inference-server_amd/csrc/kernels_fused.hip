// Fused dense-layer step for DenseNet-style blocks on small output grids (fp32): the 3x3 growth conv of layer L and the 1x1
// bottleneck conv of layer L+1 in ONE launch.
//
// Dense blocks 3-4 at batch 32 are a strict chain of 80 latency-bound launches (M = 6272 / 1568 pixels): about a third of the fp32
// forward is per-launch fixed cost (launch gap, operand preamble, first-load latency, store drain).  The chain cannot be shortened
// by running layers side by side, but two of its links need no grid-wide dependency: the 1x1 conv of layer L+1 is PER PIXEL, and of
// its K = C + 32 input channels only the last 32 come from layer L's 3x3 conv -- for the same pixels.  So a workgroup that owns a
// tile of 16*PB pixels
//   1. computes the 3x3 conv of layer L for ITS pixels (conv_win_kernel's scheme: the bottleneck window it needs -- one contiguous
//      run of 16*PB + 2W + 2 NHWC pixel rows written by the PREVIOUS launch -- through LDS, weights from the fragment-major mirror,
//      K split over the 8 waves, partial tiles summed through LDS in wave order), stores those 32 channels to the block buffer and
//      keeps them in LDS;
//   2. runs conv1x1_as_kernel's loop for layer L+1 on its pixel rows: channels [0, C) copied from the block buffer (the loads are
//      issued BEFORE step 1 and land while it runs), the 32 fresh ones from step 1, BN+ReLU prologue on the way into LDS, weights
//      streamed through a register ring, each wave 16 of the 128 output channels.
// No barrier between workgroups, no recomputed halo: launch k reads only what launch k-1 wrote.  The planner emits these steps for a
// run of dense layers (plan.cpp, FuseDenseLayers); a block of n layers becomes n+1 launches instead of 2n, and the bottleneck tensor
// ping-pongs between two buffers (one being read as halo by neighbouring tiles while the other is written).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "device_util.h"
#include "env.h"
#include "kernels.h"
#include "launch_util.h"

namespace ie {

// Pad (floats) of the LDS pixel rows.  The fragment reads are ds_read_b128 at row * pitch + k-group * 4: with a pad of 4 two lanes of
// every 16-lane service group share a 16-byte slot (2-way conflict on every read, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.42 in
// profiles/r02); pitch = 8 mod 32 banks is conflict-free for channel counts that are multiples of 32 (kernels_direct.hip, launch_as_t).
constexpr int kRowPad = 8;

// PB: 16-pixel blocks per workgroup.  8 waves.  1x1: Cout == 128 (16 per wave).  3x3: stride 1, pad 1, Cout == 32, 9 * Cin3 / 16 <= 72 chunks.
// OCC2: a variant meant to run TWO workgroups per CU (16-pixel tiles, <= 128 VGPRs, <= 80 KB of LDS): the old-channel loads are issued only
// after the 3x3's MFMAs (their registers would otherwise overlap the 3x3's weight fragments); the latency this exposes is what the
// second workgroup on the CU fills.
// NSPLIT (tile 6): a two-row grid for maps with fewer tiles than half the CUs.  Both rows run phases (a)-(i) alike (bit-identical fresh
// channels; row 0 stores them); in the 1x1 row h owns output channels [64h, 64h + 64): waves 0-3 take 16 each, ALL chunks in the usual order
// on one accumulator (the same sums as tile 1, bit for bit) behind a 16-deep weight ring -- one wave per SIMD covers the weight latency
// alone -- and waves 4-7 leave after the last barrier.
//
// fp32 MFMAs and vector-ALU instructions share the issue slot, so the kernel keeps the vector ALU for the work itself:
//   * nothing is divided (FusedConsts: reciprocals and slot counts from the host; per-lane quotients are a 24-bit multiply and a shift, wave-
//     uniform ones run on the scalar unit) and nothing is multiplied per slot: a thread keeps ONE 4-channel column in both staging loops and
//     walks rows, so a slot is one add on the global offset and one on the LDS address;
//   * rows before 0 and past M lie outside the buffer descriptors' ranges (reads give zeros, stores are dropped) -- no per-slot predicate;
//     slots are counted per launch (full slots for every active thread, one partial last slot);
//   * a wave's K slice of the 3x3 (at most Cin3 / 16 + 1 chunks) touches at most TWO taps: the lane's fragment address for each of the
//     two is formed once, an out-of-image tap points at a zeroed 64-byte row with a step of 0, and a chunk costs one add per pixel block;
//   * prologue ReLU, relu3, bias and ReLU select a code variant per launch (`; ie-mark` names the variants for scripts/isa_mix.py).
template <int PB, bool PRE, bool OCC2, bool NSPLIT = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(OCC2 ? 4 : 2, OCC2 ? 4 : 2)))
void conv_dense_fused_kernel(const ConvArgs a, const FusedArgs f, const int part_off) {
    static_assert(!NSPLIT || (PB == 1 && !OCC2), "the N-split form is a 16-pixel, one-workgroup-per-CU tile");
    constexpr int WAVES = 8, NT = 64 * WAVES, PX = 16 * PB, D = NSPLIT ? 16 : 8, MAXC3 = 9, TN3 = 2, PP = 32 + 4;
    constexpr int MAXS = PB == 1 ? 8 : 16;             // staging slots per thread for the old channels (checked by the launcher)
    constexpr int MAXW = 8;                            // window slots per thread (checked by the launcher)
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_fused[];
    const int K = a.in.c, Kold = K - 32, P = K + kRowPad, CH = K >> 4, Cin3 = f.in3.c, P3 = Cin3 + kRowPad;
    float* const sA = reinterpret_cast<float*>(smem_fused);                        // [PX][P]: the 1x1's activation rows
    // the bottleneck window of the 3x3, [npx][P3], starts at sA too: sA's rows are only written once every wave is done with the window
    float* const sPart = sA + part_off;                                            // [WAVES/2][PX][PP], behind max(sA, sWin)
    const unsigned zero_row = unsigned(part_off + (WAVES / 2) * PX * PP) * 4u;     // 16 zero floats behind the partial tiles (byte offset)
    const FusedConsts& k = f.k;

    const unsigned tid = threadIdx.x, lane = tid & 63, r = lane & 15, gk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.in.h, W = a.in.w;
    const int M = a.in.n * H * W;
    const int m0 = blockIdx.x * PX;
    const int ipitch = int(a.in.sw), opitch = int(a.out.sw), bpitch = int(f.in3.sw), o3pitch = int(f.out3.sw);
    const int nb = NSPLIT ? 4 * int(blockIdx.y) + wave : wave;                     // this wave's 16-channel block of the 1x1's output
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // the two per-thread (row, 4-channel column) splits of the staging loops: tid / columns as a 24-bit multiply and a shift
    const int c4n3 = Cin3 >> 2, c4n = Kold >> 2;
    const unsigned wrow0 = __umul24(tid, k.mg20_c4n3) >> 20, wc4 = tid - __umul24(wrow0, c4n3);
    const unsigned xrow0 = __umul24(tid, k.mg20_c4n) >> 20, xc4 = tid - __umul24(xrow0, c4n);
    const bool wact = wrow0 < unsigned(k.wrpp), wlast = wrow0 < unsigned(k.wlast);       // NT - wrpp * c4n3 threads sit the window out
    const bool xact = xrow0 < unsigned(k.rpp), xlast = xrow0 < unsigned(k.xlast);        // NT - rpp * c4n threads sit the old channels out
    if (tid < 4) *reinterpret_cast<f32x4*>(smem_fused + zero_row + tid * 16u) = zero;

    // ---- (a) bottleneck window loads (issued first: they are waited for first).  Window row w is pixel m0 - W - 1 + w: the rows before
    //      pixel 0 wrap to offsets above 2^31 and the rows from M on start past the last row's channels, both outside the descriptor ----
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(f.in3.p, 0, int((int64_t(M - 1) * bpitch + Cin3) * 4), kBufferRsrcFlags);
    u32x4 wv[MAXW];
    {
        unsigned g = unsigned(m0 - W - 1) * unsigned(bpitch) * 4u + __umul24(wrow0, unsigned(bpitch) * 4u) + wc4 * 16u;      // (the byte pitch is the scalar factor: 24-bit products)
        if (!wact) g = OOB;
        const unsigned gstep = unsigned(k.wrpp * bpitch) * 4u;
#pragma unroll
        for (int u = 0; u < MAXW; ++u) {
            if (u < k.wfull) {                         // wave-uniform
                asm volatile("; ie-mark fused-win-load u=%0" ::"n"(u));            // (the slot marks let scripts/isa_mix.py walk the path of one shape)
                wv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, g, 0, 0);
                g += gstep;
            } else if (u == k.wfull && k.wlast != 0) {
                asm volatile("; ie-mark fused-win-load-last u=%0" ::"n"(u));
                wv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, wlast ? g : OOB, 0, 0);
            }
        }
    }

    // ---- (b) the 3x3's weight fragments of this wave's K slice (fragment-major: 1 KiB per load; lane * 16 in the VGPR, the chunk scalar) ----
    const int cpt3 = Cin3 >> 4, total3 = 9 * cpt3;
    const int cb = (total3 * wave) >> 3, ce = (total3 * (wave + 1)) >> 3;
    const __amdgpu_buffer_rsrc_t rs_w3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(f.wfrag3), 0, 32 * 9 * Cin3 * 4, kBufferRsrcFlags);
    u32x4 B3[MAXC3][TN3];
    {
        const unsigned l16 = (a.debug & 4) ? OOB : lane * 16u;
#pragma unroll
        for (int i = 0; i < MAXC3; ++i)
            if (cb + i < ce) {                         // wave-uniform; the chunk loop below tests the same
#pragma unroll
                for (int j = 0; j < TN3; ++j) B3[i][j] = __builtin_amdgcn_raw_buffer_load_b128(rs_w3, l16, (j * total3 + cb + i) * 1024, 0);
            }
    }

    // ---- (c) the 1x1's old channels [0, Kold) of this tile's pixel rows: loads only, consumed after the 3x3.  A thread keeps ONE
    //      4-channel column for all its rows (rows advance by rpp per slot), so the prologue's scale/shift for that column is one pair
    //      of 16-byte loads issued here, not a dependent global round trip per slot later ----
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(a.in.p, 0, int((int64_t(M - 1) * ipitch + K) * 4), kBufferRsrcFlags);
    u32x4 xv[MAXS];
    unsigned xg = unsigned(m0) * unsigned(ipitch) * 4u + __umul24(xrow0, unsigned(ipitch) * 4u) + xc4 * 16u;
    if (!xact || (a.debug & 8)) xg = OOB;
    auto load_old_channels = [&]() {
        const unsigned gstep = unsigned(k.rpp * ipitch) * 4u;
#pragma unroll
        for (int u = 0; u < MAXS; ++u) {
            if (u < k.xfull) {                         // wave-uniform
                asm volatile("; ie-mark fused-old-load u=%0" ::"n"(u));
                xv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, xg, 0, 0);
                xg += gstep;
            } else if (u == k.xfull && k.xlast != 0) {
                asm volatile("; ie-mark fused-old-load-last u=%0" ::"n"(u));
                xv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, xlast ? xg : OOB, 0, 0);
            }
        }
    };
    if constexpr (!OCC2) load_old_channels();
    // prologue constants, 3x3 bias and epilogue bias through descriptors: an absent vector has range 0 and reads zeros, no branch
    // (the two-workgroups-per-CU variant issues them with its old-channel loads, behind the 3x3: it has 128 registers)
    f32x4 xsc = zero, xsf = zero, ebias = zero;
    f32x2 fsc = {0.f, 0.f}, fsf = {0.f, 0.f}, fb3 = {0.f, 0.f};
    const unsigned fc2 = (tid & 15) * 2;               // this thread's channel pair of the fresh 32 (phase i)
    auto load_constants = [&]() {
        if constexpr (PRE) {
            const __amdgpu_buffer_rsrc_t rs_sc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.pre_scale), 0, K * 4, kBufferRsrcFlags);
            const __amdgpu_buffer_rsrc_t rs_sf = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.pre_shift), 0, K * 4, kBufferRsrcFlags);
            xsc = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_sc, xc4 * 16u, 0, 0));
            xsf = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_sf, xc4 * 16u, 0, 0));
            fsc = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_sc, fc2 * 4u, Kold * 4, 0));
            fsf = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_sf, fc2 * 4u, Kold * 4, 0));
        }
        const __amdgpu_buffer_rsrc_t rs_b3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(f.bias3), 0, f.bias3 != nullptr ? 32 * 4 : 0, kBufferRsrcFlags);
        fb3 = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_b3, fc2 * 4u, 0, 0));
        const __amdgpu_buffer_rsrc_t rs_eb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias != nullptr ? 128 * 4 : 0, kBufferRsrcFlags);
        ebias = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_eb, gk * 16u, nb * 64, 0));      // this lane's 4 output channels
    };
    if constexpr (!OCC2) load_constants();

    // ---- (d) window -> LDS ----
    if (wact) {
        unsigned l = __umul24(wrow0, unsigned(P3) * 4u) + wc4 * 16u;
        const unsigned lstep = unsigned(k.wrpp * P3) * 4u;
        int wfull = k.wfull;
        asm volatile("" : "+s"(wfull));                // compared afresh: the load loop's eight slot conditions are not kept in registers for this
#pragma unroll
        for (int u = 0; u < MAXW; ++u) {
            if (u < wfull) {
                asm volatile("; ie-mark fused-win-put u=%0" ::"n"(u));
                *reinterpret_cast<u32x4*>(smem_fused + l) = wv[u];
                l += lstep;
            } else if (u == wfull && k.wlast != 0) {
                asm volatile("; ie-mark fused-win-put-last u=%0" ::"n"(u));
                if (wlast) *reinterpret_cast<u32x4*>(smem_fused + l) = wv[u];
            }
        }
    }
    __syncthreads();

    // ---- (e) 3x3 on 16 x 16 x 4 tiles: lane (r, gk) owns pixel r of each pixel block ----
    // The tile's first pixel sits at (oy0, ox0) of its image (scalar); the lane's pixels follow from there with two 24-bit multiplies.  A wave's
    // slice [cb, ce) starts cidx chunks into tap tapA and runs into tapA + 1 at most: per pixel block one fragment address and step for each
    // of the two (the zero row and 0 where the tap falls outside the image or the pixel past M); the switch is a wave-uniform branch.
    f32x4 acc3[PB][TN3];
    unsigned cur[PB], inc[PB], curB[PB], incB[PB];
    const unsigned tapA = udiv_uniform(unsigned(cb), unsigned(cpt3), k.mg32_cpt3);
    int cidx = cb - int(tapA) * cpt3;
    {
        const unsigned HW = unsigned(H * W);
        const unsigned rem0 = unsigned(m0) - udiv_uniform(unsigned(m0), HW, k.mg32_hw) * HW;
        const unsigned oy0 = udiv_uniform(rem0, unsigned(W), k.mg32_w), ox0 = rem0 - oy0 * unsigned(W);
        const int kyA = int(tapA * 11u) >> 5, kxA = int(tapA) - 3 * kyA;               // tap / 3 for taps 0..9
        const int kyB = int((tapA + 1u) * 11u) >> 5, kxB = int(tapA) + 1 - 3 * kyB;
        const unsigned offA = unsigned((kyA * W + kxA) * P3 + cidx * 16) * 4u, offB = unsigned((kyB * W + kxB) * P3) * 4u;
        const unsigned wl0 = __umul24(r, unsigned(P3) * 4u) + gk * 16u, zl = zero_row + gk * 16u;
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            const unsigned j = pb * 16 + r, n = ox0 + j;                               // n < W + 32
            const unsigned q = __umul24(n, k.mg20_w) >> 20;                            // image rows from the tile's first pixel on
            const int ox = int(n - __umul24(q, W));
            const unsigned y = oy0 + q;                                                // < H + 33
            const unsigned q2 = (__umul24(y, k.mg20_h) >> 20) + (y >= k.hbig ? 1u : 0u);
            const int oy = int(y - __umul24(q2, H));
            const bool mok = int(j) < M - m0;
            const bool okA = mok && unsigned(oy + kyA - 1) < unsigned(H) && unsigned(ox + kxA - 1) < unsigned(W);
            const bool okB = mok && unsigned(oy + kyB - 1) < unsigned(H) && unsigned(ox + kxB - 1) < unsigned(W);
            const unsigned base = wl0 + unsigned(pb * 16 * P3) * 4u;
            cur[pb] = okA ? base + offA : zl;
            inc[pb] = okA ? 64u : 0u;
            curB[pb] = okB ? base + offB : zl;
            incB[pb] = okB ? 64u : 0u;
#pragma unroll
            for (int j3 = 0; j3 < TN3; ++j3) acc3[pb][j3] = zero;
        }
    }
    const int ce3 = (a.debug & 1) ? cb : ce;           // debug bits: timing-only ablations, wrong results
#pragma unroll
    for (int i = 0; i < MAXC3; ++i) {
        if (cb + i < ce3) {                            // wave-uniform
            asm volatile("; ie-mark fused-chunk i=%0" ::"n"(i));
            f32x4 av[PB];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                av[pb] = *reinterpret_cast<const f32x4*>(smem_fused + cur[pb]);
                cur[pb] += inc[pb];
            }
#pragma unroll
            for (int j = 0; j < TN3; ++j) {
                const f32x4 bv = __builtin_bit_cast(f32x4, B3[i][j]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int pb = 0; pb < PB; ++pb) acc3[pb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[e], av[pb][e], acc3[pb][j], 0, 0, 0);
            }
            if (++cidx == cpt3) {                      // wave-uniform: the slice runs into its second tap (once per wave at most)
                asm volatile("; ie-mark fused-tap-switch i=%0" ::"n"(i));
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    cur[pb] = curB[pb];
                    inc[pb] = incB[pb];
                }
            }
        }
    }

    if constexpr (OCC2) {
        load_old_channels();
        load_constants();
    }

    // ---- (f) prime the 1x1's weight ring (its latency hides behind the reduction and the staging below) ----
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wfrag), 0, 128 * K * 4, kBufferRsrcFlags);
    u32x4 ring[D];
    int c_l = 0;
    const unsigned rl16 = (a.debug & 16) ? OOB : lane * 16u;
    auto issue = [&](int slot) {
        // lane * 16 in the VGPR, the rest scalar; past the last chunk the last one again (in range, never consumed): no VALU in the K loop
        ring[slot] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, rl16, (nb * CH + (c_l < CH ? c_l : CH - 1)) * 1024, 0);
        ++c_l;
    };
    if (!NSPLIT || wave < WAVES / 2) {
#pragma unroll
        for (int s = 0; s < D; ++s) issue(s);
    }

    // ---- (g) sum the eight partial 3x3 tiles in wave order: waves 4..7 publish, waves 0..3 add theirs and publish ----
    {
        float* const q0 = sPart + ((wave & (WAVES / 2 - 1)) * PX * PP + int(r) * PP + 4 * int(gk));
        if (wave >= WAVES / 2) {                       // (the partial tiles have their own storage: no need to wait for the window's readers)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
#pragma unroll
                for (int j = 0; j < TN3; ++j) *reinterpret_cast<f32x4*>(q0 + pb * 16 * PP + j * 16) = acc3[pb][j];
        }
        __syncthreads();
        if (wave < WAVES / 2) {
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
#pragma unroll
                for (int j = 0; j < TN3; ++j) {
                    float* const q = q0 + pb * 16 * PP + j * 16;
                    *reinterpret_cast<f32x4*>(q) = acc3[pb][j] + *reinterpret_cast<const f32x4*>(q);
                }
        }
    }

    // ---- (h) old channels: prologue, -> sA.  The prologue's ReLU is decided once per launch, not per element ----
    auto stage = [&](auto relu_) {
        constexpr bool RELU = decltype(relu_)::value;
        asm volatile("; ie-mark fused-stage relu=%0" ::"n"(int(RELU)));
        auto put = [&](unsigned l, const u32x4& v) {
            f32x4 x = __builtin_bit_cast(f32x4, v);
            if constexpr (PRE) x = __builtin_elementwise_fma(x, xsc, xsf);             // one rounding per element, as v_fma_f32
            if constexpr (PRE && RELU) x = __builtin_elementwise_max(x, zero);
            *reinterpret_cast<f32x4*>(smem_fused + l) = x;
        };
        if (xact) {
            unsigned l = __umul24(xrow0, unsigned(P) * 4u) + xc4 * 16u;
            const unsigned lstep = unsigned(k.rpp * P) * 4u;
            int xfull = k.xfull;
            asm volatile("" : "+s"(xfull));            // compared afresh, as in (d)
#pragma unroll
            for (int u = 0; u < MAXS; ++u) {
                if (u < xfull) {                       // wave-uniform
                    asm volatile("; ie-mark fused-stage-put relu=%0 u=%1" ::"n"(int(RELU)), "n"(u));
                    put(l, xv[u]);
                    l += lstep;
                } else if (u == xfull && k.xlast != 0) {
                    asm volatile("; ie-mark fused-stage-put-last relu=%0 u=%1" ::"n"(int(RELU)), "n"(u));
                    if (xlast) put(l, xv[u]);
                }
            }
        }
        asm volatile("; ie-mark fused-stage-end relu=%0" ::"n"(int(RELU)));
    };
    const int pre_relu = PRE ? __builtin_amdgcn_readfirstlane(a.pre_relu) : 0;
    if (pre_relu != 0) stage(std::true_type{});
    else stage(std::false_type{});
    __syncthreads();

    // ---- (i) fresh channels: final sum, 3x3 epilogue, raw value to the block buffer, prologue'd value to sA.  One (pixel, channel pair) per
    //      thread of the first PX / 4 waves; rows past M start behind the descriptor's range ----
    // the thread's three addresses (pixel tid >> 4): its partial sums, its pair in the block buffer, its pair in sA -- formed once, outside the variants
    unsigned fresh_q = unsigned(part_off) * 4u + __umul24(tid >> 4, PP * 4) + fc2 * 4u;
    unsigned fresh_g = unsigned(m0) * unsigned(o3pitch) * 4u + __umul24(tid >> 4, unsigned(o3pitch) * 4u) + fc2 * 4u;
    unsigned fresh_l = __umul24(tid >> 4, unsigned(P) * 4u) + unsigned(Kold) * 4u + fc2 * 4u;
    asm volatile("" : "+v"(fresh_q), "+v"(fresh_g), "+v"(fresh_l));
    auto fresh = [&](auto relu3_, auto relu_) {
        constexpr bool RELU3 = decltype(relu3_)::value, RELU = decltype(relu_)::value;
        asm volatile("; ie-mark fused-fresh relu3=%0 relu=%1" ::"n"(int(RELU3)), "n"(int(RELU)));
        const float* const q = reinterpret_cast<const float*>(smem_fused + fresh_q);
        f32x2 v = {0.f, 0.f};
#pragma unroll
        for (int w = 0; w < WAVES / 2; ++w) v += *reinterpret_cast<const f32x2*>(q + w * PX * PP);
        v += fb3;
        if constexpr (RELU3) v = __builtin_elementwise_max(v, f32x2{0.f, 0.f});
        if (!NSPLIT || blockIdx.y == 0) {
            const __amdgpu_buffer_rsrc_t rs_o3 = __builtin_amdgcn_make_buffer_rsrc(f.out3.p, 0, int((int64_t(M - 1) * o3pitch + 32) * 4), kBufferRsrcFlags);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs_o3, fresh_g, 0, 0);
        }
        if constexpr (PRE) v = __builtin_elementwise_fma(v, fsc, fsf);
        if constexpr (PRE && RELU) v = __builtin_elementwise_max(v, f32x2{0.f, 0.f});
        *reinterpret_cast<f32x2*>(smem_fused + fresh_l) = v;
    };
    if (PX * 16 >= NT || wave < PX * 16 / 64) {        // wave-uniform
        switch ((__builtin_amdgcn_readfirstlane(f.relu3) != 0 ? 1 : 0) | (pre_relu != 0 ? 2 : 0)) {
            case 0: fresh(std::false_type{}, std::false_type{}); break;
            case 1: fresh(std::true_type{}, std::false_type{}); break;
            case 2: fresh(std::false_type{}, std::true_type{}); break;
            default: fresh(std::true_type{}, std::true_type{}); break;
        }
    }
    __syncthreads();
    if (NSPLIT && wave >= WAVES / 2) return;           // no barrier from here on

    // ---- (k) the 1x1: conv1x1_as_kernel's loop, 16 output channels per wave ----
    f32x4 acc[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) acc[pb] = zero;
    const unsigned char* abase[PB];                    // fragment address per pixel block at the current ring trip; chunk = immediate offset
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) abase[pb] = smem_fused + (__umul24(r, unsigned(P) * 4u) + unsigned(pb * 16 * P) * 4u + gk * 16u);
    f32x4 avn[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) avn[pb] = *reinterpret_cast<const f32x4*>(abase[pb]);
    auto compute = [&](int slot) {                     // the read ahead of the last chunk runs 16 floats past K (pad + next row / the partial tiles)
        f32x4 av[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) av[pb] = avn[pb];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) avn[pb] = *reinterpret_cast<const f32x4*>(abase[pb] + (slot + 1) * 64);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb)
                acc[pb] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, ring[slot])[e], av[pb][e], acc[pb], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, PB, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * PB, 0);
    };
    const int full = (a.debug & 2) ? 0 : CH / D, rem = (a.debug & 2) ? 0 : CH - (CH / D) * D;
    for (int it = 0; it < full; ++it) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
            compute(s);
            issue(s);
        }
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) abase[pb] += D * 64;
    }
#pragma unroll
    for (int s = 0; s < D; ++s)
        if (s < rem) compute(s);

    // Epilogue: bias and ReLU are decided once per launch; the lane's row / quad offset is formed once, rows past M start behind the
    // descriptor's range ((M - 1) * pitch + 128 floats, pitch >= 128) and their stores are dropped
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(a.out.p, 0, int((int64_t(M - 1) * opitch + 128) * 4), kBufferRsrcFlags);
    const unsigned o0 = unsigned(m0) * unsigned(opitch) * 4u + __umul24(r, unsigned(opitch) * 4u) + gk * 16u;
    auto finish = [&](auto relu_, auto bias_) {
        constexpr bool RELU = decltype(relu_)::value, BIAS = decltype(bias_)::value;
        asm volatile("; ie-mark fused-finish relu=%0 bias=%1" ::"n"(int(RELU)), "n"(int(BIAS)));
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            f32x4 v = acc[pb];
            if constexpr (BIAS) v += ebias;
            if constexpr (RELU) v = __builtin_elementwise_max(v, zero);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_out, o0 + unsigned(pb * 16 * opitch) * 4u, nb * 64, 0);
        }
    };
    switch ((__builtin_amdgcn_readfirstlane(a.relu) != 0 ? 1 : 0) | (a.bias != nullptr ? 2 : 0)) {
        case 0: finish(std::false_type{}, std::false_type{}); break;
        case 1: finish(std::true_type{}, std::false_type{}); break;
        case 2: finish(std::false_type{}, std::true_type{}); break;
        default: finish(std::true_type{}, std::true_type{}); break;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Wave-specialised variant (tiles 4 / 5 = 16 / 32 pixels).  In the kernel above the two convs run one after the other inside a
// workgroup and ~9 us of loads, barriers and LDS traffic overlap nothing.  Here both operand sets are staged up front (window AND the
// old channels of the 1x1's rows: they no longer share storage), then the workgroup splits: waves 0-3 run the 3x3 (K split four
// ways, weights through a 6-chunk register ring, partial tiles summed by the same four waves behind an LDS arrival counter) while
// waves 4-7 run the 1x1 over the OLD channels (32 output channels per wave), which do not depend on the 3x3; only the last two
// 16-channel chunks wait (second arrival counter) for the fresh 32 channels.  A SIMD hosts one wave of each kind, so the two MFMA
// streams interleave on the matrix pipe and each hides the other's fragment reads, weight waits and reductions.
// The LDS counters are bumped by every 3x3 wave unconditionally (no early exit), so the waits always end.
// ------------------------------------------------------------------------------------------------------------------------
template <int PB, bool PRE>
__global__ __launch_bounds__(512) void conv_dense_fused_ws_kernel(const ConvArgs a, const FusedArgs f, const int win_off, const int part_off) {
    constexpr int NT = 512, PX = 16 * PB, D = 8, D3 = 6, TN3 = 2, PP = 32 + 4, CW = 4;      // CW: waves per role
    constexpr int MAXS = PB == 1 ? 8 : 16, MAXW = 8;
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_fused[];
    const int K = a.in.c, Kold = K - 32, P = K + kRowPad, CH = K >> 4, Cin3 = f.in3.c, P3 = Cin3 + kRowPad;
    float* const sA = reinterpret_cast<float*>(smem_fused);                        // [PX][P]
    float* const sWin = sA + win_off;                                              // [npx][P3]
    float* const sPart = sA + part_off;                                            // [CW][PX][PP]
    int* const sCnt = reinterpret_cast<int*>(sPart + CW * PX * PP);                // [2] arrival counters

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, gk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // role by wave half (waves i and i + 4 share a SIMD: measured, the parity split -- a.debug bit 32 -- is 8 % slower), so every SIMD hosts
    // one wave of each role
    const bool by_half = (a.debug & 32) == 0;
    const bool conv3 = by_half ? wave < CW : (wave & 1) == 0;      // wave-uniform role
    const int wr = by_half ? (conv3 ? wave : wave - CW) : (wave >> 1);   // index inside the role
    const int H = a.in.h, W = a.in.w;
    const int M = a.in.n * H * W;
    const int m0 = blockIdx.x * PX;
    const int ipitch = int(a.in.sw), opitch = int(a.out.sw), bpitch = int(f.in3.sw);

    // ---- phase 0 (all waves): window + old channels -> LDS; each role primes its weight ring ----
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(f.in3.p, 0, int((int64_t(M - 1) * bpitch + Cin3) * 4), kBufferRsrcFlags);
    const int c4n3 = Cin3 >> 2;
    const int p_lo = m0 - W - 1;
    const int items3 = (PX + 2 * W + 2) * c4n3;
    u32x4 wv[MAXW];
#pragma unroll
    for (int u = 0; u < MAXW; ++u) {
        const int idx = tid + u * NT;
        const int row = idx / c4n3, c4 = idx - row * c4n3;
        const int p = p_lo + row;
        wv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, (idx < items3 && p >= 0 && p < M) ? unsigned(p * bpitch + c4 * 4) * 4u : OOB, 0, 0);
    }
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(a.in.p, 0, int((int64_t(M - 1) * ipitch + K) * 4), kBufferRsrcFlags);
    const int c4n = Kold >> 2;
    const int rpp = NT / c4n;
    const int xrow0 = tid / c4n, xc4 = tid - xrow0 * c4n;
    const bool xact = xrow0 < rpp;
    u32x4 xv[MAXS];
#pragma unroll
    for (int u = 0; u < MAXS; ++u) {
        const int row = xrow0 + u * rpp;
        const int p = m0 + row;
        xv[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (xact && row < PX && p < M) ? unsigned(p * ipitch + xc4 * 4) * 4u : OOB, 0, 0);
    }
    // weight rings: one array, the role decides what it holds (3x3: D3 chunks x 2 channel blocks; 1x1: D chunks x 2 channel blocks)
    const int cpt3 = Cin3 >> 4, total3 = 9 * cpt3;
    const int cb = int(int64_t(total3) * wr / CW), ce = int(int64_t(total3) * (wr + 1) / CW);
    const __amdgpu_buffer_rsrc_t rs_w3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(f.wfrag3), 0, 32 * 9 * Cin3 * 4, kBufferRsrcFlags);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wfrag), 0, 128 * K * 4, kBufferRsrcFlags);
    u32x4 ring[D][2];
    int c_l = 0;                                       // next chunk to load (role-relative)
    auto issue = [&](int slot) {
        if (conv3) {
            const int ch = cb + c_l;
#pragma unroll
            for (int j = 0; j < TN3; ++j)
                ring[slot][j] = __builtin_amdgcn_raw_buffer_load_b128(rs_w3, ch < ce ? unsigned((j * total3 + ch) * 64 + lane) * 16u : OOB, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                ring[slot][j] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, c_l < CH ? unsigned(((2 * wr + j) * CH + c_l) * 64 + lane) * 16u : OOB, 0, 0);
        }
        ++c_l;
    };
#pragma unroll
    for (int s = 0; s < D; ++s)
        if (!conv3 || s < D3) issue(s);                // wave-uniform
    f32x4 xsc = {1.f, 1.f, 1.f, 1.f}, xsf = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PRE) {
        if (xact) {
            xsc = *reinterpret_cast<const f32x4*>(a.pre_scale + xc4 * 4);
            xsf = *reinterpret_cast<const f32x4*>(a.pre_shift + xc4 * 4);
        }
    }
    if (tid < 2) sCnt[tid] = 0;
#pragma unroll
    for (int u = 0; u < MAXW; ++u) {
        const int idx = tid + u * NT;
        if (idx < items3) {
            const int row = idx / c4n3, c4 = idx - row * c4n3;
            *reinterpret_cast<u32x4*>(sWin + row * P3 + c4 * 4) = wv[u];
        }
    }
    if (xact) {
#pragma unroll
        for (int u = 0; u < MAXS; ++u) {
            const int row = xrow0 + u * rpp;
            if (row < PX) {
                f32x4 x = __builtin_bit_cast(f32x4, xv[u]);
                if constexpr (PRE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float y = x[e] * xsc[e] + xsf[e];
                        x[e] = a.pre_relu ? fmaxf(y, 0.f) : y;
                    }
                }
                *reinterpret_cast<f32x4*>(sA + row * P + xc4 * 4) = x;
            }
        }
    }
    __syncthreads();                                   // the only workgroup-wide barrier

    if (conv3) {
        // ================= 3x3 role =================
        f32x4 acc3[PB][TN3];
        bool mok[PB];
        int oy[PB], ox[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            const int m = m0 + pb * 16 + r;
            mok[pb] = m < M;
            const int rem = (mok[pb] ? m : 0) % (H * W);
            oy[pb] = rem / W;
            ox[pb] = rem - oy[pb] * W;
#pragma unroll
            for (int j = 0; j < TN3; ++j) acc3[pb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        int c_c = 0;
        auto compute3 = [&](int slot) {
            const int ch = cb + c_c;
            const int tap = ch / cpt3, c0 = (ch - tap * cpt3) * 16;
            const int ky = tap / 3, kx = tap - ky * 3;
            f32x4 av[PB];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                const bool ok = mok[pb] && unsigned(oy[pb] + ky - 1) < unsigned(H) && unsigned(ox[pb] + kx - 1) < unsigned(W);
                av[pb] = *reinterpret_cast<const f32x4*>(sWin + (pb * 16 + r + ky * W + kx) * P3 + c0 + gk * 4);
                if (!ok) av[pb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < TN3; ++j) {
                const f32x4 bv = __builtin_bit_cast(f32x4, ring[slot][j]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int pb = 0; pb < PB; ++pb) acc3[pb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[e], av[pb][e], acc3[pb][j], 0, 0, 0);
            }
            ++c_c;
        };
        const int n3 = ce - cb, full3 = n3 / D3, rem3 = n3 - full3 * D3;
        for (int it = 0; it < full3; ++it) {
#pragma unroll
            for (int s = 0; s < D3; ++s) {
                compute3(s);
                issue(s);
            }
        }
#pragma unroll
        for (int s = 0; s < D3; ++s)
            if (s < rem3) compute3(s);
        // publish this wave's partial tile, wait for the other three
#pragma unroll
        for (int pb = 0; pb < PB; ++pb)
#pragma unroll
            for (int j = 0; j < TN3; ++j) *reinterpret_cast<f32x4*>(sPart + (wr * PX + pb * 16 + r) * PP + j * 16 + 4 * gk) = acc3[pb][j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");        // ds writes retired before the arrival is visible (workgroup scope: LDS only, no cache write-back)
        if (lane == 0) __hip_atomic_fetch_add(&sCnt[0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(&sCnt[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < CW) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // final sum of a quarter of the tile: bias / ReLU of the 3x3, raw value to the block buffer, prologue'd value into the 1x1's rows
        {
            const __amdgpu_buffer_rsrc_t rs_o3 = __builtin_amdgcn_make_buffer_rsrc(f.out3.p, 0, int((int64_t(M - 1) * int(f.out3.sw) + 32) * 4), kBufferRsrcFlags);
            constexpr int ROWS = PX / CW;              // rows per 3x3 wave
            for (int idx = lane; idx < ROWS * 16; idx += 64) {
                const int p = wr * ROWS + (idx >> 4), c2 = (idx & 15) * 2;
                f32x2 v = {0.f, 0.f};
#pragma unroll
                for (int w = 0; w < CW; ++w) {
                    const f32x2 x = *reinterpret_cast<const f32x2*>(sPart + (w * PX + p) * PP + c2);
                    v[0] += x[0];
                    v[1] += x[1];
                }
                if (f.bias3 != nullptr) { v[0] += f.bias3[c2]; v[1] += f.bias3[c2 + 1]; }
                if (f.relu3) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); }
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs_o3, m0 + p < M ? unsigned((m0 + p) * int(f.out3.sw) + c2) * 4u : OOB, 0, 0);
                if constexpr (PRE) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float y = v[e] * a.pre_scale[Kold + c2 + e] + a.pre_shift[Kold + c2 + e];
                        v[e] = a.pre_relu ? fmaxf(y, 0.f) : y;
                    }
                }
                *reinterpret_cast<f32x2*>(sA + p * P + Kold + c2) = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __hip_atomic_fetch_add(&sCnt[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }

    // ================= 1x1 role: 32 output channels per wave =================
    f32x4 acc[PB][2];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[pb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ebias[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (a.bias != nullptr) {
        ebias[0] = *reinterpret_cast<const f32x4*>(a.bias + wr * 32 + 4 * gk);
        ebias[1] = *reinterpret_cast<const f32x4*>(a.bias + wr * 32 + 16 + 4 * gk);
    }
    int c_c = 0;
    const float* const arow = sA + r * P + gk * 4;
    f32x4 avn[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) avn[pb] = *reinterpret_cast<const f32x4*>(arow + pb * 16 * P);
    auto compute = [&](int slot) {
        f32x4 av[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) av[pb] = avn[pb];
        if (c_c + 1 == CH - 2) {                       // the next fragment read is the first of the fresh channels: they must have landed
            while (__hip_atomic_load(&sCnt[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < CW) __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        const float* const nxt = arow + (c_c + 1 < CH ? c_c + 1 : c_c) * 16;
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) avn[pb] = *reinterpret_cast<const f32x4*>(nxt + pb * 16 * P);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int pb = 0; pb < PB; ++pb)
                    acc[pb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, ring[slot][j])[e], av[pb][e], acc[pb][j], 0, 0, 0);
        ++c_c;
    };
    const int full = CH / D, rem = CH - full * D;
    for (int it = 0; it < full; ++it) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
            compute(s);
            issue(s);
        }
    }
#pragma unroll
    for (int s = 0; s < D; ++s)
        if (s < rem) compute(s);

    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(a.out.p, 0, int((int64_t(M - 1) * opitch + 128) * 4), kBufferRsrcFlags);
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        const int m = m0 + pb * 16 + r;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = wr * 32 + j * 16 + 4 * gk;
            f32x4 v = acc[pb][j];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += ebias[j][e];
            if (a.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs_out, m < M ? unsigned(m * opitch + n) * 4u : OOB, 0, 0);
        }
    }
}

// LDS of the wave-specialised variant: rows, window, partial tiles (4 waves) and two counters, nothing shared
static size_t fused_ws_lds_bytes(const ConvArgs& a, const FusedArgs& f, int pb, int* win_off = nullptr, int* part_off = nullptr) {
    const size_t px = size_t(16) * pb;
    const size_t rows = px * (a.in.c + kRowPad) * 4, win = (px + 2 * a.in.w + 2) * (f.in3.c + kRowPad) * 4, part = size_t(4) * px * 36 * 4;
    if (win_off) *win_off = int(rows / 4);
    if (part_off) *part_off = int((rows + win) / 4);
    return rows + win + part + 16;
}

// LDS: the 1x1's rows and the 3x3's window share storage (the rows are staged in registers until the window is dead), the partial
// tiles of the 3x3 sit behind them.  Returns the partial tiles' offset in floats through part_off.
static size_t fused_lds_bytes(const ConvArgs& a, const FusedArgs& f, int pb, int* part_off = nullptr) {
    const size_t px = size_t(16) * pb;
    const size_t rows = px * (a.in.c + kRowPad) * 4, win = (px + 2 * a.in.w + 2) * (f.in3.c + kRowPad) * 4, part = size_t(4) * px * 36 * 4;
    const size_t first = (rows > win ? rows : win);
    if (part_off) *part_off = int(first / 4);
    return first + part + 64;                          // + the zeroed row the 3x3's out-of-image taps read
}

// ceil(2^20 / d): n / d == (n * mg) >> 20 for n * d < 2^20;  floor(2^32 / d): see udiv_uniform
static unsigned mg20(unsigned d) { return ((1u << 20) + d - 1) / d; }
static unsigned mg32(unsigned d) { return d == 1 ? 0xffffffffu : unsigned((uint64_t(1) << 32) / d); }

static FusedConsts fused_consts(const ConvArgs& a, const FusedArgs& f, int pb) {
    FusedConsts k;
    const int px = 16 * pb, c4n3 = f.in3.c / 4, c4n = (a.in.c - 32) / 4, npx = px + 2 * a.in.w + 2;
    k.mg20_c4n3 = mg20(c4n3);
    k.mg20_c4n = mg20(c4n);
    k.mg20_w = mg20(a.in.w);
    k.mg20_h = a.in.h <= 512 ? mg20(a.in.h) : 0;
    k.hbig = a.in.h <= 512 ? 0x7fffffffu : unsigned(a.in.h);
    k.mg32_hw = mg32(unsigned(a.in.h) * unsigned(a.in.w));
    k.mg32_w = mg32(a.in.w);
    k.mg32_cpt3 = mg32(f.in3.c / 16);
    k.wrpp = 512 / c4n3;
    k.wfull = npx / k.wrpp;
    k.wlast = npx % k.wrpp;
    k.rpp = 512 / c4n;
    k.xfull = px / k.rpp;
    k.xlast = px % k.rpp;
    return k;
}

static bool dense(const TensorArg& t) { return t.sc == 1 && t.sh == t.w * t.sw && t.sn == t.h * t.sh; }

// tile: 1 / 2 = 16-pixel blocks per workgroup (one workgroup per CU); 3 = 16-pixel tiles in the two-workgroups-per-CU variant;
// 4 / 5 = wave-specialised, 16 / 32 pixels; 6 = 16-pixel tiles on a two-row grid (each row half of the 1x1's output channels)
static int fused_pixel_blocks(int tile) { return tile == 3 || tile == 6 ? 1 : (tile >= 4 ? tile - 3 : tile); }

bool ConvDenseFusedEligible(const ConvArgs& a, const FusedArgs& f, int tile) {
    if (tile < 1 || tile > kNumConvDenseFusedTiles) return false;
    const int pb = fused_pixel_blocks(tile);
    const bool ws = tile == 4 || tile == 5;
    if (tile == 3 && fused_lds_bytes(a, f, 1) > size_t(80) * 1024) return false;
    if (ws && (fused_ws_lds_bytes(a, f, pb) > size_t(160) * 1024 || 9 * (f.in3.c / 16) < 4 * 1)) return false;
    if (a.in.f16 || a.out.f16 || a.in.f8 || a.out.f8 || f.in3.f16 || f.out3.f16 || f.in3.f8 || f.out3.f8) return false;
    if (a.wfrag == nullptr || f.wfrag3 == nullptr || a.res.p != nullptr) return false;
    if (a.kh != 1 || a.kw != 1 || a.sh != 1 || a.sw != 1 || a.pt != 0 || a.pl != 0) return false;
    if (a.out.c != 128 || f.out3.c != 32 || a.in.c < 48 || (a.in.c % 16) || (f.in3.c % 16)) return false;
    const int total3 = 9 * (f.in3.c / 16);
    if (total3 > 72 || total3 < 8) return false;
    // same pixel grid everywhere
    for (const TensorArg* t : {&a.out, &f.in3, &f.out3})
        if (t->n != a.in.n || t->h != a.in.h || t->w != a.in.w) return false;
    if (!dense(a.in) || !dense(a.out) || !dense(f.in3) || !dense(f.out3)) return false;
    // the fresh 32 channels are the tail of the 1x1's input view, in the same buffer rows
    if (f.out3.sw != a.in.sw || f.out3.p != a.in.p + (a.in.c - 32)) return false;
    if ((a.in.sw % 4) || (a.out.sw % 4) || (f.in3.sw % 4) || (f.out3.sw % 2)) return false;
    for (const void* p : {static_cast<const void*>(a.in.p), static_cast<const void*>(a.out.p), static_cast<const void*>(f.in3.p), static_cast<const void*>(a.wfrag),
                          static_cast<const void*>(f.wfrag3)})
        if (!Aligned16(p)) return false;
    if (reinterpret_cast<uintptr_t>(f.out3.p) & 7) return false;
    if (a.bias && !Aligned16(a.bias)) return false;
    if (a.pre_scale && (!Aligned16(a.pre_scale) || !Aligned16(a.pre_shift))) return false;
    const int64_t M = int64_t(a.in.n) * a.in.h * a.in.w;
    if (M > 65536 || (M + 64) * a.in.sw * 4 >= (int64_t(1) << 31) || M * a.out.sw * 4 >= (int64_t(1) << 31) || (M + 64) * f.in3.sw * 4 >= (int64_t(1) << 31)) return false;
    const int px = 16 * pb;
    {   // staging slots: a thread keeps one 4-channel column, rows advance by rpp = 512 / columns per slot
        const int c4n = (a.in.c - 32) / 4;
        if (c4n > 512 || (px + 512 / c4n - 1) / (512 / c4n) > (pb == 1 ? 8 : 16)) return false;
    }
    if ((a.in.c - 32) % 4 || !Aligned16(a.pre_scale) || (f.bias3 && (reinterpret_cast<uintptr_t>(f.bias3) & 7))) return false;
    if (int64_t(px + 2 * a.in.w + 2) * (f.in3.c / 4) > int64_t(8) * 512) return false;            // window slots
    if (!ws) {
        // window slots with one 4-channel column per thread (512 / columns rows per slot); 24-bit row * pitch products; every row a slot can
        // name (the window's halo and a partial last slot: < 1024 rows past M) stays below 2^31 bytes, so no offset wraps back into range
        const int wrpp = 512 / (f.in3.c / 4);
        if ((px + 2 * a.in.w + 2 + wrpp - 1) / wrpp > 8 || a.in.w > 500) return false;
        if (a.in.sw >= (int64_t(1) << 22) || a.out.sw >= (int64_t(1) << 22) || f.in3.sw >= (int64_t(1) << 22)) return false;
        if ((M + 1024) * a.in.sw * 4 >= (int64_t(1) << 31) || (M + 1024) * f.in3.sw * 4 >= (int64_t(1) << 31) || (M + 1024) * a.out.sw * 4 >= (int64_t(1) << 31)) return false;
    }
    return fused_lds_bytes(a, f, pb) <= size_t(160) * 1024;
}

hipError_t LaunchConvDenseFused(const ConvArgs& a_in, const FusedArgs& f, int tile, hipStream_t stream) {
    if (!ConvDenseFusedEligible(a_in, f, tile)) return hipErrorInvalidValue;
    const bool occ2 = tile == 3;
    const int pb = fused_pixel_blocks(tile);
    if (tile == 4 || tile == 5) {
        const int64_t Mw = int64_t(a_in.in.n) * a_in.in.h * a_in.in.w;
        const dim3 gridw(unsigned((Mw + 16 * pb - 1) / (16 * pb)));
        int win_off = 0, poff = 0;
        const size_t ldsw = fused_ws_lds_bytes(a_in, f, pb, &win_off, &poff);
        ConvArgs aw = a_in;
        const int dbgw = Knobs().debug_ablate;
        aw.debug = dbgw;
        if (pb == 1) {
            if (aw.pre_scale) conv_dense_fused_ws_kernel<1, true><<<gridw, dim3(512), ldsw, stream>>>(aw, f, win_off, poff);
            else conv_dense_fused_ws_kernel<1, false><<<gridw, dim3(512), ldsw, stream>>>(aw, f, win_off, poff);
        } else {
            if (aw.pre_scale) conv_dense_fused_ws_kernel<2, true><<<gridw, dim3(512), ldsw, stream>>>(aw, f, win_off, poff);
            else conv_dense_fused_ws_kernel<2, false><<<gridw, dim3(512), ldsw, stream>>>(aw, f, win_off, poff);
        }
        return hipGetLastError();
    }
    ConvArgs a = a_in;
    const int dbg = Knobs().debug_ablate;
    a.debug = dbg;      // timing-only ablations (wrong results): 1 no 3x3 MFMAs, 2 no 1x1 loop, 4 no 3x3 weight loads, 8 no old-channel loads, 16 no 1x1 weight loads
    const int64_t M = int64_t(a.in.n) * a.in.h * a.in.w;
    const dim3 grid(unsigned((M + 16 * pb - 1) / (16 * pb)));
    int part_off = 0;
    const size_t lds = fused_lds_bytes(a, f, pb, &part_off);
    FusedArgs fk = f;
    fk.k = fused_consts(a, f, pb);
    if (tile == 6) {
        const dim3 grid2(grid.x, 2);
        if (a.pre_scale) conv_dense_fused_kernel<1, true, false, true><<<grid2, dim3(512), lds, stream>>>(a, fk, part_off);
        else conv_dense_fused_kernel<1, false, false, true><<<grid2, dim3(512), lds, stream>>>(a, fk, part_off);
        return hipGetLastError();
    }
    if (occ2) {
        if (a.pre_scale) conv_dense_fused_kernel<1, true, true><<<grid, dim3(512), lds, stream>>>(a, fk, part_off);
        else conv_dense_fused_kernel<1, false, true><<<grid, dim3(512), lds, stream>>>(a, fk, part_off);
    } else if (pb == 1) {
        if (a.pre_scale) conv_dense_fused_kernel<1, true, false><<<grid, dim3(512), lds, stream>>>(a, fk, part_off);
        else conv_dense_fused_kernel<1, false, false><<<grid, dim3(512), lds, stream>>>(a, fk, part_off);
    } else {
        if (a.pre_scale) conv_dense_fused_kernel<2, true, false><<<grid, dim3(512), lds, stream>>>(a, fk, part_off);
        else conv_dense_fused_kernel<2, false, false><<<grid, dim3(512), lds, stream>>>(a, fk, part_off);
    }
    return hipGetLastError();
}

hipError_t InitKernelsFused() {
    hipError_t e;
#define IE_FUSED_ATTR(PB, PRE, ...)                                                                                                                                 \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dense_fused_kernel<PB, PRE, __VA_ARGS__>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)) != hipSuccess) return e;
    IE_FUSED_ATTR(1, true, false) IE_FUSED_ATTR(1, false, false) IE_FUSED_ATTR(2, true, false) IE_FUSED_ATTR(2, false, false) IE_FUSED_ATTR(1, true, true) IE_FUSED_ATTR(1, false, true)
    IE_FUSED_ATTR(1, true, false, true) IE_FUSED_ATTR(1, false, false, true)
#undef IE_FUSED_ATTR
#define IE_FUSED_WS_ATTR(PB, PRE)                                                                                                                                   \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_dense_fused_ws_kernel<PB, PRE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)) != hipSuccess) return e;
    IE_FUSED_WS_ATTR(1, true) IE_FUSED_WS_ATTR(1, false) IE_FUSED_WS_ATTR(2, true) IE_FUSED_WS_ATTR(2, false)
#undef IE_FUSED_WS_ATTR
    return hipSuccess;
}

}  // namespace ie
