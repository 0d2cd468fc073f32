// Probe: a 32x32 MFMA result used as the B operand of the next MFMA, with the k order that implies (kernels_attn.hip, the PV product).
//
//   hipcc --offload-arch=gfx950 -O2 scripts/probes/attn_pv_order.hip -o attn_pv_order && ./attn_pv_order
//
// One wave.  X^T = K . Q^T (32 keys x 32 queries, 32x32 result: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), then
// O^T = V^T . X, which sums over X's row index, with X taken from the registers it is in:
//   fp32 (v_mfma_f32_32x32x2_f32):   register r is one k-step; the A operand of lane (e = lane & 31, hf = lane >> 5) is V[(r & 3) + 8 (r >> 2) + 4 hf][e]
//   fp16 (v_mfma_f32_32x32x16_f16):  registers 8 s ... 8 s + 7, as halfs, are k-step s; element j of the A operand is V[16 s + 8 (j >> 2) + 4 hf + (j & 3)][e]
// All data are small integers, so every product and sum is exact in both formats, and V is asymmetric (V[j][e] = 3 j - 2 e + (j * e) % 5): a
// wrong k order changes almost every output.  The program compares all 32 x 32 outputs of both forms with the integer result from the host and
// prints the number of mismatches (0 expected); with NATURAL=1 in the environment it gathers V in natural k order instead, which must fail.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));

constexpr int KD = 16;      // reduction length of the first product

__host__ __device__ inline int kval(int j, int d) { return (j + 2 * d) % 5 - 2; }
__host__ __device__ inline int qval(int i, int d) { return (3 * i + d) % 4 - 1; }
__host__ __device__ inline int vval(int j, int e) { return 3 * j - 2 * e + (j * e) % 5; }

__global__ void probe(float* out32, float* out16, int natural) {
    const int lane = threadIdx.x, col = lane & 31, hf = lane >> 5;
    f32x16 x32, x16, o32, o16;
    for (int r = 0; r < 16; ++r) { x32[r] = 0.f; x16[r] = 0.f; o32[r] = 0.f; o16[r] = 0.f; }
    // X^T = K . Q^T: lane half hf supplies d = hf * KD / 2 ... of its K row (A) and of its Q row (B)
    for (int k = 0; k < KD / 2; ++k) x32 = __builtin_amdgcn_mfma_f32_32x32x2f32(float(kval(col, hf * (KD / 2) + k)), float(qval(col, hf * (KD / 2) + k)), x32, 0, 0, 0);
    h8v ka, qa;
    for (int j = 0; j < 8; ++j) { ka[j] = _Float16(kval(col, hf * 8 + j)); qa[j] = _Float16(qval(col, hf * 8 + j)); }
    x16 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka, qa, x16, 0, 0, 0);
    // O^T = V^T . X
    for (int r = 0; r < 16; ++r) {
        const int key = natural ? 2 * r + hf : (r & 3) + 8 * (r >> 2) + 4 * hf;
        o32 = __builtin_amdgcn_mfma_f32_32x32x2f32(float(vval(key, col)), x32[r], o32, 0, 0, 0);
    }
    for (int s = 0; s < 2; ++s) {
        h8v xb, va;
        for (int j = 0; j < 8; ++j) {
            const int key = natural ? 16 * s + 8 * hf + j : 16 * s + 8 * (j >> 2) + 4 * hf + (j & 3);
            xb[j] = _Float16(x16[8 * s + j]);
            va[j] = _Float16(vval(key, col));
        }
        o16 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, xb, o16, 0, 0, 0);
    }
    // O^T[e][query]: col = query, row = e
    for (int r = 0; r < 16; ++r) {
        const int e = (r & 3) + 8 * (r >> 2) + 4 * hf;
        out32[col * 32 + e] = o32[r];
        out16[col * 32 + e] = o16[r];
    }
}

int main() {
    const int natural = getenv("NATURAL") != nullptr;
    float *d32, *d16, h32[1024], h16[1024];
    if (hipMalloc(&d32, sizeof(h32)) != hipSuccess || hipMalloc(&d16, sizeof(h16)) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    probe<<<1, 64>>>(d32, d16, natural);
    if (hipMemcpy(h32, d32, sizeof(h32), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h16, d16, sizeof(h16), hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 2; }
    int bad32 = 0, bad16 = 0;
    for (int i = 0; i < 32; ++i)
        for (int e = 0; e < 32; ++e) {
            long o = 0;
            for (int j = 0; j < 32; ++j) {
                long x = 0;
                for (int d = 0; d < KD; ++d) x += kval(j, d) * qval(i, d);
                o += x * vval(j, e);
            }
            bad32 += h32[i * 32 + e] != float(o);
            bad16 += h16[i * 32 + e] != float(o);
        }
    printf("k order %s: mismatches fp32 %d / 1024, fp16 %d / 1024\n", natural ? "natural" : "permuted", bad32, bad16);
    return (bad32 || bad16) ? 1 : 0;
}
