// f32-grade products on the bf16 matrix pipe: C[16x16] = W[16x32] * Z[32x16] with both operands split EXACTLY into three bf16 pieces
// (truncation: x = x1 + x2 + x3, 8 + 8 + 8 mantissa bits) and the six largest of the nine partial products summed in f32
// (the 16x16x32 bf16 MFMA, w16_mfma_bf: 16 cycles each on gfx950 against 8 x 32 cycles of v_mfma_f32_16x16x4_f32 for the same K = 32).
// Checks the operand layout (lane 16q + m: row / column m, K slots 8q .. 8q + 7 as four dwords of bf16 pairs) and the accuracy
// against float64 and against the f32 MFMA, then times both forms with the split's VALU work included.
// The split, the products and the ReLU forms are the library's own: the w16_* primitives of epnn_amd/csrc/epnn_common.h, compiled
// here under the library's flags.  Only the forms the kernels no longer issue are defined in this file, as comparison arms.
//   python3 ../../__graft_entry__.py --micro  (or make bf16x6: the same), then  ./bf16x6      (./bf16x6 k16pairs: only the K = 16
//   pairing; ./bf16x6 rem4x4: the remainders on the 4x4x4 bf16 MFMA -- exactness, operand layout and cost beside the K = 16
//   form; ./bf16x6 clamp: the sweep tile's two ReLU forms)
// The library's flags switch packed f32 instructions off, so the timing arm "+ 8 v_pk_add_f32" is left out of that build; by hand:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffinite-math-only -fno-signed-zeros -mllvm -amdgpu-mfma-vgpr-form -Wno-unused-value \
//         -DBF16X6_PK_ADD -I ../../epnn_amd/csrc -o bf16x6 bf16x6.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "epnn_common.h"

// The same decomposition with round-to-nearest pieces: v_cvt_pk_bf16_f32 rounds and packs two values in one instruction and
// v_dot2c_f32_bf16 takes a remainder straight from the packed pair (x - 1 * piece_lo - 0 * piece_hi: exact, the result is representable),
// so no piece is ever expanded to float32 again: 7 instructions per two values instead of 11.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt_pk(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
__device__ __forceinline__ float rem_lo(unsigned pk, float x) { return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, pk), __builtin_bit_cast(bf16x2, 0x8000bf80u), x, false); }
__device__ __forceinline__ float rem_hi(unsigned pk, float x) { return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, pk), __builtin_bit_cast(bf16x2, 0xbf800000u), x, false); }
__device__ __forceinline__ void split3r(const float (&v)[8], u32x4 &p1, u32x4 &p2, u32x4 &p3) {
    float a[8], b[8];       // level by level: no instruction reads the result of the one in front of it
#pragma unroll
    for (int j = 0; j < 4; ++j) p1[j] = cvt_pk(v[2 * j], v[2 * j + 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[2 * j] = rem_lo(p1[j], v[2 * j]); a[2 * j + 1] = rem_hi(p1[j], v[2 * j + 1]); }
#pragma unroll
    for (int j = 0; j < 4; ++j) p2[j] = cvt_pk(a[2 * j], a[2 * j + 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { b[2 * j] = rem_lo(p2[j], a[2 * j]); b[2 * j + 1] = rem_hi(p2[j], a[2 * j + 1]); }
#pragma unroll
    for (int j = 0; j < 4; ++j) p3[j] = cvt_pk(b[2 * j], b[2 * j + 1]);
}
// Third form: the remainders on the MATRIX pipe.  With the pieces packed as a B operand (lane 16 q + m: column m, K slots 8 q + s =
// its values v[s]) and the values themselves as the accumulator (rows 4 q + r of row block rb = v[4 rb + r]), D = C + A B with
// A[i][k] = -1 for k = 8 (i / 4) + 4 rb + i % 4 is x - x1 in place: 2 MFMAs per level and 8 values instead of 8 v_and + 8 v_sub.
// (-1) * piece is exact, the other 31 products are zeros, the result is representable: exact if the pipe adds C unrounded.
__device__ __forceinline__ void ident_operand(u32x4 (&A)[2]) {
    const int lane = threadIdx.x & 63, qa = lane >> 4, ma = lane & 15;
    for (int rb = 0; rb < 2; ++rb)
        for (int d = 0; d < 4; ++d)
            A[rb][d] = (qa == (ma >> 2) && d == 2 * rb + ((ma & 3) >> 1)) ? (0xbf80u << (16 * (ma & 1))) : 0u;
}
__device__ __forceinline__ void split3m(const float (&v)[8], const u32x4 (&A)[2], u32x4 &p1, u32x4 &p2, u32x4 &p3) {
    f32x4 x0 = {v[0], v[1], v[2], v[3]}, x1 = {v[4], v[5], v[6], v[7]};
    p1 = w16_pack_hi(x0, x1);
    x0 = w16_mfma_bf(A[0], p1, x0); x1 = w16_mfma_bf(A[1], p1, x1);
    p2 = w16_pack_hi(x0, x1);
    x0 = w16_mfma_bf(A[0], p2, x0); x1 = w16_mfma_bf(A[1], p2, x1);
    p3 = w16_pack_hi(x0, x1);
}
// Fourth form: the same remainders with v_mfma_f32_16x16x16_bf16 (K = 16: lane 16 q + m holds K slots 4 q .. 4 q + 3; a row block's
// four values are two dwords of the packed piece, the -I operand is the same for both row blocks)
__device__ __forceinline__ f32x4 mm16(w16_u32x2 a, w16_u32x2 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(w16_s16x4, a), __builtin_bit_cast(w16_s16x4, b), c, 0, 0, 0);
}
__device__ __forceinline__ void split3k(const float (&v)[8], u32x4 &p1, u32x4 &p2, u32x4 &p3) {
    const int lane = threadIdx.x & 63, qa = lane >> 4, ma = lane & 15;
    w16_u32x2 I;
    for (int d = 0; d < 2; ++d) I[d] = (qa == (ma >> 2) && d == ((ma & 3) >> 1)) ? (0xbf80u << (16 * (ma & 1))) : 0u;
    f32x4 x0 = {v[0], v[1], v[2], v[3]}, x1 = {v[4], v[5], v[6], v[7]};
    p1 = w16_pack_hi(x0, x1);
    x0 = mm16(I, w16_u32x2{p1[0], p1[1]}, x0); x1 = mm16(I, w16_u32x2{p1[2], p1[3]}, x1);
    p2 = w16_pack_hi(x0, x1);
    x0 = mm16(I, w16_u32x2{p2[0], p2[1]}, x0); x1 = mm16(I, w16_u32x2{p2[2], p2[3]}, x1);
    p3 = w16_pack_hi(x0, x1);
}
// SPLIT 0: the truncated pieces by v_and_b32 / v_sub_f32 (w16_split3_valu), 1: nearest / dot2c, 2: remainders on the K = 32 MFMA,
// 3: on the K = 16 MFMA, 4: what the kernels issue (w16_split3: the remainders on the 4x4x4 bf16 MFMA, w16_ident / w16_rem)
template <int SPLIT> __device__ __forceinline__ void split_any(const float (&v)[8], const u32x4 (&A)[2], u32x4 &p1, u32x4 &p2, u32x4 &p3) {
    if (SPLIT == 4) w16_split3(v, p1, p2, p3); else if (SPLIT == 3) split3k(v, p1, p2, p3); else if (SPLIT == 2) split3m(v, A, p1, p2, p3); else if (SPLIT) split3r(v, p1, p2, p3); else w16_split3_valu(v, p1, p2, p3);
}
// exactness of a split: every lane splits 8 values, the host adds the pieces in float64
template <int SPLIT> __global__ void k_exact(const float *x, unsigned *pieces) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    float v[8];
    for (int s = 0; s < 8; ++s) v[s] = x[t * 8 + s];
    u32x4 p1, p2, p3, A[2];
    ident_operand(A);
    split_any<SPLIT>(v, A, p1, p2, p3);
    for (int j = 0; j < 4; ++j) { pieces[(t * 3 + 0) * 4 + j] = p1[j]; pieces[(t * 3 + 1) * 4 + j] = p2[j]; pieces[(t * 3 + 2) * 4 + j] = p3[j]; }
}
// W [16][32] row-major, Z [32][16] (k, n); out C [16][16]
template <int SPLIT> __global__ void k_check(const float *W, const float *Z, float *C6, float *C32) {
    const int lane = threadIdx.x, q = lane >> 4, m = lane & 15;
    float w[8], z[8];
    for (int s = 0; s < 8; ++s) { w[s] = W[m * 32 + 8 * q + s]; z[s] = Z[(8 * q + s) * 16 + m]; }
    u32x4 wb[2][3], z1, z2, z3;            // (w16_mm_bf takes two row blocks: this product has one, the second is a copy nobody reads)
    w16_split3_valu(w, wb[0][0], wb[0][1], wb[0][2]);      // the weights' pieces come from the host: truncation in both forms
    for (int pc = 0; pc < 3; ++pc) wb[1][pc] = wb[0][pc];
    u32x4 A[2];
    ident_operand(A);
    split_any<SPLIT>(z, A, z1, z2, z3);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    w16_mm_bf(wb, z1, z2, z3, acc);
    for (int r = 0; r < 4; ++r) C6[(4 * q + r) * 16 + m] = acc[0][r];
    f32x4 a32 = {0.f, 0.f, 0.f, 0.f};
    for (int k4 = 0; k4 < 8; ++k4)      // f32 MFMA: K = 4 per instruction, lane q supplies k = 4 k4 + q
        a32 = __builtin_amdgcn_mfma_f32_16x16x4f32(W[m * 32 + 4 * k4 + q], Z[(4 * k4 + q) * 16 + m], a32, 0, 0, 0);
    for (int r = 0; r < 4; ++r) C32[(4 * q + r) * 16 + m] = a32[r];
}
// timing: `tiles` dependent-free tiles per wave; MODE 0 = f32 MFMA (16 per tile: 2 row blocks x 8), 1 = bf16x6 incl. the split of z
// RELU 1 / 2: the tile with the pair sweep's own element-wise work around the MFMAs -- z1 = relu((P + R) + G), S += relu(acc) -- and the
// first ReLU as v_max_f32 (1) or as the output clamp of the add in front of it (2: min(max(a + b, 0), 1), one v_add_f32 ... clamp; the
// operands here keep every sum below 1, so both forms give the same bits)
template <int MODE, int EXTRA, int SPLIT, int RELU = 0>
__device__ __forceinline__ void time_body(const float *src, float *dst, int tiles) {
    const int lane = threadIdx.x & 63;
    float z[8], w32[2][8];
    u32x4 wb[2][3], A[2];
    ident_operand(A);
    for (int s = 0; s < 8; ++s) { z[s] = src[lane * 8 + s]; w32[0][s] = src[512 + lane * 8 + s]; w32[1][s] = src[1024 + lane * 8 + s]; }
    for (int rb = 0; rb < 2; ++rb) w16_split3_valu(w32[rb], wb[rb][0], wb[rb][1], wb[rb][2]);
    f32x4 S[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int t = 0; t < tiles; ++t) {
        float zz[8];
        if (RELU == 0) {
#pragma unroll
            for (int s = 0; s < 8; ++s) zz[s] = fmaxf(z[s] + S[s >> 2][s & 3] * 1e-9f, 0.f);     // (a dependence on the last tile, like S += relu(acc))
        } else {
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                f32x4 pre;
#pragma unroll
                for (int r = 0; r < 4; ++r) pre[r] = (z[4 * hb + r] + S[hb][r] * 1e-9f) + 0.25f * w32[1][4 * hb + r];
                pre = RELU == 2 ? w16_clamp01(pre) : w16_relu(pre);
#pragma unroll
                for (int r = 0; r < 4; ++r) zz[4 * hb + r] = pre[r];
            }
        }
        if (EXTRA == 1) {
#ifdef BF16X6_PK_ADD               // (inline assembly that the library's flags, packed f32 instructions off, do not assemble)
#pragma unroll
            for (int s = 0; s < 8; s += 2) {
                f32x2 a = {zz[s], zz[s + 1]}, b = {z[s], z[s + 1]}, c;
                asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(c) : "v"(a), "v"(b));
                asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(a) : "v"(c), "v"(b));
                zz[s] = a[0]; zz[s + 1] = a[1];
            }
#endif
        } else if (EXTRA == 2) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                float c;
                asm volatile("v_add_f32 %0, %1, %2" : "=v"(c) : "v"(zz[s]), "v"(z[s]));
                asm volatile("v_add_f32 %0, %1, %2" : "=v"(zz[s]) : "v"(c), "v"(z[s]));
            }
        } else if (EXTRA == 3) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                float c;
                asm volatile("v_max_f32 %0, %1, %2" : "=v"(c) : "v"(zz[s]), "v"(z[s]));
                asm volatile("v_max_f32 %0, %1, %2" : "=v"(zz[s]) : "v"(c), "v"(z[s]));
            }
        } else if (EXTRA == 4) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                float c;
                asm volatile("v_and_b32 %0, %1, %2" : "=v"(c) : "v"(zz[s]), "v"(z[s]));
                asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(zz[s]) : "v"(c), "v"(zz[s]), "v"(0x05040100u));      // (any selector: the arm times the instruction)
            }
        }
        f32x4 d[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (MODE == 0) {
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int s = 0; s < 8; ++s) d[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w32[rb][s], zz[s], d[rb], 0, 0, 0);
        } else {
            u32x4 z1, z2, z3;
            split_any<SPLIT>(zz, A, z1, z2, z3);
            w16_mm_bf(wb, z1, z2, z3, d);
        }
        if (RELU == 0) { S[0] += d[0]; S[1] += d[1]; }
        else { S[0] += w16_relu(d[0]); S[1] += w16_relu(d[1]); }
    }
    const size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    for (int r = 0; r < 4; ++r) dst[o + r] = S[0][r], dst[o + 4 + r] = S[1][r];
}
template <int MODE, int EXTRA = 0, int SPLIT = 0>
__global__ __launch_bounds__(64, 2) void k_time(const float *src, float *dst, int tiles) { time_body<MODE, EXTRA, SPLIT>(src, dst, tiles); }
// The same tile in workgroups of 256 or 512 threads -- a workgroup's wavefronts go round the CU's four SIMDs, so that is one or two
// wavefronts per SIMD by construction, with few enough workgroups that each has a CU to itself -- and timed by the wavefront's own
// clock: cyc[wavefront] = { s_memtime ticks, s_memrealtime ticks (100 MHz) } around the tile loop.
template <int SPLIT, int RELU = 0>
__global__ __launch_bounds__(512) void k_time_wg(const float *src, float *dst, int tiles, unsigned long long *cyc) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    time_body<1, 0, SPLIT, RELU>(src, dst, tiles);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if ((threadIdx.x & 63) == 0) { cyc[2 * w] = t1 - t0; cyc[2 * w + 1] = r1 - r0; }
}
// Layout probe of the 4x4x4 remainder: every lane holds four values (all zeros but in one lane of the launch), y = x - piece(x).
__global__ void k_probe4(const float *x, float *y) {
    const int lane = threadIdx.x;
    f32x4 v = {x[lane * 4], x[lane * 4 + 1], x[lane * 4 + 2], x[lane * 4 + 3]};
    const w16_u32x2 p = w16_pack_hi2(v);
    v = w16_rem(w16_ident(), p[0], p[1], v);
    for (int r = 0; r < 4; ++r) y[lane * 4 + r] = v[r];
}
// Back-to-back MFMAs of one kind, n x 32 per wavefront: INDEP 1 = eight accumulators in turn (no instruction waits for the one before
// it: the interval is what the pipe is held for), 0 = one accumulator (the instruction's latency).  KIND 0: 4x4x4, 1: 16x16x16, 2: 16x16x32.
template <int KIND, int INDEP>
__global__ __launch_bounds__(512) void k_rate(const float *src, float *dst, int n, unsigned long long *cyc) {
    const int lane = threadIdx.x & 63;
    const u32x4 a = {__float_as_uint(src[lane]) & 0xffff0000u, 0x3f803f80u, __float_as_uint(src[64 + lane]) >> 16, 0xbf800000u};
    const u32x4 b = {__float_as_uint(src[128 + lane]) >> 16, 0x3f800000u, __float_as_uint(src[192 + lane]) & 0xffff0000u, 0x3f80bf80u};
    f32x4 acc[8];
    for (int k = 0; k < 8; ++k) acc[k] = f32x4{src[256 + lane], (float)k, 0.f, 1.f};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int t = 0; t < n; ++t) {
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            f32x4 &c = acc[INDEP ? k & 7 : 0];
            if (KIND == 0) c = w16_rem(w16_u32x2{a[0], a[1]}, b[0], b[1], c);
            else if (KIND == 1) c = mm16(w16_u32x2{a[0], a[1]}, w16_u32x2{b[0], b[1]}, c);
            else c = w16_mfma_bf(a, b, c);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    f32x4 s = acc[0];
    for (int k = 1; k < 8; ++k) s += acc[k];
    const size_t o = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (int r = 0; r < 4; ++r) dst[o + r] = s[r];
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (lane == 0) { cyc[2 * w] = t1 - t0; cyc[2 * w + 1] = r1 - r0; }
}
// The K = 16 products of the fused kernels (w16_mm_bfk16, epnn_common.h): C[16x16] = W[16x16] * Z[16x16], six partial products.
// Six-instruction form (what the kernels issued before): six v_mfma_f32_16x16x16_bf16.  Paired form: w16_split3k16 and
// w16_mm_bfk16 themselves -- two K = 16 operands side by side in four consecutive registers are one K = 32 operand, so three
// 16x16x32 bf16 MFMAs take the same six products two at a time --
//     (w1|w2) . (z3|z1),   (w3|w1) . (z1|z2),   (w1|w2) . (z1|z2)
// with the kernel's row block as the two tuples w1 w2 | w3 w1 (the host's pack) and the activation as a = z3|z1 plus z2, b = z1|z2
// being a's upper half and z2 (W16K16).  Every block takes its own 16x16 pair of operands; `zs` receives the six operand dwords
// a, z2 (MFMA-remainder split), `zp` the pieces of the v_and / v_sub form in the same order.
__global__ void k_check16(const float *Wa, const float *Za, float *C6, float *C3, float *C32, unsigned *zs, unsigned *zp) {
    const int lane = threadIdx.x, q = lane >> 4, m = lane & 15, t = blockIdx.x;
    const float *W = Wa + t * 256, *Z = Za + t * 256;
    f32x4 w, x;
    for (int s = 0; s < 4; ++s) { w[s] = W[m * 16 + 4 * q + s]; x[s] = Z[(4 * q + s) * 16 + m]; }
    w16_u32x2 w1, w2, w3, y1, y2, y3;
    w16_split3k16_valu(w, w1, w2, w3);     // the weights' pieces come from the host: truncation
    w16_split3k16_valu(x, y1, y2, y3);
    const W16K16 z = w16_split3k16(x);     // the activation's split as the kernels do it: a = z3|z1, and z2
    const w16_u32x2 z3 = {z.a[0], z.a[1]}, z1 = {z.a[2], z.a[3]}, z2 = z.z2;
    f32x4 a6 = {0.f, 0.f, 0.f, 0.f};
    a6 = mm16(w1, z3, a6); a6 = mm16(w2, z2, a6); a6 = mm16(w3, z1, a6);
    a6 = mm16(w1, z2, a6); a6 = mm16(w2, z1, a6); a6 = mm16(w1, z1, a6);
    // (w16_mm_bfk16 takes two row blocks: this product has one, the second is a copy nobody reads)
    const u32x4 w12 = {w1[0], w1[1], w2[0], w2[1]}, w31 = {w3[0], w3[1], w1[0], w1[1]};      // the pack's two halves
    const u32x4 wk[2][2] = {{w12, w31}, {w12, w31}};
    f32x4 d3[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    w16_mm_bfk16(wk, z, d3);
    const f32x4 a3 = d3[0];
    f32x4 a32 = {0.f, 0.f, 0.f, 0.f};
    for (int k4 = 0; k4 < 4; ++k4)
        a32 = __builtin_amdgcn_mfma_f32_16x16x4f32(W[m * 16 + 4 * k4 + q], Z[(4 * k4 + q) * 16 + m], a32, 0, 0, 0);
    for (int r = 0; r < 4; ++r) {
        C6[t * 256 + (4 * q + r) * 16 + m] = a6[r];
        C3[t * 256 + (4 * q + r) * 16 + m] = a3[r];
        C32[t * 256 + (4 * q + r) * 16 + m] = a32[r];
    }
    const unsigned yy[6] = {y3[0], y3[1], y1[0], y1[1], y2[0], y2[1]};
    const unsigned zz[6] = {z.a[0], z.a[1], z.a[2], z.a[3], z.z2[0], z.z2[1]};
    for (int j = 0; j < 6; ++j) { zs[(t * 64 + lane) * 6 + j] = zz[j]; zp[(t * 64 + lane) * 6 + j] = yy[j]; }
}
static bool three_pieces(float v) {        // all three truncated bf16 pieces of v are non-zero
    for (int k = 0; k < 3; ++k) {
        unsigned b; memcpy(&b, &v, 4); b &= 0xffff0000u;
        float top; memcpy(&top, &b, 4);
        if (top == 0.f) return false;
        v -= top;
    }
    return true;
}
static void pieces3(float v, double (&p)[3]) {        // the truncated pieces of v
    for (int k = 0; k < 3; ++k) {
        unsigned b; memcpy(&b, &v, 4); b &= 0xffff0000u;
        float top; memcpy(&top, &b, 4);
        p[k] = top;
        v -= top;
    }
}
static int check_k16_pairs() {
    const int T = 64;
    std::vector<float> W(T * 256), Z(T * 256), C6(T * 256), C3(T * 256), C32(T * 256);
    srand(16);
    for (auto &v : W) do v = (rand() / (float)RAND_MAX - 0.5f) * 2.f; while (!three_pieces(v));
    for (auto &v : Z) do v = (rand() / (float)RAND_MAX - 0.25f) * 4.f; while (!three_pieces(v));
    float *dW, *dZ, *d6, *d3, *d32; unsigned *ds, *dp;
    const size_t nb = (size_t)T * 1024, np = (size_t)T * 64 * 6;
    hipMalloc(&dW, nb); hipMalloc(&dZ, nb); hipMalloc(&d6, nb); hipMalloc(&d3, nb); hipMalloc(&d32, nb);
    hipMalloc(&ds, np * 4); hipMalloc(&dp, np * 4);
    hipMemcpy(dW, W.data(), nb, hipMemcpyHostToDevice); hipMemcpy(dZ, Z.data(), nb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_check16, dim3(T), dim3(64), 0, 0, dW, dZ, d6, d3, d32, ds, dp);
    std::vector<unsigned> zs(np), zp(np);
    if (hipMemcpy(C6.data(), d6, nb, hipMemcpyDeviceToHost) != hipSuccess) { printf("K = 16 pairs: the kernel failed\n"); return 1; }
    hipMemcpy(C3.data(), d3, nb, hipMemcpyDeviceToHost); hipMemcpy(C32.data(), d32, nb, hipMemcpyDeviceToHost);
    hipMemcpy(zs.data(), ds, np * 4, hipMemcpyDeviceToHost); hipMemcpy(zp.data(), dp, np * 4, hipMemcpyDeviceToHost);
    double e6 = 0, e3 = 0, e32 = 0, scale = 0, s6 = 0, s3 = 0;
    long bits = 0, words = 0;
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double ref = 0, six = 0;       // six: the six partial products w_a z_b, a + b <= 4, summed in float64 (each is exact there)
                for (int k = 0; k < 16; ++k) {
                    ref += (double)W[t * 256 + i * 16 + k] * (double)Z[t * 256 + k * 16 + j];
                    double wp[3], zq[3];
                    pieces3(W[t * 256 + i * 16 + k], wp); pieces3(Z[t * 256 + k * 16 + j], zq);
                    six += wp[0] * zq[2] + wp[1] * zq[1] + wp[2] * zq[0] + wp[0] * zq[1] + wp[1] * zq[0] + wp[0] * zq[0];
                }
                const int o = t * 256 + i * 16 + j;
                s6 = fmax(s6, fabs(C6[o] - six)); s3 = fmax(s3, fabs(C3[o] - six));
                e6 = fmax(e6, fabs(C6[o] - ref)); e3 = fmax(e3, fabs(C3[o] - ref)); e32 = fmax(e32, fabs(C32[o] - ref)); scale = fmax(scale, fabs(ref));
                bits += memcmp(&C6[o], &C3[o], 4) != 0;
            }
    for (size_t i = 0; i < np; ++i) words += zs[i] != zp[i];
    printf("K = 16 pairs: max |C - float64|: paired (three K = 32 MFMAs) %.3e, six K = 16 MFMAs %.3e, f32 MFMA %.3e (largest |C| %.2f, %d outputs)\n", e3, e6, e32, scale, T * 256);
    printf("K = 16 pairs: max |C - the six partial products summed in float64|: paired %.3e, six K = 16 MFMAs %.3e\n", s3, s6);
    printf("K = 16 pairs: %ld of %d outputs differ in bits from the six-instruction form\n", bits, T * 256);
    printf("K = 16 pairs: %ld of %zu piece words differ from the v_and / v_sub form's\n", words, np);
    hipFree(dW); hipFree(dZ); hipFree(d6); hipFree(d3); hipFree(d32); hipFree(ds); hipFree(dp);
    return 0;
}
// the inputs of the default run, in the order it draws them: srand(1), the product's operands, then the split's 2^22 values
static void product_operands(std::vector<float> &W, std::vector<float> &Z) {
    srand(1);
    for (auto &v : W) v = (rand() / (float)RAND_MAX - 0.5f) * 2.f;
    for (auto &v : Z) v = (rand() / (float)RAND_MAX) * 3.f * ((rand() & 3) ? 1.f : 0.f);       // relu-like: a quarter zeros
}
// uniform, tiny, huge, negative, powers of two, bf16 numbers, zeros
static void split_values(std::vector<float> &xv) {
    for (size_t i = 0; i < xv.size(); ++i) {
        const int kind = i & 7;
        unsigned bits = ((unsigned)rand() << 16) ^ (unsigned)rand() ^ ((unsigned)rand() << 31);
        float f;
        if (kind < 3) { bits = (bits & 0x807fffffu) | ((unsigned)(100 + rand() % 56) << 23); memcpy(&f, &bits, 4); }       // 2^-27 .. 2^28
        else if (kind == 3) { bits = (bits & 0x807fffffu) | ((unsigned)(1 + rand() % 253) << 23); memcpy(&f, &bits, 4); }   // any normal exponent
        else if (kind == 4) { bits &= 0xffff0000u; bits = (bits & 0x807fffffu) | ((unsigned)(110 + rand() % 30) << 23); memcpy(&f, &bits, 4); }
        else if (kind == 5) { bits |= 0x00007fffu; bits = (bits & 0x807fffffu) | ((unsigned)(110 + rand() % 30) << 23); memcpy(&f, &bits, 4); }   // ties / all ones below
        else if (kind == 6) f = ldexpf(1.f, rand() % 60 - 30) * ((rand() & 1) ? -1.f : 1.f);
        else f = (rand() & 1) ? 0.f : (rand() / (float)RAND_MAX) * 3.f;
        xv[i] = f;
    }
}
// values of xv that the three pieces in pc ([lane][piece][4 dwords], 8 values per lane) do not add up to in float64
static long not_reproduced(const std::vector<unsigned> &pc, const std::vector<float> &xv, double &worst, bool show) {
    long bad = 0; int shown = 0;
    worst = 0;
    for (size_t t = 0; t < xv.size() / 8; ++t)
        for (int s = 0; s < 8; ++s) {
            double sum = 0;
            for (int k = 0; k < 3; ++k) {
                const unsigned w = pc[(t * 3 + k) * 4 + s / 2];
                const unsigned b = (s & 1) ? (w & 0xffff0000u) : (w << 16);
                float piece; memcpy(&piece, &b, 4);
                sum += (double)piece;
            }
            const double x = xv[t * 8 + s];
            if (sum != x) {
                ++bad; worst = fmax(worst, fabs(sum - x) / fabs(x));
                if (show && shown++ < 4) printf("   x = %.9g (%a): pieces add up to %.9g\n", x, x, sum);
            }
        }
    return bad;
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
// ./bf16x6 rem4x4: the split's remainders on the 4x4x4 bf16 MFMA (tests/test_gpu_rem4x4.py reads the first two parts)
static int check_rem4x4() {
    int fails = 0;
    {   // 1. exactness, on the default run's 2^22 values
        const int nv = 1 << 22;
        std::vector<float> W(16 * 32), Z(32 * 16), xv(nv);
        product_operands(W, Z);
        split_values(xv);
        float *dx; unsigned *dp;
        hipMalloc(&dx, (size_t)nv * 4); hipMalloc(&dp, (size_t)nv / 8 * 12 * 4);
        hipMemcpy(dx, xv.data(), (size_t)nv * 4, hipMemcpyHostToDevice);
        std::vector<unsigned> pc0((size_t)nv / 8 * 12), pc4(pc0.size());
        hipLaunchKernelGGL(k_exact<0>, dim3(nv / 512), dim3(64), 0, 0, dx, dp);
        if (hipMemcpy(pc0.data(), dp, pc0.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("rem4x4: a kernel failed\n"); return 1; }
        hipLaunchKernelGGL(k_exact<4>, dim3(nv / 512), dim3(64), 0, 0, dx, dp);
        if (hipMemcpy(pc4.data(), dp, pc4.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("rem4x4: a kernel failed\n"); return 1; }
        long diff = 0;
        for (size_t i = 0; i < pc0.size(); ++i) diff += pc4[i] != pc0[i];
        double w0, w4;
        const long bad0 = not_reproduced(pc0, xv, w0, false), bad4 = not_reproduced(pc4, xv, w4, false);
        printf("rem4x4 exactness: %ld of %zu piece words differ from the v_and / v_sub form's\n", diff, pc0.size());
        printf("rem4x4 exactness: %ld of %d values not reproduced by x1 + x2 + x3 (4x4x4 remainders), %ld (truncated form)\n", bad4, nv, bad0);
        fails += diff != 0 || bad4 != bad0;
        hipFree(dx); hipFree(dp);
    }
    {   // 2. layout: one lane of the wavefront holds values, the others zeros
        float *dx, *dy;
        hipMalloc(&dx, 1024); hipMalloc(&dy, 1024);
        const int lanes[6] = {0, 5, 18, 27, 46, 63};
        const float vals[4] = {1.2345678f, -0.0078112348f, 517.00391f, 3.0000002f};      // four different values, pieces in all three places
        for (int k = 0; k < 6; ++k) {
            const int L = lanes[k];
            std::vector<float> x(256, 0.f), y(256, -1.f);
            for (int r = 0; r < 4; ++r) x[L * 4 + r] = vals[r] * (1.f + 0.125f * k);
            hipMemcpy(dx, x.data(), 1024, hipMemcpyHostToDevice);
            hipLaunchKernelGGL(k_probe4, dim3(1), dim3(64), 0, 0, dx, dy);
            if (hipMemcpy(y.data(), dy, 1024, hipMemcpyDeviceToHost) != hipSuccess) { printf("rem4x4: a kernel failed\n"); return 1; }
            int others = 0, own = 0;
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    float want = x[l * 4 + r];
                    if (l == L) { unsigned b; memcpy(&b, &want, 4); b &= 0xffff0000u; float top; memcpy(&top, &b, 4); want -= top; }
                    const bool bad = memcmp(&y[l * 4 + r], &want, 4) != 0;
                    if (l == L) own += bad; else others += bad;
                }
            printf("rem4x4 layout: values in lane %2d (block %2d, column %d) only: %d of its 4 results are not x[r] - piece[r], %d of the other 252 results changed: %s\n",
                   L, L / 4, L % 4, own, others, own || others ? "FAILED" : "ok");
            fails += own || others;
        }
        hipFree(dx); hipFree(dy);
    }
    {   // 3. cost, by the wavefronts' own clocks: 16 workgroups (a CU each) of one or two wavefronts per SIMD
        const int groups = 16;
        float *src, *dst; unsigned long long *cyc;
        hipMalloc(&src, 1536 * 4); hipMalloc(&dst, (size_t)groups * 512 * 8 * 4); hipMalloc(&cyc, (size_t)groups * 8 * 16);
        std::vector<float> s(1536);
        for (auto &v : s) v = rand() / (float)RAND_MAX - 0.3f;
        hipMemcpy(src, s.data(), 1536 * 4, hipMemcpyHostToDevice);
        std::vector<unsigned long long> h((size_t)groups * 8 * 2);
        auto clocks = [&](int waves, double per, double &ticks, double &ghz) {       // median over wavefronts of ticks / per
            if (hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
            std::vector<double> t, g;
            for (int w = 0; w < waves; ++w) { t.push_back((double)h[2 * w] / per); g.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 0.1); }
            ticks = median(t); ghz = median(g);
            return true;
        };
        const char *kinds[3] = {"v_mfma 4x4x4 (16b bf16)  ", "v_mfma_f32_16x16x16_bf16 ", "v_mfma 16x16x32 (bf16)   "};
        const int n = 4000;
        for (int kind = 0; kind < 3; ++kind) {
            double t[2], g[2];
            for (int indep = 1; indep >= 0; --indep) {
                for (int rep = 0; rep < 2; ++rep) {          // (the second launch counts)
                    if (kind == 0 && indep) hipLaunchKernelGGL((k_rate<0, 1>), dim3(groups), dim3(256), 0, 0, src, dst, n, cyc);
                    else if (kind == 0) hipLaunchKernelGGL((k_rate<0, 0>), dim3(groups), dim3(256), 0, 0, src, dst, n, cyc);
                    else if (kind == 1 && indep) hipLaunchKernelGGL((k_rate<1, 1>), dim3(groups), dim3(256), 0, 0, src, dst, n, cyc);
                    else if (kind == 1) hipLaunchKernelGGL((k_rate<1, 0>), dim3(groups), dim3(256), 0, 0, src, dst, n, cyc);
                    else if (indep) hipLaunchKernelGGL((k_rate<2, 1>), dim3(groups), dim3(256), 0, 0, src, dst, n, cyc);
                    else hipLaunchKernelGGL((k_rate<2, 0>), dim3(groups), dim3(256), 0, 0, src, dst, n, cyc);
                    if (!clocks(groups * 4, n * 32.0, t[indep], g[indep])) { printf("rem4x4: a kernel failed\n"); return 1; }
                }
            }
            printf("rem4x4 cost: %s back to back, one wavefront per SIMD: %.2f cycles per instruction on eight accumulators in turn, %.2f on one accumulator (clock %.3f GHz)\n",
                   kinds[kind], t[1], t[0], g[1]);
        }
        const char *splits[3] = {"v_and / v_sub            ", "v_mfma_f32_16x16x16_bf16 ", "v_mfma 4x4x4 (16b bf16)  "};
        const int tiles = 4000;
        for (int sp = 0; sp < 3; ++sp) {
            double t[2], g[2];
            for (int two = 0; two < 2; ++two)
                for (int rep = 0; rep < 2; ++rep) {
                    const dim3 wg(two ? 512 : 256);
                    if (sp == 0) hipLaunchKernelGGL(k_time_wg<0>, dim3(groups), wg, 0, 0, src, dst, tiles, cyc);
                    else if (sp == 1) hipLaunchKernelGGL(k_time_wg<3>, dim3(groups), wg, 0, 0, src, dst, tiles, cyc);
                    else hipLaunchKernelGGL(k_time_wg<4>, dim3(groups), wg, 0, 0, src, dst, tiles, cyc);
                    if (!clocks(groups * (two ? 8 : 4), tiles, t[two], g[two])) { printf("rem4x4: a kernel failed\n"); return 1; }
                }
            printf("rem4x4 cost: tile (split + 12 MFMAs), remainders by %s: %.1f cycles per tile with one wavefront per SIMD, %.1f per tile and wavefront pair with two (%.1f per wavefront; clock %.3f GHz)\n",
                   splits[sp], t[0], t[1], t[1] / 2, g[1]);
        }
        hipFree(src); hipFree(dst); hipFree(cyc);
    }
    return fails ? 1 : 0;
}
// The pair sweep's tile (split with the 4x4x4 remainders + 12 MFMAs + its element-wise work) with the first ReLU as v_max_f32 and as
// the add's output clamp: the wavefronts' own clocks at one and two wavefronts per SIMD, and the two forms' results compared in bits.
static int check_clamp() {
    const int groups = 16, tiles = 4000;
    float *src, *dst; unsigned long long *cyc;
    hipMalloc(&src, 1536 * 4); hipMalloc(&dst, (size_t)groups * 512 * 8 * 4); hipMalloc(&cyc, (size_t)groups * 8 * 16);
    std::vector<float> s(1536);
    srand(1);
    for (auto &v : s) v = rand() / (float)RAND_MAX - 0.3f;
    hipMemcpy(src, s.data(), 1536 * 4, hipMemcpyHostToDevice);
    std::vector<unsigned long long> h((size_t)groups * 8 * 2);
    std::vector<unsigned> out[2];
    double t[2][2], ghz = 0;
    for (int form = 0; form < 2; ++form)
        for (int two = 0; two < 2; ++two)
            for (int rep = 0; rep < 2; ++rep) {          // (the second launch counts)
                const dim3 wg(two ? 512 : 256);
                if (form == 0) hipLaunchKernelGGL((k_time_wg<4, 1>), dim3(groups), wg, 0, 0, src, dst, tiles, cyc);
                else hipLaunchKernelGGL((k_time_wg<4, 2>), dim3(groups), wg, 0, 0, src, dst, tiles, cyc);
                if (hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("clamp: a kernel failed\n"); return 1; }
                std::vector<double> tk, g;
                for (int w = 0; w < groups * (two ? 8 : 4); ++w) { tk.push_back((double)h[2 * w] / tiles); g.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 0.1); }
                t[form][two] = median(tk); ghz = median(g);
                if (two) { out[form].resize((size_t)groups * 512 * 8); hipMemcpy(out[form].data(), dst, out[form].size() * 4, hipMemcpyDeviceToHost); }
            }
    long diff = 0;
    for (size_t i = 0; i < out[0].size(); ++i) diff += out[0][i] != out[1][i];
    const char *forms[2] = {"v_add_f32 + v_max_f32 ", "v_add_f32 ... clamp    "};
    for (int form = 0; form < 2; ++form)
        printf("clamp: sweep tile, first ReLU as %s: %.1f cycles per tile with one wavefront per SIMD, %.1f per tile and wavefront pair with two (%.1f per wavefront; clock %.3f GHz)\n",
               forms[form], t[form][0], t[form][1], t[form][1] / 2, ghz);
    printf("clamp: %ld of %zu results differ in bits between the two forms\n", diff, out[0].size());
    hipFree(src); hipFree(dst); hipFree(cyc);
    return diff ? 1 : 0;
}
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "clamp")) return check_clamp();             // only the sweep tile's two ReLU forms (profiles/r23_relu_clamp.txt)
    if (argc > 1 && !strcmp(argv[1], "k16pairs")) return check_k16_pairs();      // only the K = 16 pairing (tests/test_gpu_k16_pairs.py)
    if (argc > 1 && !strcmp(argv[1], "rem4x4")) return check_rem4x4();           // only the 4x4x4 remainders (tests/test_gpu_rem4x4.py)
    std::vector<float> W(16 * 32), Z(32 * 16), C6(256), C32(256);
    product_operands(W, Z);
    float *dW, *dZ, *d6, *d32;
    hipMalloc(&dW, 2048); hipMalloc(&dZ, 2048); hipMalloc(&d6, 1024); hipMalloc(&d32, 1024);
    hipMemcpy(dW, W.data(), 2048, hipMemcpyHostToDevice); hipMemcpy(dZ, Z.data(), 2048, hipMemcpyHostToDevice);
    for (int sp = 0; sp < 3; ++sp) {
        if (sp == 2) hipLaunchKernelGGL(k_check<2>, dim3(1), dim3(64), 0, 0, dW, dZ, d6, d32);
        else if (sp) hipLaunchKernelGGL(k_check<1>, dim3(1), dim3(64), 0, 0, dW, dZ, d6, d32);
        else hipLaunchKernelGGL(k_check<0>, dim3(1), dim3(64), 0, 0, dW, dZ, d6, d32);
        hipMemcpy(C6.data(), d6, 1024, hipMemcpyDeviceToHost); hipMemcpy(C32.data(), d32, 1024, hipMemcpyDeviceToHost);
        double e6 = 0, e32 = 0, scale = 0;
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) {
                double ref = 0;
                for (int k = 0; k < 32; ++k) ref += (double)W[i * 32 + k] * (double)Z[k * 16 + j];
                e6 = fmax(e6, fabs(C6[i * 16 + j] - ref)); e32 = fmax(e32, fabs(C32[i * 16 + j] - ref)); scale = fmax(scale, fabs(ref));
            }
        printf("max |C - float64|: bf16x6 (%s pieces) %.3e, f32 MFMA %.3e (largest |C| %.2f)\n", sp == 2 ? "truncated, remainders by MFMA" : sp ? "nearest, dot2c" : "truncated", e6, e32, scale);
    }
    {   // exactness of both splits on 2^22 values: uniform, tiny, huge, negative, powers of two, bf16 numbers, zeros
        const int nv = 1 << 22;
        std::vector<float> xv(nv);
        split_values(xv);
        float *dx; unsigned *dp;
        hipMalloc(&dx, (size_t)nv * 4); hipMalloc(&dp, (size_t)nv / 8 * 12 * 4);
        hipMemcpy(dx, xv.data(), (size_t)nv * 4, hipMemcpyHostToDevice);
        std::vector<unsigned> pc((size_t)nv / 8 * 12), pc0;
        for (int sp = 0; sp < 4; ++sp) {
            if (sp == 3) hipLaunchKernelGGL(k_exact<3>, dim3(nv / 512), dim3(64), 0, 0, dx, dp);
            else if (sp == 2) hipLaunchKernelGGL(k_exact<2>, dim3(nv / 512), dim3(64), 0, 0, dx, dp);
            else if (sp) hipLaunchKernelGGL(k_exact<1>, dim3(nv / 512), dim3(64), 0, 0, dx, dp);
            else hipLaunchKernelGGL(k_exact<0>, dim3(nv / 512), dim3(64), 0, 0, dx, dp);
            hipMemcpy(pc.data(), dp, pc.size() * 4, hipMemcpyDeviceToHost);
            double worst;
            const long bad = not_reproduced(pc, xv, worst, true);
            if (sp == 0) pc0 = pc;
            if (sp >= 2) {
                long diff = 0;
                for (size_t i = 0; i < pc.size(); ++i) diff += pc[i] != pc0[i];
                printf("truncated / MFMA remainders (K = %d): %ld of %zu piece words differ from the v_and / v_sub form's\n", sp == 2 ? 32 : 16, diff, pc.size());
            }
            printf("%s pieces: %ld of %d values not reproduced exactly by x1 + x2 + x3 (worst relative %.3g)\n", sp == 3 ? "truncated / MFMA remainders, K = 16" : sp == 2 ? "truncated / MFMA remainders" : sp ? "nearest / dot2c" : "truncated", bad, nv, worst);
        }
    }
    check_k16_pairs();
    const int blocks = 2048, tiles = 4000;
    float *src, *dst;
    hipMalloc(&src, 1536 * 4); hipMalloc(&dst, (size_t)blocks * 512 * 4);
    std::vector<float> s(1536);
    for (auto &v : s) v = rand() / (float)RAND_MAX - 0.3f;
    hipMemcpy(src, s.data(), 1536 * 4, hipMemcpyHostToDevice);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const char *names[10] = {"f32 MFMA     ", "bf16x6 + split", "  + 8 v_pk_add_f32 (16 adds)", "  + 16 v_add_f32", "  + 16 v_max_f32", "  + 8 v_and_b32 + 8 v_perm_b32", "bf16x6 + split by v_cvt_pk_bf16_f32 / v_dot2c_f32_bf16", "bf16x6 + split with the remainders by MFMA (16 per tile)", "bf16x6 + split with the remainders by v_mfma_f32_16x16x16_bf16", ""};
    for (int mode = 0; mode < 9; ++mode) {
#ifndef BF16X6_PK_ADD
        if (mode == 2) { printf("%s: not built (packed f32 instructions are off in the library's flags: see the head of this file)\n", names[mode]); continue; }
#endif
        for (int rep = 0; rep < 2; ++rep) {
            hipEventRecord(e0);
            if (mode == 0) hipLaunchKernelGGL(k_time<0>, dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 1) hipLaunchKernelGGL(k_time<1>, dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 2) hipLaunchKernelGGL((k_time<1, 1>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 3) hipLaunchKernelGGL((k_time<1, 2>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 4) hipLaunchKernelGGL((k_time<1, 3>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 5) hipLaunchKernelGGL((k_time<1, 4>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 6) hipLaunchKernelGGL((k_time<1, 0, 1>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else if (mode == 7) hipLaunchKernelGGL((k_time<1, 0, 2>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            else hipLaunchKernelGGL((k_time<1, 0, 3>), dim3(blocks), dim3(64), 0, 0, src, dst, tiles);
            hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            // 2048 wavefronts = 2 per SIMD: cycles per tile and SIMD = ms * clock / (tiles * 2)
            if (rep) printf("%s: %.3f ms, %.0f cycles per tile and wavefront pair at 2.4 GHz (%.0f per wavefront)\n", names[mode], ms, ms * 1e-3 * 2.4e9 / tiles, ms * 1e-3 * 2.4e9 / tiles / 2);
        }
    }
    return 0;
}
