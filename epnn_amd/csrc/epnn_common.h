// Shared definitions of the EPNN HIP library (gfx950 / MI355X only).
//
// Arithmetic model (exact re-association of reference charge_gn.py:56-119):
//   first Dense of every pair MLP is split by input block  W1^T[a_i|a_j|e_ij] = Wi^T a_i + Wj^T a_j + We^T e_ij,
//   so   P_i = Wi^T a_i + b1,  R_j = Wj^T a_j  (per atom)   and   G_ij = We^T e_ij  (per near pair only),
//   z1_ij = relu(P_i + R_j + G_ij),  z2_ij = relu(W2^T z1_ij + b2).
//   GNN:  sum_j m_ij = W3^T (sum_j z2_ij) + N b3 ;  EPN:  f_ij = w3 . z2_ij (+ b3, cancels in f_ij - f_ji).
//
// MFMA: v_mfma_f32_32x32x2_f32 (exact f32 fma chain).  Lane l = 32*hh + c.  Accumulator register r of lane
// (c,hh) is element (row kappa(hh,r), col c) with kappa(hh,r) = 4*hh + (r&3) + 8*(r>>2).  All 32-wide feature
// vectors that feed an MFMA as the K dimension are kept "kappa-permuted": element r of half hh is feature
// kappa(hh,r), so that an accumulator can be fed straight back as the next A/B operand (no LDS round trip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define EPNN_HID 32          // hidden width of every MLP
#define EPNN_EDIM 48         // edge channels == h_dim
#define EPNN_KA 30           // K-steps of the per-atom projection: features f = 2*s + hh, f < 60
#define EPNN_F1 59           // atom-feature slot holding the constant 1: the first Dense's bias b1 rides in Wi row 59
#define EPNN_AST 68          // LDS/HBM row stride (floats) of the even/odd atom-feature image a_eo
#define EPNN_PST 36          // LDS row stride (floats) of kappa-permuted 32-vectors (P, R, G)
#define EPNN_SST 33          // LDS row stride (floats) of out-major 32-vectors (S partial sums)
#define EPNN_MAXT 8
#define EPNN_SMALL_NMAX 32   // fused kernel handles molecules with n <= 32 real atoms

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// Offsets (in floats) into the packed weight buffer.
struct PairMlpPack {      // one message_fns[t] / pass_fns[t]
    int wiF;              // [KA][64]  Wi[2s+hh][c]      (A operand of P^T = Wi^T a^T)
    int wjF;              // [KA][64]  Wj[2s+hh][c]
    int b1p;              // [2][16]   b1[kappa(hh,r)]
    int weF;              // [24][64]  We[24hh+s][c]     (A operand of G^T = We^T e^T)
    int w2F;              // [16][64]  W2[kappa(hh,s)][c]
    int b2;               // [32]      b2[c]
    int b2p;              // [2][16]   b2[kappa(hh,r)]
    int w3p;              // [2][16]   w3[kappa(hh,r)]   (pass MLP only)
    int wqi, wqj;         // [2][16]   the q rows of Wi / Wj, kappa-permuted: P(q) = P(q = 0) + q wqi (tiled EPN stack: only q changes between steps)
};
struct UpdPack {          // update_fn with message_fns[t]'s last Dense folded in
    int u1F;              // [40][64]  s<24: Wu1[h feature][c]; s>=24: (W3_t Wu1_M)[2(s-24)+hh][c]
    int cb3p;             // [2][16]   (Wu1_M^T b3_t)[kappa(hh,r)]   (times N at run time)
    int bu1p;             // [2][16]
    int u2F;              // [16][64]  Wu2[kappa(hh,s)][c]
    int bu2p;             // [2][16]
    int u3F;              // [2][16][64] Wu3[kappa(hh,s)][32*tile+c]
    int bu3p;             // [2][2][16]
};
struct WeightIndex {
    PairMlpPack msg[EPNN_MAXT];
    PairMlpPack pas[EPNN_MAXT];
    UpdPack upd[EPNN_MAXT];
};

// ---- wave-autonomous fused kernel (epnn_wave.hip.h).  v_mfma_f32_16x16x4_f32: lane l = 16*q + m.
// A operand lane (q,m) = A[m][k=q], B operand lane (q,n) = B[k=q][n], accumulator register r of lane (q,n) =
// D[4q + r][n].  A 32-feature x 32-column product is 2 row blocks (rb) x 2 column blocks (cb) of such tiles; lane
// (q,n) then owns columns n and 16+n and, of each, the 8 features 16rb + 4q + r.  K steps are ordered so that an
// accumulator set feeds the next product directly: step s = 4rb' + r' pairs lane q with input feature
// 16rb' + 4q + r' ("acc" order).  Other K orders: "xq" feature 4s + q;  "e" channel 12q + s.
// Fragment = [rb][step / 4][64 lanes][4]: lane (q,m) holds W[in(step,q)][16rb + m], its four consecutive steps in 16 contiguous
// bytes (one global_load_dwordx4, W16_LDX).  Vectors are in natural feature order.
#define EPNN_XS 4            // K-steps of the xq block: nx + 3 <= 16
#define EPNN_ER 16           // dimension of the edge-feature subspace used by the fused kernel's own front-end
#define EPNN_ETAB_N 2049     // grid points of the table of B^T e(D) over [0, cutoff]
#define EPNN_NFLIP_MAX 128   // changes of the near flag as a function of the distance beyond dsafe that the fused front-end can hold
#define EPNN_DST 33          // LDS row stride (floats) of the per-molecule charge-transfer matrix
// (HU = units of the update MLP's hidden layers as the fused kernel sees them: 32, or 64 for k_wave_forward<.., NRU = 4>; the
//  shapes below are written for 32 -- with 64, "[2][8]" of u2 / pu1 reads [4][16], of u1s [4][8], of pwi / pwj [2][16+XS], of u3
//  [3][16], the [32] vectors of the update MLP [64]: pack_weights, epnn_api_weights.hip.h)
struct WaveGnnPack {           // GNN step t
    int we;               // [2][12][64]  e order       We_t
    int we16;             // [2][4][64]   k = 4q + s    B^T We_t   (edge features in the 16-dimensional basis)
    int we16b;            // [2][2][64][4] dwords       the same as three bf16 pieces per weight, a lane's row block = w1 w2 | w3 w1 (w16_mm_bfk16: K slot s of lane q = coefficient 4q + s)
    int w2;               // [2][8][64]   acc order     W2_t
    int w2b;              // [2][3][64][4] dwords       W2_t as three bf16 pieces per weight (w16_split3 / pack_bf16x3), K slot s of lane q = acc order
    int b2;               // [32]
    int u1s;              // [2][8][64]   acc order     W3_t Wu1_M
    int cb3, bu1;         // [32]         Wu1_M^T b3_t (times N at run time), bu1
    int u2;               // [2][8][64]   acc order     Wu2
    int bu2;              // [32]
    int pwi, pwj;         // [2][8+XS][64]  acc rows: Wu3 M_h;  xq rows: [M_h^T bu3, M_x, M_q, b1]   (M = Wi / Wj of step t+1)
    int pu1;              // [2][8][64]   acc order     Wu3 Wu1_H
    int cu3;              // [32]         Wu1_H^T bu3
    // the same kernels as three bf16 pieces per weight (32-unit update MLPs only): the per-atom chains on the bf16 matrix pipe.
    // `..hb` = the K = 32 block that multiplies nm u2 (acc order), [2][3][64][4] dwords each (w2b's layout); `..xb` = the xq block,
    // a K = 16 operand in the slot order of wave_xq_slot, [2][2][64][4] dwords each (we16b's layout: w1 w2 | w3 w1, w16_mm_bfk16)
    int u1sb, u2b, pu1b, pwihb, pwixb, pwjhb, pwjxb;
};
// K slot (lane group q, slot s of the lane: K index 4q + s of v_mfma_f32_16x16x16_bf16) of the xq block's operand -> index into xq
// (0 node mask, 1..nx x, nx + 1 q, nx + 2 one), -1 = empty.  Lane group 0: mask, one, charge, x[0]; lane group q >= 1:
// x[4q - 3 .. 4q]: nx + 3 <= 16 values fill the 16 slots exactly at nx = 13.  (Every value is a float32 -- x is whatever the
// caller's feature columns hold -- and is split into three pieces like any other operand.)
__host__ __device__ static inline int wave_xq_slot(int q, int s, int nx) {
    const int k = 4 * q + s;
    if (k < 3) return k == 0 ? 0 : (k == 1 ? nx + 2 : nx + 1);
    return k - 3 < nx ? k - 2 : -1;
}
struct WaveEpnPack {           // EPN step t
    int we, w2, b2, w3;   // w3: [32]
    int w2b;              // [2][3][64][4] dwords: W2_t as three bf16 pieces per weight (see WaveGnnPack)
    int we16;             // [2][4][64]   B^T We_t
    int we16b;            // [2][2][64][4] dwords: B^T We_t as three bf16 pieces per weight (see WaveGnnPack)
    int wi, wj;           // [2][XS+12][64]  xq rows, then h rows (acc order over 48 features): h given by the caller
    int wif, wjf;         // [2][8+XS][64]   acc rows: Wu3 M_h;  xq rows: [M_h^T bu3, M_x, M_q, b1]: h = nm (Wu3^T u2 + bu3) of the GNN stack
    int wifhb, wifxb, wjfhb, wjfxb;      // wif / wjf as bf16 pieces (see WaveGnnPack: ..hb K = 32, ..xb K = 16)
};
struct WaveIndex {
    WaveGnnPack g[EPNN_MAXT];
    WaveEpnPack e[EPNN_MAXT];
    int wi0, wj0;         // [2][XS+12][64]  first GNN step (h given by the caller, usually zeros)
    int wi0xb, wj0xb;     // [2][2][64][4] dwords: the xq rows of wi0 / wj0 as bf16 pieces (see WaveGnnPack's ..xb; 32-unit update MLPs only)
    int u1h0;             // [2][12][64]     acc order over 48 features  Wu1_H
    int u3;               // [3][8][64]      acc order  Wu3 (48 outputs = 3 row blocks)
    int bu3;              // [48]
    // The SCALED copy of this index (epnn_handle::wvidx_c, k_wave_forward's CLAMP form) only: |P'|, |R'| of a step may reach this
    // before the wavefront leaves the clamp form for that step; the host has bounded |G'| by 1 - 2 relu_lim (pack_weights)
    float relu_lim;
};
// s = 2^-EPNN_RELU_SHIFT scales the operands of the pair MLPs in k_wave_forward's CLAMP form (pack_weights says what the choice leaves
// on either side of float32's range)
#define EPNN_RELU_SHIFT 32

// A Dense stack of any widths (MLP_layer with other `nodes` than [32, 32], charge_gn.py:30-45): rows x dims[0] -> relu dims[1] ->
// ... -> dims[n] (the last Dense linear).  Kernels in Keras layout [in][out].  Used by epnn_mlp_forward_layers and by the update
// stage of the tiled path when make_model was given other `layers` (epnn_set_update_layers); plain f32 FMA loops, not the hot path.
#define EPNN_GMLP_ROWS 16     // rows per workgroup
#define EPNN_GMLP_WMAX 256    // widest layer
#define EPNN_GMLP_LMAX 8      // Dense layers
enum { EPNN_ACT_RELU = 0, EPNN_ACT_LINEAR = 1, EPNN_ACT_TANH = 2, EPNN_ACT_SIGMOID = 3 };     // (include/epnn.h: epnn_mlp_forward_layers)
struct GenMlp {
    int n;
    int act;                                             // activation of every layer but the last (EPNN_ACT_*; 0 = ReLU)
    int dims[EPNN_GMLP_LMAX + 1];
    int offW[EPNN_GMLP_LMAX], offB[EPNN_GMLP_LMAX];     // floats from `w`
    const float *w;
};

__host__ __device__ static inline int epnn_kappa(int hh, int r) { return 4 * hh + (r & 3) + 8 * (r >> 2); }

// position of atom feature f inside the even/odd image row: half (f&1), slot f>>1
__host__ __device__ static inline int epnn_aeo(int f) { return (f & 1) * 32 + (f >> 1); }

// status bits written by kernels
#define EPNN_ST_PAIR_OVERFLOW 1   // near-pair list capacity exceeded
#define EPNN_ST_TYPE_OVERFLOW 2   // tiled path, first GNN step by atom types: a molecule has more distinct feature rows than the table holds
#define EPNN_ST_RELU_RANGE 4      // fused kernel, clamp form: a wavefront ran a step in the max form (its scaled rows left the clamp's range); nothing to redo
#define EPNN_TYPE_MAX 64          // distinct atom-feature rows per molecule the first GNN step groups by (more: the all-pairs sweep runs)

#if defined(__HIPCC__)
__device__ __forceinline__ f32x16 epnn_mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 epnn_splat16(float v) {
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = v;
    return o;
}
// 16 contiguous floats (16-byte aligned) -> registers
__device__ __forceinline__ void epnn_ld16(const float *p, float (&o)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(p + 4 * q);
        o[4 * q + 0] = v[0]; o[4 * q + 1] = v[1]; o[4 * q + 2] = v[2]; o[4 * q + 3] = v[3];
    }
}
__device__ __forceinline__ void epnn_st16(float *p, const f32x16 &v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 o;
        o[0] = v[4 * q + 0]; o[1] = v[4 * q + 1]; o[2] = v[4 * q + 2]; o[3] = v[4 * q + 3];
        *reinterpret_cast<f32x4 *>(p + 4 * q) = o;
    }
}
// value held by the other half-wave's lane with the same c (lane ^ 32)
__device__ __forceinline__ float epnn_swap32(float v) {
    return __shfl_xor(v, 32, 64);
}

// ======== the 16x16 matrix-pipe primitives of the fused and tiled kernels (epnn_wave.hip.h, epnn_wave2.hip.h, epnn_large.hip.h).
// They live here, and not beside the kernels, so that the device check of this arithmetic (tools/micro/bf16x6.hip) compiles
// these very definitions under the library's flags.  The load macros refer to the kernels' `wp` (packed weights) and `lane`.
__device__ __forceinline__ f32x4 w16_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 w16_splat(float v) { return f32x4{v, v, v, v}; }
// ---- f32-grade products on the bf16 matrix pipe.  x = x1 + x2 + x3 EXACTLY, each piece the upper 16 bits of what is left (8 + 8 + 8
// mantissa bits: truncation, so the remainders are exact and the third piece fits a bf16); of the nine partial products of two such
// operands the six largest are summed in f32 -- what is left out is below 2^-24 of the product, the f32 MFMA's own rounding.  One
// v_mfma_f32_16x16x32_bf16 takes a whole K = 32 in 16 cycles: six of them 96 cycles against 8 x 32 of v_mfma_f32_16x16x4_f32
// (tools/micro/bf16x6.hip: layout, accuracy against float64 -- 1.3e-6 against the f32 MFMA's 2.4e-6 on |C| ~ 13 -- and timing).
// Operand layout: lane 16 q + m holds row / column m and the K slots 8 q .. 8 q + 7 as four dwords of bf16 pairs (even slot low).
typedef __bf16 w16_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 w16_mfma_bf(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(w16_bf16x8, a), __builtin_bit_cast(w16_bf16x8, b), c, 0, 0, 0);
}
// The remainders of a split on the MATRIX pipe (tools/micro/bf16x6.hip: exact, the pipe adds C unrounded).
// v_mfma_f32_4x4x4_16b_bf16 is sixteen independent 4x4x4 products: lane 4 b + i holds row i of block b's A, column i of its B (the
// four K slots as two dwords of bf16 pairs, even slot low) and column i of its C / D (rows 0..3 in four registers).  With A = -I in
// every block (lane 4 b + i: -1 in K slot i), a lane's four values as its accumulator and their packed upper halves as its B
// operand, D[r] = C[r] - B[r] is "x - piece" in place and INSIDE the lane: nothing has to agree between the accumulator's layout
// and the B operand's, whatever rows and columns the four values stand for.  2 MFMAs per 8 values and level instead of 8 v_and +
// 8 v_sub -- 12 vector instructions per split instead of 44, the SAME pieces bit for bit (round 5: bench 321 -> 327 M atoms/s;
// protein 0.382 -> 0.372 ms with the tiled sweep's own arrangement, epnn_large.hip.h).  The operand is two registers (four values
// are two dwords of the packed piece), the same -I for every use.  (Until round 21 this was v_mfma_f32_16x16x16_bf16 with A = -I
// over the whole 16x16 tile, which holds the pipe as long as a 16x16x32: what the 4x4x4 form costs beside it is measured in
// profiles/r21_rem4x4.txt; the K = 16 form lives on in the micro tool, as the thing compared against.)
typedef short w16_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned w16_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ w16_u32x2 w16_ident() {
    const int i = threadIdx.x & 3;
    w16_u32x2 I;
#pragma unroll
    for (int d = 0; d < 2; ++d) I[d] = (d == (i >> 1)) ? (0xbf80u << (16 * (i & 1))) : 0u;
    return I;
}
// x - piece for four values of a lane: p_lo | p_hi = the two dwords of the packed piece that hold them
__device__ __forceinline__ f32x4 w16_rem(w16_u32x2 I, unsigned p_lo, unsigned p_hi, f32x4 x) {
    return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(w16_s16x4, I), __builtin_bit_cast(w16_s16x4, w16_u32x2{p_lo, p_hi}), x, 0, 0, 0);
}
__device__ __forceinline__ u32x4 w16_pack_hi(const f32x4 &lo, const f32x4 &hi) {      // v_perm_b32: the upper halves of two floats side by side
    u32x4 p;
    p[0] = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
    p[1] = __builtin_amdgcn_perm(__float_as_uint(lo[3]), __float_as_uint(lo[2]), 0x07060302u);
    p[2] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
    p[3] = __builtin_amdgcn_perm(__float_as_uint(hi[3]), __float_as_uint(hi[2]), 0x07060302u);
    return p;
}
__device__ __forceinline__ w16_u32x2 w16_pack_hi2(const f32x4 &v) {                    // the same for four values
    w16_u32x2 p;
    p[0] = __builtin_amdgcn_perm(__float_as_uint(v[1]), __float_as_uint(v[0]), 0x07060302u);
    p[1] = __builtin_amdgcn_perm(__float_as_uint(v[3]), __float_as_uint(v[2]), 0x07060302u);
    return p;
}
// The same pieces with the remainders as v_and_b32 + v_sub_f32, 44 vector instructions per split of eight values: what the
// matrix-pipe form is checked against on the device (tools/micro/bf16x6.hip), and the split of -DEPNN_SPLIT_VALU comparison builds.
__device__ __forceinline__ void w16_split3_valu(const float (&v)[8], u32x4 &p1, u32x4 &p2, u32x4 &p3) {
    float r1[8], r2[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        r1[s] = v[s] - __uint_as_float(__float_as_uint(v[s]) & 0xffff0000u);
        r2[s] = r1[s] - __uint_as_float(__float_as_uint(r1[s]) & 0xffff0000u);
    }
    const f32x4 a0 = {v[0], v[1], v[2], v[3]}, a1 = {v[4], v[5], v[6], v[7]};
    const f32x4 b0 = {r1[0], r1[1], r1[2], r1[3]}, b1 = {r1[4], r1[5], r1[6], r1[7]};
    const f32x4 c0 = {r2[0], r2[1], r2[2], r2[3]}, c1 = {r2[4], r2[5], r2[6], r2[7]};
    p1 = w16_pack_hi(a0, a1);
    p2 = w16_pack_hi(b0, b1);
    p3 = w16_pack_hi(c0, c1);
}
// (four values: the K = 16 operands)
__device__ __forceinline__ void w16_split3k16_valu(f32x4 x, w16_u32x2 &p1, w16_u32x2 &p2, w16_u32x2 &p3) {
    f32x4 r1, r2;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        r1[s] = x[s] - __uint_as_float(__float_as_uint(x[s]) & 0xffff0000u);
        r2[s] = r1[s] - __uint_as_float(__float_as_uint(r1[s]) & 0xffff0000u);
    }
    p1 = w16_pack_hi2(x);
    p2 = w16_pack_hi2(r1);
    p3 = w16_pack_hi2(r2);
}
__device__ __forceinline__ void w16_split3(const float (&v)[8], u32x4 &p1, u32x4 &p2, u32x4 &p3) {
#ifdef EPNN_SPLIT_VALU             // (development builds, for comparison)
    w16_split3_valu(v, p1, p2, p3);
#else
    const w16_u32x2 I = w16_ident();       // (a function of the lane alone: the compiler keeps or rebuilds it as registers allow)
    f32x4 x0 = {v[0], v[1], v[2], v[3]}, x1 = {v[4], v[5], v[6], v[7]};
    p1 = w16_pack_hi(x0, x1);
    x0 = w16_rem(I, p1[0], p1[1], x0); x1 = w16_rem(I, p1[2], p1[3], x1);
    p2 = w16_pack_hi(x0, x1);
    x0 = w16_rem(I, p2[0], p2[1], x0); x1 = w16_rem(I, p2[2], p2[3], x1);
    p3 = w16_pack_hi(x0, x1);
#endif
}
// D[rb] += W[rb] z for one column block: w = the kernel's three pieces per row block, z1..z3 the activations' (smallest terms first)
__device__ __forceinline__ void w16_mm_bf(const u32x4 (&w)[2][3], u32x4 z1, u32x4 z2, u32x4 z3, f32x4 (&d)[2]) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        d[rb] = w16_mfma_bf(w[rb][0], z3, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][1], z2, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][2], z1, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][0], z2, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][1], z1, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][0], z1, d[rb]);
    }
}
// the three-piece kernel of a product: [2 row blocks][3 pieces][64 lanes][4 dwords], one 16-byte load each
#define W16_LDB(dst, off)                                                                                       \
    _Pragma("unroll") for (int rb_ = 0; rb_ < 2; ++rb_)                                                         \
        _Pragma("unroll") for (int pc_ = 0; pc_ < 3; ++pc_)                                                     \
            (dst)[rb_][pc_] = reinterpret_cast<const u32x4 *>(wp + (size_t)(unsigned)(off))[(rb_ * 3 + pc_) * 64 + lane];
// ---- the same at K = 16: operands of up to 16 values -- the pair coordinates of a G product and the xq block
// (node mask, one, charge, x: wave_xq_slot).  Lane 16 q + m holds row / column m and the K slots 4 q .. 4 q + 3 as two dwords of
// bf16 pairs; the split of a lane's four values is one remainder MFMA (w16_rem) per level.
// The six partial products are issued as THREE v_mfma_f32_16x16x32_bf16: two K = 16 operands side by side in four consecutive
// registers are one K = 32 operand (lane 16 q + m: K slots 8 q .. 8 q + 3 from the first, 8 q + 4 .. 8 q + 7 from the second), so
//     (w1|w2) . (z3|z1) = w1 z3 + w2 z1,    (w3|w1) . (z1|z2) = w3 z1 + w1 z2,    (w1|w2) . (z1|z2) = w1 z1 + w2 z2
// are the same six products, each once, the smallest terms in the first two, in half the instructions and half the links of the
// accumulate chain (measured: a K = 16 instruction keeps the pipe busy as long as a K = 32 one, profiles/r18_k16_pairs.txt: the
// pipe's busy cycles fell with the instruction count).  This pairing needs TWO four-register tuples
// on either side and none that overlap: the compiler gives every MFMA operand a register tuple of its own (it copies registers
// where two operands share some), so a third tuple is four registers or four v_mov.  Each side carries its first piece twice:
// the activation as a = z3|z1, b = z1|z2 (W16K16 holds a and z2), the kernel's row block as the 32 bytes w1 w2 | w3 w1 (the host's
// frag_bf3k16).
struct W16K16 { u32x4 a; w16_u32x2 z2; };              // (b = z1|z2 is put together where it is used: two copies, no registers held)
__device__ __forceinline__ W16K16 w16_k16(w16_u32x2 p1, w16_u32x2 p2, w16_u32x2 p3) {
    return W16K16{u32x4{p3[0], p3[1], p1[0], p1[1]}, p2};
}
__device__ __forceinline__ W16K16 w16_split3k16(f32x4 x) {
    const w16_u32x2 I = w16_ident();
    const w16_u32x2 p1 = w16_pack_hi2(x);
    x = w16_rem(I, p1[0], p1[1], x);
    const w16_u32x2 p2 = w16_pack_hi2(x);
    x = w16_rem(I, p2[0], p2[1], x);
    return w16_k16(p1, p2, w16_pack_hi2(x));
}
// D[rb] += W[rb] z: w[rb][0] = w1|w2, w[rb][1] = w3|w1
__device__ __forceinline__ void w16_mm_bfk16(const u32x4 (&w)[2][2], const W16K16 &z, f32x4 (&d)[2]) {
    const u32x4 zb = {z.a[2], z.a[3], z.z2[0], z.z2[1]};
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        d[rb] = w16_mfma_bf(w[rb][0], z.a, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][1], zb, d[rb]);
        d[rb] = w16_mfma_bf(w[rb][0], zb, d[rb]);
    }
}
// a K = 16 three-piece kernel: [2 row blocks][2 halves][64 lanes][4 dwords] (w1 w2 | w3 w1), one 16-byte load per half
#define W16_LDB16(dst, off)                                                                                     \
    _Pragma("unroll") for (int rb_ = 0; rb_ < 2; ++rb_)                                                         \
        _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_)                                                     \
            (dst)[rb_][hf_] = reinterpret_cast<const u32x4 *>(wp + (size_t)(unsigned)(off))[(rb_ * 2 + hf_) * 64 + lane];
__device__ __forceinline__ f32x4 w16_relu(f32x4 v) {
    return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
}
// ReLU of a SUM as the add's own output clamp: min(max(a + b, 0), 1) is one v_add_f32 with the clamp modifier where relu(a + b) is a
// v_add_f32 and a v_max_f32 -- the same bits wherever a + b <= 1.  The kernel's CLAMP form therefore runs every pair MLP on
// operands scaled by a power of two (pack_weights: relu(s x) = s relu(x) exactly, in float32 and in every bf16 piece) and checks,
// per wavefront and step, that the scaled pre-activations stay below 1 (k_wave_forward: `relu_lim`).
__device__ __forceinline__ f32x4 w16_clamp01(f32x4 v) {
    return f32x4{fminf(fmaxf(v[0], 0.f), 1.f), fminf(fmaxf(v[1], 0.f), 1.f), fminf(fmaxf(v[2], 0.f), 1.f), fminf(fmaxf(v[3], 0.f), 1.f)};
}
// running max |v| over a lane's eight values of a row (v_max3_f32 with abs modifiers: one instruction per two values)
__device__ __forceinline__ float w16_absmax(float m, const f32x4 (&a)[2]) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        m = fmaxf(fmaxf(m, fabsf(a[rb][0])), fabsf(a[rb][1]));
        m = fmaxf(fmaxf(m, fabsf(a[rb][2])), fabsf(a[rb][3]));
    }
    return m;
}
// sum over the four lanes q = 0..3 that share a column: two VALU lane swaps (gfx950 v_permlane16/32_swap), no LDS
// round trip; every lane ends up with the same bits ((q0 + q1) + (q2 + q3))
__device__ __forceinline__ float w16_sumq(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ f32x4 w16_ld(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void w16_st(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// LDS through explicit 32-bit addresses: a running address costs one v_add per tile, constant offsets ride in the instruction
typedef __attribute__((address_space(3))) const f32x4 w16_lds_cf4;
typedef __attribute__((address_space(3))) const unsigned short w16_lds_cu16;
__device__ __forceinline__ unsigned w16_lds_addr(const void *p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const char *)p; }
__device__ __forceinline__ f32x4 w16_lds_ld4(unsigned a) { return *(w16_lds_cf4 *)(size_t)a; }
__device__ __forceinline__ unsigned w16_lds_ldu16(unsigned a) { return *(w16_lds_cu16 *)(size_t)a; }
typedef __attribute__((address_space(3))) const unsigned w16_lds_cu32;
__device__ __forceinline__ unsigned w16_lds_ldu32(unsigned a) { return *(w16_lds_cu32 *)(size_t)a; }
typedef __attribute__((address_space(3))) u32x4 w16_lds_u4;
typedef __attribute__((address_space(3))) float w16_lds_f1;
__device__ __forceinline__ u32x4 w16_lds_ldu4(unsigned a) { return *(const w16_lds_u4 *)(size_t)a; }
__device__ __forceinline__ void w16_lds_stu4(unsigned a, u32x4 v) { *(w16_lds_u4 *)(size_t)a = v; }
__device__ __forceinline__ void w16_lds_stf(unsigned a, float v) { *(w16_lds_f1 *)(size_t)a = v; }
__device__ __forceinline__ f32x2 w16_lo(f32x4 v) { return __builtin_shufflevector(v, v, 0, 1); }
__device__ __forceinline__ f32x2 w16_hi(f32x4 v) { return __builtin_shufflevector(v, v, 2, 3); }
__device__ __forceinline__ f32x4 w16_cat(f32x2 a, f32x2 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3); }

// fragment loads: [nrb][stride / 4][64 lanes][4], steps s0 .. s0+cnt-1 of every row block (s0, cnt, stride multiples of 4).
// A lane's four consecutive K steps are 16 contiguous bytes: ONE global_load_dwordx4 per four steps (1 KB per wavefront
// instruction, fully coalesced) instead of four global_load_dword -- the kernel issued 1160 vector loads per molecule, nearly
// all of them weights, and every vector-memory instruction costs issue slots beside the matrix pipe (round 4).  One address
// per row block, the step groups as immediate offsets of the load (1 KB apart: inside the 4 KB immediate range).
#define W16_LDX(dst, off, nrb, cnt, stride, s0)                                                                   \
    _Pragma("unroll") for (int rb_ = 0; rb_ < (nrb); ++rb_) {                                                     \
        const f32x4 *fp_ = reinterpret_cast<const f32x4 *>(wp + (size_t)(unsigned)(off)) +                        \
                           (size_t)(unsigned)((rb_ * ((stride) / 4) + (s0) / 4) * 64 + lane);                     \
        _Pragma("unroll") for (int g_ = 0; g_ < (cnt) / 4; ++g_) {                                                \
            const f32x4 v_ = fp_[g_ * 64];                                                                        \
            (dst)[rb_][4 * g_] = v_[0]; (dst)[rb_][4 * g_ + 1] = v_[1]; (dst)[rb_][4 * g_ + 2] = v_[2]; (dst)[rb_][4 * g_ + 3] = v_[3]; \
        }                                                                                                         \
    }
#define W16_LD(dst, off, nrb, steps) W16_LDX(dst, off, nrb, steps, steps, 0)

// D[rb] += sum_s W[rb][s] * in[s]  for one column block (dependent chain of S MFMAs per row block).  Interleaving the row
// blocks' chains (a dependent v_mfma_f32_16x16x4_f32 can issue 40 cycles after its predecessor, the pipe takes one every 32)
// was measured in round 4: no gain with two wavefronts per SIMD, and it costs registers (spills in the block-per-wavefront kernels).
template <int NRB, int S>
__device__ __forceinline__ void w16_mm(const float (&w)[NRB][S], const float (&in)[S], f32x4 (&d)[NRB]) {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int s = 0; s < S; ++s) d[rb] = w16_mfma(w[rb][s], in[s], d[rb]);
}
// same, but K step SKIP is left out when `skip` is set (the last xq step holds only zeros when nx + 3 <= 12)
template <int NRB, int S, int SKIP>
__device__ __forceinline__ void w16_mm_skip(const float (&w)[NRB][S], const float (&in)[S], f32x4 (&d)[NRB], bool skip) {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s == SKIP) {
                if (!skip) d[rb] = w16_mfma(w[rb][s], in[s], d[rb]);
            } else {
                d[rb] = w16_mfma(w[rb][s], in[s], d[rb]);
            }
        }
}
// an accumulator set [NRB row blocks] of one column block as the next product's 4 NRB input steps
template <int NRB>
__device__ __forceinline__ void w16_feed(const f32x4 (&a)[NRB], float (&in)[4 * NRB]) {
#pragma unroll
    for (int s = 0; s < 4 * NRB; ++s) in[s] = a[s >> 2][s & 3];
}
#endif
