// Charge gradients with respect to the coordinates from the pair list (option "grad_path" = 2): the structures, the checkpointed
// forward and the all-pairs sweep.  The backward's other kernels: epnn_vjp_multi.hip.h.  Part of the one translation unit epnn_api.hip.
//
// The dense path (epnn_grad_xyz.hip.h) pads every molecule to [B][N][N] rows.  This path runs the factorised form of DESIGN.md
// section 2 backwards on per-atom rows [A][32] / [A][48], the list of pairs under the cutoff (pi, pj, pe [P][48], near weights)
// and its incidence slots (epnn_frontend.hip.h): nothing of size N^2 exists.  tests/grad_large_ref.py is the same algebra in
// float64.
//
//   forward with checkpoints     h_t [T+1][A][48], S_t [T][A][32], q_t [T+1][A]; everything else is recomputed
//   EPN stack, t = T-1 .. 0      listed pairs only, both orders of the pass MLP, seed +-0.5 w (gq_i - gq_j); the first layer's
//                                gradients go to the two atoms' incidence slots, every atom sums its own row in slot order
//   GNN step t >= 1              update MLP backward -> dS_i; all-pairs backward sweep (k_gl_sweep, f32 MFMA) as a row pass
//                                (dP_i = sum_j dz1_ij) and a column pass (dR_j = sum_i dz1_ij); near pairs as correction rows in the
//                                incidence slots; the (N - n) padded partners in closed form per atom
//   GNN step 0                   a_i = [x_i | 0 | Q/n] does not depend on the coordinates: only the listed pairs' dG
//   edges -> coordinates         gE [P][48] -> gD (float64) -> +-gD d / D into the pair's two slots, summed per atom in float64
//
// The backward runs for K seeds beside the one primal (k_gvm_*<KM>, k_gl_sweep<MODE, KC>); the single-cotangent calls are K = 1.
// A training step (option "train_path", epnn_train_large.hip.h) runs the same kernels at K = 1 with step 0 in full and a GlTape
// (their TAPE instances): they then also store the rows its weight gradients are outer products of, and the row pass adds up
// dW2 / db2 of all pairs (k_gl_sweep<1, 1, 1>).
//
// Plain float32 throughout (the Dense layers of the two sweeps on v_mfma_f32_16x16x4_f32).  Every sum has a fixed order, there
// are no float atomics: results are bit-reproducible and a molecule's rows do not depend on the rest of the batch (the number of
// pieces its partner range is cut into depends on its own size alone).
//
// Why the checkpointed forward is this file's own (k_gl_proj, k_gl_sweep<0>, k_gl_gnn_pair, k_gl_gnn_tail, k_gl_epn_*) and not the
// tiled forward of epnn_large.hip.h: the backward needs S_t and h_t of every step as rows in memory (the tiled forward folds W3 and
// Wu3 into the next step's matrices and never forms h between steps, and its first step runs by atom types), and it takes its ReLU
// decisions from recomputed f32 pre-activations, which must be the ones the forward took -- the tiled sweep's bf16 three-piece
// products round differently from the f32 MFMAs of the two backward passes.  The charges of this forward therefore agree with
// epnn_forward_xyz to float32 accumulation (2e-4 in the tests), not bit for bit, like the dense path's.
#pragma once
#include "epnn_host.h"
#include "epnn_pair_geo.hip.h"

#define GL_H 32                   // hidden width of every MLP, and of the summed messages
#define GL_E 48                   // channels of h and e

struct GlPair {                   // a message / pass MLP: first Dense split by input block (rows of W1: a_i | a_j | e_ij)
    const float *Wi, *Wj, *We, *b1, *W2, *b2, *W3, *b3;      // W3 [32][32], b3 [32] (message) or [32], [1] (pass)
};
struct GlUpd {                    // update MLP [h | M] (80) -> 32 -> 32 -> 48
    const float *U1, *c1, *U2, *c2, *U3, *c3;
};
struct GlGeom {                   // the batch
    const int *moff, *mol_of;     // [B + 1], [A]
    int A, N, nx;
};
// What a training step (epnn_train_large.hip.h) keeps of the backward kernels' intermediates for its weight gradients: the TAPE
// instances of the k_gvm_* kernels write it; the others take a GlTape{} and do not read it.  Rows of 32 unless noted.
//   z1, d2   a Dense-2 input and its output gradient: EPN pair p, order o at row 2 p + o; GNN pair p, order o at rows 4 p + 2 o
//            (with G) and 4 p + 2 o + 1 (without G, d2 negated: the correction rows' sign); GNN atom a at row pad0 + a: relu(P_a)
//            and (N - n) d2 of its padded partners
//   dz       [pairs] dz1_ij + dz1_ji with G (the We block);  r3 [2 pairs] relu(z2) times the row's seed (W3 of a pass MLP)
//   u0 [A][80], u1, u2, ud2, ud1, gm [A]   the update MLP's activations and pre-activation gradients, gm = dM
//   dv [A][64]   dP_a | dR_a, complete
struct GlTape {
    float *z1, *d2, *dz, *r3, *u0, *u1, *u2, *ud2, *ud1, *gm, *dv;
    size_t pad0;
};

// sum_k v[k] W[k][col] over the 32 rows of a [32][stride] block (v in LDS, the 32 lanes of a half read one row: coalesced)
__device__ __forceinline__ float gl_dotT(const float *W, int stride, int col, const float *v) {
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < GL_H; ++k) acc = fmaf(v[k], W[k * stride + col], acc);
    return acc;
}
// sum_k W[row][k] v[k]: the transposed product of a backward
__device__ __forceinline__ float gl_dotN(const float *W, int stride, int row, const float *v, int n) {
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = fmaf(W[row * stride + k], v[k], acc);
    return acc;
}

// ---------------------------------------------------------------------------------------------------------- per atom: projections
// One wavefront per atom: a = [x | h | q], P = Wi^T a + b1 (lanes 0..31), R = Wj^T a (lanes 32..63), then the sweeps' second
// operands Yc = b2 + W2^T P (column pass) and Yb = b2 + W2^T R (row pass).  h: rows [A][48] or null (zeros); q: [A] or null (Q/n).
__global__ __launch_bounds__(64) void k_gl_proj(GlPair M, GlGeom G, const float *x, const float *h, const float *q, const float *Q,
                                                float *P, float *R, float *Yb, float *Yc) {
    __shared__ float av[64], pr[2][GL_H];
    const int a = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int F = G.nx + GL_E + 1;
    if (lane < G.nx) av[lane] = x[(size_t)a * G.nx + lane];
    if (lane < GL_E) av[G.nx + lane] = h ? h[(size_t)a * GL_E + lane] : 0.f;
    if (lane == 63) {
        const int b = G.mol_of[a];
        av[G.nx + GL_E] = q ? q[a] : Q[b] / (float)(G.moff[b + 1] - G.moff[b]);
    }
    __syncthreads();
    const float *W = half ? M.Wj : M.Wi;
    float acc = half ? 0.f : M.b1[f];
    for (int k = 0; k < F; ++k) acc = fmaf(av[k], W[k * GL_H + f], acc);
    pr[half][f] = acc;
    (half ? R : P)[(size_t)a * GL_H + f] = acc;
    __syncthreads();
    if (Yb) (half ? Yb : Yc)[(size_t)a * GL_H + f] = M.b2[f] + gl_dotT(M.W2, GL_H, f, pr[half]);
}

// ---------------------------------------------------------------------------------------------------------- the all-pairs sweeps
// One wavefront per task = (16 resident atoms as the columns of an MFMA tile, one piece of their molecule's partner range).
// Lane 16 qd + c owns column c and of it the features 16 rb + 4 qd + r (rb = 0, 1; r = 0..3) -- the accumulator layout of
// v_mfma_f32_16x16x4_f32; with the K steps ordered s = 4 rb' + r' such a set of eight values is the next product's B operand as
// it stands.  Per partner (its rows are wave-uniform loads: 16 lanes read one address):
//     z1   = max(X_res, -X_str)                 relu(P + R) less the streamed row, which Y carries: Y = b2 + W2^T X_str
//     z2pre = W2^T z1 + Y                       16 MFMAs
//   MODE 0 (forward, row pass: resident P_i, streamed R_j, Yb_j):    S_i  += relu(z2pre)
//   MODE 1 (backward, row pass: resident P_i, dS_i):                  dP_i += [X_res > -X_str] W2 (dS_i [z2pre > 0])     16 more
//   MODE 2 (backward, column pass: resident R_j; streamed P_i, Yc_i, dS_i):  dR_j += the same with the streamed dS_i
// The sums stay in the lane that owns them; out [piece][A][32] gets one row per (piece, resident atom), written by exactly one
// wavefront (an empty piece writes zeros), and the per-atom kernels add the pieces in order.
// KC (MODE 1, 2): the cotangents of one launch.  The primal (z1, z2pre) stands once per partner; each cotangent u has its own dS (the
// first at dS, the next at dstride floats), its own 16 backward MFMAs from zero and its own out (at ostride floats), and reads
// nothing of another: a row has the same bits at every KC.  KC >= 2 runs one task per wavefront (`run` is not read).
// WG 1 (a training step's row pass, MODE 1, KC 1): the wavefront also adds up the weight gradient of the second Dense over every pair
// it sees, dW2[k][m] += sum_c z1_c[k] d2_c[m] and db2[m] += sum_c d2_c[m] with z1 = relu(P + R) itself.  That product reduces over
// the tile's columns, which the accumulator layout keeps in the lane index: the two 16 x 32 tiles go through LDS (rows of GL_TS
// floats) and come back as MFMA operands with the column on the K index, 16 more v_mfma_f32_16x16x4_f32 per partner; the 32 x 32 + 32
// sums stay in registers across the partners of all `run` tasks of the wavefront (tasks blockIdx.x * run ...) and leave as one row
// of wpart [wavefronts][1056], which k_tl_reduce_sweep adds up in order.  A gradient call has run = 1 and one task per wavefront.
#define GL_TS 36
template <int MODE, int KC = 1, int WG = 0>
__global__ __launch_bounds__(64) void k_gl_sweep(const int4 *tasks, const int *moff, int A, const float *W2, const float *Xres,
                                                 const float *Xstr, const float *Y, const float *dS, size_t dstride, float *out,
                                                 size_t ostride, int ntask, int run, float *wpart) {
    static_assert(KC == 1 || (MODE != 0 && WG == 0), "the forward pass and the weight-gradient pass carry one row");
    __shared__ float tz[WG ? 16 * GL_TS : 1], td[WG ? 16 * GL_TS : 1];
    const int lane = threadIdx.x, c = lane & 15, qd = lane >> 4;
    if (KC > 1 && (int)blockIdx.x >= ntask) return;                 // (a chunk of cotangents: one task per wavefront)
    float wf[2][8], wb[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kf = 16 * (s >> 2) + 4 * qd + (s & 3), m = 16 * rb + c;
            wf[rb][s] = W2[kf * GL_H + m];                      // out[m] = sum_k W2[k][m] z1[k]
            wb[rb][s] = W2[m * GL_H + kf];                      // out[m] = sum_k W2[m][k] d2[k]
        }
    f32x4 aw[2][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int t_end = KC == 1 ? min(ntask, ((int)blockIdx.x + 1) * run) : (int)blockIdx.x + 1;
    for (int task = KC == 1 ? (int)blockIdx.x * run : (int)blockIdx.x; task < t_end; ++task) {
        const int4 tk = tasks[task];                                // (first resident atom, molecule, piece, pieces)
        const int a0 = moff[tk.y], a1 = moff[tk.y + 1];
        const int len = (a1 - a0 + tk.w - 1) / tk.w;
        const int j0 = min(a0 + tk.z * len, a1), j1 = min(j0 + len, a1);
        const int col = tk.x + c;
        const bool valid = col < a1;
        const int colc = valid ? col : a1 - 1;
        float xr[8], ds[MODE == 1 ? KC : 1][8], acc[KC][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int f = 16 * (e >> 2) + 4 * qd + (e & 3);
            xr[e] = Xres[(size_t)colc * GL_H + f];
#pragma unroll
            for (int u = 0; u < KC; ++u) {
                if (MODE == 1) ds[u][e] = valid ? dS[u * dstride + (size_t)colc * GL_H + f] : 0.f;
                acc[u][e] = 0.f;
            }
        }
        for (int j = j0; j < j1; ++j) {
            const float *xs = Xstr + (size_t)j * GL_H + 4 * qd, *ys = Y + (size_t)j * GL_H + 4 * qd;
            const f32x4 n0 = *reinterpret_cast<const f32x4 *>(xs), n1 = *reinterpret_cast<const f32x4 *>(xs + 16);
            f32x4 o0 = *reinterpret_cast<const f32x4 *>(ys), o1 = *reinterpret_cast<const f32x4 *>(ys + 16);
            float nn[8], z1[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { nn[e] = -n0[e]; nn[4 + e] = -n1[e]; }
#pragma unroll
            for (int e = 0; e < 8; ++e) z1[e] = fmaxf(xr[e], nn[e]);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][s], z1[s], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[1][s], z1[s], o1, 0, 0, 0);
            }
            if (MODE == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[0][e] += fmaxf(o0[e], 0.f); acc[0][4 + e] += fmaxf(o1[e], 0.f); }
                continue;
            }
#pragma unroll
            for (int u = 0; u < KC; ++u) {
                float d2[8];
                if (MODE == 2) {
                    const float *dp = dS + u * dstride + (size_t)j * GL_H + 4 * qd;
                    const f32x4 d0 = *reinterpret_cast<const f32x4 *>(dp), d1 = *reinterpret_cast<const f32x4 *>(dp + 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { d2[e] = o0[e] > 0.f ? d0[e] : 0.f; d2[4 + e] = o1[e] > 0.f ? d1[e] : 0.f; }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { d2[e] = o0[e] > 0.f ? ds[u][e] : 0.f; d2[4 + e] = o1[e] > 0.f ? ds[u][4 + e] : 0.f; }
                }
                if (WG) {
                    // (an invalid column has dS = 0, so d2 = 0: its z1 row, the last real atom's, adds nothing)
                    *reinterpret_cast<f32x4 *>(&tz[c * GL_TS + 4 * qd]) = f32x4{fmaxf(xr[0] - nn[0], 0.f), fmaxf(xr[1] - nn[1], 0.f), fmaxf(xr[2] - nn[2], 0.f), fmaxf(xr[3] - nn[3], 0.f)};
                    *reinterpret_cast<f32x4 *>(&tz[c * GL_TS + 16 + 4 * qd]) = f32x4{fmaxf(xr[4] - nn[4], 0.f), fmaxf(xr[5] - nn[5], 0.f), fmaxf(xr[6] - nn[6], 0.f), fmaxf(xr[7] - nn[7], 0.f)};
                    *reinterpret_cast<f32x4 *>(&td[c * GL_TS + 4 * qd]) = f32x4{d2[0], d2[1], d2[2], d2[3]};
                    *reinterpret_cast<f32x4 *>(&td[c * GL_TS + 16 + 4 * qd]) = f32x4{d2[4], d2[5], d2[6], d2[7]};
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < 4; ++q) {                       // K = the columns 4 q .. 4 q + 3; this lane's is 4 q + qd
                        const float *zr = &tz[(4 * q + qd) * GL_TS + c], *dr = &td[(4 * q + qd) * GL_TS + c];
                        const float za = zr[0], zb = zr[16], da = dr[0], db = dr[16];
                        aw[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(za, da, aw[0][0], 0, 0, 0);
                        aw[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(za, db, aw[0][1], 0, 0, 0);
                        aw[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(zb, da, aw[1][0], 0, 0, 0);
                        aw[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(zb, db, aw[1][1], 0, 0, 0);
                    }
                    __syncthreads();
#pragma unroll
                    for (int e = 0; e < 8; ++e) bsum[e] += d2[e];
                }
                f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    g0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[0][s], d2[s], g0, 0, 0, 0);
                    g1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[1][s], d2[s], g1, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[u][e] += xr[e] > nn[e] ? g0[e] : 0.f;
                    acc[u][4 + e] += xr[4 + e] > nn[4 + e] ? g1[e] : 0.f;
                }
            }
        }
        if (valid) {
#pragma unroll
            for (int u = 0; u < KC; ++u) {
                float *o = out + u * ostride + ((size_t)tk.z * A + col) * GL_H + 4 * qd;
                *reinterpret_cast<f32x4 *>(o) = f32x4{acc[u][0], acc[u][1], acc[u][2], acc[u][3]};
                *reinterpret_cast<f32x4 *>(o + 16) = f32x4{acc[u][4], acc[u][5], acc[u][6], acc[u][7]};
            }
        }
    }
    if (WG) {
        // lane (qd, c) holds dW2[16 fa + 4 qd + r][16 fb + c]; db2: the 16 lanes of a feature are added in lane order
        float *o = wpart + (size_t)blockIdx.x * (GL_H * GL_H + GL_H);
#pragma unroll
        for (int fa = 0; fa < 2; ++fa)
#pragma unroll
            for (int fb = 0; fb < 2; ++fb)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[(16 * fa + 4 * qd + r) * GL_H + 16 * fb + c] = aw[fa][fb][r];
        *reinterpret_cast<f32x4 *>(&tz[c * GL_TS + 4 * qd]) = f32x4{bsum[0], bsum[1], bsum[2], bsum[3]};
        *reinterpret_cast<f32x4 *>(&tz[c * GL_TS + 16 + 4 * qd]) = f32x4{bsum[4], bsum[5], bsum[6], bsum[7]};
        __syncthreads();
        if (lane < GL_H) {
            float sum = 0.f;
            for (int k = 0; k < 16; ++k) sum += tz[k * GL_TS + lane];
            o[GL_H * GL_H + lane] = sum;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- per listed pair
// One wavefront per listed pair {i < j}: lanes 0..31 take the order (i, j), lanes 32..63 the order (j, i), a lane one hidden
// unit.  G = We^T e_ij is the same for both (e_ij == e_ji).
struct GlPairs {
    const int *pi, *pj, *dest_i, *dest_j;
    const float *pe, *pw;
};

// GNN step, forward: the pair's correction rows, relu(W2^T relu(P + R + G) + b2) minus the same without G, into the first atom's
// slot (corr [slots][32]).  Its backward: k_gvm_gnn_pair (epnn_vjp_multi.hip.h).
__global__ __launch_bounds__(64) void k_gl_gnn_pair(GlPair M, GlPairs L, const float *P, const float *R, float *corr) {
    __shared__ float ev[GL_E], z[2][2][GL_H];
    const int p = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int i = L.pi[p], j = L.pj[p];
    const int a = half ? j : i, b = half ? i : j;                 // this half's row is [a_a | a_b | e]
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) return;               // (a pair without both slots would be a front-end fault: write nothing)
    if (lane < GL_E) ev[lane] = L.pe[(size_t)p * GL_E + lane];
    __syncthreads();
    float g = 0.f;
    for (int k = 0; k < GL_E; ++k) g = fmaf(ev[k], M.We[k * GL_H + f], g);
    const float base = P[(size_t)a * GL_H + f] + R[(size_t)b * GL_H + f];
    const float z1g = base + g;
    z[half][0][f] = fmaxf(z1g, 0.f);
    z[half][1][f] = fmaxf(base, 0.f);
    __syncthreads();
    const float z2g = M.b2[f] + gl_dotT(M.W2, GL_H, f, z[half][0]), z2n = M.b2[f] + gl_dotT(M.W2, GL_H, f, z[half][1]);
    const int sa = half ? L.dest_j[p] : L.dest_i[p];
    corr[(size_t)sa * GL_H + f] = fmaxf(z2g, 0.f) - fmaxf(z2n, 0.f);
}

// EPN step, forward: delta = (f(a_i, a_j, e) - f(a_j, a_i, e)) / 2, slotq[dest_i] = w delta, slotq[dest_j] = -w delta.  Its
// backward: k_gvm_epn_pair (epnn_vjp_multi.hip.h).
__global__ __launch_bounds__(64) void k_gl_epn_pair(GlPair M, GlPairs L, const float *P, const float *R, float *slotq) {
    __shared__ float ev[GL_E], z[2][GL_H], red[2][GL_H];
    const int p = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int i = L.pi[p], j = L.pj[p];
    const int a = half ? j : i, b = half ? i : j;
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) return;
    if (lane < GL_E) ev[lane] = L.pe[(size_t)p * GL_E + lane];
    __syncthreads();
    float g = 0.f;
    for (int k = 0; k < GL_E; ++k) g = fmaf(ev[k], M.We[k * GL_H + f], g);
    const float z1 = P[(size_t)a * GL_H + f] + R[(size_t)b * GL_H + f] + g;
    z[half][f] = fmaxf(z1, 0.f);
    __syncthreads();
    const float z2 = M.b2[f] + gl_dotT(M.W2, GL_H, f, z[half]);
    const float w = L.pw[p];
    const int sa = half ? L.dest_j[p] : L.dest_i[p];
    red[half][f] = fmaxf(z2, 0.f) * M.W3[f];
    __syncthreads();
    if (f == 0) {
        float fi = 0.f, fj = 0.f;                               // (b3 cancels in the difference)
        for (int k = 0; k < GL_H; ++k) { fi += red[0][k]; fj += red[1][k]; }
        const float delta = 0.5f * (fi - fj);
        slotq[sa] = half ? -(w * delta) : w * delta;
    }
}

// ---------------------------------------------------------------------------------------------------------- per atom
// the pieces a molecule's partner range is cut into: by its own size alone (16 atoms per task; about 2048 tasks fill the GPU)
__host__ __device__ __forceinline__ int gl_pieces(int n) {
    const int tiles = (n + 15) / 16, want = (2048 + tiles - 1) / tiles;
    return want < 1 ? 1 : (want > 16 ? 16 : want);
}

// End of a forward GNN step, one wavefront per atom: S = pieces in order + (N - n) relu(W2^T relu(P) + b2) + the atom's correction
// slots in order; M = W3^T S + N b3; h' = update MLP([h | M]).  S and h' are the step's checkpoints.
__global__ __launch_bounds__(64) void k_gl_gnn_tail(GlPair M, GlUpd U, GlGeom G, const int *inc_off, const float *part, const float *corr,
                                                    const float *P, const float *h, float *S_out, float *h_out) {
    __shared__ float v[GL_H], u0[GL_E + GL_H], u1[GL_H], u2[GL_H];
    const int a = blockIdx.x, lane = threadIdx.x;
    const int b = G.mol_of[a], n = G.moff[b + 1] - G.moff[b];
    if (lane < GL_H) v[lane] = fmaxf(P[(size_t)a * GL_H + lane], 0.f);
    if (lane < GL_E) u0[lane] = h ? h[(size_t)a * GL_E + lane] : 0.f;
    __syncthreads();
    if (lane < GL_H) {
        float s = 0.f;
        const int np = gl_pieces(n);
        for (int k = 0; k < np; ++k) s += part[((size_t)k * G.A + a) * GL_H + lane];
        s += (float)(G.N - n) * fmaxf(M.b2[lane] + gl_dotT(M.W2, GL_H, lane, v), 0.f);
        for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += corr[(size_t)k * GL_H + lane];
        S_out[(size_t)a * GL_H + lane] = s;
        u1[lane] = s;
    }
    __syncthreads();
    if (lane < GL_H) u0[GL_E + lane] = (float)G.N * M.b3[lane] + gl_dotT(M.W3, GL_H, lane, u1);
    __syncthreads();
    float t = 0.f;
    if (lane < GL_H) {
        t = U.c1[lane];
        for (int k = 0; k < GL_E + GL_H; ++k) t = fmaf(u0[k], U.U1[k * GL_H + lane], t);
    }
    __syncthreads();
    if (lane < GL_H) u1[lane] = fmaxf(t, 0.f);
    __syncthreads();
    if (lane < GL_H) u2[lane] = fmaxf(U.c2[lane] + gl_dotT(U.U2, GL_H, lane, u1), 0.f);
    __syncthreads();
    if (lane < GL_E) h_out[(size_t)a * GL_E + lane] = U.c3[lane] + gl_dotT(U.U3, GL_E, lane, u2);
}

// EPN forward: every atom adds its transfer slots in order.
__global__ __launch_bounds__(256) void k_gl_epn_atom(int A, const int *inc_off, const float *slotq, const float *q, float *q_out) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    float s = q[a];
    for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += slotq[k];
    q_out[a] = s;
}
// the charges before the first EPN step: Q / n
__global__ __launch_bounds__(256) void k_gl_q0(GlGeom G, const float *Q, float *q) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= G.A) return;
    const int b = G.mol_of[a];
    q[a] = Q[b] / (float)(G.moff[b + 1] - G.moff[b]);
}
