// Reverse-mode derivative of the charges along K cotangents in one pass (epnn_charges_vjp_multi_xyz_cell): the kernels.  Part of the
// one translation unit epnn_api.hip.
//
// The pair-list gradient path (epnn_grad_large.hip.h) runs its checkpointed forward and then one backward from one seed g [A].  Its
// backward is linear in the seed, and every ReLU decision in it comes from the primal alone.  This file is that backward for
// K <= GVM_MAXK seeds beside the one primal: the forward (gl_forward_ckpt) and the primal projections (k_gl_proj) are the gradient
// path's own launches, run once; the kernels below recompute a pair's or an atom's primal pre-activations and masks once and then
// loop over the cotangents.
//
//   k_gvm_epn_pair, k_gvm_epn_atom_bwd            the EPN stack (k_gl_epn_pair<1>, k_gl_epn_atom_bwd)
//   k_gvm_upd_bwd                                 the update MLP (k_gl_upd_bwd)
//   k_gvm_sweep<MODE, KC>                         the two all-pairs backward sweeps (k_gl_sweep<1>, <2>), KC cotangents per launch
//   k_gvm_gnn_pair, k_gvm_gnn_atom_bwd            the listed pairs' correction rows and the end of a GNN step (k_gl_gnn_pair<1>,
//                                                 k_gl_gnn_atom_bwd); step 0 keeps the shortcut: only gE of the listed pairs
//   k_gvm_pair_xyz<GEO>, k_gvm_atom_xyz, k_gvm_strain_mol     edges -> coordinates and strain (k_gl_pair_xyz, k_gl_atom_xyz,
//                                                 k_g_strain_mol); open molecules and cells, no box instance
//
// Every cotangent buffer is K copies of one cotangent's, cotangent t at t times that size (gq [K][A], gh, ghp [K][A][48], dS
// [K][A][32], partP, partR [K][piece][A][32], slotP, slotR [K][slots][32], gE [K][P][48], slotx [K][slots][9] float64, share
// [K][A][6] float64, gxyz [K][A][3], gstrain [K][B][9]).  Each cotangent statement is the fmaf chain or MFMA sequence of the k_gl_*
// kernel it stands for: accumulators from zero, k ascending, pieces and slots added in the same order; none reads another
// cotangent.  Row t therefore has the bits epnn_charges_vjp_xyz_cell gives on "grad_path" 2 for g[t] alone, whatever K, the row's
// position and the other rows are.
//
// Plain float32 (float64 from gE on), every sum in a fixed order, no float atomics.
#pragma once
#include "epnn_grad_large.hip.h"

#define GVM_MAXK 16

// The per-pair and per-atom kernels are templated on KM >= K, the bucket of K (1, 2, 4, 8, 16), as the tangent kernels of
// epnn_jvp.hip.h are: registers and LDS are sized for the bucket, K is uniform over the block and the guards t < K are scalar branches.
//
// acc[t] = sum_k W[row][k] v[t VS + k] for t < K: gl_dotN's fmaf chain per cotangent (k ascending, from 0), each weight loaded once.
template <int KM, int VS>
__device__ __forceinline__ void gvm_dotN(const float *W, int stride, int row, const float *v, int n, int K, float (&acc)[KM]) {
#pragma unroll
    for (int t = 0; t < KM; ++t) acc[t] = 0.f;
    for (int k = 0; k < n; ++k) {
        const float w = W[row * stride + k];
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) acc[t] = fmaf(w, v[t * VS + k], acc[t]);
    }
}

// ---------------------------------------------------------------------------------------------------------- the all-pairs sweeps
// k_gl_sweep<1> (row pass: resident P_i and dS_i per cotangent, streamed R_j, Yb_j) and k_gl_sweep<2> (column pass: resident R_j,
// streamed P_i, Yc_i and dS_i per cotangent) with its tasks, lanes and layout.  Per partner the primal stands once,
//     z1 = max(X_res, -X_str),   z2pre = W2^T z1 + Y      (16 MFMAs),
// and per cotangent u of the launch's KC
//     d2_u = z2pre > 0 ? dS_u : 0,   g_u = W2 d2_u          (16 MFMAs, accumulators from zero),   acc_u += X_res > -X_str ? g_u : 0.
// dS: the chunk's first cotangent, the next at dstride floats; out [piece][A][32] likewise at ostride: one row per (piece, resident
// atom), written by exactly one wavefront (an empty piece writes zeros).
template <int MODE, int KC>
__global__ __launch_bounds__(64) void k_gvm_sweep(const int4 *tasks, const int *moff, int A, const float *W2, const float *Xres,
                                                  const float *Xstr, const float *Y, const float *dS, size_t dstride, float *out,
                                                  size_t ostride, int ntask) {
    const int lane = threadIdx.x, c = lane & 15, qd = lane >> 4;
    const int task = blockIdx.x;
    if (task >= ntask) return;
    float wf[2][8], wb[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kf = 16 * (s >> 2) + 4 * qd + (s & 3), m = 16 * rb + c;
            wf[rb][s] = W2[kf * GL_H + m];                      // out[m] = sum_k W2[k][m] z1[k]
            wb[rb][s] = W2[m * GL_H + kf];                      // out[m] = sum_k W2[m][k] d2[k]
        }
    const int4 tk = tasks[task];                                    // (first resident atom, molecule, piece, pieces)
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

// ---------------------------------------------------------------------------------------------------------- per listed pair
// One wavefront per listed pair, lanes and halves as in k_gl_gnn_pair / k_gl_epn_pair.  SL: slots of one cotangent (2 P1); A, P1:
// atoms and pair rows of one cotangent.
//
// GNN step (k_gl_gnn_pair<1>): G, z1 with and without G and the two z2 pre-activations once; per cotangent dz1 with G minus dz1
// without it into slotP of the first and slotR of the second atom (null for step 0) and gE_ij += We (dz1_ij + dz1_ji) with G.
template <int KM>
__global__ __launch_bounds__(64) void k_gvm_gnn_pair(GlPair M, GlPairs L, int K, int A, size_t P1, size_t SL, const float *P, const float *R,
                                                     const float *dS, float *slotP, float *slotR, float *gE) {
    __shared__ float ev[GL_E], z[2][2][GL_H], d2[2][2][KM][GL_H], dg[2][KM][GL_H];
    if (KM == 1) K = 1;
    const int p = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int i = L.pi[p], j = L.pj[p];
    const int a = half ? j : i, b = half ? i : j;                 // this half's row is [a_a | a_b | e]
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) return;
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
    const int sa = half ? L.dest_j[p] : L.dest_i[p], sb = half ? L.dest_i[p] : L.dest_j[p];
    for (int t = 0; t < K; ++t) {
        const float dsv = dS[((size_t)t * A + a) * GL_H + f];
        d2[half][0][t][f] = z2g > 0.f ? dsv : 0.f;
        d2[half][1][t][f] = z2n > 0.f ? dsv : 0.f;
    }
    __syncthreads();
    float ag[KM], an[KM];
    gvm_dotN<KM, GL_H>(M.W2, GL_H, f, &d2[half][0][0][0], GL_H, K, ag);
    gvm_dotN<KM, GL_H>(M.W2, GL_H, f, &d2[half][1][0][0], GL_H, K, an);
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) {
            const float dg1 = z1g > 0.f ? ag[t] : 0.f;
            const float dn1 = base > 0.f ? an[t] : 0.f;
            if (slotP) {
                slotP[((size_t)t * SL + sa) * GL_H + f] = dg1 - dn1;
                slotR[((size_t)t * SL + sb) * GL_H + f] = dg1 - dn1;
            }
            dg[half][t][f] = dg1;
        }
    __syncthreads();
    if (lane < GL_E) {
        float acc[KM];
#pragma unroll
        for (int t = 0; t < KM; ++t) acc[t] = 0.f;
        for (int k = 0; k < GL_H; ++k) {
            const float w = M.We[lane * GL_H + k];
#pragma unroll
            for (int t = 0; t < KM; ++t)
                if (t < K) acc[t] = fmaf(w, dg[0][t][k] + dg[1][t][k], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) gE[((size_t)t * P1 + p) * GL_E + lane] += acc[t];
    }
}

// EPN step (k_gl_epn_pair<1>): G, z1 and z2 once; per cotangent the row [a_i | a_j | e] is seeded with s = w (gq_i - gq_j) / 2, the
// row [a_j | a_i | e] with -s; a row's dz1 goes to slotP of its first atom and slotR of its second, and gE_ij += We (dz1_ij + dz1_ji).
template <int KM>
__global__ __launch_bounds__(64) void k_gvm_epn_pair(GlPair M, GlPairs L, int K, int A, size_t P1, size_t SL, const float *P, const float *R,
                                                     const float *gq, float *slotP, float *slotR, float *gE) {
    __shared__ float ev[GL_E], z[2][GL_H], d2[2][KM][GL_H], dg[2][KM][GL_H];
    if (KM == 1) K = 1;
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
    const int sa = half ? L.dest_j[p] : L.dest_i[p], sb = half ? L.dest_i[p] : L.dest_j[p];
    for (int t = 0; t < K; ++t) {
        const float seed = 0.5f * w * (gq[(size_t)t * A + i] - gq[(size_t)t * A + j]);
        d2[half][t][f] = z2 > 0.f ? (half ? -seed : seed) * M.W3[f] : 0.f;
    }
    __syncthreads();
    float ad[KM];
    gvm_dotN<KM, GL_H>(M.W2, GL_H, f, &d2[half][0][0], GL_H, K, ad);
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) {
            const float dz1 = z1 > 0.f ? ad[t] : 0.f;
            slotP[((size_t)t * SL + sa) * GL_H + f] = dz1;
            slotR[((size_t)t * SL + sb) * GL_H + f] = dz1;
            dg[half][t][f] = dz1;
        }
    __syncthreads();
    if (lane < GL_E) {
        float acc[KM];
#pragma unroll
        for (int t = 0; t < KM; ++t) acc[t] = 0.f;
        for (int k = 0; k < GL_H; ++k) {
            const float wv = M.We[lane * GL_H + k];
#pragma unroll
            for (int t = 0; t < KM; ++t)
                if (t < K) acc[t] = fmaf(wv, dg[0][t][k] + dg[1][t][k], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) gE[((size_t)t * P1 + p) * GL_E + lane] += acc[t];
    }
}

// ---------------------------------------------------------------------------------------------------------- per atom
// Backward of the update MLP (k_gl_upd_bwd), one wavefront per atom: u0, u1pre and u2pre from the checkpoints (h, S) once; per
// cotangent gh [48] is carried back: gh_prev [K][A][48] = the h columns of the first layer's input gradient, dS [K][A][32] = W3 (its
// M columns).
template <int KM>
__global__ __launch_bounds__(64) void k_gvm_upd_bwd(GlPair M, GlUpd U, GlGeom G, int K, const float *h, const float *S, const float *gh,
                                                    float *gh_prev, float *dS) {
    __shared__ float u0[GL_E + GL_H], sv[GL_H], u1[GL_H], gv[KM][GL_E], d2[KM][GL_H], d1[KM][GL_H], gm[KM][GL_H];
    if (KM == 1) K = 1;
    const int a = blockIdx.x, lane = threadIdx.x;
    if (lane < GL_E) {
        u0[lane] = h ? h[(size_t)a * GL_E + lane] : 0.f;
        for (int t = 0; t < K; ++t) gv[t][lane] = gh[((size_t)t * G.A + a) * GL_E + lane];
    }
    if (lane < GL_H) sv[lane] = S[(size_t)a * GL_H + lane];
    __syncthreads();
    if (lane < GL_H) u0[GL_E + lane] = (float)G.N * M.b3[lane] + gl_dotT(M.W3, GL_H, lane, sv);
    __syncthreads();
    float tt = 0.f;
    if (lane < GL_H) {
        tt = U.c1[lane];
        for (int k = 0; k < GL_E + GL_H; ++k) tt = fmaf(u0[k], U.U1[k * GL_H + lane], tt);
        u1[lane] = fmaxf(tt, 0.f);
    }
    __syncthreads();
    float acc[KM];
    if (lane < GL_H) {
        const float u2pre = U.c2[lane] + gl_dotT(U.U2, GL_H, lane, u1);
        gvm_dotN<KM, GL_E>(U.U3, GL_E, lane, &gv[0][0], GL_E, K, acc);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) d2[t][lane] = u2pre > 0.f ? acc[t] : 0.f;
    }
    __syncthreads();
    if (lane < GL_H) {
        gvm_dotN<KM, GL_H>(U.U2, GL_H, lane, &d2[0][0], GL_H, K, acc);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) d1[t][lane] = tt > 0.f ? acc[t] : 0.f;
    }
    __syncthreads();
    if (lane < GL_E) {
        gvm_dotN<KM, GL_H>(U.U1, GL_H, lane, &d1[0][0], GL_H, K, acc);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) gh_prev[((size_t)t * G.A + a) * GL_E + lane] = acc[t];
    }
    if (lane < GL_H) {
        gvm_dotN<KM, GL_H>(U.U1, GL_H, GL_E + lane, &d1[0][0], GL_H, K, acc);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) gm[t][lane] = acc[t];
    }
    __syncthreads();
    if (lane < GL_H) {
        gvm_dotN<KM, GL_H>(M.W3, GL_H, lane, &gm[0][0], GL_H, K, acc);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) dS[((size_t)t * G.A + a) * GL_H + lane] = acc[t];
    }
}

// End of a backward GNN step t >= 1 (k_gl_gnn_atom_bwd), one wavefront per atom (lanes 0..31: dP, lanes 32..63: dR): the padded
// partners' mask once; per cotangent the pieces in order, dP's padded partners in closed form, the atom's slots in order, then
// gh = gh_prev + the h columns of Wi dP + Wj dR (in place).  pstride: floats of one cotangent's pieces.
template <int KM>
__global__ __launch_bounds__(64) void k_gvm_gnn_atom_bwd(GlPair M, GlGeom G, int K, size_t pstride, size_t SL, const int *inc_off,
                                                         const float *partP, const float *partR, const float *slotP, const float *slotR,
                                                         const float *P, const float *dS, float *gh) {
    __shared__ float v[GL_H], d2[KM][GL_H], dv[2][KM][GL_H];
    if (KM == 1) K = 1;
    const int a = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int b = G.mol_of[a], n = G.moff[b + 1] - G.moff[b];
    const float pa = P[(size_t)a * GL_H + f];
    if (!half) v[f] = fmaxf(pa, 0.f);
    __syncthreads();
    if (!half) {
        const bool on = M.b2[f] + gl_dotT(M.W2, GL_H, f, v) > 0.f;
        for (int t = 0; t < K; ++t) d2[t][f] = on ? dS[((size_t)t * G.A + a) * GL_H + f] : 0.f;
    }
    __syncthreads();
    const float *part = half ? partR : partP, *slot = half ? slotR : slotP;
    const int np = gl_pieces(n);
    float pad[KM];
    if (!half) gvm_dotN<KM, GL_H>(M.W2, GL_H, f, &d2[0][0], GL_H, K, pad);
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) {
            float s = 0.f;
            for (int k = 0; k < np; ++k) s += part[t * pstride + ((size_t)k * G.A + a) * GL_H + f];
            // (one fused multiply-add, as k_gl_gnn_atom_bwd's `s += (N - n) * ...` is compiled: spelt out, so that it does not hang
            // on what the compiler contracts in a loop over cotangents)
            if (!half) s = fmaf((float)(G.N - n), pa > 0.f ? pad[t] : 0.f, s);
            for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += slot[((size_t)t * SL + k) * GL_H + f];
            dv[half][t][f] = s;
        }
    __syncthreads();
    if (lane < GL_E) {
        const int row = G.nx + lane;
        float ai[KM], aj[KM];
        gvm_dotN<KM, GL_H>(M.Wi, GL_H, row, &dv[0][0][0], GL_H, K, ai);
        gvm_dotN<KM, GL_H>(M.Wj, GL_H, row, &dv[1][0][0], GL_H, K, aj);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) gh[((size_t)t * G.A + a) * GL_E + lane] += ai[t] + aj[t];
    }
}

// EPN backward (k_gl_epn_atom_bwd), one wavefront per atom: per cotangent dP / dR from the slots in order, then gfeat += the h columns
// and gq += the q column of Wi dP + Wj dR; the weights pass once.
template <int KM>
__global__ __launch_bounds__(64) void k_gvm_epn_atom_bwd(GlPair M, GlGeom G, int K, size_t SL, const int *inc_off, const float *slotP,
                                                         const float *slotR, float *gfeat, float *gq) {
    __shared__ float dv[2][KM][GL_H];
    if (KM == 1) K = 1;
    const int a = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const float *slot = half ? slotR : slotP;
    for (int t = 0; t < K; ++t) {
        float s = 0.f;
        for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += slot[((size_t)t * SL + k) * GL_H + f];
        dv[half][t][f] = s;
    }
    __syncthreads();
    if (lane <= GL_E) {
        const int row = G.nx + lane;                               // lane 48: the charge's column
        float ai[KM], aj[KM];
        gvm_dotN<KM, GL_H>(M.Wi, GL_H, row, &dv[0][0][0], GL_H, K, ai);
        gvm_dotN<KM, GL_H>(M.Wj, GL_H, row, &dv[1][0][0], GL_H, K, aj);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) {
                const float add = ai[t] + aj[t];
                if (lane < GL_E) gfeat[((size_t)t * G.A + a) * GL_E + lane] += add;
                else gq[(size_t)t * G.A + a] += add;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------- edges -> coordinates
// k_gl_pair_xyz, one thread per listed pair: the image d, D and the 48 channel slopes de_k/dD once in float64; per cotangent
// gD = sum_k gE_k de_k/dD, w = gD / D and the pair's two slots of slotx [K][slots][9].  GEO 0 open, 2 cells.  bad as there.
template <int GEO, int KM>
__global__ __launch_bounds__(256) void k_gvm_pair_xyz(GlPairs L, int npairs, int K, size_t P1, size_t SL, const int *mol_of, const float *xyz,
                                                      const float *geo, const float *gE, double cutoff, double eta, const double *mu,
                                                      double *slotx, int *bad) {
    if (KM == 1) K = 1;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npairs) return;
    const int i = L.pi[p], j = L.pj[p], b = mol_of[i];
    double dx = (double)xyz[3 * j] - (double)xyz[3 * i], dy = (double)xyz[3 * j + 1] - (double)xyz[3 * i + 1],
           dz = (double)xyz[3 * j + 2] - (double)xyz[3 * i + 2];
    PairGeo<GEO> pg;
    pg.load_lane(geo, b);
    pg.image(dx, dy, dz);
    const double D = pair_dist(dx, dy, dz);
    double gD[KM];
#pragma unroll
    for (int t = 0; t < KM; ++t) gD[t] = 0.0;
    const bool in = D > 0.0 && D < cutoff;
    if (!(D > 0.0)) atomicOr(bad, 1);
    else if (D < cutoff) {
        const double C = edge_cut(D, cutoff), dC = edge_dcut(D, cutoff);
        for (int k = 0; k < GL_E; ++k) {
            const double u = D - mu[k];
            const double sl = edge_slope(C, dC, u, eta), ga = edge_gauss(u, eta);
#pragma unroll
            for (int t = 0; t < KM; ++t)
                if (t < K) gD[t] += (double)gE[((size_t)t * P1 + p) * GL_E + k] * sl * ga;
        }
    }
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) { atomicOr(bad, 2); return; }
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) {
            double w = 0.0;
            if (in) w = gD[t] / D;
            double *si = slotx + 9 * ((size_t)t * SL + L.dest_i[p]), *sj = slotx + 9 * ((size_t)t * SL + L.dest_j[p]);
            si[0] = -w * dx; si[1] = -w * dy; si[2] = -w * dz;
            sj[0] = w * dx; sj[1] = w * dy; sj[2] = w * dz;
            const double hw = 0.5 * w;
            const double s6[6] = {hw * dx * dx, hw * dy * dy, hw * dz * dz, hw * dy * dz, hw * dx * dz, hw * dx * dy};
            for (int k = 0; k < 6; ++k) { si[3 + k] = s6[k]; sj[3 + k] = s6[k]; }
        }
}
// k_gl_atom_xyz per (atom, cotangent = blockIdx.y): there is no primal to share, the statement is that kernel's.  gxyz [K][A][3],
// share [K][A][6] float64 or null.
__global__ __launch_bounds__(256) void k_gvm_atom_xyz(int A, size_t SL, const int *inc_off, const double *slotx, float *gxyz, double *share) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    const size_t t = blockIdx.y;
    if (a >= A) return;
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = inc_off[a]; k < inc_off[a + 1]; ++k)
        for (int c = 0; c < 9; ++c) s[c] += slotx[9 * (t * SL + k) + c];
    for (int c = 0; c < 3; ++c) gxyz[3 * (t * A + a) + c] = (float)s[c];
    if (share)
        for (int c = 0; c < 6; ++c) share[6 * (t * A + a) + c] = s[3 + c];
}
// k_g_strain_mol per (molecule, cotangent = blockIdx.y): its lanes, order and butterfly.  strain [K][A][6], out [K][B][3][3].
__global__ __launch_bounds__(64) void k_gvm_strain_mol(int A, const double *strain, const int *moff, float *out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const size_t t = blockIdx.y;
    const int a0 = moff[b], a1 = moff[b + 1];
    double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int a = a0 + lane; a < a1; a += 64)
#pragma unroll
        for (int c = 0; c < 6; ++c) W[c] += strain[6 * (t * A + a) + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double v = W[c];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        W[c] = v;
    }
    if (lane == 0) {
        float *o = out + 9 * (t * gridDim.x + b);
        o[0] = (float)W[0]; o[4] = (float)W[1]; o[8] = (float)W[2];
        o[5] = o[7] = (float)W[3];
        o[2] = o[6] = (float)W[4];
        o[1] = o[3] = (float)W[5];
    }
}
