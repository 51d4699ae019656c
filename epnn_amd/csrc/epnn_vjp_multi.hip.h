// The backward of the pair-list path, for K cotangents in one pass: the kernels.  Part of the one translation unit epnn_api.hip.
//
// The pair-list gradient path (epnn_grad_large.hip.h: the structures, the checkpointed forward and the all-pairs sweep k_gl_sweep) runs
// its forward and then a backward that is linear in the seed g, with every ReLU decision taken from the primal alone.  This file is
// that backward for K <= GVM_MAXK seeds beside the one primal: the kernels below recompute a pair's or an atom's primal
// pre-activations and masks once and then loop over the cotangents.  It is the only one: epnn_charges_vjp_xyz*, every Coulomb entry
// and the training step run it at K = 1 (gl_grad_backward, train_step_large_impl), epnn_charges_vjp_multi_xyz_cell at its K.
//
//   k_gvm_epn_pair, k_gvm_epn_atom_bwd            the EPN stack, t = T-1 .. 0
//   k_gvm_upd_bwd                                 the update MLP
//   k_gl_sweep<1, KC>, <2, KC>                    the two all-pairs backward sweeps (epnn_grad_large.hip.h), KC cotangents per launch
//   k_gvm_gnn_pair, k_gvm_gnn_atom_bwd            the listed pairs' correction rows and the end of a GNN step; step 0 keeps the
//                                                 shortcut: only gE of the listed pairs
//   k_gvm_pair_xyz<GEO>, k_gvm_atom_xyz, k_gvm_strain_mol     edges -> coordinates and strain (the dense path's k_g_strain_mol per
//                                                 cotangent); box rows at K = 1 only: the multi entry takes cells
//
// Every cotangent buffer is K copies of one cotangent's, cotangent t at t times that size (gq [K][A], gh, ghp [K][A][48], dS
// [K][A][32], partP, partR [K][piece][A][32], slotP, slotR [K][slots][32], gE [K][P][48], slotx [K][slots][9] float64, share
// [K][A][6] float64, gxyz [K][A][3], gstrain [K][B][9]).  Each cotangent statement is one fmaf chain or MFMA sequence: accumulators
// from zero, k ascending, pieces and slots added in the same order; none reads another cotangent.  Row t therefore has the same bits
// whatever K, the row's position and the other rows are: those of a K = 1 call for g[t] alone.
//
// TAPE (KM == 1 only; a training step, epnn_train_large.hip.h): the kernel also stores the rows the weight gradients are outer
// products of into the GlTape; the pair kernels then store dz and write no gE.  Other instances do not read the tape argument.
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

// ---------------------------------------------------------------------------------------------------------- per listed pair
// One wavefront per listed pair, lanes and halves as in the forward's k_gl_gnn_pair / k_gl_epn_pair.  SL: slots of one cotangent
// (2 P1); A, P1: atoms and pair rows of one cotangent.
//
// (Eight wavefronts per SIMD are asked for at KM == 1: the gradient call's instances then take 63 / 64 VGPRs instead of 65 / 66.  The
// taped GNN instance would spill under that bound and keeps 65; the buckets above 1 compile as without the hint.)
//
// GNN step: G, z1 with and without G and the two z2 pre-activations once; per cotangent dz1 with G minus dz1
// without it into slotP of the first and slotR of the second atom (null for step 0) and gE_ij += We (dz1_ij + dz1_ji) with G.
template <int KM, bool TAPE = false>
__global__ __launch_bounds__(64, KM == 1 && !TAPE ? 8 : 1) void k_gvm_gnn_pair(GlPair M, GlPairs L, int K, int A, size_t P1, size_t SL,
                                                                               const float *P, const float *R, const float *dS, float *slotP,
                                                                               float *slotR, float *gE, GlTape tp) {
    static_assert(!TAPE || KM == 1, "a training step has one cotangent");
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
    if (TAPE) {
        const size_t r = (4 * (size_t)p + 2 * half) * GL_H + f;
        tp.z1[r] = z[half][0][f]; tp.z1[r + GL_H] = z[half][1][f];
        tp.d2[r] = d2[half][0][0][f]; tp.d2[r + GL_H] = -d2[half][1][0][f];
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
    if (TAPE) {                                                   // (a training step: the We block's rows, no gE)
        if (lane < GL_H) tp.dz[(size_t)p * GL_H + lane] = dg[0][0][lane] + dg[1][0][lane];
        return;
    }
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

// EPN step: G, z1 and z2 once; per cotangent the row [a_i | a_j | e] is seeded with s = w (gq_i - gq_j) / 2, the
// row [a_j | a_i | e] with -s; a row's dz1 goes to slotP of its first atom and slotR of its second, and gE_ij += We (dz1_ij + dz1_ji).
template <int KM, bool TAPE = false>
__global__ __launch_bounds__(64, KM == 1 && !TAPE ? 8 : 1) void k_gvm_epn_pair(GlPair M, GlPairs L, int K, int A, size_t P1, size_t SL,
                                                                               const float *P, const float *R, const float *gq, float *slotP,
                                                                               float *slotR, float *gE, GlTape tp) {
    static_assert(!TAPE || KM == 1, "a training step has one cotangent");
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
        if (TAPE) {
            const size_t r = (2 * (size_t)p + half) * GL_H + f;
            tp.z1[r] = z[half][f];
            tp.d2[r] = d2[half][t][f];
            tp.r3[r] = fmaxf(z2, 0.f) * (half ? -seed : seed);
        }
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
    if (TAPE) {
        if (lane < GL_H) tp.dz[(size_t)p * GL_H + lane] = dg[0][0][lane] + dg[1][0][lane];
        return;
    }
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
// Backward of the update MLP, one wavefront per atom: u0, u1pre and u2pre from the checkpoints (h, S) once; per
// cotangent gh [48] is carried back: gh_prev [K][A][48] = the h columns of the first layer's input gradient, dS [K][A][32] = W3 (its
// M columns).
template <int KM, bool TAPE = false>
__global__ __launch_bounds__(64) void k_gvm_upd_bwd(GlPair M, GlUpd U, GlGeom G, int K, const float *h, const float *S, const float *gh,
                                                    float *gh_prev, float *dS, GlTape tp) {
    static_assert(!TAPE || KM == 1, "a training step has one cotangent");
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
        if (TAPE) tp.u2[(size_t)a * GL_H + lane] = fmaxf(u2pre, 0.f);
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
    if (TAPE) {
        tp.u0[(size_t)a * (GL_E + GL_H) + lane] = u0[lane];
        if (lane < GL_E + GL_H - 64) tp.u0[(size_t)a * (GL_E + GL_H) + 64 + lane] = u0[64 + lane];
        if (lane < GL_H) {
            const size_t r = (size_t)a * GL_H + lane;
            tp.u1[r] = u1[lane]; tp.ud2[r] = d2[0][lane]; tp.ud1[r] = d1[0][lane]; tp.gm[r] = gm[0][lane];
        }
    }
    if (lane < GL_H) {
        gvm_dotN<KM, GL_H>(M.W3, GL_H, lane, &gm[0][0], GL_H, K, acc);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) dS[((size_t)t * G.A + a) * GL_H + lane] = acc[t];
    }
}

// End of a backward GNN step t >= 1, one wavefront per atom (lanes 0..31: dP, lanes 32..63: dR): the padded
// partners' mask once; per cotangent the pieces in order, dP's padded partners in closed form, the atom's slots in order, then
// gh = gh_prev + the h columns of Wi dP + Wj dR (in place).  pstride: floats of one cotangent's pieces.
template <int KM, bool TAPE = false>
__global__ __launch_bounds__(64) void k_gvm_gnn_atom_bwd(GlPair M, GlGeom G, int K, size_t pstride, size_t SL, const int *inc_off,
                                                         const float *partP, const float *partR, const float *slotP, const float *slotR,
                                                         const float *P, const float *dS, float *gh, GlTape tp) {
    static_assert(!TAPE || KM == 1, "a training step has one cotangent");
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
            // (one fused multiply-add, spelt out: the same bits whatever the compiler contracts in a loop over cotangents)
            if (!half) s = fmaf((float)(G.N - n), pa > 0.f ? pad[t] : 0.f, s);
            for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += slot[((size_t)t * SL + k) * GL_H + f];
            dv[half][t][f] = s;
            if (TAPE) {
                tp.dv[(size_t)a * 64 + lane] = s;
                if (!half) {
                    tp.z1[(tp.pad0 + a) * GL_H + f] = v[f];
                    tp.d2[(tp.pad0 + a) * GL_H + f] = (float)(G.N - n) * d2[0][f];
                }
            }
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

// EPN backward, one wavefront per atom: per cotangent dP / dR from the slots in order, then gfeat += the h columns
// and gq += the q column of Wi dP + Wj dR; the weights pass once.
template <int KM, bool TAPE = false>
__global__ __launch_bounds__(64) void k_gvm_epn_atom_bwd(GlPair M, GlGeom G, int K, size_t SL, const int *inc_off, const float *slotP,
                                                         const float *slotR, float *gfeat, float *gq, GlTape tp) {
    static_assert(!TAPE || KM == 1, "a training step has one cotangent");
    __shared__ float dv[2][KM][GL_H];
    if (KM == 1) K = 1;
    const int a = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const float *slot = half ? slotR : slotP;
    for (int t = 0; t < K; ++t) {
        float s = 0.f;
        for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += slot[((size_t)t * SL + k) * GL_H + f];
        dv[half][t][f] = s;
        if (TAPE) tp.dv[(size_t)a * 64 + lane] = s;
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
// One thread per listed pair: the displacement d = image of r_j - r_i and D in float64 as the front-end measures them (PairGeo<GEO>,
// pair_dist: GEO 0 open, 1 box rows [B][3], 2 EpnnCell records [B]) and the 48 channel slopes de_k/dD once; per cotangent
// gD = sum_k gE_k de_k/dD, w = gD / D; the first atom's slot gets -w d, the second's +w d (d D / d r_i = (r_i - r_j) / D), and each
// gets half of w d_a d_c (xx, yy, zz, yz, xz, xy) for the strain.  slotx [K][slots][9] float64.  bad: bit 0 = two atoms or images
// coincide, bit 1 = a pair without both slots (atomicOr: the word does not depend on which thread comes last).
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
// Per (atom, cotangent = blockIdx.y): the atom adds its slots in order, in float64: gxyz [K][A][3] float32, and its strain share
// [K][A][6] float64 (k_gvm_strain_mol adds a molecule's atoms up) or null.
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
