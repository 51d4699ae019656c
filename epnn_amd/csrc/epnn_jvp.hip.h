// Forward-mode derivative of the charges (epnn_charges_jvp_xyz_cell, epnn_charges_jvp_multi_xyz_cell): the kernels.  Part of the one
// translation unit epnn_api.hip.
//
// The pair-list gradient path (epnn_grad_large.hip.h) runs the factorised form of DESIGN.md section 2 forward with checkpoints and
// then backwards.  This file runs it forward once with K <= JVM_MAXK tangents beside every row: (h, th), (q, tq), (P, tP), (R, tR),
// (S, tS), and per listed pair (e, te).  Nothing is checkpointed, nothing of size N^2 exists.  tests/jvp_ref.py is the same algebra
// in float64.
//
//   edges                        te [P][48] = de/dD * tD, tD = d'.(v_j - v_i) / D + d'^T E d' / D, float64 per listed pair
//   GNN step t                   projections (k_gl_proj) and their tangents tP = Wi^T ta, tR = Wj^T ta, ta = [0 | th | vQ / n];
//                                tangent all-pairs sweep (k_jvm_sweep, f32 MFMA): S_i and tS_i; listed pairs as correction rows
//                                of both in the incidence slots; per atom the pieces, the (N - n) padded partners in closed form,
//                                the slots, then the update MLP and its tangent
//   EPN step t                   projections of (h_T, q_t) and (th_T, tq_t); listed pairs only, both orders of the pass MLP and of its
//                                tangent, +-w delta and +-w tdelta into the two atoms' slots; every atom adds its slots in order
//
// The primal is the arithmetic of the gradient path's checkpointed forward, expression by expression (the same f32 MFMA sequence
// per partner, the same pieces, slot order and closed-form padded term): q_out has its bits, and every ReLU decision of a tangent
// is taken from the pre-activation and by the comparison the backward kernels use (P > -R, z2pre > 0, z1pre > 0, ...).  The two
// derivative modes are therefore transposes of one another up to float32 rounding of the sums, with no kink between them.
//
// Every tangent buffer is K copies of one tangent's, tangent t at t times that size (te [K][P][48], th [K][A][48], tP, tR [K][A][32],
// partT [K][piece][A][32], slotT [K][slots][32], slott [K][slots], tq [K][A]).  The primal statements and the ReLU decisions stand
// once; the tangent statements are looped over the tangents and none of them reads another tangent, so column t has the same bits
// whatever K and the other columns are.  The single-tangent entry is K = 1 of these kernels.
//
// Plain float32, every sum in a fixed order, no float atomics: bit-reproducible, and a molecule's rows do not depend on the rest
// of the batch.
#pragma once
#include "epnn_grad_large.hip.h"

#define JVM_MAXK 16

// The per-pair and per-atom kernels are templated on KM >= K, the bucket of K (1, 2, 4, 8, 16): registers and LDS are sized for
// it, not for the maximum.  K is uniform over the block, so the guards t < K are scalar branches; in the bucket KM = 1 every
// kernel sets K = 1, the guards fold away and the instantiation is a single-tangent kernel.
//
// acc[t] = sum_k v[t VS + k] W[k][col] for t < K: gl_dotT's fmaf chain per tangent (k ascending, from 0), each weight loaded once,
// acc in registers.  One tangent's 32-long sum is gl_dotT itself: its loop shape, unrolled by 8 beside the primal's, is what keeps
// k_jvm_gnn_tail<1> at 7 waves per SIMD (the loop below, which the compiler unrolls in full, leaves 5: profiles/r14_jvp_one_path.txt).
template <int KM, int VS>
__device__ __forceinline__ void jvm_dotT(const float *W, int stride, int col, const float *v, int n, int K, float (&acc)[KM]) {
    if constexpr (KM == 1)
        if (n == GL_H) { acc[0] = gl_dotT(W, stride, col, v); return; }
#pragma unroll
    for (int t = 0; t < KM; ++t) acc[t] = 0.f;
    for (int k = 0; k < n; ++k) {
        const float w = W[k * stride + col];
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) acc[t] = fmaf(v[t * VS + k], w, acc[t]);
    }
}

// ---------------------------------------------------------------------------------------------------------- edge tangents
// One thread per listed pair, the displacement d' and D in float64 from PairGeo<GEO> and pair_dist, as k_gvm_pair_xyz takes them; d', D
// and de/dD once, tD and te per tangent (tD in LDS, a thread's column; in a register at KM = 1).  v [K][A][3] or null,
// E [K][B][3][3] or null, te [K][P1][48] float32 (te_stride = P1 * 48).  bad: bit 0 = two atoms or images coincide, bit 1 = a pair
// without both incidence slots.
template <int GEO, int KM>
__global__ __launch_bounds__(256) void k_jvm_edge(GlPairs L, int npairs, const int *mol_of, const float *xyz, const float *geo, int K,
                                                  int A, int B, const float *v, const float *E, double cutoff, double eta,
                                                  const double *mu, float *te, size_t te_stride, int *bad) {
    __shared__ double tDs[KM][256];
    double tD1;
    auto tD = [&](int t) -> double & {
        if constexpr (KM == 1) return tD1;
        else return tDs[t][threadIdx.x];
    };
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
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) atomicOr(bad, 2);
    float *row = te + (size_t)p * GL_E;
    if (!(D > 0.0)) atomicOr(bad, 1);
    if (!(D > 0.0) || !(D < cutoff)) {
        for (int t = 0; t < K; ++t)
            for (int k = 0; k < GL_E; ++k) row[t * te_stride + k] = 0.f;
        return;
    }
    for (int t = 0; t < K; ++t) {
        double num = 0.0;
        if (v) {
            const float *vt = v + (size_t)t * A * 3;
            num = dx * ((double)vt[3 * j] - (double)vt[3 * i]) + dy * ((double)vt[3 * j + 1] - (double)vt[3 * i + 1]) +
                  dz * ((double)vt[3 * j + 2] - (double)vt[3 * i + 2]);
        }
        if (E) {
            const float *e = E + 9 * ((size_t)t * B + b);
            const double d[3] = {dx, dy, dz};
            for (int a = 0; a < 3; ++a)
                for (int c = 0; c < 3; ++c) num += d[a] * (double)e[3 * a + c] * d[c];
        }
        tD(t) = num / D;
    }
    const double C = edge_cut(D, cutoff), dC = edge_dcut(D, cutoff);
    for (int k = 0; k < GL_E; ++k) {
        const double u = D - mu[k];
        const double de = edge_slope(C, dC, u, eta) * edge_gauss(u, eta);
        for (int t = 0; t < K; ++t) row[t * te_stride + k] = (float)(de * tD(t));
    }
}

// ---------------------------------------------------------------------------------------------------------- projection tangents
// One wavefront per atom: ta = [0 | th | tq] per tangent (the atom features x are constants), tP = Wi^T ta (lanes 0..31),
// tR = Wj^T ta (lanes 32..63), no bias; the weights pass once.  th [K][A][48] or null (zeros), tq [K][A]; tP, tR [K][A][32].
template <int KM>
__global__ __launch_bounds__(64) void k_jvm_proj(GlPair M, GlGeom G, int K, const float *th, const float *tq, float *tP, float *tR) {
    __shared__ float av[KM][GL_E + 1];
    if (KM == 1) K = 1;
    const int a = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    for (int t = 0; t < K; ++t) {
        if (lane < GL_E) av[t][lane] = th ? th[((size_t)t * G.A + a) * GL_E + lane] : 0.f;
        if (lane == 63) av[t][GL_E] = tq[(size_t)t * G.A + a];
    }
    __syncthreads();
    const float *W = (half ? M.Wj : M.Wi) + (size_t)G.nx * GL_H;
    float acc[KM];
    jvm_dotT<KM, GL_E + 1>(W, GL_H, f, &av[0][0], GL_E + 1, K, acc);
    float *out = half ? tR : tP;
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) out[((size_t)t * G.A + a) * GL_H + f] = acc[t];
}

// ---------------------------------------------------------------------------------------------------------- the tangent sweep
// Tasks, lanes and layout of k_gl_sweep: one wavefront per (16 resident atoms as the columns of an MFMA tile, one piece of their
// molecule's partner range), lane 16 qd + c owns column c and the features 16 rb + 4 qd + r.  A launch carries KC tangents.
// Resident P_i and tP_i per tangent; streamed R_j, Yb_j = b2 + W2^T R_j and tR_j per tangent.  Per partner, all element-wise work
// in front of the MFMAs:
//     z1    = max(P, -R)              m1 = P > -R              tz1 = m1 ? tP + tR : 0        (z1 and m1 once, tz1 per tangent)
//     z2pre = W2^T z1 + Yb            16 MFMAs, k_gl_sweep<0>'s, in its order
//     tz2   = W2^T tz1                16 more per tangent, issued between them (an accumulator pair of its own each)
//     S_i  += relu(z2pre)             tS_i += z2pre > 0 ? tz2 : 0
// outS [piece][A][32], outT the same per tangent: one row per (piece, resident atom), written by exactly one wavefront (an empty
// piece writes zeros).  tP, tR: the chunk's first tangent, the next at tstride floats; outT likewise at ostride.  outS null: the
// primal rows are another launch's to store (every launch needs z2pre for its masks).
template <int KC>
__global__ __launch_bounds__(64) void k_jvm_sweep(const int4 *tasks, const int *moff, int A, const float *W2, const float *P,
                                                  const float *tP, const float *R, const float *Yb, const float *tR, size_t tstride,
                                                  float *outS, float *outT, size_t ostride, int ntask) {
    const int lane = threadIdx.x, c = lane & 15, qd = lane >> 4;
    const int task = blockIdx.x;
    if (task >= ntask) return;
    float wf[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kf = 16 * (s >> 2) + 4 * qd + (s & 3), m = 16 * rb + c;
            wf[rb][s] = W2[kf * GL_H + m];
        }
    const int4 tk = tasks[task];
    const int a0 = moff[tk.y], a1 = moff[tk.y + 1];
    const int len = (a1 - a0 + tk.w - 1) / tk.w;
    const int j0 = min(a0 + tk.z * len, a1), j1 = min(j0 + len, a1);
    const int col = tk.x + c;
    const bool valid = col < a1;
    const int colc = valid ? col : a1 - 1;
    float xr[8], acc[8], tr[KC][8], tacc[KC][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int f = 16 * (e >> 2) + 4 * qd + (e & 3);
        xr[e] = P[(size_t)colc * GL_H + f];
        acc[e] = 0.f;
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            tr[u][e] = tP[u * tstride + (size_t)colc * GL_H + f];
            tacc[u][e] = 0.f;
        }
    }
    for (int j = j0; j < j1; ++j) {
        const float *xs = R + (size_t)j * GL_H + 4 * qd, *ys = Yb + (size_t)j * GL_H + 4 * qd, *ts = tR + (size_t)j * GL_H + 4 * qd;
        const f32x4 n0 = *reinterpret_cast<const f32x4 *>(xs), n1 = *reinterpret_cast<const f32x4 *>(xs + 16);
        f32x4 o0 = *reinterpret_cast<const f32x4 *>(ys), o1 = *reinterpret_cast<const f32x4 *>(ys + 16);
        float nn[8], z1[8], tz[KC][8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { nn[e] = -n0[e]; nn[4 + e] = -n1[e]; }
#pragma unroll
        for (int e = 0; e < 8; ++e) z1[e] = fmaxf(xr[e], nn[e]);
        f32x4 t0[KC], t1[KC];
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            const f32x4 s0 = *reinterpret_cast<const f32x4 *>(ts + u * tstride), s1 = *reinterpret_cast<const f32x4 *>(ts + u * tstride + 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                tz[u][e] = xr[e] > nn[e] ? tr[u][e] + s0[e] : 0.f;
                tz[u][4 + e] = xr[4 + e] > nn[4 + e] ? tr[u][4 + e] + s1[e] : 0.f;
            }
            t0[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            t1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][s], z1[s], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[1][s], z1[s], o1, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < KC; ++u) {
                t0[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[0][s], tz[u][s], t0[u], 0, 0, 0);
                t1[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[1][s], tz[u][s], t1[u], 0, 0, 0);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += fmaxf(o0[e], 0.f);
            acc[4 + e] += fmaxf(o1[e], 0.f);
#pragma unroll
            for (int u = 0; u < KC; ++u) {
                tacc[u][e] += o0[e] > 0.f ? t0[u][e] : 0.f;
                tacc[u][4 + e] += o1[e] > 0.f ? t1[u][e] : 0.f;
            }
        }
    }
    if (valid) {
        const size_t at = ((size_t)tk.z * A + col) * GL_H + 4 * qd;
        if (outS) {
            *reinterpret_cast<f32x4 *>(outS + at) = f32x4{acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f32x4 *>(outS + at + 16) = f32x4{acc[4], acc[5], acc[6], acc[7]};
        }
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            float *t = outT + u * ostride + at;
            *reinterpret_cast<f32x4 *>(t) = f32x4{tacc[u][0], tacc[u][1], tacc[u][2], tacc[u][3]};
            *reinterpret_cast<f32x4 *>(t + 16) = f32x4{tacc[u][4], tacc[u][5], tacc[u][6], tacc[u][7]};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- per listed pair
// Lanes as in k_gl_gnn_pair: one wavefront per listed pair {i < j}, lanes 0..31 the order (i, j), lanes 32..63 the order (j, i),
// a lane one hidden unit.  G = We^T e and tG = We^T te are the same for both orders.
//
// GNN step: the correction rows of S (k_gl_gnn_pair's) and of tS into the first atom's slot: with G the first layer's tangent
// is tP_a + tR_b + tG, without it tP_a + tR_b.  G, the two first-layer rows and their ReLU decisions once; tG, tz1, tz2 per
// tangent.  te [K][P1][48], tP, tR [K][A][32], slotT [K][SL][32].
template <int KM>
__global__ __launch_bounds__(64) void k_jvm_gnn_pair(GlPair M, GlPairs L, int K, int A, size_t P1, size_t SL, const float *te, const float *P,
                                                     const float *R, const float *tP, const float *tR, float *slotS, float *slotT) {
    __shared__ float ev[GL_E], tv[KM][GL_E], z[2][2][GL_H], tz[KM][2][2][GL_H];
    if (KM == 1) K = 1;
    const int p = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int i = L.pi[p], j = L.pj[p];
    const int a = half ? j : i, b = half ? i : j;
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) return;               // (flagged by k_jvm_edge: write nothing)
    if (lane < GL_E) {
        ev[lane] = L.pe[(size_t)p * GL_E + lane];
        for (int t = 0; t < K; ++t) tv[t][lane] = te[((size_t)t * P1 + p) * GL_E + lane];
    }
    __syncthreads();
    float g = 0.f, tg[KM];
    for (int k = 0; k < GL_E; ++k) g = fmaf(ev[k], M.We[k * GL_H + f], g);
    jvm_dotT<KM, GL_E>(M.We, GL_H, f, &tv[0][0], GL_E, K, tg);
    const float base = P[(size_t)a * GL_H + f] + R[(size_t)b * GL_H + f];
    const float z1g = base + g;
    z[half][0][f] = fmaxf(z1g, 0.f);
    z[half][1][f] = fmaxf(base, 0.f);
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) {
            const float tb = tP[((size_t)t * A + a) * GL_H + f] + tR[((size_t)t * A + b) * GL_H + f];
            tz[t][half][0][f] = z1g > 0.f ? tb + tg[t] : 0.f;
            tz[t][half][1][f] = base > 0.f ? tb : 0.f;
        }
    __syncthreads();
    const float z2g = M.b2[f] + gl_dotT(M.W2, GL_H, f, z[half][0]), z2n = M.b2[f] + gl_dotT(M.W2, GL_H, f, z[half][1]);
    float t2g[KM], t2n[KM];
    jvm_dotT<KM, 4 * GL_H>(M.W2, GL_H, f, &tz[0][half][0][0], GL_H, K, t2g);
    jvm_dotT<KM, 4 * GL_H>(M.W2, GL_H, f, &tz[0][half][1][0], GL_H, K, t2n);
    const int sa = half ? L.dest_j[p] : L.dest_i[p];
    slotS[(size_t)sa * GL_H + f] = fmaxf(z2g, 0.f) - fmaxf(z2n, 0.f);
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) slotT[((size_t)t * SL + sa) * GL_H + f] = (z2g > 0.f ? t2g[t] : 0.f) - (z2n > 0.f ? t2n[t] : 0.f);
}

// EPN step: delta = (f(a_i, a_j, e) - f(a_j, a_i, e)) / 2 as k_gl_epn_pair forms it, once, and per tangent
// tf = W3 . ([z2pre > 0] W2^T ([z1pre > 0] (tP_a + tR_b + tG))), tdelta = (tf_ij - tf_ji) / 2; w delta, w tdelta into the first
// atom's slots and their negatives into the second's.  slott [K][SL].
template <int KM>
__global__ __launch_bounds__(64) void k_jvm_epn_pair(GlPair M, GlPairs L, int K, int A, size_t P1, size_t SL, const float *te, const float *P,
                                                     const float *R, const float *tP, const float *tR, float *slotq, float *slott) {
    __shared__ float ev[GL_E], tv[KM][GL_E], z[2][GL_H], tz[KM][2][GL_H], red[2][GL_H], tred[KM][2][GL_H];
    if (KM == 1) K = 1;
    const int p = blockIdx.x, lane = threadIdx.x, half = lane >> 5, f = lane & 31;
    const int i = L.pi[p], j = L.pj[p];
    const int a = half ? j : i, b = half ? i : j;
    if (L.dest_i[p] < 0 || L.dest_j[p] < 0) return;
    if (lane < GL_E) {
        ev[lane] = L.pe[(size_t)p * GL_E + lane];
        for (int t = 0; t < K; ++t) tv[t][lane] = te[((size_t)t * P1 + p) * GL_E + lane];
    }
    __syncthreads();
    float g = 0.f, tg[KM];
    for (int k = 0; k < GL_E; ++k) g = fmaf(ev[k], M.We[k * GL_H + f], g);
    jvm_dotT<KM, GL_E>(M.We, GL_H, f, &tv[0][0], GL_E, K, tg);
    const float z1 = P[(size_t)a * GL_H + f] + R[(size_t)b * GL_H + f] + g;
    z[half][f] = fmaxf(z1, 0.f);
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) tz[t][half][f] = z1 > 0.f ? tP[((size_t)t * A + a) * GL_H + f] + tR[((size_t)t * A + b) * GL_H + f] + tg[t] : 0.f;
    __syncthreads();
    const float z2 = M.b2[f] + gl_dotT(M.W2, GL_H, f, z[half]);
    float d2[KM];
    jvm_dotT<KM, 2 * GL_H>(M.W2, GL_H, f, &tz[0][half][0], GL_H, K, d2);
    const float w = L.pw[p];
    const int sa = half ? L.dest_j[p] : L.dest_i[p];
    red[half][f] = fmaxf(z2, 0.f) * M.W3[f];
#pragma unroll
    for (int t = 0; t < KM; ++t)
        if (t < K) {
            const float t2 = z2 > 0.f ? d2[t] : 0.f;
            tred[t][half][f] = t2 * M.W3[f];
        }
    __syncthreads();
    if (f == 0) {
        float fi = 0.f, fj = 0.f;                                   // (b3 cancels in the difference)
        for (int k = 0; k < GL_H; ++k) { fi += red[0][k]; fj += red[1][k]; }
        const float delta = 0.5f * (fi - fj);
        slotq[sa] = half ? -(w * delta) : w * delta;
        for (int t = 0; t < K; ++t) {
            float ti = 0.f, tj = 0.f;
            for (int k = 0; k < GL_H; ++k) { ti += tred[t][0][k]; tj += tred[t][1][k]; }
            const float tdelta = 0.5f * (ti - tj);
            slott[(size_t)t * SL + sa] = half ? -(w * tdelta) : w * tdelta;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- per atom
// End of a GNN step, one wavefront per atom.  Primal: k_gl_gnn_tail's statements.  Per tangent: tS = pieces in order +
// (N - n) [W2^T relu(P) + b2 > 0] W2^T ([P > 0] tP) + the atom's slots in order; tM = W3^T tS; the update MLP's tangent on
// [th | tM] with the ReLU decisions of its pre-activations.  tpart [K][maxp][A][32] (tp_stride = maxp * A * 32),
// tcorr [K][SL][32], tP [K][A][32], th, th_out [K][A][48].
template <int KM>
__global__ __launch_bounds__(64) void k_jvm_gnn_tail(GlPair M, GlUpd U, GlGeom G, int K, size_t tp_stride, size_t SL, const int *inc_off,
                                                     const float *part, const float *tpart, const float *corr, const float *tcorr,
                                                     const float *P, const float *tP, const float *h, const float *th, float *h_out,
                                                     float *th_out) {
    __shared__ float v[GL_H], u0[GL_E + GL_H], u1[GL_H], u2[GL_H];
    __shared__ float tv[KM][GL_H], tu0[KM][GL_E + GL_H], tu1[KM][GL_H], tu2[KM][GL_H];
    if (KM == 1) K = 1;
    const int a = blockIdx.x, lane = threadIdx.x;
    const int b = G.mol_of[a], n = G.moff[b + 1] - G.moff[b];
    if (lane < GL_H) {
        const float pa = P[(size_t)a * GL_H + lane];
        v[lane] = fmaxf(pa, 0.f);
        for (int t = 0; t < K; ++t) tv[t][lane] = pa > 0.f ? tP[((size_t)t * G.A + a) * GL_H + lane] : 0.f;
    }
    if (lane < GL_E) {
        u0[lane] = h ? h[(size_t)a * GL_E + lane] : 0.f;
        for (int t = 0; t < K; ++t) tu0[t][lane] = th ? th[((size_t)t * G.A + a) * GL_E + lane] : 0.f;
    }
    __syncthreads();
    float d[KM];
    if (lane < GL_H) {
        float s = 0.f;
        const int np = gl_pieces(n);
        for (int k = 0; k < np; ++k) s += part[((size_t)k * G.A + a) * GL_H + lane];
        const float zp = M.b2[lane] + gl_dotT(M.W2, GL_H, lane, v);
        s += (float)(G.N - n) * fmaxf(zp, 0.f);
        for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) s += corr[(size_t)k * GL_H + lane];
        u1[lane] = s;
        jvm_dotT<KM, GL_H>(M.W2, GL_H, lane, &tv[0][0], GL_H, K, d);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) {
                float ts = 0.f;
                for (int k = 0; k < np; ++k) ts += tpart[t * tp_stride + ((size_t)k * G.A + a) * GL_H + lane];
                ts += (float)(G.N - n) * (zp > 0.f ? d[t] : 0.f);
                for (int k = inc_off[a]; k < inc_off[a + 1]; ++k) ts += tcorr[((size_t)t * SL + k) * GL_H + lane];
                tu1[t][lane] = ts;
            }
    }
    __syncthreads();
    if (lane < GL_H) {
        u0[GL_E + lane] = (float)G.N * M.b3[lane] + gl_dotT(M.W3, GL_H, lane, u1);
        jvm_dotT<KM, GL_H>(M.W3, GL_H, lane, &tu1[0][0], GL_H, K, d);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) tu0[t][GL_E + lane] = d[t];
    }
    __syncthreads();
    float t1 = 0.f;
    if (lane < GL_H) {
        t1 = U.c1[lane];
        for (int k = 0; k < GL_E + GL_H; ++k) t1 = fmaf(u0[k], U.U1[k * GL_H + lane], t1);
        jvm_dotT<KM, GL_E + GL_H>(U.U1, GL_H, lane, &tu0[0][0], GL_E + GL_H, K, d);
    }
    __syncthreads();
    if (lane < GL_H) {
        u1[lane] = fmaxf(t1, 0.f);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) tu1[t][lane] = t1 > 0.f ? d[t] : 0.f;
    }
    __syncthreads();
    if (lane < GL_H) {
        const float u2pre = U.c2[lane] + gl_dotT(U.U2, GL_H, lane, u1);
        u2[lane] = fmaxf(u2pre, 0.f);
        jvm_dotT<KM, GL_H>(U.U2, GL_H, lane, &tu1[0][0], GL_H, K, d);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) tu2[t][lane] = u2pre > 0.f ? d[t] : 0.f;
    }
    __syncthreads();
    if (lane < GL_E) {
        h_out[(size_t)a * GL_E + lane] = U.c3[lane] + gl_dotT(U.U3, GL_E, lane, u2);
        jvm_dotT<KM, GL_H>(U.U3, GL_E, lane, &tu2[0][0], GL_H, K, d);
#pragma unroll
        for (int t = 0; t < KM; ++t)
            if (t < K) th_out[((size_t)t * G.A + a) * GL_E + lane] = d[t];
    }
}

// The tangents of the charges before the first EPN step, vQ / n per tangent (k_gl_q0's statement): vQ [K][B], tq [K][A].
__global__ __launch_bounds__(256) void k_jvm_q0(GlGeom G, int K, int B, const float *vQ, float *tq) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= G.A) return;
    const int b = G.mol_of[a];
    const float n = (float)(G.moff[b + 1] - G.moff[b]);
    for (int t = 0; t < K; ++t) tq[(size_t)t * G.A + a] = vQ[(size_t)t * B + b] / n;
}
// End of an EPN step, k_gl_epn_atom on the primal row and on the K slot rows: slott [K][SL], tq, tq_out [K][A].
__global__ __launch_bounds__(256) void k_jvm_epn_atom(int A, int K, size_t SL, const int *inc_off, const float *slotq, const float *q,
                                                      float *q_out, const float *slott, const float *tq, float *tq_out) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const int k0 = inc_off[a], k1 = inc_off[a + 1];
    float s = q[a];
    for (int k = k0; k < k1; ++k) s += slotq[k];
    q_out[a] = s;
    for (int t = 0; t < K; ++t) {
        float ts = tq[(size_t)t * A + a];
        for (int k = k0; k < k1; ++k) ts += slott[(size_t)t * SL + k];
        tq_out[(size_t)t * A + a] = ts;
    }
}
