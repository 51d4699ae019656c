// Charge gradients with respect to the atom coordinates (epnn_charges_vjp_xyz): the kernels.
// Part of the one translation unit epnn_api.hip.
//
// The train path's forward + backward (epnn_train.hip.h, epnn_train_fused.hip.h) runs with its loss seed replaced by a
// cotangent g of the charges.  Its backward already forms, for every sweep, the gradient at the first Dense's input rows
// [a_i | a_j | e_ij]; the columns of e_ij are summed here into gE [B][N][N][48] (T message and T pass sweeps, both orders of
// a pass sweep), and gE is carried back through get_init_edges (charge_gn.py:122-163) to the coordinates:
//     e_ijk = C(D) exp(-eta (D - mu_k)^2),  C(D) = (cos(pi D / cutoff) + 1) / 2 for D < cutoff, else 0
//     gD_ij = sum_k gE_ijk de_k/dD                                   (double, from the float32 coordinates, as the forward)
//     gxyz_i = sum_j (gD_ij + gD_ji) (r_i - r_j) / D_ij
// The pair masks (is_near, the node mask) are constants, as TensorFlow's autodiff treats comparisons.  C'(cutoff) = 0: the
// derivative is continuous there.  Every sum has a fixed order and no atomics: the result is bit-reproducible and does not
// depend on the other molecules of a batch.
#pragma once
#include "epnn_host.h"
#include "epnn_pair_geo.hip.h"
#include "epnn_train_fused.hip.h"

struct TrainState;
struct XyzGrad {                 // a forward + backward of the train path that ends in gE instead of weight gradients
    TrainState *ts;              // its own parameter copy and scratch (the training state is not touched)
    const float *yseed;          // [B][N] -g / 2: the loss seed -2 (y - pred), read with pred = 0, is exactly g
    float *zero;                 // [B][N] zeros
    float *gE;                   // [B][N][N][48] += gradient with respect to the edge features
    const int *real;             // [B][N] the slot holds a real atom
};

// layer-by-layer path: dX [R][D] of a first Dense holds the edge columns at 2F..2F+48: gE += them (real pairs)
__global__ __launch_bounds__(256) void k_g_edge_dx(const float *dX, float *gE, int R, int D, int off, int N, const int *real) {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < R * 48; idx += gridDim.x * 256) {
        const int r = idx / 48, k = idx - r * 48;
        const int j = r % N, bi = r / N, b = bi / N;
        if (real[bi] && real[b * N + j]) gE[idx] += dX[(size_t)r * D + off + k];
    }
}

// row-fused path: gE[r][k] += sum_d sum_o dz1[d][r][o] W1[2F + k][o] on v_mfma_f32_16x16x4_f32.  A wavefront owns 16 pair
// rows and the 48 channels (three 16-column tiles); the K dimension (o, 32) is taken in the order o = 8 (lane >> 4) + s, s =
// 0..7, so that a lane's eight values of a row and of a weight column are two float4 loads each.  Lane l: A[row l & 15][kk =
// l >> 4], B[kk][col l & 15], D[row 4 (l >> 4) + reg][col l & 15].  Rows of padded atoms (never written by the sweep) are read
// as zeros.
__global__ __launch_bounds__(256) void k_g_edge_dz1(const float *dz1, const float *W1e, float *gE, int R, int ND, size_t dstride,
                                                    int N, const int *real) {
    const int lane = threadIdx.x & 63, lr = lane & 15, q = lane >> 4;
    f32x4 wb[3][2];
#pragma unroll
    for (int ct = 0; ct < 3; ++ct)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) wb[ct][hh] = tm_ld4u(W1e + (16 * ct + lr) * 32 + 8 * q + 4 * hh);     // (parameter offsets: 4-byte aligned)
    const int ntiles = (R + 15) / 16;
    for (int tile = blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += gridDim.x * 4) {
        const int r0 = tile * 16;
        const int ra = r0 + lr;
        bool ok = ra < R;
        if (ok) {
            const int bi = ra / N, j = ra - bi * N, b = bi / N;
            ok = real[bi] && real[b * N + j];
        }
        f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int d = 0; d < ND; ++d) {
            f32x4 a[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            if (ok) {
                const float *p = dz1 + d * dstride + (size_t)ra * 32 + 8 * q;
                a[0] = *reinterpret_cast<const f32x4 *>(p);
                a[1] = *reinterpret_cast<const f32x4 *>(p + 4);
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s >> 2][s & 3], wb[ct][s >> 2][s & 3], acc[ct], 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = r0 + 4 * q + reg;
            if (r >= R) continue;
            const int bi = r / N, j = r - bi * N, b = bi / N;
            if (!real[bi] || !real[b * N + j]) continue;
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) gE[(size_t)r * 48 + 16 * ct + lr] += acc[ct][reg];
        }
    }
}

// Edge-featurisation backward: one wavefront per real atom (a = moff[b] + i).  Lane j (and j + 64, ...) forms the pair (i, j):
// the image and D as every path measures them (epnn_pair_geo.hip.h), gD_ij + gD_ji over the 48 channels, and its contribution
// (gD_ij + gD_ji) (r_i - r_j) / D; the lanes' sums are combined by a fixed butterfly.  bad: set when two atoms of a molecule
// coincide (D = 0: the distance has no derivative there).  GEO (GeoKind) 1: minimum-image displacements in the box rows geo [B][3]
// (their derivative is that of the unwrapped displacement: the image shift is a constant); 2: in the EpnnCell records geo [B].
// Strain derivative (GEO 2, strain != null): under r -> (1 + eps) r, a_k -> (1 + eps) a_k every image displacement d' becomes
// (1 + eps) d', so dD/d eps_ac = d'_a d'_c / D and, with F = sum_i g_i q_i,
//     dF/d eps_ac = sum over pairs i < j with D < cutoff of (gD_ij + gD_ji) d'_a d'_c / D.
// This wavefront sees each of its atom's pairs, the partner's wavefront sees them again: the atom's share is half the sum over its
// partners, kept in float64 as strain[a][xx, yy, zz, yz, xz, xy]; k_g_strain_mol adds a molecule's atoms up.
template <int GEO>
__global__ __launch_bounds__(64) void k_g_xyz(const float *xyz, const int *moff, int B, int N, const float *gE, double cutoff, double eta,
                                              const double *mu, float *gxyz, int *bad, const float *geo, double *strain) {
    const int a = blockIdx.x, lane = threadIdx.x;
    int lo = 0, hi = B;                               // molecule b: moff[b] <= a < moff[b + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (moff[mid] <= a) lo = mid; else hi = mid;
    }
    const int b = lo, a0 = moff[b], n = moff[b + 1] - a0, i = a - a0;
    const double xi = xyz[3 * a], yi = xyz[3 * a + 1], zi = xyz[3 * a + 2];
    PairGeo<GEO> pg;
    pg.load_uniform(geo, b);
    double s[3] = {0.0, 0.0, 0.0};
    double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < n; j += 64) {
        if (j == i) continue;
        const int aj = a0 + j;
        double dx = (double)xyz[3 * aj] - xi, dy = (double)xyz[3 * aj + 1] - yi, dz = (double)xyz[3 * aj + 2] - zi;
        pg.image(dx, dy, dz);
        const double D = pair_dist(dx, dy, dz);
        if (!(D > 0.0)) { *bad = 1; continue; }
        if (D >= cutoff) continue;                    // C = 0 and C' = 0 beyond the cutoff
        const double C = edge_cut(D, cutoff), dC = edge_dcut(D, cutoff);
        const float *gij = gE + (((size_t)b * N + i) * N + j) * 48, *gji = gE + (((size_t)b * N + j) * N + i) * 48;
        double gD = 0.0;
        for (int k = 0; k < 48; ++k) {
            const double u = D - mu[k];
            gD += ((double)gij[k] + (double)gji[k]) * edge_slope(C, dC, u, eta) * edge_gauss(u, eta);
        }
        const double w = gD / D;                      // d D_ij / d r_i = (r_i - r_j) / D
        s[0] -= w * dx;
        s[1] -= w * dy;
        s[2] -= w * dz;
        if (GEO == 2 && strain) {
            const double hw = 0.5 * w;
            W[0] += hw * dx * dx; W[1] += hw * dy * dy; W[2] += hw * dz * dz;
            W[3] += hw * dy * dz; W[4] += hw * dx * dz; W[5] += hw * dx * dy;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v = s[c];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        s[c] = v;
    }
    if (lane < 3) gxyz[3 * a + lane] = (float)(lane == 0 ? s[0] : (lane == 1 ? s[1] : s[2]));
    if (GEO == 2 && strain) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = W[c];
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
            if (lane == 0) strain[6 * (size_t)a + c] = v;
        }
    }
}
template __global__ decltype(k_g_xyz<0>) k_g_xyz<0>;              // (here, in this order: the device listing keeps the kernels' places)
template __global__ decltype(k_g_xyz<1>) k_g_xyz<1>;
template __global__ decltype(k_g_xyz<2>) k_g_xyz<2>;
// The per-atom strain shares of k_g_xyz<2> summed per molecule, one wavefront each: lane l adds atoms l, l + 64, ... of the
// molecule in ascending order, a fixed butterfly combines the lanes (no atomics: bit-reproducible, and a molecule's result does not
// depend on the rest of the batch).  out [B][3][3] float32, the full symmetric matrix.
__global__ __launch_bounds__(64) void k_g_strain_mol(const double *strain, const int *moff, float *out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int a0 = moff[b], a1 = moff[b + 1];
    double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int a = a0 + lane; a < a1; a += 64)
#pragma unroll
        for (int c = 0; c < 6; ++c) W[c] += strain[6 * (size_t)a + c];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double v = W[c];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        W[c] = v;
    }
    if (lane == 0) {
        float *o = out + 9 * (size_t)b;
        o[0] = (float)W[0]; o[4] = (float)W[1]; o[8] = (float)W[2];
        o[5] = o[7] = (float)W[3];
        o[2] = o[6] = (float)W[4];
        o[1] = o[3] = (float)W[5];
    }
}
