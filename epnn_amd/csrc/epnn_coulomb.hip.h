// Electrostatics of the predicted charges (epnn_coulomb_xyz): the kernels.  Part of the one translation unit epnn_api.hip.
//
// Per molecule, over its real atoms only (open systems: no cell, no images):
//     kappa(D) = 1 / D  (alpha == 0)   or   erf(alpha D) / D  (alpha > 0)
//     phi_i    = ke sum_{j != i} q_j kappa(D_ij)
//     ffix_i   = -ke q_i sum_{j != i} q_j kappa'(D_ij) (r_i - r_j) / D_ij        kappa' = -g(alpha D) / D^2,
//                g = 1 (alpha == 0),  g(u) = erf(u) - 2 / sqrt(pi) u exp(-u^2) (alpha > 0)
//     E_b      = 1/2 sum_i q_i phi_i
// k_cl_sweep is the all-pairs part: one wavefront per task = (up to 64 atoms, one per lane; one piece of a partner range), the
// partners staged 64 at a time in LDS and read at a wave-uniform address (a broadcast).  A molecule above 64 atoms is cut into
// blocks of 64 atoms times cl_pieces(n) pieces of its partner range; molecules of up to 64 atoms are packed whole, several to a
// wavefront, and every lane skips the partners of the other molecules.  Either way a lane meets the partners of its own molecule
// in index order, and the number of pieces depends on the molecule's size alone: a molecule's rows do not depend on the batch.
// Arithmetic: the displacement is the float64 difference of the float32 coordinates rounded once (exact far from the origin);
// the per-pair terms are float32 (one reciprocal square root, plus erff and expf or a short series when alpha > 0); every running
// sum is float64.  part [pieces][A][4] = (sum q_j kappa, sum q_j g dx / D^3, .. dy .., .. dz ..) is written by exactly one wavefront
// per (piece, atom); k_cl_atom adds an atom's pieces in piece order and k_cl_energy a molecule's atoms, as k_g_strain_mol does.
// No atomics on floats; the only atomic is the OR into the coincident-atoms flag.
#pragma once
#include "epnn_host.h"
#include "epnn_pair_geo.hip.h"

#define CL_BLOCK 64               // atoms of a task: one per lane
#define CL_TILE 64                // partners staged in LDS at a time: one per lane
#define CL_MINPIECE 128           // a partner range is not cut into pieces shorter than this ...
#define CL_MAXP 32                // ... nor into more pieces than this
#define CL_WANT 2048              // wavefronts a single molecule should bring

// pieces of the partner range of a molecule of n atoms: enough for CL_WANT wavefronts, within the two limits above
__host__ __device__ __forceinline__ int cl_pieces(int n) {
    if (n <= CL_BLOCK) return 1;
    const int blocks = (n + CL_BLOCK - 1) / CL_BLOCK, want = (CL_WANT + blocks - 1) / blocks, cap = (n + CL_MINPIECE - 1) / CL_MINPIECE;
    const int np = want < cap ? want : cap;
    return np < 1 ? 1 : (np > CL_MAXP ? CL_MAXP : np);
}

// g(u) = erf(u) - 2 / sqrt(pi) u exp(-u^2), erf_u = erf(u).  Below 1 the two terms cancel (g ~ 4 / (3 sqrt(pi)) u^3): the series
// 2 / sqrt(pi) sum_{k >= 1} (-1)^(k + 1) 2 k / ((2 k + 1) k!) u^(2 k + 1), whose 12th term is below 5e-9 of the sum at u = 1.
__device__ __forceinline__ float cl_g(float u, float erf_u) {
    const float two_rpi = 1.1283791670955126f;
    if (u >= 1.f) return erf_u - two_rpi * u * expf(-u * u);
    const float w = u * u;
    float s = 22.f / 918086400.f;
    s = fmaf(s, w, -20.f / 76204800.f);
    s = fmaf(s, w, 18.f / 6894720.f);
    s = fmaf(s, w, -16.f / 685440.f);
    s = fmaf(s, w, 14.f / 75600.f);
    s = fmaf(s, w, -12.f / 9360.f);
    s = fmaf(s, w, 10.f / 1320.f);
    s = fmaf(s, w, -8.f / 216.f);
    s = fmaf(s, w, 6.f / 42.f);
    s = fmaf(s, w, -4.f / 10.f);
    s = fmaf(s, w, 2.f / 3.f);
    return two_rpi * (u * w) * s;
}

// The pair-term modes of the sweeps and of k_cl_excl, a template parameter: bare 1 / D, erf(alpha D) / D with the call's one alpha, and
// erf(gamma_ij D) / D with gamma_ij = 1 / sqrt(w_i + w_j) from the atoms' own w = 2 sigma^2 (the _site entries' per-atom widths).
enum ClMode { CL_BARE = 0, CL_ERF = 1, CL_WIDTHS = 2 };
// gamma_ij of the widths mode; every other mode takes the call's alpha as it is
template <int MODE>
__device__ __forceinline__ float cl_pair_alpha(float alpha, float wi, float wj) {
    if constexpr (MODE == CL_WIDTHS) return rsqrtf(wi + wj);
    else return alpha;
}

// The float32 pair term of the open sweep and of k_cl_excl, from the squared length r2 of the rounded displacement: kap = kappa(D),
// g = g(alpha D) and r3 = 1 / D^3; kap and r3 are 0 at r2 == 0 and for a pair that does not count (use: k_cl_excl counts every one).
// MODE CL_WIDTHS: alpha is the pair's gamma_ij (cl_pair_alpha), and the term is that of CL_ERF.
template <int MODE>
__device__ __forceinline__ void cl_pair_term(bool use, float r2, float alpha, float &kap, float &g, float &r3) {
    const float rinv = (use && r2 > 0.f) ? rsqrtf(r2) : 0.f;
    g = 1.f;
    kap = rinv;
    if (MODE != CL_BARE) {
        const float u = alpha * (r2 * rinv), e = erff(u);
        kap = e * rinv;
        g = cl_g(u, e);
    }
    r3 = rinv * rinv * rinv;
}
// (the periodic sweep's pair term, with the same outputs: epnn_ewald.hip.h, beside ew_h)
template <int MODE>
__device__ __forceinline__ void ew_pair_term(bool use, float r2, float alpha, float beta, float rc, float &kap, float &g, float &r3);

// The sweep of both geometries.  task = (first atom, atoms | piece << 8, first partner, end of the partners); atoms and partners are flat
// atom indices.  CELL: the displacement goes through the minimum image of the lane's own cell, the pair term is the split one inside
// rc (EW: EwCell, of which the open file knows only that it has rc and beta) and six more sums follow the open sweep's four, the virial
// row xx yy zz yz xz xy: part [pieces][A][NS].  MODE CL_WIDTHS: site [A] = (2 sigma^2, chi, J, gamma_ii) per atom, of which the sweep takes
// the first word: the lane holds its own w_i, the partners' w_j are staged beside tq, and gamma_ij = rsqrtf(w_i + w_j) stands for alpha.
template <int MODE, bool CELL, class EW>
__device__ __forceinline__ void cl_sweep_body(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q,
                                              const float4 *site, const EpnnCell *cells, const EW *ew, int A, float alpha, double *part,
                                              int *bad) {
    constexpr int NS = CELL ? 10 : 4;                            // (10: EW_PART, asserted in epnn_ewald.hip.h)
    constexpr bool WID = MODE == CL_WIDTHS;
    __shared__ double tx[CL_TILE], ty[CL_TILE], tz[CL_TILE];
    __shared__ float tq[CL_TILE];
    __shared__ float tw[WID ? CL_TILE : 1];
    const int4 tk = tasks[blockIdx.x];
    const int lane = threadIdx.x, na = tk.y & 255, piece = tk.y >> 8;
    const bool valid = lane < na;
    const int i = tk.x + (valid ? lane : 0);
    const int b = mol_of[i], lo = moff[b], hi = moff[b + 1];
    PairGeo<CELL ? 2 : 0> pg;
    pg.load_lane(cells, b);                                      // (packed molecules: b differs between the lanes)
    float rc = 0.f, beta = 0.f;
    if constexpr (CELL) {
        rc = ew[b].rc;
        beta = ew[b].beta;
    }
    const double xi = (double)xyz[3 * (size_t)i], yi = (double)xyz[3 * (size_t)i + 1], zi = (double)xyz[3 * (size_t)i + 2];
    float wi = 0.f;
    if constexpr (WID) wi = site[i].x;
    double sum[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) sum[c] = 0.0;
    bool hit = false;
    for (int t0 = tk.z; t0 < tk.w; t0 += CL_TILE) {
        const int cnt = min(CL_TILE, tk.w - t0);
        __syncthreads();
        if (lane < cnt) {
            const size_t j = (size_t)(t0 + lane);
            tx[lane] = (double)xyz[3 * j]; ty[lane] = (double)xyz[3 * j + 1]; tz[lane] = (double)xyz[3 * j + 2];
            tq[lane] = q[j];
            if constexpr (WID) tw[lane] = site[j].x;
        }
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
            const int j = t0 + jj;
            double ex = xi - tx[jj], ey = yi - ty[jj], ez = zi - tz[jj];
            pg.image(ex, ey, ez);
            const float dx = (float)ex, dy = (float)ey, dz = (float)ez, qj = tq[jj];
            const float r2 = dx * dx + dy * dy + dz * dz;
            const bool use = valid && j != i && j >= lo && j < hi;        // the self term goes by index
            hit |= use && r2 == 0.f;
            float kap, gg, r3;
            const float al = cl_pair_alpha<MODE>(alpha, wi, WID ? tw[jj] : 0.f);
            if constexpr (CELL) ew_pair_term<MODE>(use, r2, al, beta, rc, kap, gg, r3);
            else cl_pair_term<MODE>(use, r2, al, kap, gg, r3);
            const float s = qj * gg * r3;
            const float fx = s * dx, fy = s * dy, fz = s * dz;
            sum[0] += (double)(qj * kap);
            sum[1] += (double)fx;
            sum[2] += (double)fy;
            sum[3] += (double)fz;
            if (CELL) {
                sum[4] += (double)(fx * dx);
                sum[5] += (double)(fy * dy);
                sum[6] += (double)(fz * dz);
                sum[7] += (double)(fy * dz);
                sum[8] += (double)(fx * dz);
                sum[9] += (double)(fx * dy);
            }
        }
    }
    if (valid) {
        double *o = part + ((size_t)piece * A + i) * NS;
#pragma unroll
        for (int c = 0; c < NS; ++c) o[c] = sum[c];
    }
    if (hit) atomicOr(bad, 1);
}
template <bool ERF>
__global__ __launch_bounds__(64) void k_cl_sweep(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q, int A,
                                                 float alpha, double *part, int *bad) {
    cl_sweep_body<ERF ? CL_ERF : CL_BARE, false, void>(tasks, moff, mol_of, xyz, q, nullptr, nullptr, nullptr, A, alpha, part, bad);
}
// the sweep of epnn_coulomb_xyz_site with per-atom widths
__global__ __launch_bounds__(64) void k_cl_sweep_site(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q,
                                                      const float4 *site, int A, double *part, int *bad) {
    cl_sweep_body<CL_WIDTHS, false, void>(tasks, moff, mol_of, xyz, q, site, nullptr, nullptr, A, 0.f, part, bad);
}

// every atom adds its pieces in piece order: phi [A] (float32, written twice: the backward's seed and the output), ffix [A][3],
// and its share of the energy, 1/2 q_i phi_i, in float64.  X: the listed pairs' row xpart [A][4] (k_cl_excl) is one more piece, added last.
// SITE (epnn_coulomb_xyz_site): site [A] = (2 sigma^2, chi, J, gamma_ii; gamma_ii 0 without the self term).  phi gets the self term
// ke 2 gamma_ii q_i / sqrt(pi); mu = chi + J q + phi goes into the seed and into mu [A], phi into phi [A] only; the share is
// q (chi + 1/2 J q) + 1/2 q phi.
template <bool X, bool SITE = false>
__device__ __forceinline__ void cl_atom_body(int A, const int *moff, const int *mol_of, const float *q, const double *part, const double *xpart,
                                             double ke, float *seed, float *phi, float *ffix, double *share, const float4 *site = nullptr,
                                             float *mu = nullptr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A) return;
    const int b = mol_of[i], np = cl_pieces(moff[b + 1] - moff[b]);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < np; ++k)
        for (int c = 0; c < 4; ++c) s[c] += part[((size_t)k * A + i) * 4 + c];
    if (X)
        for (int c = 0; c < 4; ++c) s[c] += xpart[(size_t)i * 4 + c];
    const double qi = (double)q[i];
    if constexpr (SITE) {
        const float4 st = site[i];
        const double p = ke * (s[0] + 1.1283791670955126 * (double)st.w * qi), chi = (double)st.y, J = (double)st.z;
        phi[i] = (float)p;
        seed[i] = mu[i] = (float)(chi + J * qi + p);
        for (int c = 0; c < 3; ++c) ffix[3 * (size_t)i + c] = (float)(ke * qi * s[1 + c]);
        share[i] = qi * (chi + 0.5 * J * qi) + 0.5 * qi * p;
    } else {
        const double p = ke * s[0];
        seed[i] = phi[i] = (float)p;
        for (int c = 0; c < 3; ++c) ffix[3 * (size_t)i + c] = (float)(ke * qi * s[1 + c]);
        share[i] = 0.5 * qi * p;
    }
}
__global__ __launch_bounds__(256) void k_cl_atom(int A, const int *moff, const int *mol_of, const float *q, const double *part, double ke,
                                                 float *seed, float *phi, float *ffix, double *share) {
    cl_atom_body<false>(A, moff, mol_of, q, part, nullptr, ke, seed, phi, ffix, share);
}
__global__ __launch_bounds__(256) void k_cl_atom_x(int A, const int *moff, const int *mol_of, const float *q, const double *part,
                                                   const double *xpart, double ke, float *seed, float *phi, float *ffix, double *share) {
    cl_atom_body<true>(A, moff, mol_of, q, part, xpart, ke, seed, phi, ffix, share);
}
// the atoms' kernel of epnn_coulomb_xyz_site; xpart NULL: no list
template <bool X>
__global__ __launch_bounds__(256) void k_cl_atom_site(int A, const int *moff, const int *mol_of, const float *q, const double *part,
                                                      const double *xpart, const float4 *site, double ke, float *seed, float *phi, float *mu,
                                                      float *ffix, double *share) {
    cl_atom_body<X, true>(A, moff, mol_of, q, part, xpart, ke, seed, phi, ffix, share, site, mu);
}

// E_b: a molecule's shares, lane by lane in atom order, then across the lanes (the order of k_g_strain_mol)
__global__ __launch_bounds__(64) void k_cl_energy(const double *share, const int *moff, double *e_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int a = moff[b] + lane; a < moff[b + 1]; a += 64) v += share[a];
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) e_out[b] = v;
}

// ---- bonded exclusions and pair scaling (epnn_coulomb_xyz_excl, epnn_coulomb_xyz_cell_excl): a listed pair counts with weight s instead
// of 1, so the sweep's full term stays and (s - 1) times the same term is added.  The list arrives as a CSR by atom (the host's
// excl_build): row_off [A + 1], partner [2 P] sorted within a row, factor [2 P] = s - 1 in float32, every pair in both directions.
#define CL_XPART 4                // sums per atom of the open correction; the periodic one has EW_PART, with the virial row
#define CL_FLAG_ZERO 1            // flag word, bit 0: two atoms at distance 0 (the sweeps set it too)
#define CL_FLAG_FAR 2             // bit 1: a listed pair of a cell beyond half the smallest perpendicular width

// One atom per lane, 64 atoms per wavefront; a lane walks its CSR row in partner order.  Displacement: the float64 difference of the
// float32 coordinates, through the cell's image (PairGeo) when CELL, rounded once.  Sums float64: xpart [A][4] = (sum f q_j kappa, sum f q_j g dx /
// D^3, .. dy, .. dz), f the row's factor; CELL: xpart [A][10], the six virial sums f q_j g d_a d_b / D^3 (xx yy zz yz xz xy) behind
// them, in the order of the periodic sweep's row.  Each word is written by exactly one lane; the only atomic is the OR into the flag word.
// cells: the batch's EpnnCell records (CELL), from which every lane takes half the smallest width, 1 / (2 max_k |g_k|).
// MODE: the pair term's (ClMode); CL_WIDTHS reads w_i and w_j from site [A] as the sweep does.
template <int MODE, bool CELL>
__global__ __launch_bounds__(64) void k_cl_excl(int A, const int *mol_of, const float *xyz, const float *q, const int *row_off, const int *partner,
                                                const float *factor, const EpnnCell *cells, const float4 *site, float alpha, double *xpart,
                                                int *bad) {
    constexpr int NS = CELL ? 10 : CL_XPART;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A) return;
    PairGeo<CELL ? 2 : 0> pg;
    float half_w = 0.f;
    if constexpr (CELL) {
        pg.load_lane(cells, mol_of[i]);
        double g2 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k += 3) g2 = fmax(g2, pg.g[k] * pg.g[k] + pg.g[k + 1] * pg.g[k + 1] + pg.g[k + 2] * pg.g[k + 2]);
        half_w = (float)(0.5 / sqrt(g2));
    }
    const double xi = (double)xyz[3 * (size_t)i], yi = (double)xyz[3 * (size_t)i + 1], zi = (double)xyz[3 * (size_t)i + 2];
    float wi = 0.f;
    if constexpr (MODE == CL_WIDTHS) wi = site[i].x;
    double sum[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) sum[c] = 0.0;
    int flag = 0;
    for (int k = row_off[i], k1 = row_off[i + 1]; k < k1; ++k) {
        const size_t j = (size_t)partner[k];
        const float fac = factor[k], qj = q[j];
        double ex = xi - (double)xyz[3 * j], ey = yi - (double)xyz[3 * j + 1], ez = zi - (double)xyz[3 * j + 2];
        pg.image(ex, ey, ez);
        const float dx = (float)ex, dy = (float)ey, dz = (float)ez;
        const float r2 = dx * dx + dy * dy + dz * dz;
        if (r2 == 0.f) flag |= CL_FLAG_ZERO;
        if (CELL && r2 > half_w * half_w) flag |= CL_FLAG_FAR;
        float kap, gg, r3;
        float wj = 0.f;
        if constexpr (MODE == CL_WIDTHS) wj = site[j].x;
        cl_pair_term<MODE>(true, r2, cl_pair_alpha<MODE>(alpha, wi, wj), kap, gg, r3);
        const float s = qj * (gg * r3);                                   // (the sweep multiplies from the left: (q_j g) / D^3)
        const float fx = fac * (s * dx), fy = fac * (s * dy), fz = fac * (s * dz);
        sum[0] += (double)(fac * (qj * kap));
        sum[1] += (double)fx;
        sum[2] += (double)fy;
        sum[3] += (double)fz;
        if (CELL) {
            sum[4] += (double)(fx * dx);
            sum[5] += (double)(fy * dy);
            sum[6] += (double)(fz * dz);
            sum[7] += (double)(fy * dz);
            sum[8] += (double)(fx * dz);
            sum[9] += (double)(fx * dy);
        }
    }
    double *o = xpart + (size_t)i * NS;
#pragma unroll
    for (int c = 0; c < NS; ++c) o[c] = sum[c];
    if (flag) atomicOr(bad, flag);
}
