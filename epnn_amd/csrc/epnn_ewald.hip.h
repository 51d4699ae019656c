// Electrostatics of the predicted charges in fully periodic cells (epnn_coulomb_xyz_cell): the Ewald sum's kernels, beside the open
// call's (epnn_coulomb.hip.h, whose tasks, pieces and g(u) they use).  Part of the one translation unit epnn_api.hip.
//
// Per cell (H its matrix, V = |det H|, Q = sum q_i, beta the splitting parameter; include/epnn.h has the whole sum):
//     real        kappa_s(D) = [e_alpha(D) - erf(beta D)] / D over the minimum image of every pair j != i with D <= rc
//                 (rc <= half the smallest perpendicular width: exactly one image per pair, no atom meets itself)
//     reciprocal  k = 2 pi (m0 g0 + m1 g1 + m2 g2) != 0, |k| <= kc;  c(k) = (4 pi / V) exp(-k^2 / 4 beta^2) / k^2;
//                 S(k) = sum_j q_j exp(i k r_j);  phi_i += sum_k c Re[exp(-i k r_i) S];  ffix_i -= q_i sum_k c k Im[exp(-i k r_i) S]
//     self        phi_i -= 2 beta / sqrt(pi) q_i;      background  phi_i -= pi Q / V (1 / beta^2 - [alpha > 0] / alpha^2)
// all times ke.  The half space m2 > 0, or m2 == 0 and (m1 > 0, or m1 == 0 and m0 > 0), is summed with c doubled.
// k_ew_sweep is k_cl_sweep with the minimum image through the lane's own cell and six more sums per lane, its virial row; k_ew_sfac
// is S(k), one wavefront per (cell, 64 k slots), a slot per lane, the atoms staged through LDS; k_ew_atom is one wavefront per (cell,
// 64 atoms), an atom per lane, the k slots staged through LDS: the reciprocal sums, then what k_cl_atom does; k_ew_energy is one
// wavefront per cell: E and the fixed-charge strain derivative from |S|^2 and the atoms' shares.
// Arithmetic, as in the open sweep: per-pair and per-(atom, k) terms float32 (displacements and phases reduced in float64 and
// rounded once: unwrapped coordinates far from the origin lose nothing), every running sum float64; no float atomics; every output
// word is written by exactly one wavefront and added in a fixed order that depends on the cell alone.
#pragma once
#include "epnn_coulomb.hip.h"
#include "epnn_frontend.hip.h"

#define EW_TILE 64                // k slots per task of k_ew_sfac, atoms per task of k_ew_atom; what either stages in LDS at a time
#define EW_SLOT_CAP (1 << 18)     // most k slots (2 M0 + 1)(2 M1 + 1)(M2 + 1) of one cell
#define EW_PART 10                // sums per (piece, atom) of k_ew_sweep: the open sweep's four and the virial row xx yy zz yz xz xy
#define EW_SHARE 7                // an atom's shares: the energy without its reciprocal part, the real-space strain xx yy zz yz xz xy

// What the device needs of one cell's Ewald parameters (the host's ew_cell_row, from the checked row of the `ewald` argument)
struct EwCell {
    double kc2;                   // kc^2
    double c0;                    // 4 pi / V
    double inv4b2;                // 1 / (4 beta^2)
    double self;                  // 2 beta / sqrt(pi)
    double bg;                    // pi / V (1 / beta^2 - [alpha > 0] / alpha^2)
    float rc, beta;
    int M0, M1, M2;
    int ns;                       // k slots: (2 M0 + 1)(2 M1 + 1)(M2 + 1)
    int soff;                     // the cell's first slot in the batch's slot arrays
    int pad;
};
static_assert(sizeof(EwCell) == 72, "EwCell is staged as 18 words");
static_assert(EW_PART == 10, "cl_sweep_body<., true> and k_cl_excl<., true> write the ten sums of k_ew_sweep's row");

// Slot s of the cell's k box -> (m0, m1, m2), k and the doubled weight 2 c(k); 0 outside the half space or the sphere (and at k = 0)
__device__ __forceinline__ double ew_slot(const EwCell &e, const double *g, int s, int &m0, int &m1, int &m2, double &kx, double &ky, double &kz) {
    const int n0 = 2 * e.M0 + 1, n1 = 2 * e.M1 + 1, t = s / n0;
    m0 = s - t * n0 - e.M0;
    m2 = t / n1;
    m1 = t - m2 * n1 - e.M1;
    const double two_pi = 6.283185307179586, d0 = (double)m0, d1 = (double)m1, d2 = (double)m2;
    kx = two_pi * (d0 * g[0] + d1 * g[3] + d2 * g[6]);
    ky = two_pi * (d0 * g[1] + d1 * g[4] + d2 * g[7]);
    kz = two_pi * (d0 * g[2] + d1 * g[5] + d2 * g[8]);
    const double k2 = kx * kx + ky * ky + kz * kz;
    const bool half = m2 > 0 || (m2 == 0 && (m1 > 0 || (m1 == 0 && m0 > 0)));
    if (!half || k2 > e.kc2) return 0.0;
    return 2.0 * e.c0 * exp(-k2 * e.inv4b2) / k2;
}

// h(u) = erfc(u) + 2 / sqrt(pi) u exp(-u^2) = 1 - g(u): no cancellation at any u
__device__ __forceinline__ float ew_h(float u) { return erfcf(u) + 1.1283791670955126f * u * expf(-u * u); }

// The split pair term of the periodic sweep, cl_pair_term's outputs: kap = kappa_s(D) = de / D, g = gs = g_alpha - g_beta = -D^2 kappa_s'
// and r3 = 1 / D^3, kap and r3 0 at r2 == 0, beyond rc and without use.  The two differences cancel where alpha D and beta D are both large
// (erf -> 1, g -> 1): there they are taken between the complements erfc and h = 1 - g.  MODE CL_WIDTHS: alpha is the pair's gamma_ij.
template <int MODE>
__device__ __forceinline__ void ew_pair_term(bool use, float r2, float alpha, float beta, float rc, float &kap, float &g, float &r3) {
    const float rinv0 = r2 > 0.f ? rsqrtf(r2) : 0.f, D = r2 * rinv0;
    const float rinv = (use && r2 > 0.f && D <= rc) ? rinv0 : 0.f;
    const float ub = beta * D;
    float de;
    if (MODE != CL_BARE) {
        const float ua = alpha * D, um = fminf(ua, ub);
        de = um >= 0.5f ? erfcf(ub) - erfcf(ua) : erff(ua) - erff(ub);
        g = um >= 1.f ? ew_h(ub) - ew_h(ua) : cl_g(ua, erff(ua)) - cl_g(ub, erff(ub));
    } else {
        de = erfcf(ub);
        g = ew_h(ub);
    }
    kap = de * rinv;
    r3 = rinv * rinv * rinv;
}

// task as in k_cl_sweep: cl_sweep_body in this file's geometry.  part [pieces][A][EW_PART] = (sum q_j kappa_s, sum q_j gs dx / D^3, .. dy,
// .. dz, then sum q_j gs d_a d_b / D^3 for ab = xx yy zz yz xz xy).
template <bool ERF>
__global__ __launch_bounds__(64) void k_ew_sweep(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q,
                                                 const EpnnCell *cells, const EwCell *ew, int A, float alpha, double *part, int *bad) {
    cl_sweep_body<ERF ? CL_ERF : CL_BARE, true>(tasks, moff, mol_of, xyz, q, nullptr, cells, ew, A, alpha, part, bad);
}
// the real-space sweep of epnn_coulomb_xyz_cell_site with per-atom widths: gamma_ij for alpha (the host has checked gamma_min >= beta)
__global__ __launch_bounds__(64) void k_ew_sweep_site(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q,
                                                      const float4 *site, const EpnnCell *cells, const EwCell *ew, int A, double *part, int *bad) {
    cl_sweep_body<CL_WIDTHS, true>(tasks, moff, mol_of, xyz, q, site, cells, ew, A, 0.f, part, bad);
}

// The per-cell sum of the site entry's background, one wavefront per cell in the order of k_cl_energy: wsum [B] = sum_j q_j w_j,
// w = 2 sigma^2 (site[j].x; 0 without widths), float64.  (Q is S(k = 0), as in the plain entry.)
__global__ __launch_bounds__(64) void k_ew_wsum(const int *moff, const float *q, const float4 *site, double *wsum) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int a = moff[b] + lane; a < moff[b + 1]; a += 64) v += (double)q[a] * (double)site[a].x;
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) wsum[b] = v;
}

// task = (cell, first slot): S(k) of 64 slots of the cell's k box, a slot per lane, over the cell's atoms in index order.  The
// phase is 2 pi frac(m . s_j): the fractional coordinates s_j = G r_j are reduced in float64 when the atoms are staged, m . s_j again,
// and sincosf sees an angle in [-pi, pi].  S [slots] float64 pairs; rec [slots] = (2 c(k), k) float32, 0 where the slot is not summed.
// The slot of m = 0 is kept (its angle is 0: S = sum_j q_j = Q in float64, which the background term needs).
__global__ __launch_bounds__(64) void k_ew_sfac(const int2 *tasks, const int *moff, const float *xyz, const float *q, const EpnnCell *cells,
                                                const EwCell *ew, double2 *S, float4 *rec) {
    __shared__ double ts[3][EW_TILE];
    __shared__ float tq[EW_TILE];
    const int2 tk = tasks[blockIdx.x];
    const int b = tk.x, lane = threadIdx.x, s = tk.y + lane;
    const EwCell e = ew[b];
    double g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = cells[b].g[k];
    const bool live = s < e.ns;
    int m0 = 0, m1 = 0, m2 = 0;
    double kx = 0.0, ky = 0.0, kz = 0.0, c2 = 0.0;
    if (live) c2 = ew_slot(e, g, s, m0, m1, m2, kx, ky, kz);
    const bool need = live && (c2 != 0.0 || (m0 == 0 && m1 == 0 && m2 == 0));
    const double d0 = (double)m0, d1 = (double)m1, d2 = (double)m2;
    double sr = 0.0, si = 0.0;
    const int lo = moff[b], hi = moff[b + 1];
    if (__any(need))
        for (int t0 = lo; t0 < hi; t0 += EW_TILE) {
            const int cnt = min(EW_TILE, hi - t0);
            __syncthreads();
            if (lane < cnt) {
                const size_t j = (size_t)(t0 + lane);
                const double x = (double)xyz[3 * j], y = (double)xyz[3 * j + 1], z = (double)xyz[3 * j + 2];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double f = g[3 * k] * x + g[3 * k + 1] * y + g[3 * k + 2] * z;
                    ts[k][lane] = f - rint(f);
                }
                tq[lane] = q[j];
            }
            __syncthreads();
            if (need)
                for (int jj = 0; jj < cnt; ++jj) {
                    double t = d0 * ts[0][jj] + d1 * ts[1][jj] + d2 * ts[2][jj];
                    t -= rint(t);
                    float sn, cs;
                    sincosf(6.2831853071795865f * (float)t, &sn, &cs);
                    const float qj = tq[jj];
                    sr += (double)(qj * cs);
                    si += (double)(qj * sn);
                }
        }
    if (live) {
        S[(size_t)e.soff + s] = make_double2(sr, si);
        rec[(size_t)e.soff + s] = make_float4((float)c2, (float)kx, (float)ky, (float)kz);
    }
}

// task = (first atom, atoms, cell, 0): up to 64 atoms of one cell, an atom per lane, over the cell's k slots in slot order (64 staged
// in LDS at a time, read at a wave-uniform address): the reciprocal part of phi and ffix.  Then every atom adds its real-space pieces
// in piece order, the self and background terms, and writes phi [A] (twice: the backward's seed and the output), ffix [A][3] and its
// shares [A][EW_SHARE] in float64: 1/2 q_i (phi_i - its reciprocal part) and -1/2 ke q_i times its virial row.
// X: the listed pairs' row xpart [A][EW_PART] (k_cl_excl) is one more piece, added behind the sweep's: its virial sums take the same 1/2.
// SITE (epnn_coulomb_xyz_cell_site): site [A] = (w = 2 sigma^2, chi, J, gamma_ii; gamma_ii 0 without the self term), wsum [B]:
// W = sum_j q_j w_j.  The background is taken per pair, phi_bg_i = -ke (pi / V) [Q / beta^2 - w_i Q - W] (e.bg is made with alpha = 0
// then); phi gets the Gaussians' self term ke 2 gamma_ii q_i / sqrt(pi); mu = chi + J q + phi goes into the seed and into mu [A], phi
// into phi [A] only; the first share gets q (chi + 1/2 J q) as well.
template <bool X, bool SITE = false>
__device__ __forceinline__ void ew_atom_body(const int4 *tasks, int A, const float *xyz, const float *q, const EpnnCell *cells, const EwCell *ew,
                                             const double2 *S, const float4 *rec, const double *part, const double *xpart, double ke, float *seed,
                                             float *phi, float *ffix, double *share, const float4 *site = nullptr, const double *wsum = nullptr,
                                             float *mu = nullptr) {
    __shared__ double tm[3][EW_TILE];
    __shared__ float4 tr[EW_TILE];
    __shared__ float2 tS[EW_TILE];
    const int4 tk = tasks[blockIdx.x];
    const int lane = threadIdx.x, b = tk.z;
    const bool valid = lane < tk.y;
    const int i = tk.x + (valid ? lane : 0);
    const EwCell e = ew[b];
    double g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = cells[b].g[k];
    double f[3];
    {
        const double x = (double)xyz[3 * (size_t)i], y = (double)xyz[3 * (size_t)i + 1], z = (double)xyz[3 * (size_t)i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = g[3 * k] * x + g[3 * k + 1] * y + g[3 * k + 2] * z;
            f[k] = v - rint(v);
        }
    }
    double pr = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
    for (int s0 = 0; s0 < e.ns; s0 += EW_TILE) {
        const int cnt = min(EW_TILE, e.ns - s0);
        __syncthreads();
        if (lane < cnt) {
            const int s = s0 + lane, n0 = 2 * e.M0 + 1, n1 = 2 * e.M1 + 1, t = s / n0, m2 = t / n1;
            tm[0][lane] = (double)(s - t * n0 - e.M0);
            tm[1][lane] = (double)(t - m2 * n1 - e.M1);
            tm[2][lane] = (double)m2;
            tr[lane] = rec[(size_t)e.soff + s];
            const double2 v = S[(size_t)e.soff + s];
            tS[lane] = make_float2((float)v.x, (float)v.y);
        }
        __syncthreads();
        for (int kk = 0; kk < cnt; ++kk) {
            const float4 r = tr[kk];
            if (r.x == 0.f) continue;                                     // (wave-uniform: outside the half space or the sphere)
            double t = tm[0][kk] * f[0] + tm[1][kk] * f[1] + tm[2][kk] * f[2];
            t -= rint(t);
            float sn, cs;
            sincosf(6.2831853071795865f * (float)t, &sn, &cs);
            const float2 v = tS[kk];
            const float w = r.x * (sn * v.x - cs * v.y);                 // -c Im[exp(-i k r_i) S]: the force is -dE/dr_i
            pr += (double)(r.x * (cs * v.x + sn * v.y));
            fx += (double)(w * r.y);
            fy += (double)(w * r.z);
            fz += (double)(w * r.w);
        }
    }
    if (!valid) return;
    const int np = cl_pieces(tk.w);
    double s[EW_PART];
#pragma unroll
    for (int c = 0; c < EW_PART; ++c) s[c] = 0.0;
    for (int k = 0; k < np; ++k)
#pragma unroll
        for (int c = 0; c < EW_PART; ++c) s[c] += part[((size_t)k * A + i) * EW_PART + c];
    if (X)
#pragma unroll
        for (int c = 0; c < EW_PART; ++c) s[c] += xpart[(size_t)i * EW_PART + c];
    const double qi = (double)q[i], Qs = S[(size_t)e.soff + (size_t)e.M1 * (2 * e.M0 + 1) + e.M0].x;
    double local, onsite = 0.0;
    if constexpr (SITE) {
        const float4 st = site[i];
        const double w = (double)st.x, chi = (double)st.y, J = (double)st.z;
        local = ke * (((s[0] - e.self * qi) - e.bg * Qs) + 0.25 * e.c0 * (w * Qs + wsum[b]) + 1.1283791670955126 * (double)st.w * qi);
        const double p = local + ke * pr;
        phi[i] = (float)p;
        seed[i] = mu[i] = (float)(chi + J * qi + p);
        onsite = qi * (chi + 0.5 * J * qi);
    } else {
        local = ke * ((s[0] - e.self * qi) - e.bg * Qs);
        const double p = local + ke * pr;
        seed[i] = phi[i] = (float)p;
    }
    ffix[3 * (size_t)i] = (float)(ke * qi * (s[1] + fx));
    ffix[3 * (size_t)i + 1] = (float)(ke * qi * (s[2] + fy));
    ffix[3 * (size_t)i + 2] = (float)(ke * qi * (s[3] + fz));
    double *o = share + EW_SHARE * (size_t)i;
    o[0] = SITE ? onsite + 0.5 * qi * local : 0.5 * qi * local;
#pragma unroll
    for (int c = 0; c < 6; ++c) o[1 + c] = -0.5 * ke * qi * s[4 + c];
}
__global__ __launch_bounds__(64) void k_ew_atom(const int4 *tasks, int A, const float *xyz, const float *q, const EpnnCell *cells, const EwCell *ew,
                                                const double2 *S, const float4 *rec, const double *part, double ke, float *seed, float *phi,
                                                float *ffix, double *share) {
    ew_atom_body<false>(tasks, A, xyz, q, cells, ew, S, rec, part, nullptr, ke, seed, phi, ffix, share);
}
__global__ __launch_bounds__(64) void k_ew_atom_x(const int4 *tasks, int A, const float *xyz, const float *q, const EpnnCell *cells, const EwCell *ew,
                                                  const double2 *S, const float4 *rec, const double *part, const double *xpart, double ke,
                                                  float *seed, float *phi, float *ffix, double *share) {
    ew_atom_body<true>(tasks, A, xyz, q, cells, ew, S, rec, part, xpart, ke, seed, phi, ffix, share);
}
// the atoms' kernel of epnn_coulomb_xyz_cell_site; X: with a list
template <bool X>
__global__ __launch_bounds__(64) void k_ew_atom_site(const int4 *tasks, int A, const float *xyz, const float *q, const EpnnCell *cells,
                                                     const EwCell *ew, const double2 *S, const float4 *rec, const double *part, const double *xpart,
                                                     const float4 *site, const double *wsum, double ke, float *seed, float *phi, float *mu,
                                                     float *ffix, double *share) {
    ew_atom_body<X, true>(tasks, A, xyz, q, cells, ew, S, rec, part, xpart, ke, seed, phi, ffix, share, site, wsum, mu);
}

// One wavefront per cell: E = sum of the atoms' shares + E_rec and the fixed-charge strain derivative [3][3] = the atoms' virial shares
// + the reciprocal part - E_bg delta_ab, with E_rec = 1/2 sum_k c |S|^2 and the reciprocal strain 1/2 sum_k c |S|^2 [-delta_ab +
// 2 k_a k_b (1 / k^2 + 1 / 4 beta^2)] over the whole sphere, here the half space with c doubled, in float64 throughout.  Lane l adds
// slots l, l + 64, ... and then atoms l, l + 64, ... in ascending order; a fixed butterfly combines the lanes (k_g_strain_mol's order).
// SITE: E_bg = -ke (pi / 2 V) [Q^2 / beta^2 - 2 Q W], W = wsum [b] (k_ew_wsum): the per-pair background of the site entry.
template <bool SITE>
__device__ __forceinline__ void ew_energy_body(const int *moff, const EpnnCell *cells, const EwCell *ew, const double2 *S, const double *share,
                                               const double *wsum, double ke, double *e_out, float *gs_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const EwCell e = ew[b];
    double g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = cells[b].g[k];
    double W[EW_SHARE] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = lane; s < e.ns; s += 64) {
        int m0, m1, m2;
        double kx, ky, kz;
        const double c2 = ew_slot(e, g, s, m0, m1, m2, kx, ky, kz);
        if (c2 == 0.0) continue;
        const double2 v = S[(size_t)e.soff + s];
        const double w = 0.5 * ke * c2 * (v.x * v.x + v.y * v.y), u = 2.0 * (1.0 / (kx * kx + ky * ky + kz * kz) + e.inv4b2);
        W[0] += w;
        W[1] += w * (u * kx * kx - 1.0); W[2] += w * (u * ky * ky - 1.0); W[3] += w * (u * kz * kz - 1.0);
        W[4] += w * (u * ky * kz); W[5] += w * (u * kx * kz); W[6] += w * (u * kx * ky);
    }
    for (int a = moff[b] + lane; a < moff[b + 1]; a += 64)
#pragma unroll
        for (int c = 0; c < EW_SHARE; ++c) W[c] += share[EW_SHARE * (size_t)a + c];
#pragma unroll
    for (int c = 0; c < EW_SHARE; ++c) {
        double v = W[c];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        W[c] = v;
    }
    if (lane == 0) {
        const double Qs = S[(size_t)e.soff + (size_t)e.M1 * (2 * e.M0 + 1) + e.M0].x;
        double e_bg = -0.5 * ke * e.bg * Qs * Qs;
        if constexpr (SITE) e_bg += 0.25 * ke * e.c0 * Qs * wsum[b];
        e_out[b] = W[0];
        float *o = gs_out + 9 * (size_t)b;
        o[0] = (float)(W[1] - e_bg); o[4] = (float)(W[2] - e_bg); o[8] = (float)(W[3] - e_bg);
        o[5] = o[7] = (float)W[4];
        o[2] = o[6] = (float)W[5];
        o[1] = o[3] = (float)W[6];
    }
}
__global__ __launch_bounds__(64) void k_ew_energy(const int *moff, const EpnnCell *cells, const EwCell *ew, const double2 *S, const double *share,
                                                  double ke, double *e_out, float *gs_out) {
    ew_energy_body<false>(moff, cells, ew, S, share, nullptr, ke, e_out, gs_out);
}
__global__ __launch_bounds__(64) void k_ew_energy_site(const int *moff, const EpnnCell *cells, const EwCell *ew, const double2 *S,
                                                       const double *share, const double *wsum, double ke, double *e_out, float *gs_out) {
    ew_energy_body<true>(moff, cells, ew, S, share, wsum, ke, e_out, gs_out);
}
