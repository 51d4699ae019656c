// Electrostatics of the predicted charges in slab cells, two periodic axes and one open one (epnn_coulomb_xyz_slab): the kernels of
// the exact two-dimensional Ewald sum, beside the periodic call's (epnn_ewald.hip.h, whose real-space sweep k_ew_sweep runs unchanged:
// its image already handles a zero row).  Part of the one translation unit epnn_api.hip.
//
// Per cell (a, b the periodic rows, A = |a x b|, nhat = a x b / A, d_ij = r_i - r_j, z = nhat . d_ij, beta the splitting parameter,
// u = k / 2 beta; include/epnn.h has the whole sum):
//     reciprocal  k = 2 pi (m0 g_a + m1 g_b) != 0, |k| <= kc:  F+ = e^{kz} erfc(u + beta z), F- = e^{-kz} erfc(u - beta z)
//                 phi_i  += sum_k (pi / A k) sum_j q_j cos(k . d_ij) [F+ + F-]                       (j == i included)
//                 ffix_i += q_i sum_k (pi / A k) sum_j q_j { k sin(k . d_ij) [F+ + F-] - nhat k cos(k . d_ij) [F+ - F-] }
//     k = 0       phi_i  -= (2 sqrt(pi) / A) sum_j q_j [exp(-beta^2 z^2) / beta + sqrt(pi) z erf(beta z)]
//                 ffix_i += q_i nhat (2 pi / A) sum_j q_j erf(beta z)
// all times ke.  The half plane m1 > 0, or m1 == 0 and m0 > 0, is summed with the weight doubled; the host lists its slots inside kc
// per cell, in float64 (SlSlot), with exp(-u^2) folded into the weight.
// F+-: with Fa the one of the two whose erfc argument is u + beta |z| and Fb the other,
//     Fa = exp(-u^2) exp(-beta^2 z^2) erfcx(u + beta |z|)                                     (no overflow, no cancellation)
//     Fb = exp(-u^2) exp(-beta^2 z^2) erfcx(u - beta |z|)                                     where u >= beta |z|
//        = 2 exp(-k |z|) - exp(-u^2) exp(-beta^2 z^2) erfcx(beta |z| - u)                     otherwise (the second term is at most half the first)
// and F+ + F- = Fa + Fb, F+ - F- = sign(z) (Fa - Fb).
// k_sl_sweep is the all-pairs part in which every pair meets every k slot: the open sweep's tasks (64 atoms a wavefront, one per lane;
// pieces of the partner range; small cells packed, several to a wavefront), the partners staged 64 at a time in LDS and the cell's
// slots likewise, both read at a wave-uniform address.  k_sl_atom adds an atom's pieces, as k_ew_atom does.
// Arithmetic: per pair z, the two fractional differences and exp(-beta^2 z^2) are float64; per (pair, slot) the phase
// 2 pi frac(m0 f0 + m1 f1) and the two erfc arguments are taken in float64 and rounded once, everything behind them is float32
// (sincosf, erfcxf, expf, the products); the five running sums of a lane are float64: phi, the in-plane force's three components and
// the force along nhat, which takes its vector in float64 in k_sl_atom.  No float atomics; every output word is written by exactly
// one wavefront, in an order that depends on the cell alone.
//
// The strain derivative (epnn_coulomb_xyz_slab_strain; the formulas are in include/epnn.h): the reciprocal and k = 0 sums have no
// structure factor, so their strain rides in the all-pairs sweep.  sl_sweep_body<STRAIN> is the one body: k_sl_sweep is its `false`
// instance, the statements of the plain call, and k_sl_sweep_strain its `true` instance with six more float64 sums per lane, in the
// basis of the slot integers (Cartesian would take ten: 1 + 3 + 6; four more float64 adds per term and eight more registers, for an
// expansion that the atoms' kernel does once per atom; 113 VGPRs against the plain instance's 93, nothing spilled):
//     [5]      sum_j q_j z_ij { sum_k (w k) cos Fd - (2 pi / A) erf(beta z_ij) }                       the z-weighted force along nhat
//     [6], [7] sum_j q_j z_ij sum_k w sin Fs (m0, m1)                                                  the z-weighted in-plane force
//     [8..10]  sum_j q_j sum_k w cos [Fs / k + |z| (Fb - Fa) + G] / k (m0^2, m0 m1, m1^2)              the k_a k_b tensor
// with G = 2 / (beta sqrt(pi)) exp(-beta^2 z^2) (exp(-u^2) is in w), the three terms of the bracket of one sign.  Per (pair, slot) these
// are float32 products of values already there; z_ij is rounded once from float64.  k_sl_atom_strain expands them through g_a, g_b
// and nhat in float64, k = 2 pi (m0 g_a + m1 g_b), and adds the virial row of k_ew_sweep and of the listed pairs; k_sl_energy_strain
// adds a cell's atoms.
#pragma once
#include "epnn_ewald.hip.h"

#define SL_TILE 64                // partners, and k slots, staged in LDS at a time
#define SL_SLOT_CAP (1 << 16)     // most slots (2 M0' + 1)(M1' + 1) of one cell's k box (M0', M1': the M of its two periodic rows)
#define SL_PART 5                 // sums per (piece, atom) of k_sl_sweep: phi, the in-plane force x y z, the force along nhat (its sign turned)
#define SL_PART_STRAIN 11         // of k_sl_sweep_strain: those five, then the six sums of the strain derivative (above)
#define SL_SHARE_W 6              // an atom's strain shares xx yy zz yz xz xy

// What the device needs of one slab cell (the host's sl_cell_row, from the checked row of the `ewald` argument)
struct SlCell {
    double ga[3], gb[3];          // the dual vectors of the two periodic rows (EpnnCell.g of those rows)
    double nh[3];                 // nhat
    double beta;
    double c0;                    // 2 sqrt(pi) / A
    double cn;                    // 2 pi / A
    double self;                  // 2 beta / sqrt(pi)
    int ns;                       // the cell's listed slots: the half plane inside kc
    int soff;                     // the first of them in the batch's slot array
};
static_assert(sizeof(SlCell) == 112, "SlCell is staged as 28 words");
// One k slot of a cell's half plane, made by the host in float64
struct SlSlot {
    double m0, m1;                // the slot's integers along the two periodic rows
    double k, u;                  // |k| and k / 2 beta
    float w, wk;                  // the doubled weight 2 pi / (A k) exp(-u^2), and k times it
    float kx, ky, kz;             // the vector k
    float ik;                     // 1 / |k| (the strain sweep's)
};
static_assert(sizeof(SlSlot) == 56, "SlSlot is staged as 14 words");

// an atom's two fractional coordinates along the periodic rows, reduced, and its height nhat . r, in float64
__device__ __forceinline__ void sl_coords(const SlCell &e, const float *p, double &s0, double &s1, double &zn) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double a = e.ga[0] * x + e.ga[1] * y + e.ga[2] * z, b = e.gb[0] * x + e.gb[1] * y + e.gb[2] * z;
    s0 = a - rint(a);
    s1 = b - rint(b);
    zn = e.nh[0] * x + e.nh[1] * y + e.nh[2] * z;
}

// task as in k_cl_sweep = (first atom, atoms | piece << 8, first partner, end of the partners).  A packed task holds several cells: they
// are taken one after another, each with its own slots, and a lane adds only while its own cell is the one in turn.  A lane meets
// (partner tile, slot tile, partner, slot) in that order; the tiles start at the piece's (or the cell's) first partner and at slot 0.
// rpart [pieces][A][SL_PART], without q_i and ke.  STRAIN: [pieces][A][SL_PART_STRAIN], the five sums by the same statements and the
// six of the strain derivative behind them (the top of this file).
template <bool STRAIN>
__device__ __forceinline__ void sl_sweep_body(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q,
                                              const SlCell *sl, const SlSlot *slots, int A, double *rpart) {
    constexpr int NS = STRAIN ? SL_PART_STRAIN : SL_PART;
    __shared__ double ts0[SL_TILE], ts1[SL_TILE], tz[SL_TILE];
    __shared__ float tq[SL_TILE];
    __shared__ SlSlot tslot[SL_TILE];
    const int4 tk = tasks[blockIdx.x];
    const int lane = threadIdx.x, na = tk.y & 255, piece = tk.y >> 8;
    const bool valid = lane < na;
    const int i = tk.x + (valid ? lane : 0);
    const int b = mol_of[i];
    double sum[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) sum[c] = 0.0;
    const int c_first = tk.w > tk.z ? mol_of[tk.z] : 0, c_last = tk.w > tk.z ? mol_of[tk.w - 1] : -1;
    for (int c = c_first; c <= c_last; ++c) {                    // (wave-uniform)
        const SlCell e = sl[c];
        const bool mine = valid && b == c;
        const int p0 = max(tk.z, moff[c]), p1 = min(tk.w, moff[c + 1]);
        double si0, si1, zi;
        sl_coords(e, xyz + 3 * (size_t)i, si0, si1, zi);         // (a lane of another cell: finite numbers that are not used)
        const float invb = (float)(1.0 / e.beta), c0 = (float)e.c0, cn = (float)e.cn;
        const float cg = STRAIN ? (float)(1.1283791670955126 / e.beta) : 0.f;         // 2 / (beta sqrt(pi)): the Gaussian term of dFs/dk
        for (int t0 = p0; t0 < p1; t0 += SL_TILE) {
            const int cnt = min(SL_TILE, p1 - t0);
            __syncthreads();
            if (lane < cnt) {
                const size_t j = (size_t)(t0 + lane);
                sl_coords(e, xyz + 3 * j, ts0[lane], ts1[lane], tz[lane]);
                tq[lane] = q[j];
            }
            __syncthreads();
            if (mine)                                            // k = 0: once per pair
                for (int jj = 0; jj < cnt; ++jj) {
                    const double dz = zi - tz[jj], az = fabs(dz), bzd = e.beta * az;
                    const float qj = tq[jj], eg = (float)exp(-bzd * bzd), er = erff((float)bzd);
                    sum[0] -= (double)((c0 * qj) * (eg * invb + 1.7724538509055160f * ((float)az * er)));
                    sum[4] -= (double)((cn * qj) * (dz < 0.0 ? -er : er));
                    if (STRAIN) sum[5] -= (double)(((cn * qj) * er) * (float)az);         // z erf(beta z) = |z| erf(beta |z|)
                }
            for (int s0 = 0; s0 < e.ns; s0 += SL_TILE) {
                const int scnt = min(SL_TILE, e.ns - s0);
                __syncthreads();
                if (lane < scnt) tslot[lane] = slots[(size_t)e.soff + s0 + lane];
                __syncthreads();
                for (int jj = 0; mine && jj < cnt; ++jj) {
                    const double dz = zi - tz[jj], f0 = si0 - ts0[jj], f1 = si1 - ts1[jj], az = fabs(dz), bzd = e.beta * az;
                    const float qj = tq[jj], eg = (float)exp(-bzd * bzd), sg = dz < 0.0 ? -1.f : 1.f;
                    const float zf = STRAIN ? (float)dz : 0.f, azf = STRAIN ? (float)az : 0.f, ge = STRAIN ? cg * eg : 0.f;
                    for (int kk = 0; kk < scnt; ++kk) {
                        const SlSlot &r = tslot[kk];
                        double t = r.m0 * f0 + r.m1 * f1;
                        t -= rint(t);
                        float sn, cs;
                        sincosf(6.2831853071795865f * (float)t, &sn, &cs);
                        const double amd = r.u - bzd;
                        const float Fa = eg * erfcxf((float)(r.u + bzd));
                        float Fb = eg * erfcxf((float)fabs(amd));
                        if (amd < 0.0) {                                  // 2 exp(u^2 - k |z|) - ...: the exponent in float64, split in two
                            const double x = r.k * az - r.u * r.u;
                            const float xh = (float)x, xl = (float)(x - (double)xh);
                            Fb = 2.f * (expf(-xh) * (1.f - xl)) - Fb;
                        }
                        const float wq = r.w * qj, Fs = Fa + Fb, Fd = sg * (Fa - Fb);
                        const float a = (wq * sn) * Fs;
                        sum[0] += (double)((wq * cs) * Fs);
                        sum[1] += (double)(a * r.kx);
                        sum[2] += (double)(a * r.ky);
                        sum[3] += (double)(a * r.kz);
                        sum[4] += (double)(((r.wk * qj) * cs) * Fd);
                        if (STRAIN) {
                            const float m0 = (float)r.m0, m1 = (float)r.m1;         // (integers: exact)
                            const float pz = a * zf;
                            sum[5] += (double)((((r.wk * qj) * cs) * Fd) * zf);
                            sum[6] += (double)(pz * m0);
                            sum[7] += (double)(pz * m1);
                            // Fs / k^2 - (dFs/dk) / k = [Fs / k + |z| (Fb - Fa) + G] / k, three terms of one sign (Fa <= Fb)
                            const float tt = ((wq * cs) * r.ik) * ((Fs * r.ik + azf * (Fb - Fa)) + ge);
                            const float tm = tt * m0;
                            sum[8] += (double)(tm * m0);
                            sum[9] += (double)(tm * m1);
                            sum[10] += (double)((tt * m1) * m1);
                        }
                    }
                }
            }
        }
    }
    if (valid) {
        double *o = rpart + ((size_t)piece * A + i) * NS;
#pragma unroll
        for (int c = 0; c < NS; ++c) o[c] = sum[c];
    }
}
__global__ __launch_bounds__(64) void k_sl_sweep(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz, const float *q,
                                                 const SlCell *sl, const SlSlot *slots, int A, double *rpart) {
    sl_sweep_body<false>(tasks, moff, mol_of, xyz, q, sl, slots, A, rpart);
}
__global__ __launch_bounds__(64) void k_sl_sweep_strain(const int4 *tasks, const int *moff, const int *mol_of, const float *xyz,
                                                        const float *q, const SlCell *sl, const SlSlot *slots, int A, double *rpart) {
    sl_sweep_body<true>(tasks, moff, mol_of, xyz, q, sl, slots, A, rpart);
}

// Every atom adds, in this order: its real-space pieces in piece order (the first four sums of each EW_PART row of k_ew_sweep), its
// reciprocal pieces in piece order, X: the listed pairs' row (k_cl_excl<., true>, its first four sums), the self term.  phi [A] is
// written twice (the backward's seed and the output), then ffix [A][3] and the atom's share of the energy, 1/2 q_i phi_i, in float64.
// STRAIN (the rows of k_sl_sweep_strain): the same additions in the same order, and the atom's strain shares wshare [A][SL_SHARE_W]
// (xx yy zz yz xz xy) in float64: -1/2 ke q_i times its virial row (the six sums behind the four, the listed pairs' added behind the
// sweep's, as k_ew_atom does) and 1/2 ke q_i times the reciprocal and k = 0 sums, expanded through g_a, g_b and nhat.
// SITE (epnn_coulomb_xyz_slab_site, _slab_strain_site): site [A] = (2 sigma^2, chi, J, gamma_ii; gamma_ii 0 without the self term).  phi
// gets the Gaussians' self term ke 2 gamma_ii q_i / sqrt(pi) behind the split's; mu = chi + J q + phi goes into the seed and into
// mu [A], phi into phi [A] only; the share is q (chi + 1/2 J q) + 1/2 q phi.  Neither term has a strain: wshare is made as without SITE.
template <bool X, bool STRAIN, bool SITE = false>
__device__ __forceinline__ void sl_atom_body(int A, const int *moff, const int *mol_of, const float *q, const SlCell *sl, const double *part,
                                             const double *rpart, const double *xpart, double ke, float *seed, float *phi, float *ffix,
                                             double *share, double *wshare, const float4 *site = nullptr, float *mu = nullptr) {
    constexpr int NS = STRAIN ? SL_PART_STRAIN : SL_PART;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A) return;
    const int b = mol_of[i], np = cl_pieces(moff[b + 1] - moff[b]);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, r[SL_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < np; ++k)
        for (int c = 0; c < 4; ++c) s[c] += part[((size_t)k * A + i) * EW_PART + c];
    for (int k = 0; k < np; ++k)
        for (int c = 0; c < SL_PART; ++c) r[c] += rpart[((size_t)k * A + i) * NS + c];
    for (int c = 0; c < 3; ++c) s[1 + c] += r[1 + c] - sl[b].nh[c] * r[4];
    s[0] += r[0];
    if (X)
        for (int c = 0; c < 4; ++c) s[c] += xpart[(size_t)i * EW_PART + c];
    const double qi = (double)q[i];
    if constexpr (SITE) {
        const float4 st = site[i];
        const double p = ke * ((s[0] - sl[b].self * qi) + 1.1283791670955126 * (double)st.w * qi), chi = (double)st.y, J = (double)st.z;
        phi[i] = (float)p;
        seed[i] = mu[i] = (float)(chi + J * qi + p);
        for (int c = 0; c < 3; ++c) ffix[3 * (size_t)i + c] = (float)(ke * qi * s[1 + c]);
        share[i] = qi * (chi + 0.5 * J * qi) + 0.5 * qi * p;
    } else {                                                     // (the statements of the plain entries, in their order)
        const double p = ke * (s[0] - sl[b].self * qi);
        seed[i] = phi[i] = (float)p;
        for (int c = 0; c < 3; ++c) ffix[3 * (size_t)i + c] = (float)(ke * qi * s[1 + c]);
        share[i] = 0.5 * qi * p;
    }
    if (STRAIN) {
        double v[SL_SHARE_W] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[SL_PART_STRAIN - SL_PART] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < np; ++k)
            for (int c = 0; c < SL_SHARE_W; ++c) v[c] += part[((size_t)k * A + i) * EW_PART + 4 + c];
        if (X)
            for (int c = 0; c < SL_SHARE_W; ++c) v[c] += xpart[(size_t)i * EW_PART + 4 + c];
        for (int k = 0; k < np; ++k)
            for (int c = 0; c < SL_PART_STRAIN - SL_PART; ++c) t[c] += rpart[((size_t)k * A + i) * NS + SL_PART + c];
        const SlCell &e = sl[b];
        const double two_pi = 6.283185307179586, P[3] = {two_pi * (t[1] * e.ga[0] + t[2] * e.gb[0]), two_pi * (t[1] * e.ga[1] + t[2] * e.gb[1]),
                                                         two_pi * (t[1] * e.ga[2] + t[2] * e.gb[2])};
        const int ia[SL_SHARE_W] = {0, 1, 2, 1, 0, 0}, ib[SL_SHARE_W] = {0, 1, 2, 2, 2, 1};
        for (int c = 0; c < SL_SHARE_W; ++c) {
            const int x = ia[c], y = ib[c];
            const double nn = e.nh[x] * e.nh[y];
            const double kk = two_pi * two_pi * (t[3] * e.ga[x] * e.ga[y] + t[4] * (e.ga[x] * e.gb[y] + e.gb[x] * e.ga[y]) + t[5] * e.gb[x] * e.gb[y]);
            const double rec = kk - r[0] * ((x == y ? 1.0 : 0.0) - nn) + nn * t[0] - (e.nh[x] * P[y] + P[x] * e.nh[y]);
            wshare[SL_SHARE_W * (size_t)i + c] = 0.5 * ke * qi * (rec - v[c]);
        }
    }
}
__global__ __launch_bounds__(256) void k_sl_atom(int A, const int *moff, const int *mol_of, const float *q, const SlCell *sl, const double *part,
                                                 const double *rpart, double ke, float *seed, float *phi, float *ffix, double *share) {
    sl_atom_body<false, false>(A, moff, mol_of, q, sl, part, rpart, nullptr, ke, seed, phi, ffix, share, nullptr);
}
__global__ __launch_bounds__(256) void k_sl_atom_x(int A, const int *moff, const int *mol_of, const float *q, const SlCell *sl, const double *part,
                                                   const double *rpart, const double *xpart, double ke, float *seed, float *phi, float *ffix,
                                                   double *share) {
    sl_atom_body<true, false>(A, moff, mol_of, q, sl, part, rpart, xpart, ke, seed, phi, ffix, share, nullptr);
}
// the atoms' kernel of the strain call; xpart: the listed pairs' rows, or NULL without a list
__global__ __launch_bounds__(256) void k_sl_atom_strain(int A, const int *moff, const int *mol_of, const float *q, const SlCell *sl,
                                                        const double *part, const double *rpart, const double *xpart, double ke, float *seed,
                                                        float *phi, float *ffix, double *share, double *wshare) {
    if (xpart) sl_atom_body<true, true>(A, moff, mol_of, q, sl, part, rpart, xpart, ke, seed, phi, ffix, share, wshare);
    else sl_atom_body<false, true>(A, moff, mol_of, q, sl, part, rpart, nullptr, ke, seed, phi, ffix, share, wshare);
}
// the atoms' kernels of epnn_coulomb_xyz_slab_site (X: with a list) and of epnn_coulomb_xyz_slab_strain_site (xpart NULL: no list)
template <bool X>
__global__ __launch_bounds__(256) void k_sl_atom_site(int A, const int *moff, const int *mol_of, const float *q, const SlCell *sl,
                                                      const double *part, const double *rpart, const double *xpart, const float4 *site, double ke,
                                                      float *seed, float *phi, float *mu, float *ffix, double *share) {
    sl_atom_body<X, false, true>(A, moff, mol_of, q, sl, part, rpart, xpart, ke, seed, phi, ffix, share, nullptr, site, mu);
}
__global__ __launch_bounds__(256) void k_sl_atom_strain_site(int A, const int *moff, const int *mol_of, const float *q, const SlCell *sl,
                                                             const double *part, const double *rpart, const double *xpart, const float4 *site,
                                                             double ke, float *seed, float *phi, float *mu, float *ffix, double *share,
                                                             double *wshare) {
    if (xpart) sl_atom_body<true, true, true>(A, moff, mol_of, q, sl, part, rpart, xpart, ke, seed, phi, ffix, share, wshare, site, mu);
    else sl_atom_body<false, true, true>(A, moff, mol_of, q, sl, part, rpart, nullptr, ke, seed, phi, ffix, share, wshare, site, mu);
}

// One wavefront per cell: E_b by k_cl_energy's additions on the same shares (its bits), and the fixed-charge strain derivative
// [3][3]: the atoms' six strain shares, lane by lane in atom order, then across the lanes (the butterfly of k_ew_energy and
// k_g_strain_mol), mirrored into nine slots.
__global__ __launch_bounds__(64) void k_sl_energy_strain(const double *share, const double *wshare, const int *moff, double *e_out, float *gs_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = 0.0, W[SL_SHARE_W] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int a = moff[b] + lane; a < moff[b + 1]; a += 64) v += share[a];
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    for (int a = moff[b] + lane; a < moff[b + 1]; a += 64)
#pragma unroll
        for (int c = 0; c < SL_SHARE_W; ++c) W[c] += wshare[SL_SHARE_W * (size_t)a + c];
#pragma unroll
    for (int c = 0; c < SL_SHARE_W; ++c) {
        double w = W[c];
        for (int m = 32; m >= 1; m >>= 1) w += __shfl_xor(w, m);
        W[c] = w;
    }
    if (lane == 0) {
        e_out[b] = v;
        float *o = gs_out + 9 * (size_t)b;
        o[0] = (float)W[0]; o[4] = (float)W[1]; o[8] = (float)W[2];
        o[5] = o[7] = (float)W[3];
        o[2] = o[6] = (float)W[4];
        o[1] = o[3] = (float)W[5];
    }
}
