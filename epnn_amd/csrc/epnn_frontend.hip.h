// Front-end kernels: coordinates -> near-pair list with Gaussian edge features.
//
// Replaces get_init_edges (reference charge_gn.py:122-163) and the dense e/mask tensors that
// gen_padded_init_state builds from it (charge_gn.py:331-364).  Instead of an (n,n,48) tensor per molecule the
// device keeps one entry per UNORDERED pair {i<j} with D_ij < cutoff (the only pairs whose e is non-zero), in
// row-major (i, then j) order:  pi, pj (flat atom index), pe[48] (float32, computed in float64 like NumPy does),
// wi = wj = near flag (max_k e_k > tol as float32, charge_gn.py:90-94) and sym = 1 (e_ij == e_ji).
//
// Beside the pair list every atom gets its INCIDENCE ROW: one slot per pair it takes part in (as either index), rows in
// ascending partner order, inc_off[A+1] the row starts.  A pair's two slots (dest_i, dest_j) are where the tiled kernels
// deposit what the pair contributes to its two atoms (GNN correction rows, EPN charge transfers); an atom then sums its
// own contiguous row in slot order -- no second index list, no indirection, a fixed order.  Four launches: count (both
// directions in one pass over the partners), scan (both prefix sums), fill, link (position of i in row j).
#pragma once
#include "epnn_common.h"

struct FrontArgs {
    const float *xyz;      // [A][3]
    const int *mol_of;     // [A]
    const int *moff;       // [B+1]
    const int *mflag;      // [B]  != 0: the molecule runs on the tiled path (its pairs' records are marked valid)
    int A;
    double cutoff, eta;
    float tol;
    int e_dim;
    const double *mu;      // [e_dim] linspace(0.1, cutoff, e_dim) evaluated like NumPy
    int *row_cnt;          // [A]     pairs with this atom as FIRST index (partner j > i)
    int *row_off;          // [A+1]
    int *deg;              // [A]     all partners under the cutoff, either side
    int *inc_off;          // [A+1]   incidence rows (prefix sum of deg)
    int *nbr;              // [2 pcap] partners of every atom, ascending
    int *dest_i, *dest_j;  // [pcap]  incidence slots of a pair's first / second atom
    int4 *prec;            // [2 pcap] per pair: (i, j, inc_lo_i, inc_hi_i), (inc_lo_j, inc_hi_j, dest_i, dest_j)
    double cut2;           // smallest double whose correctly rounded sqrt reaches the cutoff: D < cutoff <=> D^2 < cut2
    unsigned long long *bits;   // [A][bits_w] or null: the count pass leaves every row's D < cutoff decisions as a bit per candidate of the
    int bits_w;                 // row's molecule (word t = candidates 64 t .. 64 t + 63): the fill pass walks the set bits instead of
                                // measuring all n distances a second time (systems of up to 4096 atoms)
    int pcap;
    int *pi, *pj, *psym;
    float *pe, *pwi, *pwj;
    int *status;
};

// distance exactly as scipy.spatial.distance_matrix on float32 coordinates promoted to float64
// (charge_gn.py:124): sqrt((dx*dx + dy*dy) + dz*dz).
__device__ __forceinline__ double epnn_dist(const float *xyz, int i, int j) {
    double dx = (double)xyz[3 * j + 0] - (double)xyz[3 * i + 0];
    double dy = (double)xyz[3 * j + 1] - (double)xyz[3 * i + 1];
    double dz = (double)xyz[3 * j + 2] - (double)xyz[3 * i + 2];
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// squared distance in the same float64 arithmetic (no sqrt: the compare against the cutoff is made on cut2)
__device__ __forceinline__ double epnn_dist2(const float *xyz, int i, int j) {
    double dx = (double)xyz[3 * j + 0] - (double)xyz[3 * i + 0];
    double dy = (double)xyz[3 * j + 1] - (double)xyz[3 * i + 1];
    double dz = (double)xyz[3 * j + 2] - (double)xyz[3 * i + 2];
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// squared distance from the row atom (xi, yi, zi: its float32 coordinates as float64) to coordinates p[0..2]
__device__ __forceinline__ double epnn_dist2p(double xi, double yi, double zi, const float *p) {
    const double dx = (double)p[0] - xi, dy = (double)p[1] - yi, dz = (double)p[2] - zi;
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Periodic cells (orthorhombic; include/epnn.h): box[b][k] > 0 is the length of periodic axis k of molecule b, 0 an open axis.
// Minimum image of a float64 displacement d: d - k L with k = rint(d / L) (|d - k L| <= L / 2).  k L is exact (k is small, L a
// float32), and so is the difference for any d within a few box lengths; the host reference computes the same expression.
__device__ __forceinline__ double epnn_mic(double d, double L) {
    return L > 0.0 ? __dadd_rn(d, -__dmul_rn(L, rint(d / L))) : d;
}
// epnn_dist2p with minimum-image components (L* the box row as float64)
__device__ __forceinline__ double epnn_dist2p_pbc(double xi, double yi, double zi, const float *p, double Lx, double Ly, double Lz) {
    const double dx = epnn_mic((double)p[0] - xi, Lx), dy = epnn_mic((double)p[1] - yi, Ly), dz = epnn_mic((double)p[2] - zi, Lz);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
// a coordinate moved into [0, L] on a periodic axis (for the float32 pre-test only: the float64 test measures unwrapped coordinates)
__device__ __forceinline__ float epnn_wrap_coord(float x, float L) {
    if (!(L > 0.f)) return x;
    const double Ld = (double)L;
    return (float)((double)x - Ld * floor((double)x / Ld));
}
// General (triclinic) cells (include/epnn.h): what the device needs of one molecule's cell, prepared in float64 by the host's
// check_cell.  Row k of `a` is lattice vector a_k (the caller's float32 entries), row k of `g` its dual vector g_k inside the span
// of the periodic rows (g_k . a_l = delta_kl); an open axis has a zero row in both, so that it drops out of every sum below
// without a branch (n_k = rint(0) = 0, d - 0 * 0 = d exactly).
struct EpnnCell {
    double g[9];
    float a[9];
    float pre_eps;                    // float32 pre-test (front_scan_row): a fractional part this close to 1/2 is not trusted
    float pre_margin;                 // ... and the factor on cutoff^2 it compares with
    float pre_ext;                    // ... and the largest component a position may have to take part in it
};
static_assert(sizeof(EpnnCell) == 120, "EpnnCell is staged as 30 words");
// The image of a float64 displacement that the cell contract names: n_k = rint(g_k . d) from the unshifted d (products and sums in
// this order, nothing contracted), then d' = ((d - n_0 a_0) - n_1 a_1) - n_2 a_2 per component.  n_k a_kc is exact (a small integer
// times a float32).  A diagonal cell reduces to epnn_mic per axis except at rounding ties, which lie a cutoff away.
__device__ __forceinline__ void epnn_mic_cell(double &dx, double &dy, double &dz, const double *g, const double *a) {
    const double n0 = rint(__dadd_rn(__dadd_rn(__dmul_rn(g[0], dx), __dmul_rn(g[1], dy)), __dmul_rn(g[2], dz)));
    const double n1 = rint(__dadd_rn(__dadd_rn(__dmul_rn(g[3], dx), __dmul_rn(g[4], dy)), __dmul_rn(g[5], dz)));
    const double n2 = rint(__dadd_rn(__dadd_rn(__dmul_rn(g[6], dx), __dmul_rn(g[7], dy)), __dmul_rn(g[8], dz)));
    dx = __dadd_rn(__dadd_rn(__dadd_rn(dx, -__dmul_rn(n0, a[0])), -__dmul_rn(n1, a[3])), -__dmul_rn(n2, a[6]));
    dy = __dadd_rn(__dadd_rn(__dadd_rn(dy, -__dmul_rn(n0, a[1])), -__dmul_rn(n1, a[4])), -__dmul_rn(n2, a[7]));
    dz = __dadd_rn(__dadd_rn(__dadd_rn(dz, -__dmul_rn(n0, a[2])), -__dmul_rn(n1, a[5])), -__dmul_rn(n2, a[8]));
}
// a cell's dual and lattice vectors as float64 registers (cell index wave-uniform: scalar loads)
struct EpnnCellD {
    double g[9], a[9];
    float ext;
    __device__ __forceinline__ void load(const EpnnCell *cells, int b) {
        const EpnnCell &c = cells[__builtin_amdgcn_readfirstlane(b)];
#pragma unroll
        for (int k = 0; k < 9; ++k) { g[k] = c.g[k]; a[k] = (double)c.a[k]; }
        ext = c.pre_ext;
    }
};
// epnn_dist2p with the displacement of epnn_mic_cell
__device__ __forceinline__ double epnn_dist2p_cell(double xi, double yi, double zi, const float *p, const EpnnCellD &c) {
    double dx = (double)p[0] - xi, dy = (double)p[1] - yi, dz = (double)p[2] - zi;
    epnn_mic_cell(dx, dy, dz, c.g, c.a);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
// a position moved into the cell along its periodic axes, r - sum_k floor(g_k . r) a_k in float64, rounded to float32 (for the
// float32 pre-test only).  Along open directions nothing is wrapped: a position with a component above pre_ext afterwards is
// marked (x = EPNN_PRE_SKIP) and its pairs go to the float64 test untested.
#define EPNN_PRE_SKIP 1e30f
__device__ __forceinline__ void epnn_wrap_cell(float &x, float &y, float &z, const EpnnCellD &c) {
    const double rx = x, ry = y, rz = z;
    const double n0 = floor(c.g[0] * rx + c.g[1] * ry + c.g[2] * rz), n1 = floor(c.g[3] * rx + c.g[4] * ry + c.g[5] * rz),
                 n2 = floor(c.g[6] * rx + c.g[7] * ry + c.g[8] * rz);
    x = (float)(rx - n0 * c.a[0] - n1 * c.a[3] - n2 * c.a[6]);
    y = (float)(ry - n0 * c.a[1] - n1 * c.a[4] - n2 * c.a[7]);
    z = (float)(rz - n0 * c.a[2] - n1 * c.a[5] - n2 * c.a[8]);
    if (fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))) > c.ext) x = EPNN_PRE_SKIP;
}
// A workgroup = four consecutive rows, one wave each.  The candidates' coordinates go through LDS in blocks of
// EPNN_FRONT_JB atoms, staged once for the four rows with every load of a thread in flight (a wave that fetched its 64
// candidates per trip straight from memory paid one L2 round trip per trip: 35 of them for a 2220-atom system).  Rows of a
// workgroup that belong to another molecule than its first row (molecule boundaries) read memory directly.
#define EPNN_FRONT_JB 2048
// calls body(j, near, d2, trip) for every candidate j of the row's molecule, 64 per trip (trip t = candidates 64 t .. of the
// molecule), lane = candidate; wave-uniform trips.  PBC 1: minimum-image distances in the cells of `box` [B][3]; PBC 2: in the
// general cells that `box` points to (EpnnCell [B]).
template <int PBC = 0, typename Body>
__device__ __forceinline__ void front_scan_row(const FrontArgs &F, float *sx, int row, bool live, Body &&body, const float *box = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int row0 = row - (tid >> 6);                        // the workgroup's first row
    const int b0 = F.mol_of[row0], beg0 = F.moff[b0], end0 = F.moff[b0 + 1];
    const int b = live ? F.mol_of[row] : b0;
    const bool shared = live && b == b0;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    float xf = 0.f, yf = 0.f, zf = 0.f;
    if (live) {
        xf = F.xyz[3 * row]; yf = F.xyz[3 * row + 1]; zf = F.xyz[3 * row + 2];
        xi = (double)xf; yi = (double)yf; zi = (double)zf;
    }
    // float32 first: only a candidate whose float32 squared distance comes within 1e-4 (relative) of the cutoff's gets the
    // float64 evaluation that decides (float32 differences, squares and sums are good to a few 1e-7)
    float cut2f = (float)(F.cut2 * 1.0001);
    float Lxf = 0.f, Lyf = 0.f, Lzf = 0.f, ixf = 0.f, iyf = 0.f, izf = 0.f;
    double Lx = 0.0, Ly = 0.0, Lz = 0.0;                      // the row's cell
    EpnnCellD cr, c0;                                         // PBC 2: the row's cell, and the staged molecule's
    float gf[9], af[9], peps = 0.f;
    if (PBC == 2) {
        // General-cell pre-test.  S = |a_0| + |a_1| + |a_2|, w = the smallest width, u = 2^-24.  The staged candidates and the row
        // atom are moved into the cell along its periodic axes in float64 (epnn_wrap_cell) and rounded.  Inside the span of the
        // periodic rows every component is then at most S in magnitude; along open directions (zero rows, which need not be
        // Cartesian axes: a tilted slab or wire) nothing bounds it, and the rounding error grows with it.  So a position takes part
        // only if all its components are at most X = S + 1024 A (no open axis: X = S, which always holds); any other position is
        // marked and every pair with it goes to the float64 test untested.  For the rest: a rounded component is good to u X, the
        // float32 difference f of two of them (|f_c| <= 2 X) to 4 u X.  With float32 copies of the dual vectors (relative error
        // u), p_k = g_k . f is computed with an error of at most
        //     |g_k| (sqrt(3) 4 u X + u |f| + 3 u |f|) <= 21 u X / w_k                                   (|f| <= 2 sqrt(3) X),
        // so pre_eps = 32 u X / w bounds it on every axis.  The exact p_k differs from g_k . d of the unwrapped float64 displacement
        // by an integer.  If the float64 test accepts the pair (D < c), its image has |g_k . d'| <= D / w_k < 1/2 on every axis.
        //   (a) Some |p_k - rintf(p_k)| >= 1/2 - pre_eps: the float32 rounding may pick another image than the float64 one, which
        //       in a sheared cell can be much longer.  Such a candidate is passed on to the float64 test untested.
        //   (b) Otherwise the exact fractional parts lie inside (-1/2, 1/2) around the same integers: n_k is the float64 choice,
        //       and f - sum n_k a_k (three fmaf per component, operands <= 3 X: 9 u X more) differs from d' by at most
        //       13 u X per component; 16 u X is used.  With D < c the float32 sum of squares is at most
        //           (c^2 + 2 sqrt(3) 16 u X c + 3 (16 u X)^2) (1 + 4 u)  =  c^2 (1 + 55.4 r + 768 r^2 + 4 u),   r = u X / c,
        //       and pre_margin = 1.0001 + 96 r + 1024 r^2 covers it.
        // Either way the pre-test never rejects a pair the float64 test accepts, for any valid cell (pre_eps >= 1/2, an extremely
        // thin and long cell, just switches the pre-test off), for coordinates any number of cells outside it (the wrap is
        // done in float64) and any distance out along an open direction.  check_cell computes the constants in float64;
        // tests/test_cell_pretest.py runs the same arithmetic in NumPy against the float64 rule.
        const EpnnCell *cells = reinterpret_cast<const EpnnCell *>(box);
        c0.load(cells, b0);
        cr.load(cells, b);
#pragma unroll
        for (int k = 0; k < 9; ++k) { gf[k] = (float)c0.g[k]; af[k] = (float)c0.a[k]; }
        const EpnnCell &cc = cells[__builtin_amdgcn_readfirstlane(b0)];
        peps = 0.5f - cc.pre_eps;
        cut2f = (float)(F.cut2 * (double)cc.pre_margin);
        epnn_wrap_cell(xf, yf, zf, c0);
    }
    if (PBC == 1) {
        // Periodic pre-test: the staged candidates and the row atom are first moved into the cell (epnn_wrap_coord: float64, then
        // rounded, error <= u L with u = 2^-24), their float32 difference (|.| <= L, error <= u L) is wrapped again by
        // rint(f / L).  A component then differs from the float64 minimum image by at most 3 u L -- the same image -- or, where the
        // two roundings pick different images (|d| within a few u L of L / 2), its magnitude exceeds the float64 one's by at most
        // ~6 u L; 8 u L bounds both.  With D < c the float32 sum of squares is then at most
        //     (c^2 + 2 sqrt(3) 8 u L c + 3 (8 u L)^2) (1 + 4 u)  =  c^2 (1 + 27.7 r + 192 r^2 + 4 u),   r = u L / c,
        // so the margin 1e-4 + 64 r + 256 r^2 (L the longest periodic axis) never rejects a pair the float64 test accepts, for any
        // box length and for coordinates any number of box lengths outside the cell (the wrap is done in float64).
        const float *bx = box + 3 * b0;
        Lxf = bx[0]; Lyf = bx[1]; Lzf = bx[2];
        ixf = Lxf > 0.f ? 1.f / Lxf : 0.f; iyf = Lyf > 0.f ? 1.f / Lyf : 0.f; izf = Lzf > 0.f ? 1.f / Lzf : 0.f;
        const double r = 0x1p-24 * (double)fmaxf(Lxf, fmaxf(Lyf, Lzf)) / F.cutoff;
        cut2f = (float)(F.cut2 * (1.0001 + r * (64.0 + 256.0 * r)));
        const float *br = box + 3 * b;
        Lx = (double)br[0]; Ly = (double)br[1]; Lz = (double)br[2];
        xf = epnn_wrap_coord(xf, Lxf); yf = epnn_wrap_coord(yf, Lyf); zf = epnn_wrap_coord(zf, Lzf);
    }
    for (int jb = beg0; jb < end0; jb += EPNN_FRONT_JB) {
        const int nb = min(EPNN_FRONT_JB, end0 - jb);
        __syncthreads();
        if (PBC == 2) {
            for (int jj = tid; jj < nb; jj += 256) {
                float px = F.xyz[((size_t)jb + jj) * 3], py = F.xyz[((size_t)jb + jj) * 3 + 1], pz = F.xyz[((size_t)jb + jj) * 3 + 2];
                epnn_wrap_cell(px, py, pz, c0);
                sx[3 * jj] = px; sx[3 * jj + 1] = py; sx[3 * jj + 2] = pz;
            }
        } else if (PBC == 1) {
            for (int i = tid; i < nb * 3; i += 256) {
                const int k = i % 3;
                sx[i] = epnn_wrap_coord(F.xyz[(size_t)jb * 3 + i], k == 0 ? Lxf : (k == 1 ? Lyf : Lzf));
            }
        } else {
            for (int i = tid; i < nb * 3; i += 256) sx[i] = F.xyz[(size_t)jb * 3 + i];
        }
        __syncthreads();
        if (shared)
            for (int j0 = 0; j0 < nb; j0 += 64) {
                const int j = j0 + lane;
                double d2 = 0.0;
                bool near = false;
                if (j < nb && jb + j != row) {
                    float fx = sx[3 * j] - xf, fy = sx[3 * j + 1] - yf, fz = sx[3 * j + 2] - zf;
                    bool pass = false;
                    if (PBC == 1) {
                        fx = fmaf(-Lxf, rintf(fx * ixf), fx);
                        fy = fmaf(-Lyf, rintf(fy * iyf), fy);
                        fz = fmaf(-Lzf, rintf(fz * izf), fz);
                    }
                    if (PBC == 2) {
                        const float p0 = gf[0] * fx + gf[1] * fy + gf[2] * fz, p1 = gf[3] * fx + gf[4] * fy + gf[5] * fz,
                                    p2 = gf[6] * fx + gf[7] * fy + gf[8] * fz;
                        const float n0 = rintf(p0), n1 = rintf(p1), n2 = rintf(p2);
                        pass = !(fmaxf(fabsf(p0 - n0), fmaxf(fabsf(p1 - n1), fabsf(p2 - n2))) < peps) ||
                               fmaxf(fabsf(sx[3 * j]), fabsf(xf)) > 0.5f * EPNN_PRE_SKIP;
                        fx = fmaf(-n2, af[6], fmaf(-n1, af[3], fmaf(-n0, af[0], fx)));
                        fy = fmaf(-n2, af[7], fmaf(-n1, af[4], fmaf(-n0, af[1], fy)));
                        fz = fmaf(-n2, af[8], fmaf(-n1, af[5], fmaf(-n0, af[2], fz)));
                    }
                    if ((PBC == 2 && pass) || fx * fx + fy * fy + fz * fz < cut2f) {
                        d2 = PBC == 2   ? epnn_dist2p_cell(xi, yi, zi, F.xyz + 3 * ((size_t)jb + j), cr)
                             : PBC == 1 ? epnn_dist2p_pbc(xi, yi, zi, F.xyz + 3 * ((size_t)jb + j), Lx, Ly, Lz)
                                        : epnn_dist2p(xi, yi, zi, sx + 3 * j);
                        near = d2 < F.cut2;
                    }
                }
                body(jb + j, near, d2, (jb - beg0 + j0) >> 6);
            }
    }
    if (live && !shared) {
        const int beg = F.moff[b], end = F.moff[b + 1];
        for (int j0 = beg; j0 < end; j0 += 64) {
            const int j = j0 + lane;
            double d2 = 0.0;
            bool near = false;
            if (j < end && j != row) {
                d2 = PBC == 2   ? epnn_dist2p_cell(xi, yi, zi, F.xyz + 3 * j, cr)
                     : PBC == 1 ? epnn_dist2p_pbc(xi, yi, zi, F.xyz + 3 * j, Lx, Ly, Lz)
                                : epnn_dist2p(xi, yi, zi, F.xyz + 3 * j);
                near = d2 < F.cut2;
            }
            body(j, near, d2, (j0 - beg) >> 6);
        }
    }
}

// one wave per row i: partners j != i of the same molecule with D < cutoff -- how many in all, how many with j > i
template <int PBC = 0>
__device__ __forceinline__ void front_count_body(const FrontArgs &F, float *sx, int blk, const float *box = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blk * 4 + wave;
    const bool live = row < F.A;
    int up = 0, all = 0;
    unsigned long long mine = 0ull;                           // lane t keeps the decisions of trip t
    front_scan_row<PBC>(F, sx, row, live, [&](int j, bool near, double, int trip) {
        const unsigned long long bal = __ballot(near);
        all += __popcll(bal);
        up += __popcll(__ballot(near && j > row));
        if (trip == lane) mine = bal;
    }, box);
    if (live && lane == 0) {
        F.row_cnt[row] = up;
        F.deg[row] = all;
    }
    if (live && F.bits && lane < F.bits_w) F.bits[(size_t)row * F.bits_w + lane] = mine;
}
__global__ __launch_bounds__(256) void k_front_count(FrontArgs F) {
    __shared__ float sx[EPNN_FRONT_JB * 3];
    front_count_body(F, sx, (int)blockIdx.x);
}
// ... in the periodic cells box [B][3] (epnn_forward_xyz_pbc)
__global__ __launch_bounds__(256) void k_front_count_pbc(FrontArgs F, const float *box) {
    __shared__ float sx[EPNN_FRONT_JB * 3];
    front_count_body<1>(F, sx, (int)blockIdx.x, box);
}
// ... in the general cells `cells` [B] (epnn_forward_xyz_cell)
__global__ __launch_bounds__(256) void k_front_count_cell(FrontArgs F, const EpnnCell *cells) {
    __shared__ float sx[EPNN_FRONT_JB * 3];
    front_count_body<2>(F, sx, (int)blockIdx.x, reinterpret_cast<const float *>(cells));
}

// both prefix sums in ONE single-workgroup launch (1024 threads x 8 elements per round, a carry between rounds): a
// 2220-atom system is one round, 100 k atoms thirteen
__device__ __forceinline__ void front_scan_both_body(const FrontArgs &F, int *wsA, int *wsB, int &carryA, int &carryB) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { carryA = 0; carryB = 0; }
    __syncthreads();
    for (int base = 0; base < F.A; base += 8192) {
        const int i0 = base + tid * 8;
        int va[8], vb[8], ta = 0, tb = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ic = min(i0 + k, F.A - 1);                   // unconditional loads (a load under a condition is a branch
            const int ta_ = F.row_cnt[ic], tb_ = F.deg[ic];        // and waits for the load before it), a select after
            va[k] = i0 + k < F.A ? ta_ : 0;
            vb[k] = i0 + k < F.A ? tb_ : 0;
            ta += va[k];
            tb += vb[k];
        }
        int ia = ta, ib = tb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int oa = __shfl_up(ia, d, 64), ob = __shfl_up(ib, d, 64);
            if (lane >= d) { ia += oa; ib += ob; }
        }
        if (lane == 63) { wsA[wave] = ia; wsB[wave] = ib; }
        __syncthreads();
        int wa = 0, wb = 0;
        for (int w = 0; w < wave; ++w) { wa += wsA[w]; wb += wsB[w]; }
        const int ca = carryA, cb = carryB;
        int ra = ca + wa + ia - ta, rb = cb + wb + ib - tb;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 + k < F.A) { F.row_off[i0 + k] = ra; F.inc_off[i0 + k] = rb; }
            ra += va[k];
            rb += vb[k];
        }
        __syncthreads();
        if (tid == 1023) { carryA = ra; carryB = rb; }
        __syncthreads();
    }
    if (tid == 0) {
        F.row_off[F.A] = carryA;
        F.inc_off[F.A] = carryB;
        if (carryA > F.pcap) atomicOr(F.status, EPNN_ST_PAIR_OVERFLOW);
    }
}
__global__ __launch_bounds__(1024) void k_front_scan_both(FrontArgs F) {
    __shared__ int wsA[16], wsB[16];
    __shared__ int carryA, carryB;
    front_scan_both_body(F, wsA, wsB, carryA, carryB);
}

// exclusive scan of row_cnt[0..A) -> row_off[0..A] in two passes: (1) every block of 256 threads scans 2048
// elements locally and publishes its total, (2) every block adds the totals of the blocks before it.
#define EPNN_SCAN_ELEMS 2048
__global__ __launch_bounds__(256) void k_front_scan1(FrontArgs F, int *bsum) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * EPNN_SCAN_ELEMS + tid * 8;
    int v[8], tot = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int t_ = F.row_cnt[min(base + k, F.A - 1)];
        v[k] = base + k < F.A ? t_ : 0;
        tot += v[k];
    }
    int incl = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    int run = woff + incl - tot;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (base + k < F.A) F.row_off[base + k] = run;
        run += v[k];
    }
    if (tid == 255) {
        bsum[blockIdx.x] = run;
        if (gridDim.x == 1) {                      // a single block: the total is known here, k_front_scan2 is not launched
            F.row_off[F.A] = run;
            if (run > F.pcap) atomicOr(F.status, EPNN_ST_PAIR_OVERFLOW);
        }
    }
}
__global__ __launch_bounds__(256) void k_front_scan2(FrontArgs F, const int *bsum) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int part = 0;
    for (int b = tid; b < (int)blockIdx.x; b += 256) part += bsum[b];
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == 0) wsum[wave] = part;
    __syncthreads();
    const int boff = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int base = blockIdx.x * EPNN_SCAN_ELEMS + tid * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (base + k < F.A) F.row_off[base + k] += boff;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        const int total = boff + bsum[blockIdx.x];
        F.row_off[F.A] = total;
        if (total > F.pcap) atomicOr(F.status, EPNN_ST_PAIR_OVERFLOW);
    }
}

// one wave per row: the atom's incidence row (partners, ascending) and the pairs in which it is the first index
struct FrontFillShared {
    float sx[EPNN_FRONT_JB * 3];
    int s_j[4][64];
    double s_D[4][64];
    double s_C[4][64];
    int s_max[4][64];
};
// INLINE: no scan launch ran -- the workgroup works out its four rows' places in the two prefix sums itself, from the counts of all
// rows (systems of up to EPNN_FRONT_INLINE_A atoms: 2 x 2220 words per workgroup for the protein, against a launch of a single
// workgroup, 6.9 us, between the count and the fill), writes them for the later launches, and the last workgroup the totals
#define EPNN_FRONT_INLINE_A 8192
template <bool INLINE = false, int PBC = 0>
__device__ __forceinline__ void front_fill_body(const FrontArgs &F, FrontFillShared &Sh, int blk, const float *box = nullptr) {
    float *sx = Sh.sx;
    auto &s_j = Sh.s_j;
    auto &s_D = Sh.s_D;
    auto &s_C = Sh.s_C;
    auto &s_max = Sh.s_max;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blk * 4 + wave;
    int slot0 = 0, inc0 = 0;
    bool live = row < F.A;
    if (INLINE) {
        const int tid = threadIdx.x, row0 = blk * 4;
        int bc = 0, bd = 0, tc = 0, td = 0;                      // counts in front of the workgroup's first row | of all rows
        for (int r0 = 0; r0 < F.A; r0 += 256 * 4) {
            int c[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                       // unconditional loads of a clamped index, eight in flight
                const int r = min(r0 + u * 256 + tid, F.A - 1);
                c[u] = F.row_cnt[r];
                d[u] = F.deg[r];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + u * 256 + tid;
                if (r < F.A) {
                    tc += c[u]; td += d[u];
                    if (r < row0) { bc += c[u]; bd += d[u]; }
                }
            }
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            bc += __shfl_xor(bc, dd, 64); bd += __shfl_xor(bd, dd, 64);
            tc += __shfl_xor(tc, dd, 64); td += __shfl_xor(td, dd, 64);
        }
        int *red = reinterpret_cast<int *>(Sh.s_j);            // [4 waves][4] (the pair staging is not in use yet)
        if (lane == 0) { red[wave * 4] = bc; red[wave * 4 + 1] = bd; red[wave * 4 + 2] = tc; red[wave * 4 + 3] = td; }
        __syncthreads();
        bc = red[0] + red[4] + red[8] + red[12];
        bd = red[1] + red[5] + red[9] + red[13];
        tc = red[2] + red[6] + red[10] + red[14];
        td = red[3] + red[7] + red[11] + red[15];
        __syncthreads();
        // this wavefront's row: the rows of the workgroup before it
        for (int k = 0; k < wave; ++k)
            if (row0 + k < F.A) { bc += F.row_cnt[row0 + k]; bd += F.deg[row0 + k]; }
        slot0 = bc;
        inc0 = bd;
        if (live && lane == 0) { F.row_off[row] = bc; F.inc_off[row] = bd; }
        if (row == F.A - 1 && lane == 0) {
            F.row_off[F.A] = tc;
            F.inc_off[F.A] = td;
            if (tc > F.pcap) atomicOr(F.status, EPNN_ST_PAIR_OVERFLOW);
        }
        live = live && tc <= F.pcap;                           // overflow: host regrows and reruns
    } else {
        live = live && F.row_off[F.A] <= F.pcap;               // overflow: host regrows and reruns
        slot0 = live ? F.row_off[row] : 0;
        inc0 = live ? F.inc_off[row] : 0;
    }
    const double pi_d = 3.141592653589793;
    auto body = [&](int j, bool near, double d2, int) {
        const unsigned long long bal = __ballot(near);
        if (bal == 0ull) return;
        const int pos = inc0 + __popcll(bal & ((1ull << lane) - 1ull));      // this partner's slot in the atom's incidence row
        if (near) F.nbr[pos] = j;
        inc0 += __popcll(bal);
        const bool upn = near && j > row;
        const unsigned long long bup = __ballot(upn);
        const int m = __popcll(bup);
        if (m == 0) return;
        if (upn) {
            const int rank = __popcll(bup & ((1ull << lane) - 1ull));
            const double D = sqrt(d2);                         // charge_gn.py:124 (scipy distance_matrix)
            s_j[wave][rank] = j;
            s_D[wave][rank] = D;
            // charge_gn.py:148-152: C = (cos(pi*D/cutoff)+1)/2 ; C[D<=0] = 1 (D>=cutoff excluded, diagonal not listed)
            double C = (cos(pi_d * (D - 0.0) / F.cutoff) + 1.0) / 2.0;
            if (D <= 0.0) C = 1.0;
            s_C[wave][rank] = C;
            s_max[wave][rank] = 0;
            F.dest_i[slot0 + rank] = pos;
        }
        __builtin_amdgcn_wave_barrier();
        const int total = m * F.e_dim;
        for (int idx = lane; idx < total; idx += 64) {
            const int pr = idx / F.e_dim, ch = idx - pr * F.e_dim;
            const double d = s_D[wave][pr] - F.mu[ch];
            const double val = s_C[wave][pr] * exp(-F.eta * (d * d));      // charge_gn.py:160
            const float ef = (float)val;                                      // :161
            F.pe[(size_t)(slot0 + pr) * F.e_dim + ch] = ef;
            atomicMax(&s_max[wave][pr], __float_as_int(ef));                  // e >= 0: int order == float order
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < m) {
            const int s = slot0 + lane;
            F.pi[s] = row;
            F.pj[s] = s_j[wave][lane];
            const float w = __int_as_float(s_max[wave][lane]) > F.tol ? 1.0f : 0.0f;   // charge_gn.py:90-94
            F.pwi[s] = w;
            F.pwj[s] = w;
            F.psym[s] = 1;
        }
        __builtin_amdgcn_wave_barrier();
        slot0 += m;
    };
    if (F.bits) {
        // the count pass left this row's decisions: only the trips with a set bit are looked at, only their near candidates measured
        const int b = live ? F.mol_of[row] : 0, beg = live ? F.moff[b] : 0;
        const unsigned long long word = live && lane < F.bits_w ? F.bits[(size_t)row * F.bits_w + lane] : 0ull;
        unsigned long long trips = __ballot(word != 0ull);
        double xi = 0.0, yi = 0.0, zi = 0.0, Lx = 0.0, Ly = 0.0, Lz = 0.0;
        if (live) { xi = (double)F.xyz[3 * row]; yi = (double)F.xyz[3 * row + 1]; zi = (double)F.xyz[3 * row + 2]; }
        if (PBC == 1 && live) { Lx = (double)box[3 * b]; Ly = (double)box[3 * b + 1]; Lz = (double)box[3 * b + 2]; }
        EpnnCellD cr;
        if (PBC == 2) cr.load(reinterpret_cast<const EpnnCell *>(box), b);
        while (trips) {
            const int t = __ffsll((long long)trips) - 1;
            trips &= trips - 1ull;
            const unsigned long long bal = __shfl(word, t, 64);
            const int j = beg + 64 * t + lane;
            const bool near = (bal >> lane) & 1ull;
            const double d2 = !near       ? 0.0
                              : PBC == 2 ? epnn_dist2p_cell(xi, yi, zi, F.xyz + 3 * j, cr)
                              : PBC == 1 ? epnn_dist2p_pbc(xi, yi, zi, F.xyz + 3 * j, Lx, Ly, Lz)
                                         : epnn_dist2p(xi, yi, zi, F.xyz + 3 * j);
            body(j, near, d2, t);
        }
        return;
    }
    front_scan_row<PBC>(F, sx, row, live, body, box);
}
__global__ __launch_bounds__(256) void k_front_fill(FrontArgs F) {
    __shared__ FrontFillShared Sh;
    front_fill_body<false>(F, Sh, (int)blockIdx.x);
}
__global__ __launch_bounds__(256) void k_front_fill_pbc(FrontArgs F, const float *box) {
    __shared__ FrontFillShared Sh;
    front_fill_body<false, 1>(F, Sh, (int)blockIdx.x, box);
}
__global__ __launch_bounds__(256) void k_front_fill_cell(FrontArgs F, const EpnnCell *cells) {
    __shared__ FrontFillShared Sh;
    front_fill_body<false, 2>(F, Sh, (int)blockIdx.x, reinterpret_cast<const float *>(cells));
}

// one thread per pair (i, j): where does i sit in j's incidence row?  (rows are ascending and short: a few loads in flight)
__device__ __forceinline__ void front_link_body(const FrontArgs &F, int blk, int nblk) {
    const int np = F.row_off[F.A];
    if (np > F.pcap) return;
    for (int p = blk * 256 + threadIdx.x; p < np; p += nblk * 256) {
        const int i = F.pi[p], j = F.pj[p];
        const int lo = F.inc_off[j], hi = F.inc_off[j + 1];
        int found = -1;
        for (int k0 = lo; k0 < hi && found < 0; k0 += 8) {
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = F.nbr[min(k0 + u, hi - 1)];       // unconditional; a repeated last entry finds nothing new
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < hi && v[u] == i) found = k0 + u;
        }
        const int di = F.dest_i[p];
        F.dest_j[p] = found;
        const int iv = F.mflag[F.mol_of[i]] ? i : -1 - i;
        F.prec[2 * p] = make_int4(iv, j, F.inc_off[i], F.inc_off[i + 1]);
        F.prec[2 * p + 1] = make_int4(lo, hi, di, found);
    }
}
__global__ __launch_bounds__(256) void k_front_link(FrontArgs F) { front_link_body(F, (int)blockIdx.x, (int)gridDim.x); }

// epnn_edges: dense (n,n,e_dim) tensor exactly like get_init_edges, one thread per (i,j,ch).  PBC: minimum-image distances in the
// cell box[3] (epnn_edges_pbc); PBC 2: in the general cell that box points to (one EpnnCell, epnn_edges_cell)
template <int PBC>
__device__ __forceinline__ void edges_dense_body(const float *xyz, const float *box, int n, int e_dim, double cutoff, double eta,
                                                 const double *mu, float *e_out, double *c_out) {
    const size_t total = (size_t)n * n * e_dim;
    const double pi_d = 3.141592653589793;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int ch = (int)(idx % e_dim);
        const size_t pr = idx / e_dim;
        const int j = (int)(pr % n), i = (int)(pr / n);
        double D;
        if (PBC == 2) {
            EpnnCellD c;
            c.load(reinterpret_cast<const EpnnCell *>(box), 0);
            D = sqrt(epnn_dist2p_cell((double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], xyz + 3 * j, c));
        } else if (PBC == 1)
            D = sqrt(epnn_dist2p_pbc((double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], xyz + 3 * j, (double)box[0],
                                     (double)box[1], (double)box[2]));
        else
            D = epnn_dist(xyz, i, j);
        double C = (cos(pi_d * (D - 0.0) / cutoff) + 1.0) / 2.0;
        if (D >= cutoff) C = 0.0;
        if (D <= 0.0) C = 1.0;
        if (i == j) C = 0.0;
        const double d = D - mu[ch];
        e_out[idx] = (float)(C * exp(-eta * (d * d)));
        if (c_out && ch == 0) c_out[pr] = C;                  // the cutoff weights the reference returns tiled (charge_gn.py:163)
    }
}
__global__ __launch_bounds__(256) void k_edges_dense(const float *xyz, int n, int e_dim, double cutoff, double eta,
                                                     const double *mu, float *e_out, double *c_out) {
    edges_dense_body<0>(xyz, nullptr, n, e_dim, cutoff, eta, mu, e_out, c_out);
}
__global__ __launch_bounds__(256) void k_edges_dense_pbc(const float *xyz, const float *box, int n, int e_dim, double cutoff, double eta,
                                                         const double *mu, float *e_out, double *c_out) {
    edges_dense_body<1>(xyz, box, n, e_dim, cutoff, eta, mu, e_out, c_out);
}
__global__ __launch_bounds__(256) void k_edges_dense_cell(const float *xyz, const EpnnCell *cell, int n, int e_dim, double cutoff,
                                                          double eta, const double *mu, float *e_out, double *c_out) {
    edges_dense_body<2>(xyz, reinterpret_cast<const float *>(cell), n, e_dim, cutoff, eta, mu, e_out, c_out);
}
