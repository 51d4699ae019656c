// epnn_coulomb_xyz and epnn_coulomb_xyz_excl: charges, electrostatic potential, Coulomb energy and total forces of a flat coordinate
// batch in one call (kernels: epnn_coulomb.hip.h).  Here: the sweep's task table, the exclusion list's validator and CSR, and the two
// open entries; the driver they share with the periodic and the slab entries, coulomb_run, is defined in epnn_api_coulomb_run.hip.h.
// Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_grad.hip.h"
#include "epnn_api_jvp.hip.h"
#include "epnn_coulomb.hip.h"

// The sweep's tasks (k_cl_sweep): molecules of up to CL_BLOCK atoms whole and packed in batch order while they fit one wavefront,
// larger ones as blocks of CL_BLOCK atoms times cl_pieces(n) pieces of their partner range.  Returns the most pieces of a molecule.
static int cl_build_tasks(int B, const int32_t *offsets, std::vector<int4> &tasks) {
    int maxp = 1;
    for (int b = 0; b < B;) {
        const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
        if (n <= CL_BLOCK) {
            int b1 = b + 1;
            while (b1 < B && offsets[b1 + 1] - offsets[b1] <= CL_BLOCK && offsets[b1 + 1] - lo <= CL_BLOCK) ++b1;
            tasks.push_back(make_int4(lo, offsets[b1] - lo, lo, offsets[b1]));
            b = b1;
            continue;
        }
        const int np = cl_pieces(n), len = (n + np - 1) / np;
        maxp = std::max(maxp, np);
        for (int a0 = lo; a0 < hi; a0 += CL_BLOCK)
            for (int k = 0; k < np; ++k) {
                const int p0 = std::min(lo + k * len, hi), p1 = std::min(p0 + len, hi);
                tasks.push_back(make_int4(a0, std::min(CL_BLOCK, hi - a0) | (k << 8), p0, p1));
            }
        ++b;
    }
    return maxp;
}

// ---- bonded exclusions and pair scaling: the list of the two _excl entries, checked and turned into a CSR by atom.  One blob, staged
// as one span: row_off [A + 1] | partner [2 P] | factor [2 P] (= s - 1 in float32); every pair is entered in both directions and every
// row is sorted by partner, so the order of every sum is the CSR's and the caller's order cannot reach the bits.
struct ExclCsr {
    std::vector<char> blob;
    int A = 0;
    int64_t P = 0;
    size_t o_partner() const { return ((size_t)A + 1) * 4; }
    size_t o_factor() const { return o_partner() + 8 * (size_t)P; }
    const int *row_off() const { return reinterpret_cast<const int *>(blob.data()); }
    const int *partner() const { return reinterpret_cast<const int *>(blob.data() + o_partner()); }
    const float *factor() const { return reinterpret_cast<const float *>(blob.data() + o_factor()); }
};
// bytes of the staged CSR and of the kernel's row per atom (include/epnn.h quotes both)
static size_t excl_csr_bytes(int A, int64_t P) { return ((size_t)A + 1) * 4 + 16 * (size_t)P; }
static size_t excl_xpart_bytes(int A, bool cell) { return (size_t)A * (cell ? 10 : CL_XPART) * 8; }      // (10: EW_PART, asserted in epnn_ewald.hip.h)

// Refused by name, each with the pair's position in the list: a bad count, a NULL list, an index outside [0, A), i == j, atoms of two
// molecules, a factor that is not finite, a pair listed twice (in either order).  offsets are already checked.
static int excl_build(const char *name, int B, const int32_t *offsets, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j,
                      const float *ex_scale, ExclCsr &out) {
    const int A = offsets[B];
    if (npairs < 0) EPNN_FAIL("%s: npairs = %lld is negative", name, (long long)npairs);
    if (npairs > (int64_t)0x3fffffff) EPNN_FAIL("%s: npairs = %lld: 2 npairs must not exceed 2^31 - 1", name, (long long)npairs);
    if (npairs > 0 && (!ex_i || !ex_j || !ex_scale)) EPNN_FAIL("%s: a NULL exclusion list with npairs = %lld", name, (long long)npairs);
    std::vector<int> mol_of((size_t)A);
    for (int b = 0; b < B; ++b)
        for (int a = offsets[b]; a < offsets[b + 1]; ++a) mol_of[a] = b;
    out.A = A;
    out.P = npairs;
    out.blob.assign(excl_csr_bytes(A, npairs), 0);
    int *row_off = reinterpret_cast<int *>(out.blob.data());
    int *partner = reinterpret_cast<int *>(out.blob.data() + out.o_partner());
    float *factor = reinterpret_cast<float *>(out.blob.data() + out.o_factor());
    for (int64_t p = 0; p < npairs; ++p) {
        const int i = ex_i[p], j = ex_j[p];
        if (i < 0 || i >= A || j < 0 || j >= A)
            EPNN_FAIL("%s: exclusion pair %lld = (%d, %d): an atom index outside [0, %d)", name, (long long)p, i, j, A);
        if (i == j) EPNN_FAIL("%s: exclusion pair %lld = (%d, %d): an atom paired with itself", name, (long long)p, i, j);
        if (mol_of[i] != mol_of[j])
            EPNN_FAIL("%s: exclusion pair %lld = (%d, %d): the atoms are in different molecules (%d and %d)", name, (long long)p, i, j, mol_of[i],
                      mol_of[j]);
        if (!epnn_finite(ex_scale[p])) EPNN_FAIL("%s: exclusion pair %lld = (%d, %d): its factor is not finite", name, (long long)p, i, j);
        ++row_off[i + 1];
        ++row_off[j + 1];
    }
    for (int a = 0; a < A; ++a) row_off[a + 1] += row_off[a];
    // Rows sorted by partner without a sort: the directed entries go into their rows in list order first (partner, position), then
    // the atoms are walked in ascending order and every entry a -> j puts a into row j, so each row fills in ascending partner order.
    std::vector<int> cur(row_off, row_off + A), first(2 * (size_t)npairs), pos(2 * (size_t)npairs), where(2 * (size_t)npairs);
    for (int64_t p = 0; p < npairs; ++p) {
        const int ki = cur[ex_i[p]]++, kj = cur[ex_j[p]]++;
        first[ki] = ex_j[p]; pos[ki] = (int)p;
        first[kj] = ex_i[p]; pos[kj] = (int)p;
    }
    std::copy(row_off, row_off + A, cur.begin());
    for (int a = 0; a < A; ++a)
        for (int k = row_off[a]; k < row_off[a + 1]; ++k) {
            const int j = first[k], slot = cur[j]++;
            if (slot > row_off[j] && partner[slot - 1] == a) {
                const int64_t p1 = std::max(pos[k], where[slot - 1]), p0 = std::min(pos[k], where[slot - 1]);
                EPNN_FAIL("%s: exclusion pair %lld = (%d, %d) is listed twice: pair %lld names the same two atoms", name, (long long)p1, ex_i[p1],
                          ex_j[p1], (long long)p0);
            }
            partner[slot] = a;
            where[slot] = pos[k];
            factor[slot] = ex_scale[pos[k]] - 1.f;
        }
    return 0;
}
// the correction's launch: one lane per atom (k_cl_excl), on the stream, behind the sweep; d_cells: the periodic entries' cells, or NULL
// d_site: the site entries' per-atom rows when they carry widths (the pair term's third mode), or NULL
static void excl_launch(epnn_handle *h, const GlCall &c, const char *d_csr, const ExclCsr &ex, const float *q_dev, const EpnnCell *d_cells,
                        const float4 *d_site, double alpha, double *xpart, int *hit) {
    const int A = ex.A;
    const int *row_off = reinterpret_cast<const int *>(d_csr), *partner = reinterpret_cast<const int *>(d_csr + ex.o_partner());
    const float *factor = reinterpret_cast<const float *>(d_csr + ex.o_factor());
    auto *kern = d_cells ? (d_site ? k_cl_excl<CL_WIDTHS, true> : alpha > 0.0 ? k_cl_excl<CL_ERF, true> : k_cl_excl<CL_BARE, true>)
                         : (d_site ? k_cl_excl<CL_WIDTHS, false> : alpha > 0.0 ? k_cl_excl<CL_ERF, false> : k_cl_excl<CL_BARE, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)((A + 63) / 64)), dim3(64), 0, h->stream, A, c.d_molof, c.d_xyz, q_dev, row_off, partner, factor,
                       d_cells, d_site, (float)alpha, xpart, hit);
}

// what an _excl entry adds to its plain entry's arguments, and the outputs of the six entries (the strain rows: the entries with strain)
struct ExclArgs { int64_t npairs; const int32_t *i, *j; const float *scale; };
struct CoulombOut { float *q, *phi; double *e; float *f, *ffix, *fq, *gs, *gs_fix, *gs_q, *mu; };      // mu: the site entries' dE/dq, may be NULL

// ---- per-atom Gaussian widths, self-energy and on-site terms (epnn_coulomb_xyz_site, epnn_coulomb_xyz_cell_site): one float4 per atom,
// (w = 2 sigma^2, chi, J, gamma_ii), made in float64 and rounded once, staged as one more span.  widths: sigma was given and the pair
// terms take gamma_ij = 1 / sqrt(w_i + w_j); otherwise w = 0 and the call's alpha holds.  gamma_ii = 1 / (2 sigma_i), or alpha, with
// the self term and 0 without it.  sigma_max: per molecule, for the cells' width check.
struct CoulombSite {
    std::vector<float4> rows;
    std::vector<double> sigma_max;
    bool widths = false;
};
// Refused by name, each with the atom: sigma together with alpha > 0; a width that is not finite and positive, or whose 2 sigma^2 is not
// a positive finite float32; chi or J not finite; self_term other than 0 or 1, or 1 with neither sigma nor alpha > 0.
static int site_build(const char *name, int B, const int32_t *offsets, double alpha, const float *sigma, const float *chi, const float *hard,
                      int self_term, CoulombSite &out) {
    const int A = offsets[B];
    if (self_term != 0 && self_term != 1) EPNN_FAIL("%s: self_term = %d must be 0 or 1", name, self_term);
    if (sigma && alpha > 0.0)
        EPNN_FAIL("%s: both sigma and alpha = %g are given: per-atom widths take alpha == 0 (equal widths sigma are alpha = 1 / (2 sigma))", name,
                  alpha);
    if (self_term && !sigma && !(alpha > 0.0))
        EPNN_FAIL("%s: self_term = 1 with neither sigma nor alpha > 0: the self-energy of a point charge is infinite", name);
    out.widths = sigma != nullptr;
    out.rows.assign((size_t)A, make_float4(0.f, 0.f, 0.f, 0.f));
    out.sigma_max.assign((size_t)B, 0.0);
    for (int b = 0; b < B; ++b)
        for (int a = offsets[b]; a < offsets[b + 1]; ++a) {
            float4 &r = out.rows[a];
            double gii = alpha;
            if (sigma) {
                const double sg = (double)sigma[a];
                const float w = (float)(2.0 * sg * sg);
                if (!epnn_finite(sigma[a]) || !(sg > 0.0)) EPNN_FAIL("%s: sigma[%d] (molecule %d) must be finite and positive", name, a, b);
                if (!epnn_finite(w) || !(w > 0.f))
                    EPNN_FAIL("%s: sigma[%d] = %g (molecule %d): 2 sigma^2 is not a positive finite float32", name, a, sg, b);
                r.x = w;
                gii = 0.5 / sg;
                out.sigma_max[b] = std::max(out.sigma_max[b], sg);
            }
            if (chi) {
                if (!epnn_finite(chi[a])) EPNN_FAIL("%s: chi[%d] (molecule %d) is not finite", name, a, b);
                r.y = chi[a];
            }
            if (hard) {
                if (!epnn_finite(hard[a])) EPNN_FAIL("%s: hard[%d] (molecule %d) is not finite", name, a, b);
                r.z = hard[a];
            }
            r.w = self_term ? (float)gii : 0.f;
        }
    return 0;
}
// what a site entry adds to its _excl entry's arguments
struct SiteArgs { const float *sigma, *chi, *hard; int self_term; };

// What an entry adds to the open call: the kind of its sum, whether the strain rows are made, the cells' checked parameters (ew: the
// real-space sweep's; sl and slots: the slab's reciprocal sweep's, types of epnn_ewald_slab.hip.h) and the caller's list for excl_name_far.
struct EwCell;
struct SlCell;
struct SlSlot;
enum CoulombKind { CL_OPEN, CL_CELL, CL_SLAB };
struct CoulombSum {
    CoulombKind kind;
    bool strain;
    std::vector<EwCell> *ew;
    const std::vector<SlCell> *sl;
    const std::vector<SlSlot> *slots;
    const ExclArgs *xa;
};

// The one driver behind the six entries, defined in epnn_api_coulomb_run.hip.h, where the three kernel files are known; the open entries
// hand it no sum, and then it stages no cell parameters, launches no Ewald kernel and allocates no strain rows.
static int coulomb_run(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                       const HostGeo &geo, double ke, double alpha, const CoulombSum *sum, const ExclCsr *ex, const CoulombOut &out,
                       const CoulombSite *site = nullptr);

// sa: the site entry's arguments; with nothing in them the call is the _excl entry's (the existing kernels) and mu is phi
static bool site_plain(const SiteArgs *sa) { return !sa || (!sa->sigma && !sa->chi && !sa->hard && sa->self_term == 0); }
static int coulomb_enter(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                         double ke, double alpha, const ExclArgs *xa, const CoulombOut &out, const SiteArgs *sa = nullptr) {
    if (!out.phi || !out.e) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(ke)) EPNN_FAIL("%s: ke must be finite", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    GeoArg arg;                                                  // (open molecules: the entry takes no cell)
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, nullptr, 1, out.q, out.f, arg)) return 1;
    ExclCsr ex;
    if (xa && excl_build(name, B, offsets, xa->npairs, xa->i, xa->j, xa->scale, ex)) return 1;
    CoulombSite site;
    if (sa && site_build(name, B, offsets, alpha, sa->sigma, sa->chi, sa->hard, sa->self_term, site)) return 1;
    if (sa && xa && xa->npairs == 0) xa = nullptr;                       // (a site entry takes its list or none: one entry per geometry)
    return coulomb_run(h, name, B, N, offsets, xyz, x, Q, arg.geo, ke, alpha, nullptr, xa ? &ex : nullptr, out,
                       site_plain(sa) ? nullptr : &site);
}

extern "C" int epnn_coulomb_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                double ke, double alpha, float *q_out, float *phi_out, double *e_out, float *f_out, float *ffix_out,
                                float *fq_out) {
    return coulomb_enter(h, "epnn_coulomb_xyz", B, N, offsets, xyz, x, Q, ke, alpha, nullptr,
                         CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, nullptr, nullptr, nullptr});
}

extern "C" int epnn_coulomb_xyz_excl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                     double ke, double alpha, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale,
                                     float *q_out, float *phi_out, double *e_out, float *f_out, float *ffix_out, float *fq_out) {
    const ExclArgs xa{npairs, ex_i, ex_j, ex_scale};
    return coulomb_enter(h, "epnn_coulomb_xyz_excl", B, N, offsets, xyz, x, Q, ke, alpha, &xa,
                         CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, nullptr, nullptr, nullptr});
}
