// epnn_coulomb_xyz_slab: epnn_coulomb_xyz in slab cells (two periodic axes, one open one) by the exact two-dimensional Ewald sum
// (kernels: epnn_ewald_slab.hip.h); epnn_coulomb_xyz_slab_strain, the same call with the sum's strain derivative; and
// epnn_ewald_slab_params, the host-only rule that chooses the sum's parameters.  Here: the slab cell's geometry, the rule and the row
// check over its two periodic rows (ew_rule_rows, ew_row_check), the slot list and the two entries; the driver is coulomb_run
// (epnn_api_coulomb_run.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_coulomb_cell.hip.h"
#include "epnn_ewald_slab.hip.h"

// What the rule and the entry's checks need of one slab cell [3][3], in float64: its two periodic rows pa < pb and the open row, their
// lengths, the dual vectors (check_cell's formulas: the values of EpnnCell.g), the perpendicular widths 1 / |g|, A = |a x b| and nhat.
// Refused by name: an entry that is not finite, three periodic rows, fewer than two, dependent rows.
struct SlGeom { int pa, pb, open; double len[2], ga[3], gb[3], nh[3], wmin, area; };
static int sl_cell_geom(const char *what, int b, const float *cell, SlGeom &o) {
    double a[3][3];
    int per[3], m = 0;
    o.open = 0;
    for (int k = 0; k < 3; ++k) {
        bool nz = false;
        for (int x = 0; x < 3; ++x) {
            if (!epnn_finite(cell[3 * k + x])) EPNN_FAIL("%s: cell[%d][%d][%d] is not finite (molecule %d, axis %d)", what, b, k, x, b, k);
            a[k][x] = (double)cell[3 * k + x];
            nz = nz || cell[3 * k + x] != 0.f;
        }
        if (nz) per[m++] = k;
        else o.open = k;
    }
    if (m == 3)
        EPNN_FAIL("%s: cell[%d] (molecule %d) has three periodic axes: use epnn_coulomb_xyz_cell (the slab sum takes two periodic axes and one "
                  "row of zeros)", what, b, b);
    if (m < 2)
        EPNN_FAIL("%s: cell[%d] (molecule %d) has %d periodic ax%s: the sum for one periodic axis (wires) is not built, and open molecules "
                  "go to epnn_coulomb_xyz", what, b, b, m, m == 1 ? "is" : "es");
    o.pa = per[0];
    o.pb = per[1];
    const double *u = a[o.pa], *v = a[o.pb];
    o.len[0] = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    o.len[1] = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    o.area = sqrt(n2);
    if (!(o.area > 1e-12 * o.len[0] * o.len[1]))
        EPNN_FAIL("%s: rows %d and %d of cell[%d] (molecule %d) are linearly dependent (axis %d is parallel to axis %d)", what, o.pa, o.pb, b, b,
                  o.pb, o.pa);
    const double t0[3] = {v[1] * n[2] - v[2] * n[1], v[2] * n[0] - v[0] * n[2], v[0] * n[1] - v[1] * n[0]};       // a_q x n
    const double t1[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};       // n x a_p
    for (int x = 0; x < 3; ++x) { o.ga[x] = t0[x] / n2; o.gb[x] = t1[x] / n2; o.nh[x] = n[x] / o.area; }
    const double wa = 1.0 / sqrt(o.ga[0] * o.ga[0] + o.ga[1] * o.ga[1] + o.ga[2] * o.ga[2]),
                 wb = 1.0 / sqrt(o.gb[0] * o.gb[0] + o.gb[1] * o.gb[1] + o.gb[2] * o.gb[2]);
    o.wmin = std::min(wa, wb);
    return 0;
}

// The k box of the two periodic rows' M: its slots (2 M0' + 1)(M1' + 1), refused above SL_SLOT_CAP (every slot meets every pair)
static int sl_box_slots(const char *what, int b, double Ma, double Mb) {
    const double slots = (2.0 * Ma + 1.0) * (Mb + 1.0);
    if (slots > (double)SL_SLOT_CAP)
        EPNN_FAIL("%s: cell[%d] (molecule %d): the k box M = (%g, %g) of the two periodic rows has %g slots, above the cap of %d (the cell's "
                  "aspect ratio is too extreme for this sum, or tol too small)", what, b, b, Ma, Mb, slots, SL_SLOT_CAP);
    return 0;
}

// The rule (include/epnn.h): that of epnn_ewald_params over the two periodic rows; M of the open row is 0.
static int sl_rule(const char *what, int b, const float *cell, double alpha, double tol, double *out) {
    SlGeom G;
    if (sl_cell_geom(what, b, cell, G)) return 1;
    const int rows[2] = {G.pa, G.pb};
    out[3 + G.open] = 0.0;
    ew_rule_rows(G.wmin, 2, rows, G.len, alpha, tol, out);
    return sl_box_slots(what, b, out[3 + G.pa], out[3 + G.pb]);
}

extern "C" int epnn_ewald_slab_params(const float *cell, double alpha, double tol, double *out) {
    const char *name = "epnn_ewald_slab_params";
    return ew_params_args(name, cell, out, alpha, tol) || sl_rule(name, 0, cell, alpha, tol, out);
}

// One checked row of the entry's `ewald` argument -> what the kernels take: the sweep's (rc, beta) in an EwCell, the cell's SlCell, and
// its slots behind the batch's: the half plane m1 > 0, or m1 == 0 and m0 > 0, inside kc, m1 then m0 ascending, in float64.
static int sl_cell_row(const char *what, int b, const float *cell, const double *row, double alpha, EwCell &e, SlCell &c, std::vector<SlSlot> &slots) {
    SlGeom G;
    if (sl_cell_geom(what, b, cell, G)) return 1;
    const int rows[2] = {G.pa, G.pb};
    memset(&e, 0, sizeof(e));
    if (ew_row_check(what, b, row, alpha, G.wmin, "smaller", 2, rows, G.len, G.open, e)) return 1;
    const double beta = row[0], kc = row[2], *M = row + 3;
    if (sl_box_slots(what, b, M[G.pa], M[G.pb])) return 1;
    const double pi = 3.141592653589793;
    memset(&c, 0, sizeof(c));
    for (int x = 0; x < 3; ++x) { c.ga[x] = G.ga[x]; c.gb[x] = G.gb[x]; c.nh[x] = G.nh[x]; }
    c.beta = beta;
    c.c0 = 2.0 * sqrt(pi) / G.area;
    c.cn = 2.0 * pi / G.area;
    c.self = 2.0 * beta / sqrt(pi);
    c.soff = (int)slots.size();
    const int Ma = (int)M[G.pa], Mb = (int)M[G.pb];
    for (int m1 = 0; m1 <= Mb; ++m1)
        for (int m0 = (m1 == 0 ? 1 : -Ma); m0 <= Ma; ++m0) {
            double kv[3];
            for (int x = 0; x < 3; ++x) kv[x] = 2.0 * pi * ((double)m0 * G.ga[x] + (double)m1 * G.gb[x]);
            const double k = sqrt(kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2]);
            if (k > kc) continue;
            const double u = 0.5 * k / beta, w = 2.0 * pi / (G.area * k) * exp(-u * u);
            slots.push_back(SlSlot{(double)m0, (double)m1, k, u, (float)w, (float)(w * k), (float)kv[0], (float)kv[1], (float)kv[2], (float)(1.0 / k)});
        }
    c.ns = (int)slots.size() - c.soff;
    return 0;
}

// the slab entries: the checks, the cells' rows and slots, the list; out.gs: the strain entries' required output, or NULL.  sa: the
// _site entries' arguments (epnn_api_site.hip.h): the per-atom rows and the slab case of the width check, sigma_max against the row's beta;
// with nothing in them the call is the plain entry's (the existing kernels) and mu is phi
static int coulomb_slab_enter(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                              const float *Q, const float *cell, const double *ewald, double ke, double alpha, int64_t npairs,
                              const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale, bool strain, const CoulombOut &out,
                              const SiteArgs *sa = nullptr) {
    if (!cell || !ewald || !out.phi || !out.e || (strain && !out.gs)) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(ke)) EPNN_FAIL("%s: ke must be finite", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    GeoArg arg;
    if (h && offsets && B >= 1) {                                // (the slab's own refusals come before the cell's general checks)
        SlGeom G;
        for (int b = 0; b < B; ++b)
            if (sl_cell_geom(name, b, cell + 9 * (size_t)b, G)) return 1;
    }
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, cell, 1, out.q, out.f, arg)) return 1;
    std::vector<EwCell> ew((size_t)B);
    std::vector<SlCell> sl((size_t)B);
    std::vector<SlSlot> slots;
    for (int b = 0; b < B; ++b) {
        if (sl_cell_row(name, b, cell + 9 * (size_t)b, ewald + 6 * (size_t)b, alpha, ew[b], sl[b], slots)) return 1;
        if (slots.size() > ((size_t)1 << 24)) EPNN_FAIL("%s: the batch's k slots exceed 2^24: send fewer cells per call", name);
    }
    const ExclArgs xa{npairs, ex_i, ex_j, ex_scale};
    ExclCsr ex;
    if (excl_build(name, B, offsets, npairs, ex_i, ex_j, ex_scale, ex)) return 1;
    CoulombSite site;
    if (sa && site_build(name, B, offsets, alpha, sa->sigma, sa->chi, sa->hard, sa->self_term, site)) return 1;
    for (int b = 0; sa && b < B; ++b)
        if (site_width_check(name, b, site.sigma_max[b], ewald[6 * (size_t)b])) return 1;
    const CoulombSum sum{CL_SLAB, strain, &ew, &sl, &slots, &xa};
    return coulomb_run(h, name, B, N, offsets, xyz, x, Q, arg.geo, ke, alpha, &sum, npairs > 0 ? &ex : nullptr, out,
                       site_plain(sa) ? nullptr : &site);
}

extern "C" int epnn_coulomb_xyz_slab(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                     const float *cell, const double *ewald, double ke, double alpha, int64_t npairs, const int32_t *ex_i,
                                     const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out, double *e_out, float *f_out,
                                     float *ffix_out, float *fq_out) {
    return coulomb_slab_enter(h, "epnn_coulomb_xyz_slab", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, npairs, ex_i, ex_j, ex_scale, false,
                              CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, nullptr, nullptr, nullptr});
}

extern "C" int epnn_coulomb_xyz_slab_strain(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                            const float *cell, const double *ewald, double ke, double alpha, int64_t npairs, const int32_t *ex_i,
                                            const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out, double *e_out, float *f_out,
                                            float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out) {
    return coulomb_slab_enter(h, "epnn_coulomb_xyz_slab_strain", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, npairs, ex_i, ex_j, ex_scale,
                              true, CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, gstrain_out, gstrain_fix_out, gstrain_q_out});
}
