// epnn_coulomb_xyz_cell and epnn_coulomb_xyz_cell_excl: epnn_coulomb_xyz in fully periodic cells, by an Ewald sum (kernels:
// epnn_ewald.hip.h), and epnn_ewald_params, the host-only rule that chooses the sum's parameters.  Here: the cell's geometry, the rule
// and the check of an `ewald` row over a cell's periodic rows (shared with the slab entries), the tasks of the reciprocal passes and the
// two entries; the driver is coulomb_run (epnn_api_coulomb_run.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_coulomb.hip.h"
#include "epnn_ewald.hip.h"

// What the rule and the entry's checks need of one cell [3][3], in float64: |a_k|, the perpendicular widths |det| / |a_k+1 x a_k+2|,
// the smallest of them and the volume.  Refused in the style of check_cell: an entry that is not finite, an open axis, dependent rows.
struct EwGeom { double len[3], w[3], wmin, vol; };
static int ew_cell_geom(const char *what, int b, const float *cell, EwGeom &o) {
    double a[3][3];
    for (int k = 0; k < 3; ++k) {
        for (int x = 0; x < 3; ++x) {
            if (!epnn_finite(cell[3 * k + x])) EPNN_FAIL("%s: cell[%d][%d][%d] is not finite (molecule %d, axis %d)", what, b, k, x, b, k);
            a[k][x] = (double)cell[3 * k + x];
        }
        o.len[k] = sqrt(a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2]);
        if (!(o.len[k] > 0.0))
            EPNN_FAIL("%s: cell[%d] (molecule %d): axis %d is open (a row of zeros); the Ewald sum is built for fully periodic cells (two- "
                      "and one-dimensional sums are different mathematics)", what, b, b, k);
    }
    double cr[3][3];                                             // cr[k] = a_(k+1) x a_(k+2)
    for (int k = 0; k < 3; ++k) {
        const double *u = a[(k + 1) % 3], *v = a[(k + 2) % 3];
        cr[k][0] = u[1] * v[2] - u[2] * v[1]; cr[k][1] = u[2] * v[0] - u[0] * v[2]; cr[k][2] = u[0] * v[1] - u[1] * v[0];
    }
    const double det = a[0][0] * cr[0][0] + a[0][1] * cr[0][1] + a[0][2] * cr[0][2];
    if (!(fabs(det) > 1e-12 * o.len[0] * o.len[1] * o.len[2]))
        EPNN_FAIL("%s: the rows of cell[%d] (molecule %d) are linearly dependent (axis 2 lies in the plane of axes 0 and 1)", what, b, b);
    o.vol = fabs(det);
    for (int k = 0; k < 3; ++k) {
        o.w[k] = o.vol / sqrt(cr[k][0] * cr[k][0] + cr[k][1] * cr[k][1] + cr[k][2] * cr[k][2]);
        o.wmin = k == 0 ? o.w[0] : std::min(o.wmin, o.w[k]);
    }
    return 0;
}

// The k box of M: its slots, refused above EW_SLOT_CAP (a cell of extreme aspect ratio is refused by name, not served slowly)
static int ew_box_slots(const char *what, int b, const double *M, int &ns) {
    const double slots = (2.0 * M[0] + 1.0) * (2.0 * M[1] + 1.0) * (M[2] + 1.0);
    if (slots > (double)EW_SLOT_CAP)
        EPNN_FAIL("%s: cell[%d] (molecule %d): the k box M = (%g, %g, %g) has %g slots, above the cap of %d (the cell's aspect ratio is "
                  "too extreme for this sum, or tol too small)", what, b, b, M[0], M[1], M[2], slots, EW_SLOT_CAP);
    ns = (int)slots;
    return 0;
}

// The rule (include/epnn.h) over the n periodic rows of a cell, rows[t] of length len[t]: s = sqrt(-ln tol), rc = w_min / 2,
// beta = s / rc, capped at alpha where alpha > 0 (there the real-space term vanishes identically: rc is reported as 0), kc = 2 beta s,
// M_k = ceil(kc |a_k| / 2 pi).  out [6] = beta, rc, kc, M0, M1, M2; the M of a row that is not periodic is the caller's.
static double ew_mk(double kc, double len) { return kc * len / 6.283185307179586; }
static void ew_rule_rows(double wmin, int n, const int *rows, const double *len, double alpha, double tol, double *out) {
    const double s = sqrt(-log(tol));
    double rc = 0.5 * wmin, beta = s / rc;
    if (alpha > 0.0 && alpha <= beta) { beta = alpha; rc = 0.0; }
    const double kc = 2.0 * beta * s;
    out[0] = beta; out[1] = rc; out[2] = kc;
    for (int t = 0; t < n; ++t) out[3 + rows[t]] = ceil(ew_mk(kc, len[t]));
}
static const int EW_ROWS[3] = {0, 1, 2};
static int ew_rule(const char *what, int b, const float *cell, double alpha, double tol, double *out) {
    EwGeom G;
    if (ew_cell_geom(what, b, cell, G)) return 1;
    ew_rule_rows(G.wmin, 3, EW_ROWS, G.len, alpha, tol, out);
    int ns;
    return ew_box_slots(what, b, out + 3, ns);
}

// the arguments of the two rule entries, epnn_ewald_params and epnn_ewald_slab_params
static int ew_params_args(const char *name, const float *cell, const double *out, double alpha, double tol) {
    if (!cell || !out) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    if (!epnn_finite(tol) || !(tol > 0.0 && tol < 1.0)) EPNN_FAIL("%s: tol must be finite and inside (0, 1)", name);
    return 0;
}
extern "C" int epnn_ewald_params(const float *cell, double alpha, double tol, double *out) {
    const char *name = "epnn_ewald_params";
    return ew_params_args(name, cell, out, alpha, tol) || ew_rule(name, 0, cell, alpha, tol, out);
}

// One row [6] of an entry's `ewald` argument against its cell's n periodic rows, rows[t] of length len[t]: w_min is the `which`
// ("smallest" / "smaller") of the cell's perpendicular widths, open the row whose M must be 0 (slabs) or -1.  A row that passes sets
// the real-space sweep's part of e: rc, rounded down to float32, and beta.  The k box and its cap are the caller's.
static int ew_row_check(const char *what, int b, const double *row, double alpha, double wmin, const char *which, int n, const int *rows,
                        const double *len, int open, EwCell &e) {
    for (int k = 0; k < 6; ++k)
        if (!epnn_finite(row[k])) EPNN_FAIL("%s: ewald[%d][%d] is not finite", what, b, k);
    const double beta = row[0], rc = row[1], kc = row[2], *M = row + 3;
    if (!(beta > 0.0)) EPNN_FAIL("%s: ewald[%d]: beta = %g must be positive", what, b, beta);
    if (!(kc >= 0.0)) EPNN_FAIL("%s: ewald[%d]: kc = %g must not be negative", what, b, kc);
    if (!(rc >= 0.0 && rc <= 0.5 * wmin))
        EPNN_FAIL("%s: ewald[%d]: rc = %g must lie in [0, w_min / 2]: half the %s perpendicular width of cell %d is %g, and beyond "
                  "it a pair has more than one image in range", what, b, rc, which, b, 0.5 * wmin);
    if (rc == 0.0 && !(alpha > 0.0 && beta == alpha))
        EPNN_FAIL("%s: ewald[%d]: rc = 0 (no real-space part) takes beta == alpha > 0; beta = %g, alpha = %g", what, b, beta, alpha);
    if (open >= 0 && M[open] != 0.0)
        EPNN_FAIL("%s: ewald[%d]: M%d = %g, but axis %d of cell %d is open: its M must be 0", what, b, open, M[open], open, b);
    for (int t = 0; t < n; ++t) {
        const int k = rows[t];
        const double need = ceil(ew_mk(kc, len[t]) - 1e-9);
        if (!(M[k] >= 0.0 && M[k] <= 1e6 && M[k] == floor(M[k]) && M[k] >= need))
            EPNN_FAIL("%s: ewald[%d]: M%d = %g is not consistent with kc = %g: an integer of at least ceil(kc |a_%d| / 2 pi) = %g", what, b, k,
                      M[k], kc, k, need);
    }
    e.rc = (float)rc;
    if ((double)e.rc > rc) e.rc = nextafterf(e.rc, 0.f);
    e.beta = (float)beta;
    return 0;
}

// One checked row of the entry's `ewald` argument -> what the kernels take.  The entry runs at exactly these values.
static int ew_cell_row(const char *what, int b, const float *cell, const double *row, double alpha, EwCell &e) {
    EwGeom G;
    if (ew_cell_geom(what, b, cell, G) || ew_row_check(what, b, row, alpha, G.wmin, "smallest", 3, EW_ROWS, G.len, -1, e)) return 1;
    const double beta = row[0], kc = row[2], *M = row + 3;
    if (ew_box_slots(what, b, M, e.ns)) return 1;
    const double pi = 3.141592653589793;
    e.kc2 = kc * kc;
    e.c0 = 4.0 * pi / G.vol;
    e.inv4b2 = 0.25 / (beta * beta);
    e.self = 2.0 * beta / sqrt(pi);
    e.bg = pi / G.vol * (1.0 / (beta * beta) - (alpha > 0.0 ? 1.0 / (alpha * alpha) : 0.0));
    e.M0 = (int)M[0]; e.M1 = (int)M[1]; e.M2 = (int)M[2];
    e.soff = 0;
    e.pad = 0;
    return 0;
}

// The tasks of k_ew_atom, (first atom, atoms, cell, atoms of the cell), and of k_ew_sfac, (cell, first slot): 64 atoms or slots of
// one cell each; the cells' first slots.  Returns the batch's slots.
static size_t ew_build_tasks(int B, const int32_t *offsets, std::vector<EwCell> &ew, std::vector<int4> &atasks, std::vector<int2> &stasks) {
    size_t slots = 0;
    for (int b = 0; b < B; ++b) {
        const int lo = offsets[b], hi = offsets[b + 1];
        ew[b].soff = (int)std::min<size_t>(slots, 0x7fffffff);
        slots += (size_t)ew[b].ns;
        for (int a0 = lo; a0 < hi; a0 += EW_TILE) atasks.push_back(make_int4(a0, std::min(EW_TILE, hi - a0), b, hi - lo));
        for (int s0 = 0; s0 < ew[b].ns; s0 += EW_TILE) stasks.push_back(make_int2(b, s0));
    }
    return slots;
}
// The refusal behind the device's CL_FLAG_FAR: the first listed pair whose nearest image lies beyond half the smallest perpendicular
// width of its cell, found again on the host (the image of epnn_mic_cell, the width as k_cl_excl takes it: 1 / max_k |g_k|).
static int excl_name_far(const char *name, const int32_t *offsets, const float *xyz, const HostGeo &geo, const ExclArgs &xa) {
    const EpnnCell *cells = static_cast<const EpnnCell *>(geo.rows);
    for (int64_t p = 0; p < xa.npairs; ++p) {
        const int i = xa.i[p], j = xa.j[p];
        int b = 0;
        while (offsets[b + 1] <= i) ++b;
        const EpnnCell &c = cells[b];
        double d[3], n[3], g2 = 0.0;
        for (int k = 0; k < 3; ++k) d[k] = (double)xyz[3 * (size_t)i + k] - (double)xyz[3 * (size_t)j + k];
        for (int k = 0; k < 3; ++k) {
            n[k] = rint(c.g[3 * k] * d[0] + c.g[3 * k + 1] * d[1] + c.g[3 * k + 2] * d[2]);
            g2 = std::max(g2, c.g[3 * k] * c.g[3 * k] + c.g[3 * k + 1] * c.g[3 * k + 1] + c.g[3 * k + 2] * c.g[3 * k + 2]);
        }
        for (int k = 0; k < 3; ++k) d[k] -= n[0] * (double)c.a[k] + n[1] * (double)c.a[3 + k] + n[2] * (double)c.a[6 + k];
        const double D = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), half_w = 0.5 / sqrt(g2);
        if ((float)D > (float)half_w)
            EPNN_FAIL("%s: exclusion pair %lld = (%d, %d): its atoms are %g apart, beyond half the smallest perpendicular width of cell %d (%g): "
                      "past it the rounding rule no longer returns the nearest image (bonded atoms are never that far apart)", name,
                      (long long)p, i, j, D, b, half_w);
    }
    EPNN_FAIL("%s: an exclusion pair lies beyond half the smallest perpendicular width of its cell", name);
}

// The site entry's widths against a cell's split: the real-space term [erf(gamma_ij D) - erf(beta D)] / D is cut at rc, where only
// erfc(beta rc) is known to be under tol, so every gamma_ij must be at least beta: gamma_min = 1 / (2 sigma_max) >= beta.
static int site_width_check(const char *name, int b, double sigma_max, double beta) {
    if (sigma_max > 0.0 && !(0.5 / sigma_max >= beta))
        EPNN_FAIL("%s: cell %d: sigma_max = %g is above the largest width 1 / (2 beta) = %g its Ewald split allows (beta = %g): beyond it the "
                  "erf(gamma D) tail at rc is not under tol; a larger tol, or an ewald row with a smaller beta, moves the limit",
                  name, b, sigma_max, 0.5 / beta, beta);
    return 0;
}

static int coulomb_cell_enter(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                              const float *Q, const float *cell, const double *ewald, double ke, double alpha, const ExclArgs *xa,
                              const CoulombOut &out, const SiteArgs *sa = nullptr) {
    if (!cell || !ewald || !out.phi || !out.e || !out.gs) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(ke)) EPNN_FAIL("%s: ke must be finite", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    GeoArg arg;
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, cell, 1, out.q, out.f, arg)) return 1;
    std::vector<EwCell> ew((size_t)B);
    for (int b = 0; b < B; ++b)
        if (ew_cell_row(name, b, cell + 9 * (size_t)b, ewald + 6 * (size_t)b, alpha, ew[b])) return 1;
    ExclCsr ex;
    if (xa && excl_build(name, B, offsets, xa->npairs, xa->i, xa->j, xa->scale, ex)) return 1;
    CoulombSite site;
    if (sa && site_build(name, B, offsets, alpha, sa->sigma, sa->chi, sa->hard, sa->self_term, site)) return 1;
    for (int b = 0; sa && b < B; ++b)
        if (site_width_check(name, b, site.sigma_max[b], ewald[6 * (size_t)b])) return 1;
    if (sa && xa && xa->npairs == 0) xa = nullptr;                       // (a site entry takes its list or none: one entry per geometry)
    const CoulombSum sum{CL_CELL, true, &ew, nullptr, nullptr, xa};
    return coulomb_run(h, name, B, N, offsets, xyz, x, Q, arg.geo, ke, alpha, &sum, xa ? &ex : nullptr, out, site_plain(sa) ? nullptr : &site);
}

extern "C" int epnn_coulomb_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                     const float *cell, const double *ewald, double ke, double alpha, float *q_out, float *phi_out,
                                     double *e_out, float *f_out, float *gstrain_out, float *ffix_out, float *fq_out,
                                     float *gstrain_fix_out, float *gstrain_q_out) {
    return coulomb_cell_enter(h, "epnn_coulomb_xyz_cell", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, nullptr,
                              CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, gstrain_out, gstrain_fix_out, gstrain_q_out});
}

extern "C" int epnn_coulomb_xyz_cell_excl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                          const float *cell, const double *ewald, double ke, double alpha, int64_t npairs, const int32_t *ex_i,
                                          const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out, double *e_out, float *f_out,
                                          float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out) {
    const ExclArgs xa{npairs, ex_i, ex_j, ex_scale};
    return coulomb_cell_enter(h, "epnn_coulomb_xyz_cell_excl", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, &xa,
                              CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, gstrain_out, gstrain_fix_out, gstrain_q_out});
}
