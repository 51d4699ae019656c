// epnn_coulomb_xyz_site, epnn_coulomb_xyz_cell_site, epnn_coulomb_xyz_slab_site and epnn_coulomb_xyz_slab_strain_site: the Coulomb calls
// with per-atom Gaussian widths, the Gaussians' self-energy and on-site terms (include/epnn.h has the sums).  The four entries alone:
// their arguments' checks and the per-atom rows are site_build (epnn_api_coulomb.hip.h), the width check of cells and slabs
// site_width_check (epnn_api_coulomb_cell.hip.h), and they enter through the _excl and slab entries' coulomb_enter, coulomb_cell_enter
// and coulomb_slab_enter into the one driver, coulomb_run.  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_coulomb_run.hip.h"

extern "C" int epnn_coulomb_xyz_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                     double ke, double alpha, const float *sigma, const float *chi, const float *hard, int self_term,
                                     int64_t npairs, const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale, float *q_out,
                                     float *phi_out, float *mu_out, double *e_out, float *f_out, float *ffix_out, float *fq_out) {
    const ExclArgs xa{npairs, ex_i, ex_j, ex_scale};
    const SiteArgs sa{sigma, chi, hard, self_term};
    return coulomb_enter(h, "epnn_coulomb_xyz_site", B, N, offsets, xyz, x, Q, ke, alpha, &xa,
                         CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, nullptr, nullptr, nullptr, mu_out}, &sa);
}

extern "C" int epnn_coulomb_xyz_cell_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                          const float *cell, const double *ewald, double ke, double alpha, const float *sigma, const float *chi,
                                          const float *hard, int self_term, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j,
                                          const float *ex_scale, float *q_out, float *phi_out, float *mu_out, double *e_out, float *f_out,
                                          float *gstrain_out, float *ffix_out, float *fq_out, float *gstrain_fix_out, float *gstrain_q_out) {
    const ExclArgs xa{npairs, ex_i, ex_j, ex_scale};
    const SiteArgs sa{sigma, chi, hard, self_term};
    return coulomb_cell_enter(h, "epnn_coulomb_xyz_cell_site", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, &xa,
                              CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, gstrain_out, gstrain_fix_out, gstrain_q_out, mu_out}, &sa);
}

extern "C" int epnn_coulomb_xyz_slab_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                          const float *cell, const double *ewald, double ke, double alpha, const float *sigma, const float *chi,
                                          const float *hard, int self_term, int64_t npairs, const int32_t *ex_i, const int32_t *ex_j,
                                          const float *ex_scale, float *q_out, float *phi_out, float *mu_out, double *e_out, float *f_out,
                                          float *ffix_out, float *fq_out) {
    const SiteArgs sa{sigma, chi, hard, self_term};
    return coulomb_slab_enter(h, "epnn_coulomb_xyz_slab_site", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, npairs, ex_i, ex_j, ex_scale,
                              false, CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, nullptr, nullptr, nullptr, mu_out}, &sa);
}

extern "C" int epnn_coulomb_xyz_slab_strain_site(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                                 const float *Q, const float *cell, const double *ewald, double ke, double alpha,
                                                 const float *sigma, const float *chi, const float *hard, int self_term, int64_t npairs,
                                                 const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale, float *q_out, float *phi_out,
                                                 float *mu_out, double *e_out, float *f_out, float *gstrain_out, float *ffix_out, float *fq_out,
                                                 float *gstrain_fix_out, float *gstrain_q_out) {
    const SiteArgs sa{sigma, chi, hard, self_term};
    return coulomb_slab_enter(h, "epnn_coulomb_xyz_slab_strain_site", B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, npairs, ex_i, ex_j,
                              ex_scale, true,
                              CoulombOut{q_out, phi_out, e_out, f_out, ffix_out, fq_out, gstrain_out, gstrain_fix_out, gstrain_q_out, mu_out}, &sa);
}
