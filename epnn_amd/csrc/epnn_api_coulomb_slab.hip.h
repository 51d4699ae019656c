// epnn_coulomb_xyz_slab: epnn_coulomb_xyz in slab cells (two periodic axes, one open one) by the exact two-dimensional Ewald sum
// (kernels: epnn_ewald_slab.hip.h); epnn_coulomb_xyz_slab_strain, the same call with the sum's strain derivative, on the same driver;
// and epnn_ewald_slab_params, the host-only rule that chooses the sum's parameters.  The driver is a
// sibling of coulomb_run: it shares gl_grad_forward, the open sweep's task table, k_ew_sweep, the exclusion list's kernel, the backward
// and the one download; the plain and periodic entries keep their driver.  Part of the one translation unit epnn_api.hip.
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
    const double s = sqrt(-log(tol));
    double rc = 0.5 * G.wmin, beta = s / rc;
    if (alpha > 0.0 && alpha <= beta) { beta = alpha; rc = 0.0; }
    const double kc = 2.0 * beta * s;
    out[0] = beta; out[1] = rc; out[2] = kc;
    out[3 + G.open] = 0.0;
    out[3 + G.pa] = ceil(kc * G.len[0] / 6.283185307179586);
    out[3 + G.pb] = ceil(kc * G.len[1] / 6.283185307179586);
    return sl_box_slots(what, b, out[3 + G.pa], out[3 + G.pb]);
}

extern "C" int epnn_ewald_slab_params(const float *cell, double alpha, double tol, double *out) {
    const char *name = "epnn_ewald_slab_params";
    if (!cell || !out) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    if (!epnn_finite(tol) || !(tol > 0.0 && tol < 1.0)) EPNN_FAIL("%s: tol must be finite and inside (0, 1)", name);
    return sl_rule(name, 0, cell, alpha, tol, out);
}

// One checked row of the entry's `ewald` argument -> what the kernels take: the sweep's (rc, beta) in an EwCell, the cell's SlCell, and
// its slots behind the batch's: the half plane m1 > 0, or m1 == 0 and m0 > 0, inside kc, m1 then m0 ascending, in float64.
static int sl_cell_row(const char *what, int b, const float *cell, const double *row, double alpha, EwCell &e, SlCell &c, std::vector<SlSlot> &slots) {
    SlGeom G;
    if (sl_cell_geom(what, b, cell, G)) return 1;
    for (int k = 0; k < 6; ++k)
        if (!epnn_finite(row[k])) EPNN_FAIL("%s: ewald[%d][%d] is not finite", what, b, k);
    const double beta = row[0], rc = row[1], kc = row[2], *M = row + 3;
    if (!(beta > 0.0)) EPNN_FAIL("%s: ewald[%d]: beta = %g must be positive", what, b, beta);
    if (!(kc >= 0.0)) EPNN_FAIL("%s: ewald[%d]: kc = %g must not be negative", what, b, kc);
    if (!(rc >= 0.0 && rc <= 0.5 * G.wmin))
        EPNN_FAIL("%s: ewald[%d]: rc = %g must lie in [0, w_min / 2]: half the smaller perpendicular width of cell %d is %g, and beyond "
                  "it a pair has more than one image in range", what, b, rc, b, 0.5 * G.wmin);
    if (rc == 0.0 && !(alpha > 0.0 && beta == alpha))
        EPNN_FAIL("%s: ewald[%d]: rc = 0 (no real-space part) takes beta == alpha > 0; beta = %g, alpha = %g", what, b, beta, alpha);
    if (M[G.open] != 0.0) EPNN_FAIL("%s: ewald[%d]: M%d = %g, but axis %d of cell %d is open: its M must be 0", what, b, G.open, M[G.open], G.open, b);
    const int rows[2] = {G.pa, G.pb};
    for (int t = 0; t < 2; ++t) {
        const int k = rows[t];
        const double need = ceil(kc * G.len[t] / 6.283185307179586 - 1e-9);
        if (!(M[k] >= 0.0 && M[k] <= 1e6 && M[k] == floor(M[k]) && M[k] >= need))
            EPNN_FAIL("%s: ewald[%d]: M%d = %g is not consistent with kc = %g: an integer of at least ceil(kc |a_%d| / 2 pi) = %g", what, b, k,
                      M[k], kc, k, need);
    }
    if (sl_box_slots(what, b, M[G.pa], M[G.pb])) return 1;
    const double pi = 3.141592653589793;
    memset(&e, 0, sizeof(e));
    e.rc = (float)rc;
    if ((double)e.rc > rc) e.rc = nextafterf(e.rc, 0.f);
    e.beta = (float)beta;
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

// The slab call: the pair-list gradient call with its seed made on the device, as coulomb_run.  Set-up and checkpointed forward; on that
// forward's charges the real-space sweep (k_ew_sweep), the reciprocal sweep (k_sl_sweep), the listed pairs' correction (ex) and the
// energy, phi = dE/dq into the seed; the shared backward; one download.  strain (epnn_coulomb_xyz_slab_strain): the reciprocal sweep is
// k_sl_sweep_strain with its wider rows, the atoms write their strain shares, one wavefront per cell adds them, the backward runs with
// its strain flag and the download carries both strain rows; without it the plain entry's kernels, bits and scratch.
static int coulomb_slab_run(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                            const float *Q, const HostGeo &geo, double ke, double alpha, const std::vector<EwCell> &ew,
                            const std::vector<SlCell> &sl, const std::vector<SlSlot> &slots, const ExclCsr *ex, const ExclArgs &xa,
                            bool strain, const CoulombOut &out) {
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int T = h->cfg.T, A = offsets[B];
    std::vector<int4> ctasks;
    const size_t cpieces = (size_t)cl_build_tasks(B, offsets, ctasks);
    bool sweep = false;
    for (int b = 0; b < B; ++b) sweep = sweep || ew[b].rc > 0.f;
    // one staged span: the sweeps' task table, the cells' parameters of either sweep and the slots, each at a multiple of 16 bytes
    const size_t o_ew = ctasks.size() * sizeof(int4), o_sl = o_ew + (((size_t)B * sizeof(EwCell) + 15) & ~size_t(15)),
                 o_slot = o_sl + (size_t)B * sizeof(SlCell), blob_bytes = o_slot + slots.size() * sizeof(SlSlot);
    std::vector<char> blob(blob_bytes, 0);
    memcpy(blob.data(), ctasks.data(), o_ew);
    memcpy(blob.data() + o_ew, ew.data(), (size_t)B * sizeof(EwCell));
    memcpy(blob.data() + o_sl, sl.data(), (size_t)B * sizeof(SlCell));
    if (!slots.empty()) memcpy(blob.data() + o_slot, slots.data(), slots.size() * sizeof(SlSlot));
    // [A] phi | [A][3] ffix | flag, then [B] E in float64: directly behind the backward's output block, one download for both; the two
    // sweeps' partial rows [pieces][A][EW_PART] and [pieces][A][SL_PART] and the atoms' energy shares [A] in float64.  strain: [B][9]
    // the fixed-charge strain behind E, rows of SL_PART_STRAIN, and the atoms' strain shares [A][SL_SHARE_W] behind the energy's
    const size_t o_E = (((size_t)A * 4 + 1) * 4 + 7) & ~size_t(7), o_gsf = o_E + (size_t)B * 8, co_bytes = o_gsf + (strain ? (size_t)B * 36 : 0);
    const size_t o_rpart = cpieces * (size_t)A * EW_PART * 8, o_share = o_rpart + cpieces * (size_t)A * (strain ? SL_PART_STRAIN : SL_PART) * 8,
                 o_wshare = o_share + (size_t)A * 8, sc_bytes = o_wshare + (strain ? (size_t)A * SL_SHARE_W * 8 : 0);
    const GlSpan spans[2] = {GlSpan{blob.data(), blob_bytes, false}, GlSpan{ex ? ex->blob.data() : nullptr, ex ? ex->blob.size() : 0, false}};
    const size_t more[3] = {co_bytes, sc_bytes, ex ? excl_xpart_bytes(A, true) : 0};
    GlGrad r;
    if (gl_grad_forward(h, gl, name, B, N, offsets, xyz, x, Q, geo, spans, ex ? 2 : 1, more, ex ? 3 : 2, false, r)) return 1;
    const GlCall &c = r.c;
    char *co = c.dw + r.o_more[0], *sc = c.dw + r.o_more[1];
    float *phi = reinterpret_cast<float *>(co), *ffix = phi + A, *gsf = reinterpret_cast<float *>(co + o_gsf);
    int *hit = reinterpret_cast<int *>(phi + 4 * (size_t)A);
    double *E = reinterpret_cast<double *>(co + o_E), *part = reinterpret_cast<double *>(sc), *rpart = reinterpret_cast<double *>(sc + o_rpart),
           *share = reinterpret_cast<double *>(sc + o_share), *wshare = reinterpret_cast<double *>(sc + o_wshare);
    double *xpart = ex ? reinterpret_cast<double *>(c.dw + r.o_more[2]) : nullptr;
    const float *q_dev = r.qck + (size_t)T * A;
    const char *d_blob = reinterpret_cast<const char *>(c.d_extra[0]), *d_csr = ex ? reinterpret_cast<const char *>(c.d_extra[1]) : nullptr;
    const int4 *d_ctasks = reinterpret_cast<const int4 *>(d_blob);
    const EwCell *d_ew = reinterpret_cast<const EwCell *>(d_blob + o_ew);
    const SlCell *d_sl = reinterpret_cast<const SlCell *>(d_blob + o_sl);
    const SlSlot *d_slots = reinterpret_cast<const SlSlot *>(d_blob + o_slot);
    const EpnnCell *d_cells = c.geo.cells();
    const dim3 gsweep((unsigned)ctasks.size()), wave(64);
    // ---- the sum on the forward's own charges: phi is the backward's seed
    HIPCHK(hipMemsetAsync(hit, 0, 4, h->stream));
    if (!sweep)                                                  // beta == alpha in every cell: the real-space term vanishes identically
        HIPCHK(hipMemsetAsync(part, 0, o_rpart, h->stream));
    else
        hipLaunchKernelGGL((alpha > 0.0 ? k_ew_sweep<true> : k_ew_sweep<false>), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz,
                           q_dev, d_cells, d_ew, A, (float)alpha, part, hit);
    hipLaunchKernelGGL((strain ? k_sl_sweep_strain : k_sl_sweep), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz, q_dev, d_sl,
                       d_slots, A, rpart);
    if (ex) excl_launch(h, c, d_csr, *ex, q_dev, d_cells, alpha, xpart, hit);
    if (strain) {
        hipLaunchKernelGGL(k_sl_atom_strain, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl, (const double *)part,
                           (const double *)rpart, (const double *)xpart, ke, r.gq, phi, ffix, share, wshare);
        hipLaunchKernelGGL(k_sl_energy_strain, dim3((unsigned)B), wave, 0, h->stream, (const double *)share, (const double *)wshare, c.d_moff, E, gsf);
    } else {
        if (ex)
            hipLaunchKernelGGL(k_sl_atom_x, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl, (const double *)part,
                               (const double *)rpart, (const double *)xpart, ke, r.gq, phi, ffix, share);
        else
            hipLaunchKernelGGL(k_sl_atom, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl, (const double *)part,
                               (const double *)rpart, ke, r.gq, phi, ffix, share);
        hipLaunchKernelGGL(k_cl_energy, dim3((unsigned)B), wave, 0, h->stream, (const double *)share, c.d_moff, E);
    }
    HIPCHK(hipGetLastError());
    if (gl_grad_backward(h, gl, r, B, strain)) return 1;
    // ---- one download: q | gxyz | flag | the charges' strain rows (plain: unused) | (the step to the next buffer) | phi | ffix | flag | E
    // | strain: the fixed-charge strain
    const char *from = reinterpret_cast<const char *>(r.q_fin);
    const size_t nbytes = (size_t)(co + co_bytes - from), at_co = (size_t)(co - from);
    if (gl->pin_out.ensure(nbytes)) return 1;
    char *back = gl->pin_out.as<char>();
    HIPCHK(hipMemcpyAsync(back, from, nbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const float *bq = reinterpret_cast<const float *>(back), *bgx = bq + A, *bphi = reinterpret_cast<const float *>(back + at_co), *bffix = bphi + A;
    const int flag = reinterpret_cast<const int *>(bq)[4 * (size_t)A], chit = reinterpret_cast<const int *>(bphi)[4 * (size_t)A];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (flag == 0 && chit == CL_FLAG_FAR && ex) return excl_name_far(name, offsets, xyz, geo, xa);
    if (flag != 0 || chit != 0)
        EPNN_FAIL("%s: two atoms of a cell or their periodic images coincide (distance 0: neither the Coulomb terms nor the edge features "
                  "have a derivative there)", name);
    memcpy(out.q, bq, (size_t)A * 4);
    memcpy(out.phi, bphi, (size_t)A * 4);
    memcpy(out.e, back + at_co + o_E, (size_t)B * 8);
    for (size_t k = 0; k < 3 * (size_t)A; ++k) {
        const float fq = -bgx[k];
        out.f[k] = bffix[k] + fq;
        if (out.fq) out.fq[k] = fq;
    }
    if (out.ffix) memcpy(out.ffix, bffix, (size_t)A * 12);
    if (!strain) return 0;
    const float *bgs = bq + 4 * (size_t)A + 1, *bgsf = reinterpret_cast<const float *>(back + at_co + o_gsf);
    for (size_t k = 0; k < 9 * (size_t)B; ++k) out.gs[k] = bgsf[k] + bgs[k];
    if (out.gs_fix) memcpy(out.gs_fix, bgsf, (size_t)B * 36);
    if (out.gs_q) memcpy(out.gs_q, bgs, (size_t)B * 36);
    return 0;
}

// the two slab entries: the checks, the cells' rows and slots, the list; out.gs: the strain entry's required output, or NULL
static int coulomb_slab_enter(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                              const float *Q, const float *cell, const double *ewald, double ke, double alpha, int64_t npairs,
                              const int32_t *ex_i, const int32_t *ex_j, const float *ex_scale, bool strain, const CoulombOut &out) {
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
    return coulomb_slab_run(h, name, B, N, offsets, xyz, x, Q, arg.geo, ke, alpha, ew, sl, slots, npairs > 0 ? &ex : nullptr, xa, strain, out);
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
