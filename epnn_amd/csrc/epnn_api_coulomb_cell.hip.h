// epnn_coulomb_xyz_cell and epnn_coulomb_xyz_cell_excl: epnn_coulomb_xyz in fully periodic cells, by an Ewald sum (kernels:
// epnn_ewald.hip.h); epnn_ewald_params, the host-only rule that chooses the sum's parameters; and coulomb_run, the driver of all four
// Coulomb entries, which needs both kernel files.  The open entries reach it without a periodic part and keep their path, bits and scratch.
// Part of the one translation unit epnn_api.hip.
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

// The rule (include/epnn.h): s = sqrt(-ln tol), rc = w_min / 2, beta = s / rc, capped at alpha where alpha > 0 (there the real-space
// term vanishes identically: rc is reported as 0), kc = 2 beta s, M_k = ceil(kc |a_k| / 2 pi).  out [6] = beta, rc, kc, M0, M1, M2.
static int ew_rule(const char *what, int b, const float *cell, double alpha, double tol, double *out) {
    EwGeom G;
    if (ew_cell_geom(what, b, cell, G)) return 1;
    const double s = sqrt(-log(tol));
    double rc = 0.5 * G.wmin, beta = s / rc;
    if (alpha > 0.0 && alpha <= beta) { beta = alpha; rc = 0.0; }
    const double kc = 2.0 * beta * s;
    out[0] = beta; out[1] = rc; out[2] = kc;
    for (int k = 0; k < 3; ++k) out[3 + k] = ceil(kc * G.len[k] / 6.283185307179586);
    int ns;
    return ew_box_slots(what, b, out + 3, ns);
}

extern "C" int epnn_ewald_params(const float *cell, double alpha, double tol, double *out) {
    const char *name = "epnn_ewald_params";
    if (!cell || !out) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    if (!epnn_finite(tol) || !(tol > 0.0 && tol < 1.0)) EPNN_FAIL("%s: tol must be finite and inside (0, 1)", name);
    return ew_rule(name, 0, cell, alpha, tol, out);
}

// One checked row of the entry's `ewald` argument -> what the kernels take.  The entry runs at exactly these values.
static int ew_cell_row(const char *what, int b, const float *cell, const double *row, double alpha, EwCell &e) {
    EwGeom G;
    if (ew_cell_geom(what, b, cell, G)) return 1;
    for (int k = 0; k < 6; ++k)
        if (!epnn_finite(row[k])) EPNN_FAIL("%s: ewald[%d][%d] is not finite", what, b, k);
    const double beta = row[0], rc = row[1], kc = row[2], *M = row + 3;
    if (!(beta > 0.0)) EPNN_FAIL("%s: ewald[%d]: beta = %g must be positive", what, b, beta);
    if (!(kc >= 0.0)) EPNN_FAIL("%s: ewald[%d]: kc = %g must not be negative", what, b, kc);
    if (!(rc >= 0.0 && rc <= 0.5 * G.wmin))
        EPNN_FAIL("%s: ewald[%d]: rc = %g must lie in [0, w_min / 2]: half the smallest perpendicular width of cell %d is %g, and beyond "
                  "it a pair has more than one image in range", what, b, rc, b, 0.5 * G.wmin);
    if (rc == 0.0 && !(alpha > 0.0 && beta == alpha))
        EPNN_FAIL("%s: ewald[%d]: rc = 0 (no real-space part) takes beta == alpha > 0; beta = %g, alpha = %g", what, b, beta, alpha);
    for (int k = 0; k < 3; ++k) {
        const double need = ceil(kc * G.len[k] / 6.283185307179586 - 1e-9);
        if (!(M[k] >= 0.0 && M[k] <= 1e6 && M[k] == floor(M[k]) && M[k] >= need))
            EPNN_FAIL("%s: ewald[%d]: M%d = %g is not consistent with kc = %g: an integer of at least ceil(kc |a_%d| / 2 pi) = %g", what, b, k,
                      M[k], kc, k, need);
    }
    if (ew_box_slots(what, b, M, e.ns)) return 1;
    const double pi = 3.141592653589793;
    e.kc2 = kc * kc;
    e.c0 = 4.0 * pi / G.vol;
    e.inv4b2 = 0.25 / (beta * beta);
    e.self = 2.0 * beta / sqrt(pi);
    e.bg = pi / G.vol * (1.0 / (beta * beta) - (alpha > 0.0 ? 1.0 / (alpha * alpha) : 0.0));
    e.rc = (float)rc;
    if ((double)e.rc > rc) e.rc = nextafterf(e.rc, 0.f);
    e.beta = (float)beta;
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

// what a periodic entry adds to the driver's arguments: the cells' checked parameters, and the caller's list for excl_name_far
struct CoulombPeriodic {
    std::vector<EwCell> ew;
    const ExclArgs *xa;
};

// The driver of the four entries: the pair-list gradient call with its seed made on the device.  Set-up and checkpointed forward; on
// that forward's charges the sweep (per: the Ewald sum), the listed pairs' correction (ex) and the energy, phi = dE/dq into the
// seed; the shared backward; one download.
static int coulomb_run(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                       const HostGeo &geo, double ke, double alpha, CoulombPeriodic *per, const ExclCsr *ex, const CoulombOut &out) {
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int T = h->cfg.T, A = offsets[B];
    std::vector<int4> ctasks, atasks;
    std::vector<int2> stasks;
    const size_t cpieces = (size_t)cl_build_tasks(B, offsets, ctasks);
    size_t slots = 0;
    bool sweep = !per;
    if (per) {
        slots = ew_build_tasks(B, offsets, per->ew, atasks, stasks);
        if (slots > ((size_t)1 << 27)) EPNN_FAIL("%s: the batch's k boxes have %zu slots, above 2^27: send fewer cells per call", name, slots);
        for (int b = 0; b < B; ++b) sweep = sweep || per->ew[b].rc > 0.f;
    }
    // one staged span: the sweep's task table and, per, the two Ewald task tables and the cells' parameters, each at a multiple of 16 bytes
    const size_t o_at = ctasks.size() * sizeof(int4), o_st = o_at + atasks.size() * sizeof(int4),
                 o_ew = o_st + ((stasks.size() * sizeof(int2) + 15) & ~size_t(15)), blob_bytes = o_ew + (per ? (size_t)B * sizeof(EwCell) : 0);
    std::vector<char> blob(blob_bytes, 0);
    memcpy(blob.data(), ctasks.data(), ctasks.size() * sizeof(int4));
    if (per) {
        memcpy(blob.data() + o_at, atasks.data(), atasks.size() * sizeof(int4));
        memcpy(blob.data() + o_st, stasks.data(), stasks.size() * sizeof(int2));
        memcpy(blob.data() + o_ew, per->ew.data(), (size_t)B * sizeof(EwCell));
    }
    // [A] phi | [A][3] ffix | flag, then [B] E in float64 and, per, [B][9] the fixed-charge strain: directly behind the backward's output
    // block, one download for both; the sweep's partial rows [pieces][A][4 or EW_PART] and the atoms' shares [A][1 or EW_SHARE] in
    // float64, then, per, S and the slots' records
    const size_t o_E = (((size_t)A * 4 + 1) * 4 + 7) & ~size_t(7), o_gsf = o_E + (size_t)B * 8, co_bytes = o_gsf + (per ? (size_t)B * 36 : 0);
    const size_t o_share = cpieces * (size_t)A * (per ? EW_PART : 4) * 8, share_end = o_share + (size_t)A * (per ? EW_SHARE : 1) * 8,
                 o_S = (share_end + 15) & ~size_t(15), o_rec = o_S + slots * 16;
    // (the _excl entries: the CSR is one more span beside the blob, the correction's rows [A][4 or EW_PART] one more buffer behind the others)
    const GlSpan spans[2] = {GlSpan{blob.data(), blob_bytes, false}, GlSpan{ex ? ex->blob.data() : nullptr, ex ? ex->blob.size() : 0, false}};
    const size_t more[3] = {co_bytes, per ? o_rec + slots * 16 : share_end, ex ? excl_xpart_bytes(A, per != nullptr) : 0};
    GlGrad r;
    if (gl_grad_forward(h, gl, name, B, N, offsets, xyz, x, Q, geo, spans, ex ? 2 : 1, more, ex ? 3 : 2, false, r)) return 1;
    const GlCall &c = r.c;
    char *co = c.dw + r.o_more[0], *sc = c.dw + r.o_more[1];
    float *phi = reinterpret_cast<float *>(co), *ffix = phi + A, *gsf = reinterpret_cast<float *>(co + o_gsf);
    int *hit = reinterpret_cast<int *>(phi + 4 * (size_t)A);
    double *E = reinterpret_cast<double *>(co + o_E), *part = reinterpret_cast<double *>(sc), *share = reinterpret_cast<double *>(sc + o_share);
    double *xpart = ex ? reinterpret_cast<double *>(c.dw + r.o_more[2]) : nullptr;
    double2 *S = reinterpret_cast<double2 *>(sc + o_S);
    float4 *rec = reinterpret_cast<float4 *>(sc + o_rec);
    const float *q_dev = r.qck + (size_t)T * A;
    const char *d_blob = reinterpret_cast<const char *>(c.d_extra[0]), *d_csr = ex ? reinterpret_cast<const char *>(c.d_extra[1]) : nullptr;
    const int4 *d_ctasks = reinterpret_cast<const int4 *>(d_blob), *d_atasks = reinterpret_cast<const int4 *>(d_blob + o_at);
    const int2 *d_stasks = reinterpret_cast<const int2 *>(d_blob + o_st);
    const EwCell *d_ew = reinterpret_cast<const EwCell *>(d_blob + o_ew);
    const EpnnCell *d_cells = per ? c.geo.cells() : nullptr;
    const dim3 gsweep((unsigned)ctasks.size()), gatom((unsigned)atasks.size()), wave(64);
    // ---- the sum on the forward's own charges: phi is the backward's seed
    HIPCHK(hipMemsetAsync(hit, 0, 4, h->stream));
    if (!sweep)                                                  // beta == alpha in every cell: the real-space term vanishes identically
        HIPCHK(hipMemsetAsync(part, 0, o_share, h->stream));
    else if (per)
        hipLaunchKernelGGL((alpha > 0.0 ? k_ew_sweep<true> : k_ew_sweep<false>), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz,
                           q_dev, d_cells, d_ew, A, (float)alpha, part, hit);
    else
        hipLaunchKernelGGL((alpha > 0.0 ? k_cl_sweep<true> : k_cl_sweep<false>), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz,
                           q_dev, A, (float)alpha, part, hit);
    if (per) hipLaunchKernelGGL(k_ew_sfac, dim3((unsigned)stasks.size()), wave, 0, h->stream, d_stasks, c.d_moff, c.d_xyz, q_dev, d_cells, d_ew, S, rec);
    if (ex) excl_launch(h, c, d_csr, *ex, q_dev, d_cells, alpha, xpart, hit);     // (nothing of it depends on rc: it runs on a zeroed `part` too)
    if (per) {
        if (ex)
            hipLaunchKernelGGL(k_ew_atom_x, gatom, wave, 0, h->stream, d_atasks, A, c.d_xyz, q_dev, d_cells, d_ew, (const double2 *)S,
                               (const float4 *)rec, (const double *)part, (const double *)xpart, ke, r.gq, phi, ffix, share);
        else
            hipLaunchKernelGGL(k_ew_atom, gatom, wave, 0, h->stream, d_atasks, A, c.d_xyz, q_dev, d_cells, d_ew, (const double2 *)S,
                               (const float4 *)rec, (const double *)part, ke, r.gq, phi, ffix, share);
        hipLaunchKernelGGL(k_ew_energy, dim3((unsigned)B), wave, 0, h->stream, c.d_moff, d_cells, d_ew, (const double2 *)S, (const double *)share,
                           ke, E, gsf);
    } else {
        if (ex)
            hipLaunchKernelGGL(k_cl_atom_x, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, (const double *)part,
                               (const double *)xpart, ke, r.gq, phi, ffix, share);
        else
            hipLaunchKernelGGL(k_cl_atom, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, (const double *)part, ke, r.gq, phi,
                               ffix, share);
        hipLaunchKernelGGL(k_cl_energy, dim3((unsigned)B), wave, 0, h->stream, (const double *)share, c.d_moff, E);
    }
    HIPCHK(hipGetLastError());
    if (gl_grad_backward(h, gl, r, B, per != nullptr)) return 1;
    // ---- one download: q | gxyz | flag | the charges' strain rows (open: unused) | (the step to the next buffer) | phi | ffix | flag | E
    // | per: the fixed-charge strain
    const char *from = reinterpret_cast<const char *>(r.q_fin);
    const size_t nbytes = (size_t)(co + co_bytes - from), at_co = (size_t)(co - from);
    if (gl->pin_out.ensure(nbytes)) return 1;
    char *back = gl->pin_out.as<char>();
    HIPCHK(hipMemcpyAsync(back, from, nbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const float *bq = reinterpret_cast<const float *>(back), *bgx = bq + A, *bgs = bq + 4 * (size_t)A + 1,
                *bphi = reinterpret_cast<const float *>(back + at_co), *bffix = bphi + A, *bgsf = reinterpret_cast<const float *>(back + at_co + o_gsf);
    const int flag = reinterpret_cast<const int *>(bq)[4 * (size_t)A], chit = reinterpret_cast<const int *>(bphi)[4 * (size_t)A];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (per && flag == 0 && chit == CL_FLAG_FAR && ex && per->xa) return excl_name_far(name, offsets, xyz, geo, *per->xa);
    if (flag != 0 || chit != 0)
        EPNN_FAIL(per ? "%s: two atoms of a cell or their periodic images coincide (distance 0: neither the Coulomb terms nor the edge features "
                        "have a derivative there)"
                      : "%s: two atoms of a molecule coincide (distance 0: neither the Coulomb terms nor the edge features have a derivative there)",
                  name);
    memcpy(out.q, bq, (size_t)A * 4);
    memcpy(out.phi, bphi, (size_t)A * 4);
    memcpy(out.e, back + at_co + o_E, (size_t)B * 8);
    for (size_t k = 0; k < 3 * (size_t)A; ++k) {
        const float fq = -bgx[k];
        out.f[k] = bffix[k] + fq;
        if (out.fq) out.fq[k] = fq;
    }
    if (out.ffix) memcpy(out.ffix, bffix, (size_t)A * 12);
    if (!per) return 0;
    for (size_t k = 0; k < 9 * (size_t)B; ++k) out.gs[k] = bgsf[k] + bgs[k];
    if (out.gs_fix) memcpy(out.gs_fix, bgsf, (size_t)B * 36);
    if (out.gs_q) memcpy(out.gs_q, bgs, (size_t)B * 36);
    return 0;
}

static int coulomb_cell_enter(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                              const float *Q, const float *cell, const double *ewald, double ke, double alpha, const ExclArgs *xa,
                              const CoulombOut &out) {
    if (!cell || !ewald || !out.phi || !out.e || !out.gs) EPNN_FAIL("%s: null argument", name);
    if (!epnn_finite(ke)) EPNN_FAIL("%s: ke must be finite", name);
    if (!epnn_finite(alpha) || alpha < 0.0) EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    GeoArg arg;
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, cell, 1, out.q, out.f, arg)) return 1;
    CoulombPeriodic per{std::vector<EwCell>((size_t)B), xa};
    for (int b = 0; b < B; ++b)
        if (ew_cell_row(name, b, cell + 9 * (size_t)b, ewald + 6 * (size_t)b, alpha, per.ew[b])) return 1;
    ExclCsr ex;
    if (xa && excl_build(name, B, offsets, xa->npairs, xa->i, xa->j, xa->scale, ex)) return 1;
    return coulomb_run(h, name, B, N, offsets, xyz, x, Q, arg.geo, ke, alpha, &per, xa ? &ex : nullptr, out);
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

