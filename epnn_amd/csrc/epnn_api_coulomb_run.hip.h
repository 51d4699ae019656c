// coulomb_run, the one host driver of the six Coulomb entries (open: epnn_api_coulomb.hip.h, fully periodic cells:
// epnn_api_coulomb_cell.hip.h, slabs: epnn_api_coulomb_slab.hip.h), and the layout of what it stages and allocates.  It sits behind the
// three entry files because it launches the kernels of all three families.  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_coulomb_slab.hip.h"

// consecutive offsets at a stated alignment (a power of two): append a segment of `bytes` behind `end`, get its offset
static size_t seg_add(size_t &end, size_t bytes, size_t align = 1) {
    const size_t o = (end + align - 1) & ~(align - 1);
    end = o + bytes;
    return o;
}

// The byte offsets of one call (include/epnn.h quotes the sums; epnn_last_stats reports them).  A segment a kind does not have is absent,
// not empty: nothing is rounded for it.
//   blob, the one staged span: ctasks | cell: atasks | stasks | kinds with cells: EwCell [B] at 16 | slab: SlCell [B] at 16 | SlSlot []
//   co, directly behind the backward's output block, one download for both: [A] phi | [A][3] ffix | flag | [B] E in float64 at 8 |
//       strain: [B][9] the fixed-charge strain | site: [A] mu
//   sc, float64: part [pieces][A][4 or EW_PART] | slab: rpart [pieces][A][SL_PART or SL_PART_STRAIN] | share [A][1, cell: EW_SHARE] |
//       slab with strain: wshare [A][SL_SHARE_W] | cell: S [slots] at 16 | rec [slots] | cell with site: wsum [B]
//   site, one more staged span of the site entries: [A] float4 = (2 sigma^2, chi, J, gamma_ii)
struct CoulombLayout {
    size_t atasks, stasks, ew, sl, slot, blob_bytes;
    size_t E, gsf, mu, co_bytes;
    size_t part_bytes, rpart, share, wshare, S, rec, wsum, sc_bytes;
    size_t site_bytes;
};
static CoulombLayout coulomb_layout(CoulombKind kind, bool strain, size_t A, size_t B, size_t nctasks, size_t natasks, size_t nstasks,
                                    size_t cpieces, size_t slots, bool site = false) {
    CoulombLayout L{};
    size_t end = 0;
    seg_add(end, nctasks * sizeof(int4));
    if (kind == CL_CELL) {
        L.atasks = seg_add(end, natasks * sizeof(int4));
        L.stasks = seg_add(end, nstasks * sizeof(int2));
    }
    if (kind != CL_OPEN) L.ew = seg_add(end, B * sizeof(EwCell), 16);
    if (kind == CL_SLAB) {
        L.sl = seg_add(end, B * sizeof(SlCell), 16);
        L.slot = seg_add(end, slots * sizeof(SlSlot));
    }
    L.blob_bytes = end;
    end = 0;
    seg_add(end, (A * 4 + 1) * 4);
    L.E = seg_add(end, B * 8, 8);
    L.gsf = seg_add(end, strain ? B * 36 : 0);
    if (site) L.mu = seg_add(end, A * 4);
    L.co_bytes = end;
    end = 0;
    seg_add(end, L.part_bytes = cpieces * A * (kind == CL_OPEN ? 4 : EW_PART) * 8);
    if (kind == CL_SLAB) L.rpart = seg_add(end, cpieces * A * (strain ? SL_PART_STRAIN : SL_PART) * 8);
    L.share = seg_add(end, A * (kind == CL_CELL ? EW_SHARE : 1) * 8);
    if (kind == CL_SLAB && strain) L.wshare = seg_add(end, A * SL_SHARE_W * 8);
    if (kind == CL_CELL) {
        L.S = seg_add(end, slots * 16, 16);
        L.rec = seg_add(end, slots * 16);
        if (site) L.wsum = seg_add(end, B * 8);
    }
    L.sc_bytes = end;
    L.site_bytes = site ? A * sizeof(float4) : 0;
    return L;
}

// The driver of the six entries: the pair-list gradient call with its seed made on the device.  Set-up and checkpointed forward; on
// that forward's charges the real-space sweep, the listed pairs' correction (ex), the rest of the sum by its kind and the energy,
// phi = dE/dq into the seed; the shared backward; one download.  sum->strain: the fixed-charge strain rows are made, the backward runs
// with its strain flag and the download carries both strain rows (the cells' entries always, the slab's strain entries).  site (every
// kind): the per-atom rows of the site entries; the atoms' kernels are the _site ones, the seed is mu, and with widths the real-space
// sweeps too (slabs: k_ew_sweep_site, as in cells; the reciprocal and k = 0 sweep is the point charges', unchanged).
static int coulomb_run(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                       const HostGeo &geo, double ke, double alpha, const CoulombSum *sum, const ExclCsr *ex, const CoulombOut &out,
                       const CoulombSite *site) {
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const CoulombKind kind = sum ? sum->kind : CL_OPEN;
    const bool strain = sum && sum->strain;
    const int T = h->cfg.T, A = offsets[B];
    std::vector<int4> ctasks, atasks;
    std::vector<int2> stasks;
    const size_t cpieces = (size_t)cl_build_tasks(B, offsets, ctasks);
    size_t slots = kind == CL_SLAB ? sum->slots->size() : 0;
    if (kind == CL_CELL) {
        slots = ew_build_tasks(B, offsets, *sum->ew, atasks, stasks);
        if (slots > ((size_t)1 << 27)) EPNN_FAIL("%s: the batch's k boxes have %zu slots, above 2^27: send fewer cells per call", name, slots);
    }
    bool sweep = kind == CL_OPEN;
    for (int b = 0; sum && b < B; ++b) sweep = sweep || (*sum->ew)[b].rc > 0.f;
    const CoulombLayout L = coulomb_layout(kind, strain, (size_t)A, (size_t)B, ctasks.size(), atasks.size(), stasks.size(), cpieces, slots,
                                           site != nullptr);
    std::vector<char> blob(L.blob_bytes, 0);
    memcpy(blob.data(), ctasks.data(), ctasks.size() * sizeof(int4));
    if (kind == CL_CELL) {
        memcpy(blob.data() + L.atasks, atasks.data(), atasks.size() * sizeof(int4));
        memcpy(blob.data() + L.stasks, stasks.data(), stasks.size() * sizeof(int2));
    }
    if (sum) memcpy(blob.data() + L.ew, sum->ew->data(), (size_t)B * sizeof(EwCell));
    if (kind == CL_SLAB) {
        memcpy(blob.data() + L.sl, sum->sl->data(), (size_t)B * sizeof(SlCell));
        if (slots) memcpy(blob.data() + L.slot, sum->slots->data(), slots * sizeof(SlSlot));
    }
    // (the entries with a list: the CSR is one more span beside the blob, the correction's rows [A][4 or EW_PART] one more buffer behind the others)
    // (the site entries: the atoms' rows are a third span; without a list the second one is empty)
    const GlSpan spans[3] = {GlSpan{blob.data(), L.blob_bytes, false}, GlSpan{ex ? ex->blob.data() : nullptr, ex ? ex->blob.size() : 0, false},
                             GlSpan{site ? site->rows.data() : nullptr, L.site_bytes, false}};
    const size_t more[3] = {L.co_bytes, L.sc_bytes, ex ? excl_xpart_bytes(A, sum != nullptr) : 0};
    GlGrad r;
    if (gl_grad_forward(h, gl, name, B, N, offsets, xyz, x, Q, geo, 1, spans, site ? 3 : ex ? 2 : 1, more, ex ? 3 : 2, false, r)) return 1;
    const GlCall &c = r.c;
    char *co = c.dw + r.o_more[0], *sc = c.dw + r.o_more[1];
    float *phi = reinterpret_cast<float *>(co), *ffix = phi + A, *gsf = reinterpret_cast<float *>(co + L.gsf);
    int *hit = reinterpret_cast<int *>(phi + 4 * (size_t)A);
    double *E = reinterpret_cast<double *>(co + L.E), *part = reinterpret_cast<double *>(sc), *rpart = reinterpret_cast<double *>(sc + L.rpart),
           *share = reinterpret_cast<double *>(sc + L.share), *wshare = reinterpret_cast<double *>(sc + L.wshare);
    double *xpart = ex ? reinterpret_cast<double *>(c.dw + r.o_more[2]) : nullptr;
    double2 *S = reinterpret_cast<double2 *>(sc + L.S);
    float4 *rec = reinterpret_cast<float4 *>(sc + L.rec);
    float *mu = reinterpret_cast<float *>(co + L.mu);
    double *wsum = reinterpret_cast<double *>(sc + L.wsum);
    const float4 *d_site = site ? reinterpret_cast<const float4 *>(c.d_extra[2]) : nullptr, *d_wid = site && site->widths ? d_site : nullptr;
    const float *q_dev = r.qck + (size_t)T * A;
    const char *d_blob = reinterpret_cast<const char *>(c.d_extra[0]), *d_csr = ex ? reinterpret_cast<const char *>(c.d_extra[1]) : nullptr;
    const int4 *d_ctasks = reinterpret_cast<const int4 *>(d_blob), *d_atasks = reinterpret_cast<const int4 *>(d_blob + L.atasks);
    const int2 *d_stasks = reinterpret_cast<const int2 *>(d_blob + L.stasks);
    const EwCell *d_ew = reinterpret_cast<const EwCell *>(d_blob + L.ew);
    const SlCell *d_sl = reinterpret_cast<const SlCell *>(d_blob + L.sl);
    const SlSlot *d_slots = reinterpret_cast<const SlSlot *>(d_blob + L.slot);
    const EpnnCell *d_cells = sum ? c.geo.cells() : nullptr;
    const dim3 gsweep((unsigned)ctasks.size()), gatom((unsigned)atasks.size()), gmol((unsigned)B), wave(64);
    // ---- the sum on the forward's own charges: phi is the backward's seed
    HIPCHK(hipMemsetAsync(hit, 0, 4, h->stream));
    if (!sweep)                                                  // beta == alpha in every cell: the real-space term vanishes identically
        HIPCHK(hipMemsetAsync(part, 0, L.part_bytes, h->stream));
    else if (d_wid && sum)
        hipLaunchKernelGGL(k_ew_sweep_site, gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz, q_dev, d_wid, d_cells, d_ew, A, part,
                           hit);
    else if (d_wid)
        hipLaunchKernelGGL(k_cl_sweep_site, gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz, q_dev, d_wid, A, part, hit);
    else if (sum)
        hipLaunchKernelGGL((alpha > 0.0 ? k_ew_sweep<true> : k_ew_sweep<false>), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz,
                           q_dev, d_cells, d_ew, A, (float)alpha, part, hit);
    else
        hipLaunchKernelGGL((alpha > 0.0 ? k_cl_sweep<true> : k_cl_sweep<false>), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz,
                           q_dev, A, (float)alpha, part, hit);
    if (ex) excl_launch(h, c, d_csr, *ex, q_dev, d_cells, d_wid, alpha, xpart, hit);     // (nothing of it depends on rc: it runs on a zeroed `part` too)
    switch (kind) {
    case CL_OPEN:
        if (site)
            hipLaunchKernelGGL((ex ? k_cl_atom_site<true> : k_cl_atom_site<false>), dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev,
                               (const double *)part, (const double *)xpart, d_site, ke, r.gq, phi, mu, ffix, share);
        else if (ex)
            hipLaunchKernelGGL(k_cl_atom_x, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, (const double *)part,
                               (const double *)xpart, ke, r.gq, phi, ffix, share);
        else
            hipLaunchKernelGGL(k_cl_atom, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, (const double *)part, ke, r.gq, phi,
                               ffix, share);
        hipLaunchKernelGGL(k_cl_energy, gmol, wave, 0, h->stream, (const double *)share, c.d_moff, E);
        break;
    case CL_CELL:
        hipLaunchKernelGGL(k_ew_sfac, dim3((unsigned)stasks.size()), wave, 0, h->stream, d_stasks, c.d_moff, c.d_xyz, q_dev, d_cells, d_ew, S, rec);
        if (site) {
            hipLaunchKernelGGL(k_ew_wsum, gmol, wave, 0, h->stream, c.d_moff, q_dev, d_site, wsum);
            hipLaunchKernelGGL((ex ? k_ew_atom_site<true> : k_ew_atom_site<false>), gatom, wave, 0, h->stream, d_atasks, A, c.d_xyz, q_dev, d_cells,
                               d_ew, (const double2 *)S, (const float4 *)rec, (const double *)part, (const double *)xpart, d_site,
                               (const double *)wsum, ke, r.gq, phi, mu, ffix, share);
            hipLaunchKernelGGL(k_ew_energy_site, gmol, wave, 0, h->stream, c.d_moff, d_cells, d_ew, (const double2 *)S, (const double *)share,
                               (const double *)wsum, ke, E, gsf);
            break;
        }
        if (ex)
            hipLaunchKernelGGL(k_ew_atom_x, gatom, wave, 0, h->stream, d_atasks, A, c.d_xyz, q_dev, d_cells, d_ew, (const double2 *)S,
                               (const float4 *)rec, (const double *)part, (const double *)xpart, ke, r.gq, phi, ffix, share);
        else
            hipLaunchKernelGGL(k_ew_atom, gatom, wave, 0, h->stream, d_atasks, A, c.d_xyz, q_dev, d_cells, d_ew, (const double2 *)S,
                               (const float4 *)rec, (const double *)part, ke, r.gq, phi, ffix, share);
        hipLaunchKernelGGL(k_ew_energy, gmol, wave, 0, h->stream, c.d_moff, d_cells, d_ew, (const double2 *)S, (const double *)share, ke, E, gsf);
        break;
    case CL_SLAB:
        hipLaunchKernelGGL((strain ? k_sl_sweep_strain : k_sl_sweep), gsweep, wave, 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz, q_dev, d_sl,
                           d_slots, A, rpart);
        if (site) {                                              // (the sweeps above are the point charges': the site terms are the atoms' alone)
            if (strain) {
                hipLaunchKernelGGL(k_sl_atom_strain_site, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl,
                                   (const double *)part, (const double *)rpart, (const double *)xpart, d_site, ke, r.gq, phi, mu, ffix, share,
                                   wshare);
                hipLaunchKernelGGL(k_sl_energy_strain, gmol, wave, 0, h->stream, (const double *)share, (const double *)wshare, c.d_moff, E, gsf);
                break;
            }
            hipLaunchKernelGGL((ex ? k_sl_atom_site<true> : k_sl_atom_site<false>), dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof,
                               q_dev, d_sl, (const double *)part, (const double *)rpart, (const double *)xpart, d_site, ke, r.gq, phi, mu, ffix,
                               share);
            hipLaunchKernelGGL(k_cl_energy, gmol, wave, 0, h->stream, (const double *)share, c.d_moff, E);
            break;
        }
        if (strain) {
            hipLaunchKernelGGL(k_sl_atom_strain, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl, (const double *)part,
                               (const double *)rpart, (const double *)xpart, ke, r.gq, phi, ffix, share, wshare);
            hipLaunchKernelGGL(k_sl_energy_strain, gmol, wave, 0, h->stream, (const double *)share, (const double *)wshare, c.d_moff, E, gsf);
            break;
        }
        if (ex)
            hipLaunchKernelGGL(k_sl_atom_x, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl, (const double *)part,
                               (const double *)rpart, (const double *)xpart, ke, r.gq, phi, ffix, share);
        else
            hipLaunchKernelGGL(k_sl_atom, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, d_sl, (const double *)part,
                               (const double *)rpart, ke, r.gq, phi, ffix, share);
        hipLaunchKernelGGL(k_cl_energy, gmol, wave, 0, h->stream, (const double *)share, c.d_moff, E);
        break;
    }
    HIPCHK(hipGetLastError());
    if (gl_grad_backward(h, gl, r, B, strain)) return 1;
    // ---- one download: q | gxyz | flag | the charges' strain rows (without strain: unused) | (the step to the next buffer) | phi | ffix
    // | flag | E | strain: the fixed-charge strain
    const char *from = reinterpret_cast<const char *>(r.q_fin);
    const size_t nbytes = (size_t)(co + L.co_bytes - from), at_co = (size_t)(co - from);
    if (gl->pin_out.ensure(nbytes)) return 1;
    char *back = gl->pin_out.as<char>();
    HIPCHK(hipMemcpyAsync(back, from, nbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const float *bq = reinterpret_cast<const float *>(back), *bgx = bq + A, *bgs = bq + 4 * (size_t)A + 1,
                *bphi = reinterpret_cast<const float *>(back + at_co), *bffix = bphi + A, *bgsf = reinterpret_cast<const float *>(back + at_co + L.gsf);
    const int flag = reinterpret_cast<const int *>(bq)[4 * (size_t)A], chit = reinterpret_cast<const int *>(bphi)[4 * (size_t)A];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (sum && flag == 0 && chit == CL_FLAG_FAR && ex && sum->xa) return excl_name_far(name, offsets, xyz, geo, *sum->xa);
    if (flag != 0 || chit != 0)
        EPNN_FAIL(sum ? "%s: two atoms of a cell or their periodic images coincide (distance 0: neither the Coulomb terms nor the edge features "
                        "have a derivative there)"
                      : "%s: two atoms of a molecule coincide (distance 0: neither the Coulomb terms nor the edge features have a derivative there)",
                  name);
    memcpy(out.q, bq, (size_t)A * 4);
    memcpy(out.phi, bphi, (size_t)A * 4);
    if (out.mu) memcpy(out.mu, site ? back + at_co + L.mu : reinterpret_cast<const char *>(bphi), (size_t)A * 4);
    memcpy(out.e, back + at_co + L.E, (size_t)B * 8);
    for (size_t k = 0; k < 3 * (size_t)A; ++k) {
        const float fq = -bgx[k];
        out.f[k] = bffix[k] + fq;
        if (out.fq) out.fq[k] = fq;
    }
    if (out.ffix) memcpy(out.ffix, bffix, (size_t)A * 12);
    if (!strain) return 0;
    for (size_t k = 0; k < 9 * (size_t)B; ++k) out.gs[k] = bgsf[k] + bgs[k];
    if (out.gs_fix) memcpy(out.gs_fix, bgsf, (size_t)B * 36);
    if (out.gs_q) memcpy(out.gs_q, bgs, (size_t)B * 36);
    return 0;
}
