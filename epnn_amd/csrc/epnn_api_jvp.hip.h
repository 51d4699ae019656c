// epnn_charges_jvp_xyz_cell, epnn_charges_jvp_multi_xyz_cell: charges and their directional derivatives along K tangents
// (vxyz, vstrain, vQ) of a flat coordinate batch (kernels and arithmetic: epnn_jvp.hip.h).  Part of the one translation unit
// epnn_api.hip.
#pragma once
#include "epnn_jvp.hip.h"

// (jvm_chunk, jvm_bucket: epnn_api_pairlist.hip.h, shared with the reverse-mode backward)
template <int KC>
static void jvm_sweep_launch(epnn_handle *h, const GlCall &c, const float *W2, const float *P, const float *tP, const float *R, const float *Yb,
                             const float *tR, size_t tstride, float *outS, float *outT, size_t ostride) {
    hipLaunchKernelGGL(k_jvm_sweep<KC>, dim3(c.nt), dim3(64), 0, h->stream, c.d_tasks, c.d_moff, c.G.A, W2, P, tP, R, Yb, tR, tstride, outS, outT,
                       ostride, (int)c.nt);
}

// The listed pairs' edge tangents te in the call's geometry: open molecules or cells (charges_jvp_multi_impl refuses box rows: no box instance)
template <int KM>
static void launch_jvm_edge(epnn_handle *h, const GlCall &c, int K, int B, const float *d_v, const float *d_E, float *te, int *bad) {
    geo_dispatch(c.geo.kind, [&](auto kind) {
        if constexpr (decltype(kind)::value != GEO_BOX)
            hipLaunchKernelGGL((k_jvm_edge<decltype(kind)::value, KM>), dim3((unsigned)((c.np + 255) / 256)), dim3(256), 0, h->stream, c.L, c.np,
                               c.d_molof, c.d_xyz, c.geo.words(), K, c.G.A, B, d_v, d_E, (double)h->cfg.cutoff, (double)h->cfg.eta,
                               h->d_mu.as<double>(), te, c.P1 * GL_E, bad);
    });
}

// K tangents beside the one primal; the single-tangent entry is K = 1.  The call shares the pair-list gradient path's state
// (GradLarge: the weights in plain Keras layout, refreshed when weights_gen moves on, and the input / scratch buffers, which keep the
// size of the largest call of either kind): neither the training state nor the forward's plan and pair list are touched.
static int charges_jvp_multi_impl(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                  const float *Q, const HostGeo &geo, int K, const float *vxyz, const float *vstrain, const float *vQ,
                                  float *q_out, float *tq_out) {
    if (geo.kind == GEO_BOX) EPNN_FAIL("%s: internal error (box rows: the tangent kernels take cells)", name);
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int T = h->cfg.T, A = offsets[B];
    const size_t Kz = (size_t)K;
    // the tangents: vQ as zeros when null, vxyz and vstrain left out
    const GlSpan spans[3] = {{vQ, Kz * B * 4, true}, {vxyz, vxyz ? Kz * A * 12 : 0, false}, {vstrain, vstrain ? Kz * B * 36 : 0, false}};
    GlCall c;
    if (gl_call_count(h, gl, name, B, N, offsets, xyz, x, Q, geo, spans, 3, c)) return 1;
    const size_t P1 = c.P1, SL = 2 * P1, nH = (size_t)A * GL_H, nE = (size_t)A * GL_E, rowH = nH * 4, rowE = nE * 4, maxp = (size_t)c.maxp;
    // the primal rows once, the tangent rows K times (one buffer each, tangent t at t times one tangent's size)
    const size_t o_te = c.place(Kz * P1 * GL_E * 4), o_h = c.place(2 * rowE), o_th = c.place(2 * Kz * rowE),
                 o_P = c.place(rowH), o_R = c.place(rowH), o_Yb = c.place(rowH), o_Yc = c.place(rowH), o_tP = c.place(Kz * rowH),
                 o_tR = c.place(Kz * rowH), o_partS = c.place(maxp * rowH), o_partT = c.place(Kz * maxp * rowH),
                 o_slotS = c.place(SL * GL_H * 4), o_slotT = c.place(Kz * SL * GL_H * 4), o_slotq = c.place(SL * 4),
                 o_slott = c.place(Kz * SL * 4), o_q = c.place(2 * (size_t)A * 4), o_tq = c.place(2 * Kz * A * 4),
                 o_out = c.place(((size_t)A * (1 + Kz) + 1) * 4);
    if (gl_call_fill(h, gl, c, c.in_total)) return 1;
    const int np = c.np;
    const unsigned gP = (unsigned)np, gA = c.gA;
    const GlGeom &G = c.G;
    const GlPairs &L = c.L;
    const int *inc = c.inc;
    const float *d_x = c.d_x, *d_Q = c.d_Q, *d_vQ = c.d_extra[0], *d_v = c.d_extra[1], *d_E = c.d_extra[2];
    float *out = c.fp(o_out);                                      // [A] q | [K][A] tq | bad
    int *bad = reinterpret_cast<int *>(out + (1 + Kz) * A);
    HIPCHK(hipMemsetAsync(bad, 0, 4, h->stream));
    float *te = c.fp(o_te);
    if (np > 0) {
        // ---- edge tangents
        jvm_bucket(K, [&](auto km) { launch_jvm_edge<decltype(km)::value>(h, c, K, B, d_v, d_E, te, bad); });
        HIPCHK(hipGetLastError());
    }
    float *hb[2] = {c.fp(o_h), c.fp(o_h) + nE}, *thb[2] = {c.fp(o_th), c.fp(o_th) + Kz * nE};
    float *qb[2] = {c.fp(o_q), c.fp(o_q) + A}, *tqb[2] = {c.fp(o_tq), c.fp(o_tq) + Kz * A};
    float *dP = c.fp(o_P), *dR = c.fp(o_R), *Yb = c.fp(o_Yb), *Yc = c.fp(o_Yc), *tP = c.fp(o_tP), *tR = c.fp(o_tR), *partS = c.fp(o_partS), *partT = c.fp(o_partT),
          *slotS = c.fp(o_slotS), *slotT = c.fp(o_slotT), *slotq = c.fp(o_slotq), *slott = c.fp(o_slott);
    const dim3 w64(64);
    const size_t pstride = maxp * nH;
    // the charges before the first EPN step and their tangents: Q / n, vQ / n (every GNN step sees these)
    hipLaunchKernelGGL(k_gl_q0, dim3(gA), dim3(256), 0, h->stream, G, d_Q, qb[0]);
    hipLaunchKernelGGL(k_jvm_q0, dim3(gA), dim3(256), 0, h->stream, G, K, B, d_vQ, tqb[0]);
    // ---- GNN steps
    for (int t = 0; t < T; ++t) {
        const float *ht = t ? hb[t & 1] : nullptr, *tht = t ? thb[t & 1] : nullptr;
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_jvm_proj<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->msg[t], G, K, tht, (const float *)tqb[0],
                               tP, tR);
        });
        for (int k0 = 0; k0 < K;) {                                 // the first chunk's launch stores the primal rows
            const int kc = jvm_chunk(K - k0);
            const float *cP = tP + k0 * nH, *cR = tR + k0 * nH;
            float *oS = k0 ? nullptr : partS, *oT = partT + k0 * pstride;
            if (kc == 4) jvm_sweep_launch<4>(h, c, gl->msg[t].W2, dP, cP, dR, Yb, cR, nH, oS, oT, pstride);
            else if (kc == 2) jvm_sweep_launch<2>(h, c, gl->msg[t].W2, dP, cP, dR, Yb, cR, nH, oS, oT, pstride);
            else jvm_sweep_launch<1>(h, c, gl->msg[t].W2, dP, cP, dR, Yb, cR, nH, oS, oT, pstride);
            k0 += kc;
        }
        if (np > 0)
            jvm_bucket(K, [&](auto km) {
                hipLaunchKernelGGL((k_jvm_gnn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->msg[t], L, K, A, P1, SL,
                                   (const float *)te, (const float *)dP, (const float *)dR, (const float *)tP, (const float *)tR, slotS,
                                   slotT);
            });
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_jvm_gnn_tail<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->msg[t], gl->upd, G, K, pstride, SL,
                               inc, (const float *)partS, (const float *)partT, (const float *)slotS, (const float *)slotT,
                               (const float *)dP, (const float *)tP, ht, tht, hb[(t + 1) & 1], thb[(t + 1) & 1]);
        });
    }
    HIPCHK(hipGetLastError());
    // ---- EPN steps
    const float *feats = hb[T & 1], *tfeats = thb[T & 1];
    for (int t = 0; t < T; ++t) {
        const float *qt = qb[t & 1], *tqt = tqb[t & 1];
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->pas[t], G, d_x, feats, qt, d_Q, dP, dR, (float *)nullptr, (float *)nullptr);
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_jvm_proj<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->pas[t], G, K, tfeats, tqt, tP, tR);
        });
        if (np > 0)
            jvm_bucket(K, [&](auto km) {
                hipLaunchKernelGGL((k_jvm_epn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->pas[t], L, K, A, P1, SL,
                                   (const float *)te, (const float *)dP, (const float *)dR, (const float *)tP, (const float *)tR, slotq,
                                   slott);
            });
        hipLaunchKernelGGL(k_jvm_epn_atom, dim3(gA), dim3(256), 0, h->stream, A, K, SL, inc, (const float *)slotq, qt, qb[(t + 1) & 1],
                           (const float *)slott, tqt, tqb[(t + 1) & 1]);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, qb[T & 1], (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(out + A, tqb[T & 1], Kz * A * 4, hipMemcpyDeviceToDevice, h->stream));
    const size_t nback = (size_t)A * (1 + Kz) + 1;                  // one download: q, the K A tangents and the flag word
    if (gl->pin_out.ensure(nback * 4)) return 1;
    float *back = gl->pin_out.as<float>();
    HIPCHK(hipMemcpyAsync(back, out, nback * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int flag = reinterpret_cast<const int *>(back)[nback - 1];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (flag != 0)
        EPNN_FAIL("%s: two atoms of a molecule%s coincide (distance 0: the edge features have no derivative there)", name,
                  geo.periodic() ? " or their periodic images" : "");
    memcpy(q_out, back, (size_t)A * 4);
    memcpy(tq_out, back + A, Kz * A * 4);
    return 0;
}

// What the two entries check and settle before the call (K = 1: the single-tangent entry); arg: the checked cell (a null cell: open molecules).
static int charges_jvp_enter(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                             const float *Q, const float *cell, int K, const float *q_out, const float *tq_out, GeoArg &arg) {
    if (!h || !offsets || !xyz || !x || !Q || !q_out || !tq_out) EPNN_FAIL("%s: null argument", name);
    if (K < 1 || K > JVM_MAXK) EPNN_FAIL("%s: K must be in 1..%d, got %d", name, JVM_MAXK, K);
    if (check_flat_batch(name, B, N, offsets)) return 1;
    EPNN_NOT_FUSED_ONLY(h, name);
    if (cell && arg.cell(B, cell, (double)h->cfg.cutoff, name)) return 1;
    if (h->upd_generic) EPNN_FAIL("%s is built for update layers [32, 32] only (epnn_set_update_layers changed them)", name);
    if (h->part_world != 1) EPNN_FAIL("%s does not run on a partitioned handle (epnn_set_partition)", name);
    HIPCHK(hipSetDevice(h->device));
    if (h->pending.active && finish_forward(h)) return 1;
    // the weights epnn_forward_xyz would use: a training step still in flight is waited for, device masters it has updated are
    // pulled into the host copies (what any inference call does first)
    return train_quiesce(h) || pack_weights(h);
}

extern "C" int epnn_charges_jvp_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                         const float *Q, const float *cell, const float *vxyz, const float *vstrain, const float *vQ,
                                         float *q_out, float *tq_out) {
    const char *name = "epnn_charges_jvp_xyz_cell";
    GeoArg arg;
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, cell, 1, q_out, tq_out, arg)) return 1;
    return charges_jvp_multi_impl(h, name, B, N, offsets, xyz, x, Q, arg.geo, 1, vxyz, vstrain, vQ, q_out, tq_out);
}

extern "C" int epnn_charges_jvp_multi_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                               const float *Q, const float *cell, int K, const float *vxyz, const float *vstrain,
                                               const float *vQ, float *q_out, float *tq_out) {
    const char *name = "epnn_charges_jvp_multi_xyz_cell";
    GeoArg arg;
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, cell, K, q_out, tq_out, arg)) return 1;
    return charges_jvp_multi_impl(h, name, B, N, offsets, xyz, x, Q, arg.geo, K, vxyz, vstrain, vQ, q_out, tq_out);
}
